// gossip_dump.hip — read-back of the engine's state and statistics for tests, tools and the
// bench: members, views, queues (heads and tails), dedup buffers, rumors, the delivery log,
// phase times, totals and the guard-zone / canary diagnostics.  Nothing here runs in a round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gossip_ctx.h"
#include "gossip_queue4.h"

extern "C" {

// diagnostic (RSF_GUARD_ZONES builds): changed bytes in the guard zones, in the order before
// stage_dec, after stage_dec, before big_ids, after big_ids (synchronises); -1 without zones
int rsf_gossip_debug_zones(rsf_gossip* g, uint64_t* out4) {
  if (!g || !out4) return gerr("null argument");
  if (!kZone) return -1;
  RSF_HIP(hipStreamSynchronize(g->stream));
  const char* z[4] = {g->dec_base, g->dec_base + kZone + g->stage_cap * 4, g->big_base,
                      g->big_base + kZone + g->c.n_loc * 4};
  std::vector<uint8_t> v(kZone);
  for (int k = 0; k < 4; ++k) {
    RSF_HIP(hipMemcpy(v.data(), z[k], kZone, hipMemcpyDeviceToHost));
    uint64_t c = 0;
    for (uint8_t b : v) c += b != 0xA5;
    out4[k] = c;
  }
  return RSF_OK;
}

// the canaries past the hipCUB temporaries (rsf::CubTemp): radix sorts, group count
// reduce/scan, run-merge scan; 1 = intact (or never allocated), 0 = overrun (synchronises)
int rsf_gossip_debug_canaries(rsf_gossip* g, int* out3) {
  if (!g || !out3) return gerr("null argument");
  RSF_HIP(hipSetDevice(g->device));
  const rsf::CubTemp* t[3] = {&g->sort_tmp, &g->grp_tmp, &g->scan_tmp};
  for (int k = 0; k < 3; ++k) {
    const int r = t[k]->canary_intact(g->stream);
    if (r < 0) return r;
    out3[k] = r;
  }
  return RSF_OK;
}

static int check_stats(rsf_gossip* g, uint64_t* num_queued, uint64_t* n_warn, uint64_t* n_pruned) {
  unsigned long long st[kCheckStatWords];
  RSF_HIP(hipMemcpyAsync(st, g->d_counters + kCtrCheckStats, sizeof(st), hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  for (int q = 0; q < 3; ++q) {
    if (num_queued) num_queued[q] = st[q];
    if (n_warn) n_warn[q] = st[3 + q];
    if (n_pruned) n_pruned[q] = st[6 + q];
  }
  return RSF_OK;
}

int rsf_gossip_checker_stats(rsf_gossip* g, uint64_t* num_queued, uint64_t* n_warn, uint64_t* n_pruned, int reset) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  const bool have = g->occ_hist != nullptr;
  int rc = RSF_OK;
  if (have) {
    rc = check_stats(g, num_queued, n_warn, n_pruned);
  } else {
    for (int q = 0; q < 3; ++q) {
      if (num_queued) num_queued[q] = 0;
      if (n_warn) n_warn[q] = 0;
      if (n_pruned) n_pruned[q] = 0;
    }
  }
  if (!rc && reset && have) {
    RSF_HIP(hipMemsetAsync(g->occ_hist, 0, kOccHistWords * 4, g->stream));
    RSF_HIP(hipMemsetAsync(g->d_counters + kCtrCheckStats, 0, kCheckStatWords * 8, g->stream));
  }
  return rc;
}

int rsf_gossip_action_status(rsf_gossip* g, int32_t* status, uint32_t n) {
  if (!g || (n && !status)) return gerr("null argument");
  if (n > g->last_n_acts) return gerr("n exceeds the last round's action count");
  if (!n) return RSF_OK;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(status, g->d_act_status, (size_t)n * 4, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_checker_occupancy(rsf_gossip* g, uint32_t* hist, uint32_t* max3, uint32_t* bin, uint32_t* bins) {
  if (!g) return gerr("null context");
  if (bin) *bin = kOccBin;
  if (bins) *bins = kOccBins + 1;
  if (!hist && !max3) return RSF_OK;
  std::vector<uint32_t> h(kOccHistWords, 0u);
  if (g->occ_hist) {
    RSF_HIP(hipSetDevice(g->device));
    RSF_HIP(hipMemcpyAsync(h.data(), g->occ_hist, h.size() * 4, hipMemcpyDeviceToHost, g->stream));
    RSF_HIP(hipStreamSynchronize(g->stream));
  }
  if (hist) std::copy(h.begin(), h.begin() + 3 * (kOccBins + 1), hist);
  if (max3) std::copy(h.begin() + 3 * (kOccBins + 1), h.end(), max3);
  return RSF_OK;
}

int rsf_gossip_flush(rsf_gossip* g) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  return flush_pending(g);
}

int rsf_gossip_pruned_total(rsf_gossip* g, int flush, uint64_t* total) {
  if (!g || !total) return gerr("null argument");
  RSF_HIP(hipSetDevice(g->device));
  int rc;
  if (flush && (rc = flush_pending(g))) return rc;
  std::vector<uint32_t> v(g->c.n_loc);
  RSF_HIP(hipMemcpyAsync(v.data(), g->s.q_pruned, g->c.n_loc * 4, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  uint64_t t = 0;
  for (uint32_t x : v) t += x;
  *total = t;
  return RSF_OK;
}

int rsf_gossip_dump_pruned(rsf_gossip* g, uint32_t* pruned, uint32_t* expired) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);
  if (rc) return rc;
  if (pruned) RSF_HIP(hipMemcpyAsync(pruned, g->s.q_pruned, g->c.n_loc * 4, hipMemcpyDeviceToHost, g->stream));
  if (expired) RSF_HIP(hipMemcpyAsync(expired, g->s.q_expired, g->c.n_loc * 4, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_delivery_log(rsf_gossip* g, uint32_t per_member) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipStreamSynchronize(g->stream));
  if (g->s.dlog) hipFree(g->s.dlog);
  if (g->s.dmeta) hipFree(g->s.dmeta);
  if (g->s.dcnt) hipFree(g->s.dcnt);
  g->s.dlog = nullptr;
  g->s.dmeta = nullptr;
  g->s.dcnt = nullptr;
  g->c.dcap = 0;
  if (!per_member) return RSF_OK;
  int rc;
  if ((rc = rsf::dmalloc((void**)&g->s.dlog, (size_t)g->c.n_loc * per_member * 16)) ||
      (rc = rsf::dmalloc((void**)&g->s.dmeta, (size_t)g->c.n_loc * per_member)) ||
      (rc = rsf::dmalloc((void**)&g->s.dcnt, g->c.n_loc * 4)))
    return rc;
  RSF_HIP(hipMemsetAsync(g->s.dcnt, 0, g->c.n_loc * 4, g->stream));
  g->c.dcap = per_member;
  return RSF_OK;
}

int rsf_gossip_dump_deliveries(rsf_gossip* g, rsf_delivery* out, uint64_t cap, uint64_t* n_out) {
  if (!g || !n_out || (cap && !out)) return gerr("null argument");
  *n_out = 0;
  const GCfg& c = g->c;
  if (!c.dcap) return RSF_OK;
  std::vector<uint32_t> cnt(c.n_loc);
  std::vector<uint4> log((size_t)c.n_loc * c.dcap);
  std::vector<uint8_t> meta((size_t)c.n_loc * c.dcap);
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(cnt.data(), g->s.dcnt, c.n_loc * 4, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipMemcpyAsync(log.data(), g->s.dlog, log.size() * 16, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipMemcpyAsync(meta.data(), g->s.dmeta, meta.size(), hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  uint64_t o = 0;
  for (uint64_t l = 0; l < c.n_loc; ++l)
    for (uint32_t k = 0; k < std::min(cnt[l], c.dcap); ++k) {
      if (o >= cap) return rsf::set_error(RSF_ERR_OVERFLOW, "delivery dump capacity exceeded");
      const uint4 e = log[l * c.dcap + k];
      const uint64_t lt = ((uint64_t)e.y << 32) | e.x;
      rsf_delivery& d = out[o++];
      const uint8_t f = meta[l * c.dcap + k];
      const bool mev = (f & kLogMember) != 0;
      d.ltime = lt;
      d.key = ((uint64_t)e.w << 32) | e.z;
      d.member = (uint32_t)(c.lo + l);
      d.cc = (f & kLogCc) ? 1 : 0;
      d.kind = mev ? RSF_DELIVERY_MEMBER_EVENT : RSF_DELIVERY_USER_EVENT;
      d._r[0] = d._r[1] = 0;
    }
  *n_out = o;
  return RSF_OK;
}

int rsf_gossip_dump_members(rsf_gossip* g, uint64_t* clock, uint64_t* ec, uint64_t* qc, uint64_t* digest, uint32_t* err,
                            uint8_t* serf_state) {
  if (!g) return gerr("null context");
  const uint64_t n = g->c.n_loc;
  hipStream_t st = g->stream;
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);  // queue-prune flags
  if (rc) return rc;
  if (clock) RSF_HIP(hipMemcpyAsync(clock, g->s.clock, n * 8, hipMemcpyDeviceToHost, st));
  if (ec) RSF_HIP(hipMemcpyAsync(ec, g->s.eclock, n * 8, hipMemcpyDeviceToHost, st));
  if (qc) RSF_HIP(hipMemcpyAsync(qc, g->s.qclock, n * 8, hipMemcpyDeviceToHost, st));
  if (digest) RSF_HIP(hipMemcpyAsync(digest, g->s.digest, n * 8, hipMemcpyDeviceToHost, st));
  if (err) RSF_HIP(hipMemcpyAsync(err, g->s.err, n * 4, hipMemcpyDeviceToHost, st));
  if (serf_state) RSF_HIP(hipMemcpyAsync(serf_state, g->s.serf_state, n, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipStreamSynchronize(st));
  return RSF_OK;
}

int rsf_gossip_dump_view_rows(rsf_gossip* g, uint64_t row0, uint64_t rows, uint64_t* ltime, uint8_t* status,
                              uint8_t* kind, uint32_t* time) {
  if (!g || !ltime || !status || !kind) return gerr("null argument");
  if (row0 > g->c.n_loc || rows > g->c.n_loc - row0) return gerr("rows outside the shard");
  const uint64_t cnt = rows * g->c.S;
  const GCfg& c = g->c;
  std::vector<uint4> raw(rows * c.vrow / 16);
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(raw.data(), vrow_of(g->s, c, row0), rows * c.vrow, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  ViewS* const base = reinterpret_cast<ViewS*>(raw.data());
  for (uint64_t i = 0; i < cnt; ++i) {
    const ViewE v = *view_at(view_row(base, c.vrow, i / c.S), (uint32_t)(i % c.S));
    ltime[i] = v.ltime;
    status[i] = (uint8_t)(v.meta & 0xFF);
    kind[i] = (uint8_t)((v.meta >> 8) & 0xFF);
    if (time) time[i] = v.t;  // (mod 2^27)
  }
  return RSF_OK;
}

int rsf_gossip_dump_view(rsf_gossip* g, uint64_t* ltime, uint8_t* status, uint8_t* kind, uint32_t* time) {
  if (!g) return gerr("null argument");
  return rsf_gossip_dump_view_rows(g, 0, g->c.n_loc, ltime, status, kind, time);
}

// head and tail merged on the host into [n_loc][3][D] in send order
// every queue of local rows [r0, r0 + n) merged from head and tail (tail only on deep
// contexts), sorted, first D items; output row 0 = local row r0
static int dump_queues_deep(rsf_gossip* g, uint32_t D, uint32_t* rumor, uint32_t* seq, uint16_t* tx, uint16_t* len,
                            uint32_t* max_live, uint64_t r0 = 0, uint64_t rows = ~0ull) {
  const GCfg& c = g->c;
  const uint64_t n = std::min<uint64_t>(rows, c.n_loc - r0), hc = n * 3 * c.qcap;
  uint32_t most = 0;
  std::vector<uint32_t> hr(hc), hs(hc), ht(hc);
  std::vector<uint4> sum(n * 3);
  std::vector<std::vector<uint4>> tail(3);
  std::vector<uint64_t> tail0;  // the intent queue's packed items
  std::vector<uint32_t> nseq(n * 3);
  hipStream_t st = g->stream;
  const uint64_t h0 = r0 * 3 * c.qcap;
  RSF_HIP(hipMemcpyAsync(hr.data(), g->s.q_rumor + h0, hc * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipMemcpyAsync(hs.data(), g->s.q_seq + h0, hc * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipMemcpyAsync(ht.data(), g->s.q_txlen + h0, hc * 4, hipMemcpyDeviceToHost, st));
  // tails and their summaries exist only on deep contexts; otherwise every queue is its head
  if (c.deep) RSF_HIP(hipMemcpyAsync(sum.data(), g->s.tsum + r0 * 3, n * 3 * 16, hipMemcpyDeviceToHost, st));
  for (uint32_t q = 0; q < 3; ++q)
    if (tcap_of(c, q)) {
      if (q == 0) {
        tail0.resize(n * c.tstride0);
        RSF_HIP(hipMemcpyAsync(tail0.data(), g->s.tail0 + r0 * c.tstride0, tail0.size() * 8, hipMemcpyDeviceToHost, st));
      } else {
        tail[q].resize(n * tstride_of(c, q));
        RSF_HIP(hipMemcpyAsync(tail[q].data(), tail16(g->s, q) + r0 * tstride_of(c, q), tail[q].size() * 16,
                               hipMemcpyDeviceToHost, st));
      }
    }
  RSF_HIP(hipMemcpyAsync(nseq.data(), g->s.q_next_seq + r0 * 3, n * 3 * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipStreamSynchronize(st));
  std::vector<std::pair<uint64_t, uint32_t>> items;
  for (uint64_t l = 0; l < n; ++l)
    for (uint32_t q = 0; q < 3; ++q) {
      items.clear();
      const uint64_t hb = (l * 3 + q) * c.qcap;
      for (uint32_t i = 0; i < c.qcap; ++i)
        if (hr[hb + i] != kEmpty) items.push_back({tlq_key(ht[hb + i] & 0xFFFF, ht[hb + i] >> 16, hs[hb + i]), hr[hb + i]});
      if (tcap_of(c, q))
        for (uint32_t i = 0; i < sum[l * 3 + q].x; ++i) {
          const uint4 e = q == 0 ? tail_unpack(c, tail0[l * c.tstride0 + i], nseq[l * 3])
                                 : tail[q][l * tstride_of(c, q) + i];
          items.push_back({tlq_key(e.z & 0xFFFF, e.z >> 16, e.y), e.x});
        }
      std::sort(items.begin(), items.end());
      most = std::max<uint32_t>(most, (uint32_t)items.size());
      const uint64_t ob = (l * 3 + q) * D;
      for (uint32_t i = 0; i < D; ++i) {
        const bool live = i < items.size();
        const uint64_t k = live ? items[i].first : 0ull;
        rumor[ob + i] = live ? items[i].second : kEmpty;
        seq[ob + i] = live ? 0xFFFFFFFFu - (uint32_t)k : 0u;
        tx[ob + i] = live ? (uint16_t)(k >> 48) : 0;
        len[ob + i] = live ? (uint16_t)(0xFFFF - ((k >> 32) & 0xFFFF)) : 0;
      }
    }
  if (max_live) *max_live = most;
  return RSF_OK;
}

int rsf_gossip_dump_queues_width(rsf_gossip* g, uint32_t width, uint32_t* rumor, uint32_t* seq, uint16_t* tx,
                                 uint16_t* len, uint32_t* next_seq, uint32_t* max_live) {
  if (!g || !rumor || !seq || !tx || !len || !next_seq || !width) return gerr("null argument");
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);
  if (rc) return rc;
  RSF_HIP(hipMemcpyAsync(next_seq, g->s.q_next_seq, g->c.n_loc * 3 * 4, hipMemcpyDeviceToHost, g->stream));
  return dump_queues_deep(g, width, rumor, seq, tx, len, max_live);
}

int rsf_gossip_dump_queues_rows(rsf_gossip* g, uint64_t row0, uint64_t rows, uint32_t width, uint32_t* rumor,
                                uint32_t* seq, uint16_t* tx, uint16_t* len, uint32_t* max_live) {
  if (!g || !rumor || !seq || !tx || !len || !width || row0 + rows > g->c.n_loc) return gerr("bad argument");
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);
  if (rc) return rc;
  return dump_queues_deep(g, width, rumor, seq, tx, len, max_live, row0, rows);
}

int rsf_gossip_dump_queues(rsf_gossip* g, uint32_t* rumor, uint32_t* seq, uint16_t* tx, uint16_t* len,
                           uint32_t* next_seq) {
  if (!g || !rumor || !seq || !tx || !len || !next_seq) return gerr("null argument");
  if (g->c.deep) {
    const uint32_t D = g->c.qcap + std::max(g->c.tcap0, std::max(g->c.tcap1, g->c.tcap2));
    return rsf_gossip_dump_queues_width(g, D, rumor, seq, tx, len, next_seq, nullptr);
  }
  const uint64_t cnt = g->c.n_loc * 3 * g->c.qcap;
  std::vector<uint32_t> tl(cnt);
  hipStream_t st = g->stream;
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);
  if (rc) return rc;
  RSF_HIP(hipMemcpyAsync(rumor, g->s.q_rumor, cnt * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipMemcpyAsync(seq, g->s.q_seq, cnt * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipMemcpyAsync(tl.data(), g->s.q_txlen, cnt * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipMemcpyAsync(next_seq, g->s.q_next_seq, g->c.n_loc * 3 * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipStreamSynchronize(st));
  for (uint64_t i = 0; i < cnt; ++i) {
    tx[i] = (uint16_t)(tl[i] & 0xFFFF);
    len[i] = (uint16_t)(tl[i] >> 16);
  }
  return RSF_OK;
}

int rsf_gossip_deep_stats(rsf_gossip* g, uint64_t* slow_total, uint64_t* slow_since_last) {
  if (!g) return gerr("null context");
  unsigned long long t = 0;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(&t, g->d_counters + kCtrDeepTotal, 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  if (slow_total) *slow_total = t;
  if (slow_since_last) *slow_since_last = t - g->deep_last;
  g->deep_last = t;
  return RSF_OK;
}

int rsf_gossip_deep_class_stats(rsf_gossip* g, uint64_t* out4) {
  if (!g || !out4) return gerr("null argument");
  unsigned long long t[8];
  RSF_HIP(hipSetDevice(g->device));
  // lists 0 (kDeepSmall), 1 (the full depth), 2 (kDeepTiny) at kCtrDeepClass + list,
  // list 3 (kDeepMid) at kCtrDeepMid
  static_assert(kCtrDeepMid - kCtrDeepClass == 7, "t[7] below is list 3");
  RSF_HIP(hipMemcpyAsync(t, g->d_counters + kCtrDeepClass, sizeof(t), hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  out4[0] = t[2];
  out4[1] = t[0];
  out4[2] = t[7];
  out4[3] = t[1];
  return RSF_OK;
}

int rsf_gossip_deep_full_items(rsf_gossip* g, uint64_t* sum, uint64_t* max) {
  if (!g || !sum || !max) return gerr("null argument");
  unsigned long long t[2] = {0, 0};
  RSF_HIP(hipSetDevice(g->device));
  if (g->c.deep) {
    RSF_HIP(hipMemcpyAsync(t, g->s.deep_n + kDeepFullItems, sizeof(t), hipMemcpyDeviceToHost, g->stream));
    RSF_HIP(hipStreamSynchronize(g->stream));
  }
  *sum = t[0];
  *max = t[1];
  return RSF_OK;
}

int rsf_gossip_dump_tails(rsf_gossip* g, uint32_t q, uint32_t* count, uint32_t* sealed) {
  if (!g || q > 2) return gerr("bad argument");
  const GCfg& c = g->c;
  const uint64_t n = c.n_loc;
  RSF_HIP(hipSetDevice(g->device));
  std::vector<uint4> ts(n * 3), tz(n * 3);
  if (c.deep) {
    RSF_HIP(hipMemcpyAsync(ts.data(), g->s.tsum, n * 3 * sizeof(uint4), hipMemcpyDeviceToHost, g->stream));
    RSF_HIP(hipMemcpyAsync(tz.data(), g->s.tseal, n * 3 * sizeof(uint4), hipMemcpyDeviceToHost, g->stream));
    RSF_HIP(hipStreamSynchronize(g->stream));
  }
  const bool dq = c.deep && tcap_of(c, q);
  for (uint64_t l = 0; l < n; ++l) {
    if (count) count[l] = dq ? ts[l * 3 + q].x : 0u;
    if (sealed) sealed[l] = dq ? std::min(tz[l * 3 + q].x, ts[l * 3 + q].x) : 0u;
  }
  return RSF_OK;
}

// per (member, queue): live items of the head (its leading slots) plus the tail's count
__global__ void __launch_bounds__(256) queue_lengths_kernel(GCfg c, GState s, uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= c.n_loc * 3) return;
  const uint64_t base = t * c.qcap;
  uint32_t n = 0;
  while (n < c.qcap && s.q_rumor[base + n] != kEmpty) n++;
  if (tcap_of(c, (uint32_t)(t % 3))) n += s.tsum[t].x;
  out[t] = n;
}

int rsf_gossip_queue_lengths(rsf_gossip* g, uint32_t* out) {
  if (!g || !out) return gerr("null argument");
  const GCfg& c = g->c;
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g);
  if (rc) return rc;
  void* dv = nullptr;
  const size_t bytes = c.n_loc * 3 * sizeof(uint32_t);
  if ((rc = g->scratch.take(&bytes, 1, &dv))) return rc;
  uint32_t* d = (uint32_t*)dv;
  hipLaunchKernelGGL(queue_lengths_kernel, dim3(grid1(c.n_loc * 3)), dim3(256), 0, g->stream, c, g->s, d);
  RSF_HIP(hipGetLastError());
  RSF_HIP(hipMemcpyAsync(out, d, c.n_loc * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_dump_buffers(rsf_gossip* g, uint64_t* eb_ltime, uint32_t* eb_cnt, uint64_t* eb_keys, uint64_t* qb_ltime,
                            uint32_t* qb_cnt, uint32_t* qb_ids) {
  if (!g) return gerr("null context");
  const GCfg& c = g->c;
  hipStream_t st = g->stream;
  RSF_HIP(hipSetDevice(g->device));
  if (eb_ltime) RSF_HIP(hipMemcpyAsync(eb_ltime, g->s.eb_ltime, c.n_loc * c.ebuf * 8, hipMemcpyDeviceToHost, st));
  if (eb_cnt) RSF_HIP(hipMemcpyAsync(eb_cnt, g->s.eb_cnt, c.n_loc * c.ebuf * 4, hipMemcpyDeviceToHost, st));
  if (eb_keys)
    RSF_HIP(hipMemcpyAsync(eb_keys, g->s.eb_keys, c.n_loc * c.ebuf * c.slot_k * 8, hipMemcpyDeviceToHost, st));
  if (qb_ltime) RSF_HIP(hipMemcpyAsync(qb_ltime, g->s.qb_ltime, c.n_loc * c.qbuf * 8, hipMemcpyDeviceToHost, st));
  if (qb_cnt) RSF_HIP(hipMemcpyAsync(qb_cnt, g->s.qb_cnt, c.n_loc * c.qbuf * 4, hipMemcpyDeviceToHost, st));
  if (qb_ids)
    RSF_HIP(hipMemcpyAsync(qb_ids, g->s.qb_ids, c.n_loc * c.qbuf * c.slot_k * 4, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipStreamSynchronize(st));
  return RSF_OK;
}

int rsf_gossip_dump_rumors(rsf_gossip* g, uint32_t first, uint32_t count, rsf_rumor* out) {
  if (!g || (count && !out)) return gerr("null argument");
  if ((uint64_t)first + count > 2ull * g->max_rumors) return gerr("rumor range out of bounds");
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(out, g->s.rumors + first, (size_t)count * sizeof(rsf_rumor), hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_dump_refutes(rsf_gossip* g, uint32_t* count, uint64_t* ltimes) {
  if (!g || !count || !ltimes) return gerr("null argument");
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(count, g->s.refute_cnt, g->c.S * 4, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipMemcpyAsync(ltimes, g->s.refute_ltime, (size_t)g->c.S * g->c.max_refute * 8, hipMemcpyDeviceToHost,
                         g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_profiling(rsf_gossip* g, int on) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  if (on && !g->events_made) {
    for (auto& row : g->ev)
      for (auto& e : row) RSF_HIP(hipEventCreate(&e));
    g->events_made = true;
  }
  g->profiling = on != 0;
  g->prof_rounds = 0;
  return RSF_OK;
}

int rsf_gossip_phase_times(rsf_gossip* g, double* ms_out, uint32_t* rounds_out) {
  if (!g || !ms_out) return gerr("null argument");
  for (int k = 0; k < rsf_gossip::kMarks - 1; ++k) ms_out[k] = 0.0;
  RSF_HIP(hipSetDevice(g->device));
  for (int r = 0; r < g->prof_rounds; ++r) {
    RSF_HIP(hipEventSynchronize(g->ev[r][rsf_gossip::kMarks - 1]));
    for (int k = 0; k + 1 < rsf_gossip::kMarks; ++k) {
      float ms = 0.f;
      RSF_HIP(hipEventElapsedTime(&ms, g->ev[r][k], g->ev[r][k + 1]));
      ms_out[k] += ms;
    }
  }
  if (rounds_out) *rounds_out = (uint32_t)g->prof_rounds;
  g->prof_rounds = 0;
  return RSF_OK;
}

int rsf_gossip_totals(rsf_gossip* g, uint64_t* merged_total) {
  if (!g || !merged_total) return gerr("null argument");
  unsigned long long t = 0;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(&t, g->d_counters + kCtrMergedTotal, 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  *merged_total = t + g->total_merged_host;
  return RSF_OK;
}

int rsf_gossip_last_round_stats(rsf_gossip* g, uint64_t* sent, uint64_t* merged) {
  if (!g) return gerr("null context");
  unsigned long long nv = 0;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(&nv, g->d_counters + kCtrSent, 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  if (g->merged_from_buckets) {  // bucket exchange: this shard's merged records; emission is not summed
    RSF_HIP(hipMemcpyAsync(&nv, g->d_counters + kCtrBktMerged, 8, hipMemcpyDeviceToHost, g->stream));
    RSF_HIP(hipStreamSynchronize(g->stream));
    if (sent) *sent = 0;
    if (merged) *merged = nv;
    return RSF_OK;
  }
  if (sent) *sent = nv;
  if (merged) *merged = g->merged_from_stage ? nv : g->last_merged;
  return RSF_OK;
}

}  // extern "C"
