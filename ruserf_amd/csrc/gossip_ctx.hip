// gossip_ctx.hip — the gossip context's life cycle: creation (validation, allocation, initial
// state), destruction, the stream, and the setters that load state before or between rounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "gossip_ctx.h"
#include "gossip_queue.h"

namespace {

__global__ void init_views_kernel(ViewS* view, uint64_t vrow, uint64_t n_loc, uint32_t S, const uint8_t* kind,
                                  const uint8_t* status, const uint64_t* ltime) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_loc * S) return;
  uint32_t subj = (uint32_t)(i % S);
  ViewE v;
  v.ltime = ltime[subj];
  v.meta = vmeta(status[subj], kind[subj]);
  v.t = 0;
  *view_at(view_row(view, vrow, i / S), subj) = v;
}

__global__ void tsum_init_kernel(uint4* p, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = kTSumEmpty;
}

__global__ void iota_u32_kernel(uint32_t* p, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (uint32_t)i;
}

__global__ void fill_u64_kernel(uint64_t* p, uint64_t n, uint64_t v) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

extern "C" {

int rsf_gossip_create(rsf_gossip** out, const rsf_gossip_cfg* cfg, int device) {
  if (!out || !cfg) return gerr("null argument");
  *out = nullptr;
  const uint64_t N = cfg->n_members;
  if (N < 2 || N >= 0xFFFFFFFFull) return gerr("n_members must be in [2, 2^32-1)");
  if (cfg->shard_lo >= cfg->shard_hi || cfg->shard_hi > N) return gerr("bad shard range");
  if (cfg->n_subjects == 0 || cfg->n_subjects > N) return gerr("n_subjects must be in [1, n_members]");
  if (cfg->queue_cap == 0 || cfg->queue_cap > 256) return gerr("queue_cap must be 1..256");
  if (cfg->event_buffer_size == 0 || cfg->query_buffer_size == 0) return gerr("dedup buffers must be non-empty");
  if (cfg->slot_k == 0 || cfg->slot_k > 64) return gerr("slot_k must be 1..64");
  if (cfg->fanout == 0 || cfg->fanout > 8 || cfg->fanout >= N) return gerr("fanout must be 1..8 and < n_members");
  if (cfg->gossip_limit > 0xFFFFFF || cfg->gossip_overhead > 0xFFFF) return gerr("gossip budget too large");
  if (cfg->max_refute == 0 || cfg->max_refute > 4) return gerr("max_refute must be 1..4");
  if (cfg->max_rumors == 0 || (cfg->max_rumors & (cfg->max_rumors - 1)) || cfg->max_rumors > (1u << 30))
    return gerr("max_rumors must be a power of two <= 2^30 (the rumor ring)");
  if (cfg->max_user_event_size > RSF_USER_EVENT_SIZE_LIMIT)  // Serf::new_in (base.rs:69-70)
    return rsf::set_error(RSF_ERR_USER_EVENT_LIMIT, "max_user_event_size exceeds USER_EVENT_SIZE_LIMIT (9 KiB)");
  if (cfg->query_size_limit > 0xFFFE) return gerr("query_size_limit must be <= 65534 (16-bit message lengths)");
  for (int q = 0; q < 3; ++q) {
    const uint32_t d = cfg->queue_depth[q];
    if (d && d < cfg->queue_cap) return gerr("queue_depth must be 0 or >= queue_cap");
    if (d > cfg->queue_cap && cfg->queue_cap > kWave) return gerr("deep queues need queue_cap <= 64 (the register head)");
    if (d > RSF_MAX_QUEUE_DEPTH) return gerr("queue_depth exceeds RSF_MAX_QUEUE_DEPTH");
  }
  RSF_HIP(hipSetDevice(device));
  rsf_gossip* g = new (std::nothrow) rsf_gossip();
  if (!g) return rsf::set_error(RSF_ERR_NOMEM, "host allocation failed");
  g->device = device;
  GCfg& c = g->c;
  c.N = N;
  c.lo = cfg->shard_lo;
  c.n_loc = cfg->shard_hi - cfg->shard_lo;
  c.S = cfg->n_subjects;
  c.vrow = view_row_bytes(c.S);
  c.qcap = cfg->queue_cap;
  c.ebuf = cfg->event_buffer_size;
  c.qbuf = cfg->query_buffer_size;
  c.slot_k = cfg->slot_k;
  c.fanout = cfg->fanout;
  c.limit = cfg->gossip_limit;
  c.overhead = cfg->gossip_overhead;
  {  // memberlist retransmitLimit = mult * ceil(log10(n+1))
    uint64_t x = N + 1, p = 1;
    uint32_t d = 0;
    while (p < x) {
      p *= 10;
      d++;
    }
    c.tx_limit = cfg->retransmit_mult * d;
  }
  c.max_refute = cfg->max_refute;
  c.max_ue = cfg->max_user_event_size ? cfg->max_user_event_size : 512u;  // options.rs:526
  c.query_limit = cfg->query_size_limit ? cfg->query_size_limit : 1024u;  // options.rs:519
  uint32_t max_depth = c.qcap;
  {  // deep queues: the tail behind the register head
    uint32_t tc[3];
    for (int q = 0; q < 3; ++q) {
      const uint32_t d = cfg->queue_depth[q];
      tc[q] = d > c.qcap ? d - c.qcap : 0u;
      c.deep |= tc[q] ? 1u : 0u;
      max_depth = std::max(max_depth, c.qcap + tc[q]);
    }
    c.tcap0 = tc[0];
    c.tcap1 = tc[1];
    c.tcap2 = tc[2];
    c.tstride0 = tc[0] ? tc[0] + kTailSlack : 0u;
    c.tstride1 = tc[1] ? tc[1] + kTailSlack : 0u;
    c.tstride2 = tc[2] ? tc[2] + kTailSlack : 0u;
  }
  {
    uint64_t per = c.limit / (c.overhead + kMinMsgLen);
    c.cap_t = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(3ull * max_depth, per));
  }
  c.k0 = (uint32_t)cfg->seed;
  c.k1 = (uint32_t)(cfg->seed >> 32);
  g->max_rumors = cfg->max_rumors;
  c.rbits = 0;
  while ((1u << c.rbits) < cfg->max_rumors) c.rbits++;
  c.rmask = (cfg->max_rumors << 1) - 1;
  c.gen = 0;
  g->end_bit = bits_for(N);
  auto fail = [&](int code) {
    rsf_gossip_destroy(g);
    return code;
  };
  // the intent queue's packed tail items (tail_pack): the ring slot and parity in 27 bits,
  // transmits in 6
  if (c.tcap0 && c.rbits > 26) return fail(gerr("a deep intent queue needs max_rumors <= 2^26 (packed tail items)"));
  if (c.tcap0 && c.tx_limit > 64)
    return fail(gerr("a deep intent queue needs a retransmit limit <= 64 (packed tail items)"));
  if (hipStreamCreateWithFlags(&g->own, hipStreamNonBlocking) != hipSuccess)
    return fail(rsf::set_error(RSF_ERR_HIP, "hipStreamCreate failed"));
  g->stream = g->own;
  if (hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev_emitted, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev_ahead, hipEventDisableTiming) != hipSuccess)
    return fail(rsf::set_error(RSF_ERR_HIP, "hipStreamCreate / hipEventCreate failed"));
  {
    const char* e = getenv("RSF_PEERS_AHEAD");
    g->ahead_on = !(e && e[0] == '0');
  }
  GState& s = g->s;
  const uint64_t n = c.n_loc, S = c.S;
  int rc;
#define GA(p, bytes) ((rc = dmalloc((void**)&(p), (bytes))) != 0)
  if (GA(s.clock, n * 8) || GA(s.eclock, n * 8) || GA(s.qclock, n * 8) || GA(s.emin, n * 8) || GA(s.qmin, n * 8) ||
      GA(s.digest, n * 8) || GA(s.err, n * 4) || GA(s.alive, N) || GA(s.serf_state, n) || GA(s.member_subj, n * 4) ||
      GA(s.subj_member, S * 4) || GA(s.refute_cnt, S * 4) || GA(s.refute_ltime, S * c.max_refute * 8) ||
      GA(s.view, n * c.vrow) || GA(s.q_rumor, n * 3 * c.qcap * 4) || GA(s.q_seq, n * 3 * c.qcap * 4) ||
      GA(s.q_txlen, n * 3 * c.qcap * 4) || GA(s.q_dec, n * c.qcap * 4) || GA(s.q_next_seq, n * 3 * 4) || GA(s.q_pruned, n * 4) || GA(s.q_expired, n * 4) || GA(s.eb_ltime, n * c.ebuf * 8) ||
      GA(s.eb_cnt, n * c.ebuf * 4) || GA(s.eb_keys, n * c.ebuf * c.slot_k * 8) || GA(s.qb_ltime, n * c.qbuf * 8) ||
      GA(s.qb_cnt, n * c.qbuf * 4) || GA(s.qb_ids, n * c.qbuf * c.slot_k * 4) ||
      GA(s.rumors, (size_t)cfg->max_rumors * 2 * sizeof(rsf_rumor)) ||
      GA(s.rdec, (size_t)cfg->max_rumors * 2 * 4) || GA(s.rbody, (size_t)cfg->max_rumors * 2 * 16) ||
      GA(s.p_ent, n * kPend * sizeof(GState::PendE)) || GA(s.p_cnt, n * 4))
    return fail(rc);
  if (c.deep) {  // tails, their summaries, the deferred-member list (also the checker's, 3 per member)
    for (int q = 0; q < 3; ++q)
      if (tcap_of(c, q) && (q == 0 ? GA(s.tail0, n * c.tstride0 * sizeof(uint64_t))
                                   : GA(q == 1 ? s.tail1 : s.tail2, n * tstride_of(c, q) * sizeof(uint4))))
        return fail(rc);
    if (GA(s.tsum, n * 3 * sizeof(uint4)) || GA(s.tseal, n * 3 * sizeof(uint4)) || GA(s.deep_ids, n * 5 * 4))
      return fail(rc);
  }
  g->stage_cap = n * c.fanout * c.cap_t;
  if (g->stage_cap >= 0xFFFFFFFFull) return fail(gerr("n_members x fanout x per-target records must fit 32 bits"));
  g->recv_cap = g->stage_cap + g->stage_cap / 2 + 4096;
  const uint64_t pipe = std::max(g->stage_cap, g->recv_cap);
  if (GA(g->stage_key, pipe * 4) || GA(g->stage_val, pipe * 4) || GA(g->sort_key, pipe * 4) ||
      GA(g->sort_val, pipe * 4) || GA(g->seg_start, n * 4) || GA(g->seg_end, n * 4) || GA(g->send_buf, pipe * 8) || GA(g->rec_dec, pipe * 4) ||
      GA(g->d_counters, kCtrWords * 8))
    return fail(rc);
  g->n_groups = n * c.fanout;
  if (GA(g->grp_key, g->n_groups * 4) || GA(g->grp_cnt, g->n_groups * 4) || GA(g->grp_key_s, g->n_groups * 4) ||
      GA(g->grp_id, g->n_groups * 4) || GA(g->grp_id_s, g->n_groups * 4) || GA(g->grp_slot, g->n_groups * 4) ||
      GA(g->grp_off, g->n_groups * 4) || GA(g->dec_base, g->stage_cap * 4 + 2 * kZone) ||
      GA(g->big_base, n * 4 + 2 * kZone))
    return fail(rc);
  g->stage_dec = (uint32_t*)(g->dec_base + kZone);
  g->big_ids = (uint32_t*)(g->big_base + kZone);
  if (kZone) {
    bool zok = true;
    for (char* z : {g->dec_base, g->dec_base + kZone + g->stage_cap * 4, g->big_base, g->big_base + kZone + n * 4})
      zok = zok && hipMemset(z, 0xA5, kZone) == hipSuccess;
    if (!zok) return fail(rsf::set_error(RSF_ERR_HIP, "guard zone init failed"));
  }
#undef GA
  if ((rc = resident_grids(g))) return fail(rc);
  // the hipCUB temporaries are sized per call at their first use (rsf::cub_run)
  hipStream_t st = g->stream;
  bool ok = true;
  auto ms = [&](void* p, int v, size_t b) { ok = ok && hipMemsetAsync(p, v, b, st) == hipSuccess; };
  ms(g->d_counters, 0, kCtrWords * 8);  // status flags and running totals start at zero
  // deferred members: the counts of lists 0..4 ([kCtrDeepTotal] their total)
  s.deep_n = reinterpret_cast<uint32_t*>(g->d_counters + kCtrDeepLists);
  ms(s.emin, 0, n * 8);
  ms(s.qmin, 0, n * 8);
  ms(s.digest, 0, n * 8);
  ms(s.err, 0, n * 4);
  ms(s.alive, 1, N);
  ms(s.serf_state, 0, n);
  ms(s.member_subj, 0xFF, n * 4);
  ms(s.subj_member, 0, S * 4);
  ms(s.refute_cnt, 0, S * 4);
  ms(s.refute_ltime, 0, S * c.max_refute * 8);
  ms(s.view, 0, n * c.vrow);
  ms(s.q_rumor, 0xFF, n * 3 * c.qcap * 4);
  ms(s.q_seq, 0, n * 3 * c.qcap * 4);
  ms(s.q_txlen, 0, n * 3 * c.qcap * 4);
  ms(s.q_dec, 0, n * c.qcap * 4);
  ms(s.q_next_seq, 0, n * 3 * 4);
  ms(s.q_pruned, 0, n * 4);
  ms(s.q_expired, 0, n * 4);
  ms(s.p_cnt, 0, n * 4);
  ms(s.eb_ltime, 0, n * c.ebuf * 8);
  ms(s.eb_cnt, 0, n * c.ebuf * 4);
  ms(s.eb_keys, 0, n * c.ebuf * c.slot_k * 8);
  ms(s.qb_ltime, 0, n * c.qbuf * 8);
  ms(s.qb_cnt, 0, n * c.qbuf * 4);
  ms(s.qb_ids, 0, n * c.qbuf * c.slot_k * 4);
  ms(s.rumors, 0, (size_t)cfg->max_rumors * 2 * sizeof(rsf_rumor));
  ms(s.rdec, 0, (size_t)cfg->max_rumors * 2 * 4);
  ms(s.rbody, 0, (size_t)cfg->max_rumors * 2 * 16);
  // emission's group slots and the record stage start defined (grp_index_kernel writes the
  // slot of every group with a receiver each round; a slot it did not write stays in range)
  ms(g->grp_slot, 0, g->n_groups * 4);
  ms(g->stage_val, 0, g->stage_cap * 4);
  ms(g->stage_dec, 0xFF, g->stage_cap * 4);
  if (!ok) return fail(rsf::set_error(RSF_ERR_HIP, "context initialisation failed"));
  // Serf::new increments every clock once (base.rs:195-199)
  hipLaunchKernelGGL(fill_u64_kernel, dim3(grid1(n)), dim3(256), 0, st, s.clock, n, 1ull);
  hipLaunchKernelGGL(fill_u64_kernel, dim3(grid1(n)), dim3(256), 0, st, s.eclock, n, 1ull);
  hipLaunchKernelGGL(fill_u64_kernel, dim3(grid1(n)), dim3(256), 0, st, s.qclock, n, 1ull);
  hipLaunchKernelGGL(iota_u32_kernel, dim3(grid1(g->n_groups)), dim3(256), 0, st, g->grp_id, g->n_groups);
  if (c.deep) {  // empty tails, no sealed prefix (m = 0)
    hipLaunchKernelGGL(tsum_init_kernel, dim3(grid1(n * 3)), dim3(256), 0, st, s.tsum, n * 3);
    hipLaunchKernelGGL(tsum_init_kernel, dim3(grid1(n * 3)), dim3(256), 0, st, s.tseal, n * 3);
  }
  if (hipStreamSynchronize(st) != hipSuccess) return fail(rsf::set_error(RSF_ERR_HIP, "context init sync failed"));
  *out = g;
  return RSF_OK;
}

int rsf_gossip_destroy(rsf_gossip* g) {
  if (!g) return RSF_OK;
  hipSetDevice(g->device);
  if (g->side) hipStreamSynchronize(g->side);
  if (g->stream) hipStreamSynchronize(g->stream);
  GState& s = g->s;
  void* ptrs[] = {s.clock,  s.eclock,      s.qclock,       s.emin,        s.qmin,     s.digest,     s.err,
                  s.alive,  s.serf_state,  s.member_subj,  s.subj_member, s.refute_cnt, s.refute_ltime, s.view,
                  s.q_rumor, s.q_seq,      s.q_txlen,      s.q_dec,      s.q_next_seq,  s.q_pruned, s.q_expired,  s.eb_ltime, s.eb_cnt,     s.eb_keys,
                  s.qb_ltime, s.qb_cnt,    s.qb_ids,       s.rumors,      s.rdec,       s.rbody,      g->d_ml,    g->d_acts,    g->stage_key,
                  g->stage_val, g->sort_key, g->sort_val,  g->seg_start,  g->seg_end, g->send_buf,  g->d_counters, g->rec_dec, g->pp_buf,
                  g->run_start, g->run_end, g->run_base, g->run_total, g->d_run_off,
                  g->grp_key, g->grp_cnt, g->grp_key_s, g->grp_id, g->grp_id_s,
                  g->grp_slot, g->grp_off, g->dec_base, s.dlog, s.dmeta, s.dcnt,
                  g->bkt_send, g->bkt_recv, g->d_rstart, g->d_rend, g->d_wstart, s.snap_bits, s.snap_sn,
                  s.p_ent, s.p_cnt, g->big_base, s.tail0, s.tail1, s.tail2, s.tsum, s.deep_ids,
                  s.tseal, g->qmax, g->d_act_status, g->occ_hist};
  for (void* p : ptrs)
    if (p) hipFree(p);
  g->scratch.release();
  for (int k = 0; k < 2; ++k) {
    if (g->pin[k]) hipHostFree(g->pin[k]);
    if (g->pin_ev[k]) hipEventDestroy(g->pin_ev[k]);
  }
  g->sort_tmp.release();
  g->grp_tmp.release();
  g->scan_tmp.release();
  if (g->events_made)
    for (auto& row : g->ev)
      for (auto& e : row) hipEventDestroy(e);
  if (g->own) hipStreamDestroy(g->own);
  if (g->side) hipStreamDestroy(g->side);
  if (g->ev_emitted) hipEventDestroy(g->ev_emitted);
  if (g->ev_ahead) hipEventDestroy(g->ev_ahead);
  delete g;
  return RSF_OK;
}

int rsf_gossip_set_stream(rsf_gossip* g, void* st) {
  if (!g) return gerr("null context");
  g->stream = st ? (hipStream_t)st : g->own;
  return RSF_OK;
}

int rsf_gossip_sync(rsf_gossip* g) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  if (g->ahead_launched) RSF_HIP(hipStreamSynchronize(g->side));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_subjects(rsf_gossip* g, const uint32_t* subj_member) {
  if (!g || !subj_member) return gerr("null argument");
  const GCfg& c = g->c;
  std::vector<int32_t> ms(c.n_loc, -1);
  std::vector<uint8_t> seen(c.N, 0);
  for (uint32_t s = 0; s < c.S; ++s) {
    uint32_t m = subj_member[s];
    if (m >= c.N) return gerr("subject member out of range");
    if (seen[m]++) return gerr("a member is the subject of two slots");
    if (m >= c.lo && m < c.lo + c.n_loc) ms[m - c.lo] = (int32_t)s;
  }
  g->subj_sorted.assign(subj_member, subj_member + c.S);
  std::sort(g->subj_sorted.begin(), g->subj_sorted.end());
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(g->s.subj_member, subj_member, c.S * 4, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipMemcpyAsync(g->s.member_subj, ms.data(), c.n_loc * 4, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_init_views(rsf_gossip* g, const uint8_t* kind, const uint8_t* status, const uint64_t* ltime) {
  if (!g || !kind || !status || !ltime) return gerr("null argument");
  const GCfg& c = g->c;
  for (uint32_t i = 0; i < c.S; ++i)
    if (kind[i] > RSF_KIND_KNOWN || status[i] > RSF_STATUS_FAILED) return gerr("bad view kind/status");
  RSF_HIP(hipSetDevice(g->device));
  size_t b[3] = {c.S, c.S, (size_t)c.S * 8};
  void* d[3];
  int rc = g->scratch.take(b, 3, d);
  if (rc) return rc;
  RSF_HIP(hipMemcpyAsync(d[0], kind, c.S, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipMemcpyAsync(d[1], status, c.S, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipMemcpyAsync(d[2], ltime, (size_t)c.S * 8, hipMemcpyHostToDevice, g->stream));
  hipLaunchKernelGGL(init_views_kernel, dim3(grid1(c.n_loc * c.S)), dim3(256), 0, g->stream, g->s.view, c.vrow, c.n_loc, c.S,
                     (const uint8_t*)d[0], (const uint8_t*)d[1], (const uint64_t*)d[2]);
  RSF_HIP(hipGetLastError());
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_view(rsf_gossip* g, uint64_t m, uint32_t subj, uint8_t kind, uint8_t status, uint64_t ltime) {
  if (!g) return gerr("null context");
  const GCfg& c = g->c;
  if (m < c.lo || m >= c.lo + c.n_loc || subj >= c.S) return gerr("member/subject out of range");
  if (kind > RSF_KIND_KNOWN || status > RSF_STATUS_FAILED) return gerr("bad view kind/status");
  ViewE e;
  e.ltime = ltime;
  e.meta = status | ((uint32_t)kind << 8);
  e.t = 0;
  ViewS v;
  v = e;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(vent(g->s, c, m - c.lo, subj), &v, sizeof(v), hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_alive(rsf_gossip* g, const uint8_t* alive) {
  if (!g || !alive) return gerr("null argument");
  RSF_HIP(hipSetDevice(g->device));
  int rc = ahead_drop(g);  // liveness changes: peers drawn ahead are stale
  if (rc) return rc;
  RSF_HIP(hipMemcpyAsync(g->s.alive, alive, g->c.N, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

static int set_u64(rsf_gossip* g, uint64_t* dst, uint64_t v) {
  RSF_HIP(hipMemcpyAsync(dst, &v, 8, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_clocks(rsf_gossip* g, uint64_t m, uint64_t clock, uint64_t ec, uint64_t qc) {
  if (!g) return gerr("null context");
  if (m < g->c.lo || m >= g->c.lo + g->c.n_loc) return gerr("member out of shard");
  uint64_t l = m - g->c.lo;
  RSF_HIP(hipSetDevice(g->device));
  int rc;
  if ((rc = set_u64(g, g->s.clock + l, clock)) || (rc = set_u64(g, g->s.eclock + l, ec)) ||
      (rc = set_u64(g, g->s.qclock + l, qc)))
    return rc;
  return RSF_OK;
}

int rsf_gossip_set_min_times(rsf_gossip* g, uint64_t m, uint64_t emin, uint64_t qmin) {
  if (!g) return gerr("null context");
  if (m < g->c.lo || m >= g->c.lo + g->c.n_loc) return gerr("member out of shard");
  uint64_t l = m - g->c.lo;
  RSF_HIP(hipSetDevice(g->device));
  int rc;
  if ((rc = set_u64(g, g->s.emin + l, emin)) || (rc = set_u64(g, g->s.qmin + l, qmin))) return rc;
  return RSF_OK;
}

int rsf_gossip_set_serf_state(rsf_gossip* g, uint64_t m, uint8_t state) {
  if (!g) return gerr("null context");
  if (m < g->c.lo || m >= g->c.lo + g->c.n_loc || state > 3) return gerr("bad member/state");
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(g->s.serf_state + (m - g->c.lo), &state, 1, hipMemcpyHostToDevice, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_set_checker(rsf_gossip* g, uint32_t max_queue_depth, uint32_t min_queue_depth, uint32_t depth_warning,
                           uint32_t period) {
  if (!g) return gerr("null context");
  RSF_HIP(hipSetDevice(g->device));
  g->chk_period = period;
  g->chk_max = max_queue_depth;
  g->chk_min = min_queue_depth;
  g->chk_warn = depth_warning;
  return rsf_gossip_checker_stats(g, nullptr, nullptr, nullptr, 1);
}

}  // extern "C"
