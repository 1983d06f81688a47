// gossip_state.hip — member state changed outside the round: the direct-handler batch
// (apply_batch) and the reaper.  (Push/pull is in gossip.hip: pp_merge_kernel refutes through
// push_refute, whose range guard writes the round unit's diagnostics global.)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "gossip_ctx.h"
#include "gossip_queue4.h"

namespace {

// ---- Reaper (M8; core/src/serf/base.rs:519-601, 1782-1784).  One wave per live
// member, lanes over subject slots (16-B coalesced view reads).  Pass 1 erases
// failed members past reconnect_timeout and intents past recent_intent_timeout
// and digests the failed reaps in slot order; pass 2 (only where a left member
// is due) erases left members past tombstone_timeout and digests them, so every
// failed Reap event precedes every left one, as reap_failed precedes reap_left.
__global__ void __launch_bounds__(256) reap_kernel(GCfg c, GState s, uint32_t now, uint32_t rc_to, uint32_t ts_to,
                                                   uint32_t in_to) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t l = (uint64_t)blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (l >= c.n_loc) return;
  if (!s.alive[c.lo + l]) return;
  ViewS* vrow = vrow_of(s, c, l);
  uint64_t dig = s.digest[l];
  const uint64_t d0 = dig;
  uint32_t lerr = 0;  // delivery-log overflow
  bool any_left = false;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && !any_left) break;
    for (uint32_t base = 0; base < c.S; base += kWave) {
      const uint32_t subj = base + lane;
      ViewE v{};
      if (subj < c.S) v = *view_at(vrow, subj);
      // (stamps are kept mod 2^27: the age is exact below 2^27 rounds)
      const uint32_t kind = vkind(v.meta), st = vstatus(v.meta), age = (now - v.t) & kViewTMask;
      const bool known = subj < c.S && kind == RSF_KIND_KNOWN;
      const bool failed = known && st == RSF_STATUS_FAILED && age > rc_to;   // leave_time.elapsed() > timeout
      const bool left = known && st == RSF_STATUS_LEFT && age > ts_to;
      const bool intent = subj < c.S && (kind == RSF_KIND_INTENT_JOIN || kind == RSF_KIND_INTENT_LEAVE) && age > in_to;
      const bool reap = pass == 0 ? failed : left;
      if (reap || (pass == 0 && intent)) *view_at(vrow, subj) = ViewE{0ull, 0u, 0u};  // erase_node / reap_intents
      if (pass == 0) any_left = any_left || ballot(left) != 0;
      uint64_t mm = ballot(reap);
      while (mm) {  // Reap member events, slot order
        const int i = __ffsll((long long)mm) - 1;
        mm &= mm - 1;
        dig = digest_mix(dig, kDigMember | ((uint64_t)kEvReap << 32) | (base + (uint32_t)i));
        if (lane == 0) mlog_put(c, s, l, lerr, kEvReap, base + (uint32_t)i);
      }
    }
  }
  if (lane == 0 && dig != d0) s.digest[l] = dig;
  if (lane == 0 && lerr) s.err[l] |= lerr;
}

// direct-handler batch: one thread per receiver segment (array order within a receiver)
__global__ void __launch_bounds__(256) apply_kernel(GCfg c, GState s, const rsf_msg* __restrict__ msgs,
                                                    const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ seg_start,
                                                    const uint32_t* __restrict__ seg_end, int32_t* __restrict__ flags,
                                                    uint64_t* __restrict__ refute) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= c.n_loc) return;
  uint32_t st = seg_start[l], en = seg_end[l];
  if (st >= en) return;
  MRegs r;
  load_regs(s, l, r);
  ViewS* vrow = vrow_of(s, c, l);
  for (uint32_t i = st; i < en; ++i) {
    uint32_t k = order[i];
    rsf_msg x = msgs[k];
    uint64_t ref = 0;
    int f = 0;
    switch (x.type) {
      case RSF_MSG_JOIN: f = h_join_intent(view_at(vrow, x.subject), r, x.ltime, c.now); break;
      case RSF_MSG_LEAVE:
        f = h_leave_intent(view_at(vrow, x.subject), r, x.subject, x.ltime, x.flags & 1, ref, c.now);
        mlog_intent(c, s, l, r.err, f, x.subject);
        break;
      case RSF_MSG_USER_EVENT: f = h_user_event(c, s, l, r, x.ltime, x.key, x.flags & 1); break;
      case RSF_MSG_QUERY: f = h_query(c, s, l, r, x.ltime, (uint32_t)x.key, x.flags & 1); break;
      default: f = 0; break;
    }
    flags[k] = f;
    refute[k] = ref;
  }
  store_regs(s, l, r);
}

__global__ void keys_from_msgs_kernel(const rsf_msg* __restrict__ msgs, uint64_t n, uint64_t lo,
                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = (uint32_t)(msgs[i].receiver - lo);
  idx[i] = (uint32_t)i;
}

}  // namespace

extern "C" {

int rsf_gossip_apply_batch(rsf_gossip* g, const rsf_msg* msgs, uint64_t n, int32_t* flags_out, uint64_t* refute_out) {
  if (!g || (n && (!msgs || !flags_out))) return gerr("null argument");
  if (n == 0) return RSF_OK;
  const GCfg& c = g->c;
  if (n > 0xFFFFFFFFull) return gerr("batch too large");
  for (uint64_t i = 0; i < n; ++i) {
    if (msgs[i].receiver < c.lo || msgs[i].receiver >= c.lo + c.n_loc) return gerr("receiver outside shard");
    uint8_t t = msgs[i].type;
    if (t != RSF_MSG_JOIN && t != RSF_MSG_LEAVE && t != RSF_MSG_USER_EVENT && t != RSF_MSG_QUERY)
      return gerr("unsupported message type");
    if ((t == RSF_MSG_JOIN || t == RSF_MSG_LEAVE) && msgs[i].subject >= c.S) return gerr("subject out of range");
  }
  RSF_HIP(hipSetDevice(g->device));
  size_t b[7] = {n * sizeof(rsf_msg), n * 4, n * 4, n * 4, n * 4, n * 4, n * 8};
  void* d[7];
  int rc = g->scratch.take(b, 7, d);
  if (rc) return rc;
  size_t tmp = 0;
  RSF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (uint32_t*)d[1], (uint32_t*)d[2], (uint32_t*)d[3],
                                             (uint32_t*)d[4], (int)n, 0, bits_for(c.n_loc), g->stream));
  void* tmpbuf;
  if ((rc = g->scratch.take_extra(tmp, &tmpbuf))) return rc;
  RSF_HIP(hipMemcpyAsync(d[0], msgs, n * sizeof(rsf_msg), hipMemcpyHostToDevice, g->stream));
  hipLaunchKernelGGL(keys_from_msgs_kernel, dim3(grid1(n)), dim3(256), 0, g->stream, (const rsf_msg*)d[0], n, c.lo,
                     (uint32_t*)d[1], (uint32_t*)d[3]);
  RSF_HIP(hipcub::DeviceRadixSort::SortPairs(tmpbuf, tmp, (uint32_t*)d[1], (uint32_t*)d[2], (uint32_t*)d[3],
                                             (uint32_t*)d[4], (int)n, 0, bits_for(c.n_loc), g->stream));
  if ((rc = segment_bounds(g, (const uint32_t*)d[2], n, 0ull, nullptr, nullptr, nullptr, 0u))) return rc;
  hipLaunchKernelGGL(apply_kernel, dim3(grid1(c.n_loc)), dim3(256), 0, g->stream, c, g->s, (const rsf_msg*)d[0],
                     (const uint32_t*)d[4], g->seg_start, g->seg_end, (int32_t*)d[5], (uint64_t*)d[6]);
  RSF_HIP(hipGetLastError());
  RSF_HIP(hipMemcpyAsync(flags_out, d[5], n * 4, hipMemcpyDeviceToHost, g->stream));
  if (refute_out) RSF_HIP(hipMemcpyAsync(refute_out, d[6], n * 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}

int rsf_gossip_reap(rsf_gossip* g, uint32_t now, uint32_t reconnect_timeout, uint32_t tombstone_timeout,
                    uint32_t recent_intent_timeout) {
  if (!g) return gerr("null context");
  const GCfg& c = g->c;
  RSF_HIP(hipSetDevice(g->device));
  hipLaunchKernelGGL(reap_kernel, dim3(grid1(c.n_loc, kWavesPerBlock)), dim3(kWave * kWavesPerBlock), 0, g->stream, c,
                     g->s, now, reconnect_timeout, tombstone_timeout, recent_intent_timeout);
  RSF_HIP(hipGetLastError());
  return RSF_OK;
}

int rsf_gossip_set_now(rsf_gossip* g, uint32_t now) {
  if (!g) return gerr("null context");
  g->c.now = now;
  return RSF_OK;
}

}  // extern "C"
