// gossip.hip — the batched gossip round on CDNA4 (gfx950): Lamport-clock
// member-state merge + retransmit-limited dissemination.
//
// One round (see DESIGN.md "Round model"):
//   ml_kernel        memberlist transitions at every live member (handle_node_join/leave)
//   refute_kernel    broadcast_join for refutations spawned last round (base.rs:1437-1447)
//   originate_kernel api entry points: join/leave/force_leave/user_event/query
//   emit_kernel      ONE WAVE PER SENDER: the three queues live in registers (lane = queue slot);
//                    k distinct live peers (Philox); per peer broadcast_messages drains
//                    intent -> query -> event under the byte budget with wave argmin
//                    selection (TransmitLimitedQueue::get_broadcasts model)
//   radix sort       stable by receiver (hipCUB onesweep) -> canonical (sender, position) order
//   segment_kernel   receiver segment bounds in the sorted record stream
//   merge_kernel     ONE WAVE PER RECEIVER: lane 0 runs the handlers in canonical order, the
//                    wave re-queues rebroadcasts (ballot for a free slot / wave max for the prune)
//
// This unit holds the round itself: its kernels, the QueueChecker (whose deep prune shares the
// deep emission's code) and, because __device__ globals are per translation unit, every kernel
// that writes the diagnostics globals together with their readers (gossip_diag.h) -- which puts
// push/pull here too (pp_merge_kernel refutes through push_refute and its range guard).  The
// rest of the engine is in gossip_ctx / gossip_exchange / gossip_state / gossip_dump /
// gossip_snapshot (.hip); gossip_ctx.h maps them.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gossip_ctx.h"
#include "gossip_diag.h"
#include "gossip_deep.h"
#include "gossip_merge.h"
#include "gossip_queue4.h"

namespace {

// every member's pending re-queues applied (before anything but emission reads the queues)
__global__ void __launch_bounds__(256) pend_flush_kernel(GCfg c, GState s, uint32_t period, uint32_t phase) {
  __shared__ QLds4 rows[kWavesPerBlock];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t l = phase_first(c, period, phase) +
                     ((uint64_t)blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)) *
                         period;
  if (l >= c.n_loc) return;
  const uint32_t pc = s.p_cnt[l];
  if (!pc) return;
  if (pend_flush_any(c, s, l, lane, pc, rows[threadIdx.x / kWave]) && lane == 0) s.err[l] |= kErrQueue;
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(256) ml_kernel(GCfg c, GState s, const rsf_ml_event* __restrict__ ml,
                                                 uint32_t n_ml) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= c.n_loc) return;
  const uint32_t m = (uint32_t)(c.lo + l);
  bool al = s.alive[m] != 0;
  MRegs r;
  load_regs(s, l, r);
  bool touched = false;
  for (uint32_t e = 0; e < n_ml; ++e) {
    uint32_t subj = ml[e].subject, sm = s.subj_member[subj];
    if (sm == m && ml[e].set_alive == 1) {
      al = true;
      r.serf_state = kSerfAlive;
      touched = true;
    }
    if (al && m != sm) {
      ViewS* v = vent(s, c, l, subj);
      if (ml[e].kind == RSF_ML_JOIN) {
        h_node_join(v, r, subj);
        snap_member(c, s, l, subj, true);
        mlog_put(c, s, l, r.err, kEvJoin, subj);
      } else if (ml[e].kind == RSF_ML_UPDATE) {
        if (h_node_update(v, r, subj)) mlog_put(c, s, l, r.err, kEvUpdate, subj);
      } else {
        const int f = h_node_leave(v, r, subj, c.now);
        if (f & RSF_F_MEMBER_EVENT) {
          snap_member(c, s, l, subj, false);
          mlog_put(c, s, l, r.err, (uint32_t)f >> kFEvShift, subj);
        }
      }
      touched = true;
    }
    if (sm == m && ml[e].set_alive == 0) al = false;
  }
  if (touched) store_regs(s, l, r);
  s.alive[m] = al ? 1 : 0;
}

// liveness of every member (replicated array): last set_alive per subject wins
__global__ void ml_alive_kernel(GState s, const rsf_ml_event* __restrict__ ml, uint32_t n_ml) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint32_t e = 0; e < n_ml; ++e) {
    uint32_t sm = s.subj_member[ml[e].subject];
    if (ml[e].set_alive == 1) s.alive[sm] = 1;
    if (ml[e].set_alive == 0) s.alive[sm] = 0;
  }
}

__device__ __forceinline__ void put_rumor(const GCfg& c, const GState& s, uint32_t rid, uint8_t type, uint8_t flags, uint32_t subj,
                                          uint64_t L, uint64_t key, uint32_t len) {
  rsf_rumor ru;
  ru.ltime = L;
  ru.key = key;
  ru.subject = subj;
  ru.type = type;
  ru.flags = flags;
  ru.msg_len = (uint16_t)len;
  s.rumors[rid & c.rmask] = ru;
}

// broadcast_join (base.rs:396-412)
__device__ __forceinline__ void broadcast_join(const GCfg& c, const GState& s, uint64_t l, MRegs& r, uint64_t L,
                                               uint32_t rid) {
  uint32_t subj = (uint32_t)r.subj;
  witness(r.clock, L);
  h_join_intent(vent(s, c, l, subj), r, L, c.now);
  uint32_t len = msg_len(RSF_MSG_JOIN, L, 0, 0);
  put_rumor(c, s, rid, RSF_MSG_JOIN, 0, subj, L, 0, len);
  pend_push_serial(c, s, l, kQIntent, rid, subj, len, r);
}

__global__ void __launch_bounds__(256) refute_kernel(GCfg c, GState s, uint32_t base) {
  uint32_t subj = blockIdx.x * blockDim.x + threadIdx.x;
  if (subj >= c.S) return;
  uint32_t m = s.subj_member[subj];
  if (m < c.lo || m >= c.lo + c.n_loc) return;
  uint32_t cnt = s.refute_cnt[subj];
  if (!cnt) return;
  s.refute_cnt[subj] = 0;
  if (!s.alive[m]) return;
  uint64_t l = m - c.lo;
  MRegs r;
  load_regs(s, l, r);
  for (uint32_t i = 0; i < cnt; ++i)
    broadcast_join(c, s, l, r, s.refute_ltime[(uint64_t)subj * c.max_refute + i], base + subj * c.max_refute + i);
  store_regs(s, l, r);
}

// status[a] = the entry point's result (rsf_gossip_action_status): RSF_OK, RSF_SKIPPED (not
// this shard's member, or its process is down), or a size-limit error, in which case the
// action does nothing at all (the reference returns before any clock or queue moves).
__global__ void __launch_bounds__(256) originate_kernel(GCfg c, GState s, const rsf_action* __restrict__ acts,
                                                        uint32_t n_acts, uint32_t abase, int32_t* __restrict__ status) {
  uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_acts) return;
  rsf_action x = acts[a];
  uint32_t m = x.member;
  if (m < c.lo || m >= c.lo + c.n_loc || !s.alive[m]) {
    status[a] = RSF_SKIPPED;
    return;
  }
  uint64_t l = m - c.lo;
  uint32_t rid = abase + a;
  if (x.act == RSF_ACT_USER_EVENT || x.act == RSF_ACT_QUERY) {
    const int32_t e = x.act == RSF_ACT_USER_EVENT
                          ? user_event_size_check(c.max_ue, s.eclock[l], x.name_len, x.payload_len)
                          : query_size_check(c.query_limit, s.qclock[l], x.name_len, x.payload_len);
    if (e) {
      status[a] = e;
      return;
    }
  }
  MRegs r;
  load_regs(s, l, r);
  // join / leave of the member itself: only a tracked subject has a view entry about itself
  // (rsf_gossip_round_begin rejects the call on the host; this keeps the status truthful)
  if ((x.act == RSF_ACT_JOIN_SELF || x.act == RSF_ACT_LEAVE_SELF) && (uint32_t)r.subj >= c.S) {
    status[a] = RSF_ERR_ARG;
    return;
  }
  status[a] = RSF_OK;
  uint64_t ref = 0;
  switch (x.act) {
    case RSF_ACT_JOIN_SELF:
      r.serf_state = kSerfAlive;
      broadcast_join(c, s, l, r, r.clock, rid);
      break;
    case RSF_ACT_LEAVE_SELF: {
      r.serf_state = kSerfLeaving;
      uint64_t lt = r.clock;
      if (s.snap_sn && !(s.snap_sn[l * 4 + 3] & 1)) {
        // Snapshot::leave (snapshot.rs:568-586): the clock ticker's last value, then the
        // alive set is dropped (unless rejoin_after_leave) and recording stops
        s.snap_sn[l * 4 + 2] = lt ? lt - 1 : 0;
        s.snap_sn[l * 4 + 3] |= 1;
        if (!c.snap_rejoin)
          for (uint32_t k = 0; k < c.snap_w; ++k) s.snap_bits[l * c.snap_w + k] = 0;
      }
      r.clock++;
      uint32_t subj = (uint32_t)r.subj;
      mlog_intent(c, s, l, r.err, h_leave_intent(vent(s, c, l, subj), r, subj, lt, false, ref, c.now), subj);
      uint32_t len = msg_len(RSF_MSG_LEAVE, lt, 0, 0);
      put_rumor(c, s, rid, RSF_MSG_LEAVE, 0, subj, lt, 0, len);
      pend_push_serial(c, s, l, kQIntent, rid, subj, len, r);
      break;
    }
    case RSF_ACT_FORCE_LEAVE: {
      uint64_t lt = r.clock;
      bool prune = x.flags & 1;
      int f = h_leave_intent(vent(s, c, l, x.subject), r, x.subject, lt, prune, ref, c.now);
      mlog_intent(c, s, l, r.err, f, x.subject);
      if (f & RSF_F_REFUTE) push_refute(c, s, r, ref);
      uint32_t len = msg_len(RSF_MSG_LEAVE, lt, 0, 0);
      put_rumor(c, s, rid, RSF_MSG_LEAVE, prune ? 1 : 0, x.subject, lt, 0, len);
      pend_push_serial(c, s, l, kQIntent, rid, x.subject, len, r);
      break;
    }
    case RSF_ACT_USER_EVENT: {
      uint64_t lt = r.eclock;
      r.eclock++;
      const bool cc = x.flags & 1;
      h_user_event(c, s, l, r, lt, x.key, cc);
      uint32_t len = msg_len(RSF_MSG_USER_EVENT, lt, x.name_len, x.payload_len);
      put_rumor(c, s, rid, RSF_MSG_USER_EVENT, cc ? 1 : 0, 0, lt, x.key, len);
      pend_push_serial(c, s, l, kQEvent, rid, kDecEvent, len, r);
      break;
    }
    case RSF_ACT_QUERY: {
      uint64_t lt = r.qclock;
      bool nb = x.flags & 1;
      h_query(c, s, l, r, lt, (uint32_t)x.key, nb);
      uint32_t len = msg_len(RSF_MSG_QUERY, lt, x.name_len, x.payload_len);
      put_rumor(c, s, rid, RSF_MSG_QUERY, nb ? 1 : 0, 0, lt, (uint32_t)x.key, len);
      pend_push_serial(c, s, l, kQQuery, rid, kDecQuery, len, r);
      break;
    }
    default: break;
  }
  store_regs(s, l, r);
}

// Peer selection (memberlist kRandomNodes model): attempts a = 0,1,2,... in order, each a
// Philox draw over the other N-1 members, kept if live and not yet chosen, until `fanout`
// peers.  One thread per member; grp_key[l*fanout + j] = j-th peer (kSentinel: none, or a
// dead sender).  Sender l's records to its j-th peer form GROUP l*fanout + j.
constexpr uint32_t kPeerBatch = 4;
__global__ void __launch_bounds__(256) peers_kernel(GCfg c, GState s, uint32_t round, uint32_t* __restrict__ grp_key) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= c.n_loc) return;
  const uint32_t m = (uint32_t)(c.lo + l);
  uint32_t peers[8];
  uint32_t np = 0;
  if (s.alive[m]) {
    const uint32_t attempts = 64 * c.fanout;
    for (uint32_t a0 = 0; a0 < attempts && np < c.fanout; a0 += kPeerBatch) {
      uint32_t p[kPeerBatch];
      bool ok[kPeerBatch];
#pragma unroll
      for (uint32_t b = 0; b < kPeerBatch; ++b) {  // the batch's liveness loads go out together
        u32x4 o = philox4x32_10(a0 + b, kPurposePeer << 24, m, round, c.k0, c.k1);
        p[b] = mulhi32(o.x, (uint32_t)(c.N - 1));
        if (p[b] >= m) p[b]++;
        ok[b] = a0 + b < attempts && s.alive[p[b]] != 0;
      }
#pragma unroll
      for (uint32_t b = 0; b < kPeerBatch; ++b) {
        if (!ok[b] || np >= c.fanout) continue;
        bool dup = false;
        for (uint32_t j = 0; j < np; ++j) dup |= peers[j] == p[b];
        if (!dup) peers[np++] = p[b];
      }
    }
  }
  for (uint32_t j = 0; j < c.fanout; ++j) grp_key[l * c.fanout + j] = j < np ? peers[j] : kSentinel;
}

// After the stable sort of the groups by receiver: slot[gid] = the group's position in
// receiver order (where emit_kernel writes its records: cap_t slots per group), and, for
// a context that merges its own records, each receiver's range of groups.
// Bucket emission (wstart non-null): a group's slot word is its destination shard w (top
// kBktWBits bits) and its place in that shard's bucket (i - wstart[w]), so emission needs
// neither a division nor a dependent load of wstart.
__global__ void __launch_bounds__(256) grp_index_kernel(const uint32_t* __restrict__ key_s,
                                                        const uint32_t* __restrict__ id_s, uint64_t n, uint64_t lo,
                                                        uint32_t* __restrict__ slot, uint32_t* __restrict__ seg_start,
                                                        uint32_t* __restrict__ seg_end,
                                                        const uint32_t* __restrict__ wstart = nullptr, uint32_t per = 0,
                                                        uint32_t* __restrict__ bkt_keys = nullptr, uint64_t bstride = 0,
                                                        uint32_t gcap = 0) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = key_s[i];
  if (key == kSentinel) return;
  if (RSF_BAD(2, id_s[i] >= n, id_s[i]) || RSF_BAD(3, seg_start && key - lo >= n, key)) return;
  if (wstart) {
    const uint32_t w = key / per;
    // a place past the field (an overflowing bucket) saturates to kBktIdxMask, which is >= the
    // bucket capacity (rsf_gossip_bucket_buffers), so emission skips it instead of wrapping
    const uint64_t place = (uint64_t)i - wstart[w];
    slot[id_s[i]] = (w << kBktWShift) | (uint32_t)(place < kBktIdxMask ? place : kBktIdxMask);
    // the bucket's receiver keys, in sorted order: coalesced here instead of scattered from
    // the emission (one 4-B write per group into a random sector)
    if (place < gcap) bkt_keys[(uint64_t)w * bstride + place] = key;
    return;
  }
  slot[id_s[i]] = (uint32_t)i;
  if (seg_start) {
    if (i == 0 || key_s[i - 1] != key) seg_start[key - lo] = (uint32_t)i;
    if (i + 1 == n || key_s[i + 1] != key) seg_end[key - lo] = (uint32_t)(i + 1);
  }
}

// ONE WAVE PER SENDER: lane i owns slot i of each of its three queues.  For each peer
// (grp_key, from peers_kernel) broadcast_messages drains intent -> query -> event under
// one byte budget; the group's records (rumor id + decoration) go to cap_t slots at the
// group's sorted position, its record count to cnt_s.
// Members per wave in emit_kernel / merge_kernel: with more than one, a wave issues the
// first round trip of every member it owns before working through them, so the loads
// of the next member are in flight while the current one runs (the kernels run at the
// 8-waves/SIMD hardware cap and wait on memory half the time).
#ifndef RSF_EMIT_WPB
#define RSF_EMIT_WPB 1  // waves per emit_kernel block (1 measured ~1% faster than 2 or 4; 16: +8%)
#endif
#ifndef RSF_EMIT_PER_WAVE
#define RSF_EMIT_PER_WAVE 1  // emit: 2, 8 and 16 per wave measured slower
#endif
#ifndef RSF_MERGE_PER_WAVE
#define RSF_MERGE_PER_WAVE 8  // merge: 8 receivers per wave measured fastest (4.30 -> 4.06 ms at 2M; 2, 4, 16, 32 between)
#endif


// a sender's first round trip: the intent queue (the common case; a sorted queue is
// empty iff its slot 0 is free), the peers and their group slots, and one lane-distributed
// word per lane (`head`): lanes 1, 2 the query / event queue heads, kEhPend the pending
// re-queue counts, kEhSeq + q the queues' next insertion seqs, kEhPruned, kEhErr
enum : uint32_t { kEhPend = 3, kEhSeq = 4, kEhPruned = 7, kEhErr = 8 };
struct EmitIn {
  QRegs Q0;
  uint32_t head, gk, gs;
  uint4 ts;  // deep queues: lane q < 3 holds queue q's tail summary (tsum)
};
template <uint32_t DEEP = 0>
__device__ __forceinline__ void emit_load(const GCfg& c, const GState& s, const uint32_t* __restrict__ grp_key,
                                          const uint32_t* __restrict__ slot, uint64_t l, uint32_t lane, EmitIn& e) {
  e.Q0 = QRegs{kEmpty, 0, 0};
  e.head = kEmpty;
  e.gk = kSentinel;
  e.gs = 0;
  e.ts = kTSumEmpty;
  if (l >= c.n_loc) return;  // wave-uniform: a wave's last member may lie past the shard
  q_load(c, s, l, 0, lane, e.Q0);
  if (DEEP && lane < 3) e.ts = s.tsum[l * 3 + lane];
  const uint32_t* hp = nullptr;
  if (lane == 1 || lane == 2) hp = s.q_rumor + (l * 3 + lane) * c.qcap;
  else if (lane == kEhPend) hp = s.p_cnt + l;
  else if (lane >= kEhSeq && lane < kEhSeq + 3) hp = s.q_next_seq + l * 3 + (lane - kEhSeq);
  else if (lane == kEhPruned) hp = s.q_pruned + l;
  else if (lane == kEhErr) hp = s.err + l;
  if (hp) e.head = *hp;
  e.gk = lane < c.fanout ? grp_key[l * c.fanout + lane] : kSentinel;
  e.gs = lane < c.fanout ? slot[l * c.fanout + lane] : 0u;
}
// buckets: when nothing will be emitted, lanes < np write their group's zero count into the
// destination bucket (the groups' receiver keys are written by grp_index_kernel, in sorted order)
__device__ __forceinline__ void bkt_zero_counts(const Buckets& bk, uint32_t lane, uint32_t np, uint32_t gs) {
  if (lane >= np) return;
  const uint32_t w = gs >> kBktWShift, idx = gs & kBktIdxMask;  // pre-encoded by grp_index_kernel
  if (idx >= bk.gcap) return;  // over the bucket capacity: flagged by the bounds kernel
  bk.send[(uint64_t)w * bk.stride_u32 + bk.cnt_off + idx] = 0u;
}
// DEEP (queues with an HBM tail): the emission runs on the heads as below; it is committed
// only if every pick was decided by the head alone (q_pick_peers' checks against the tails'
// bounds) and every spill fits its tail -- otherwise nothing is stored (records written to the
// group slots are rewritten) and the member is listed for emit_deep_wave_kernel.
// DEEP: bit q set = queue q may have a tail (1: the intent queue only, 7: all three); the
// other queues' tail code is compiled away
template <bool BKT, uint32_t DEEP = 0>
__device__ __forceinline__ void emit_run(const GCfg& c, const GState& s, uint64_t l, uint32_t lane, EmitIn& e,
                                         uint32_t* __restrict__ cnt_s, uint32_t* __restrict__ out_val,
                                         uint32_t* __restrict__ out_dec, const Buckets& bk, QLds& row) {
#if RSF_EMIT_PROF
  uint64_t ep_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t g_eprof_sub[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // inside q_pick_peers (intent queue)
#endif
  EPROF_T(t0);
  QRegs& Q0 = e.Q0;
  QRegs Q1{kEmpty, 0, 0, kDecQuery}, Q2{kEmpty, 0, 0, kDecEvent};
  const uint64_t pm = ballot(e.gk != kSentinel);  // peers are a prefix of the fanout slots
  const uint32_t np = (uint32_t)__popcll(pm);
  const uint32_t pc = shfl_u32(e.head, kEhPend), npend = pend_total(pc);
  if (RSF_BAD2(8, npend > kPend || ((pc >> 24) != 0), pc)) return;
  // deep queues: a queue is non-empty if its tail holds items too
  constexpr bool D0 = DEEP & 1, D1 = DEEP & 2, D2 = DEEP & 4;
  const uint32_t tc0 = D0 ? shfl_u32(e.ts.x, 0) : 0u, tc1 = D1 ? shfl_u32(e.ts.x, 1) : 0u,
                 tc2 = D2 ? shfl_u32(e.ts.x, 2) : 0u;
  const bool ne0 = shfl_u32(Q0.r, 0) != kEmpty || (pc & 0xFF) || tc0,
             ne1 = shfl_u32(e.head, 1) != kEmpty || ((pc >> 8) & 0xFF) || tc1,
             ne2 = shfl_u32(e.head, 2) != kEmpty || ((pc >> 16) & 0xFF) || tc2;
  // no peers: nothing is sent, and the pending re-queues wait for the next emission
  if (np == 0 || !(ne0 || ne1 || ne2)) {
    if (BKT) bkt_zero_counts(bk, lane, np, e.gs);
    return;
  }
  // (three named tails, not an array: a dynamically indexed array goes to scratch)
  Spill sp0, sp1, sp2;
  bool unsafe = false;
  if (DEEP) {
    auto get = [&](Spill& x, uint32_t q) {
      spill_row(c, s, l, q, x);
      x.cnt = shfl_u32(e.ts.x, q);
      x.minlen = shfl_u32(e.ts.y, q);
      x.minkey = ((uint64_t)shfl_u32(e.ts.w, q) << 32) | shfl_u32(e.ts.z, q);
    };
    if (D0 && c.tcap0) get(sp0, 0);
    if (D1 && c.tcap1) get(sp1, 1);
    if (D2 && c.tcap2) get(sp2, 2);
  }
  EPROF_T(t1);
  EPROF_ADD(0, t0, t1);
  bool d0 = false, d1 = false, d2 = false;
  uint32_t err = 0;
  // the pending re-queues (merge_kernel's and the originations' since the last emission)
  PendRegs pr;
  pend_load(s, l, lane, npend, pr);
  // buckets: each peer's destination shard (the slot word holds the shard and the bucket place)
  uint32_t wdst = 0;
  if (BKT && lane < np) wdst = e.gs >> kBktWShift;
  if (ne1) q_load(c, s, l, 1, lane, Q1);
  if (ne2) q_load(c, s, l, 2, lane, Q2);
#if RSF_EMIT_PROF
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // diagnostic split: round trip 2 vs the apply
  EPROF_T(t1b);
  EPROF_ADD(1, t1, t1b);
#endif
  uint32_t drops_all = 0;
  if (npend) {
    // applied first: in the reference they were queued when the messages arrived
    uint32_t& drops = drops_all;
    if (pc & 0xFF) {
      if (D0 && c.tcap0) pend_apply<true, true>(c, Q0, lane, 0, npend, pr, shfl_u32(e.head, kEhSeq), row, &sp0);
      else drops += pend_apply<true>(c, Q0, lane, 0, npend, pr, shfl_u32(e.head, kEhSeq), row);
      d0 = true;
    }
    if ((pc >> 8) & 0xFF) {
      if (D1 && c.tcap1) pend_apply<false, true>(c, Q1, lane, 1, npend, pr, shfl_u32(e.head, kEhSeq + 1), row, &sp1);
      else drops += pend_apply<false>(c, Q1, lane, 1, npend, pr, shfl_u32(e.head, kEhSeq + 1), row);
      d1 = true;
    }
    if ((pc >> 16) & 0xFF) {
      if (D2 && c.tcap2) pend_apply<false, true>(c, Q2, lane, 2, npend, pr, shfl_u32(e.head, kEhSeq + 2), row, &sp2);
      else drops += pend_apply<false>(c, Q2, lane, 2, npend, pr, shfl_u32(e.head, kEhSeq + 2), row);
      d2 = true;
    }
    if (drops) err |= kErrQueue;
    // a tail past its capacity needs the bounded queue's exact prune over head and tail
    if (DEEP) unsafe = (D0 && sp0.cnt > c.tcap0) || (D1 && sp1.cnt > c.tcap1) || (D2 && sp2.cnt > c.tcap2);
    if (DEEP && unsafe) RSF_DEEP_WHY(6);
    // (the list's bookkeeping -- count, next seqs, prune count -- is written at the end: a store
    // here would make the compiler wait for it before reusing its registers)
  }
  EPROF_T(t2);
#if RSF_EMIT_PROF
  EPROF_ADD(2, t1b, t2);
#endif
  {
    // queue-major: every peer's picks from the intent queue, then the query queue, then the
    // event queue (q_pick_peers).  Lane j < np holds peer j's group: where its records go
    // (off: element offset from the output base) and where its count goes (oc).
    if (RSF_BAD2_W(7, !BKT && lane < np && e.gs >= c.n_loc * c.fanout, e.gs)) return;
    uint64_t off = ~0ull;
    uint32_t* ov = out_val;
    uint32_t* od = out_dec;
    uint32_t* oc = nullptr;
    if (lane < np) {
      if (BKT) {
        const uint32_t idx = e.gs & kBktIdxMask;
        if (idx < bk.gcap) {
          off = (uint64_t)wdst * bk.stride_u32 + bk.vals_off + (uint64_t)idx * c.cap_t;
          oc = bk.send + (uint64_t)wdst * bk.stride_u32 + bk.cnt_off + idx;
        }
      } else {
        off = (uint64_t)e.gs * c.cap_t;
        oc = cnt_s + e.gs;
      }
    }
    if (BKT) {
      ov = bk.send;
      od = bk.send + (bk.decs_off - bk.vals_off);  // (off addresses the vals: the decs sit a fixed distance on)
    }
    uint32_t used_v = 0, nrec_v = 0;
#if RSF_EMIT_PROF
    uint64_t* const ep = g_eprof_sub;
#else
    uint64_t* const ep = nullptr;
#endif
    if (DEEP) {
      // a tail's bounds (~0: empty) as of after the spills above
#define RSF_TB(q) (sp##q.cnt ? sp##q.minkey : ~0ull), (sp##q.cnt ? sp##q.minlen : ~0u)
      if (ne0 && !unsafe) {
        if (D0) q_pick_peers<true, true>(c, Q0, lane, np, used_v, nrec_v, off, ov, od, err, d0, row, ep, RSF_TB(0), &unsafe);
        else q_pick_peers<true>(c, Q0, lane, np, used_v, nrec_v, off, ov, od, err, d0, row, ep);
      }
      if (ne1 && !unsafe) {
        if (D1) q_pick_peers<false, true>(c, Q1, lane, np, used_v, nrec_v, off, ov, od, err, d1, row, nullptr, RSF_TB(1), &unsafe);
        else q_pick_peers<false>(c, Q1, lane, np, used_v, nrec_v, off, ov, od, err, d1, row);
      }
      if (ne2 && !unsafe) {
        if (D2) q_pick_peers<false, true>(c, Q2, lane, np, used_v, nrec_v, off, ov, od, err, d2, row, nullptr, RSF_TB(2), &unsafe);
        else q_pick_peers<false>(c, Q2, lane, np, used_v, nrec_v, off, ov, od, err, d2, row);
      }
#undef RSF_TB
      if (unsafe) {  // nothing committed: the whole-queue path redoes this member's emission
        // by the LDS capacity its largest queue needs: list 2 (kDeepTiny; from n_loc), list 0
        // (kDeepSmall; from the front), list 3 (kDeepMid; from 3 n_loc), list 1 (the full depth;
        // from 3 n_loc - 1 down)
        uint32_t need = c.qcap + max(max(tc0 + (pc & 0xFF), tc1 + ((pc >> 8) & 0xFF)), tc2 + ((pc >> 16) & 0xFF));
        // only the intent queue in use with a sealed tail prefix: the deferred path reads the
        // tail's recent part only (deep_wave_member's recent mode; it re-lists the member for the
        // full depth if that cannot decide)
        if (D0 && c.tcap0 && !ne1 && !ne2 && tc0 + (pc & 0xFF) <= c.tcap0) {
          const uint32_t m0 = s.tseal[l * 3].x;
          if (m0 && m0 <= tc0) need = c.qcap + (tc0 - m0) + (pc & 0xFF);
        }
        if (lane == 0) {
          if (need <= kDeepTiny) s.deep_ids[c.n_loc + atomicAdd(s.deep_n + 2, 1u)] = (uint32_t)l;
          else if (need <= kDeepSmall) s.deep_ids[atomicAdd(s.deep_n, 1u)] = (uint32_t)l;
          else if (need <= kDeepMid) s.deep_ids[c.n_loc * 3 + atomicAdd(s.deep_n + 3, 1u)] = (uint32_t)l;
          else s.deep_ids[c.n_loc * 3 - 1 - atomicAdd(s.deep_n + 1, 1u)] = (uint32_t)l;
        }
        return;
      }
    } else {
      if (ne0) q_pick_peers<true>(c, Q0, lane, np, used_v, nrec_v, off, ov, od, err, d0, row, ep);
      if (ne1) q_pick_peers<false>(c, Q1, lane, np, used_v, nrec_v, off, ov, od, err, d1, row);
      if (ne2) q_pick_peers<false>(c, Q2, lane, np, used_v, nrec_v, off, ov, od, err, d2, row);
    }
    if (oc && (BKT || nrec_v)) *oc = min(nrec_v, c.cap_t);  // buckets: every group's count
  }
  EPROF_T(t2b);
  EPROF_ADD(3, t2, t2b);
  EPROF_T(t3);
  EPROF_ADD(4, t2b, t3);
  if (d0) q_store(c, s, l, 0, lane, Q0, true);
  if (d1) q_store(c, s, l, 1, lane, Q1, true);
  if (d2) q_store(c, s, l, 2, lane, Q2, true);
  if (DEEP) {  // the tails' new counts and bounds (their spilled items are written), lane q for queue q
    const bool l0 = lane == 0, l1 = lane == 1;
    const uint32_t tc = l0 ? tc0 : l1 ? tc1 : tc2;
    const uint32_t tcap = l0 ? (D0 ? c.tcap0 : 0u) : l1 ? (D1 ? c.tcap1 : 0u) : (D2 ? c.tcap2 : 0u);
    const uint32_t cnt = l0 ? sp0.cnt : l1 ? sp1.cnt : sp2.cnt, mlen = l0 ? sp0.minlen : l1 ? sp1.minlen : sp2.minlen;
    const uint64_t mkey = l0 ? sp0.minkey : l1 ? sp1.minkey : sp2.minkey;
    if (lane < 3 && tcap && cnt != tc) s.tsum[l * 3 + lane] = make_uint4(cnt, mlen, (uint32_t)mkey, (uint32_t)(mkey >> 32));
  }
  // the member's bookkeeping as ONE lane-distributed store (each lane of `head` writes its own
  // word back where it changed): the applied pending list's count (0) and the queues' next
  // seqs, the prune count, the error flags (a queue prune, a stage overflow; only when new)
  {
    const uint32_t qi = lane - kEhSeq;
    const uint32_t nq = qi < 3 ? (pc >> (8 * qi)) & 0xFF : 0u;
    const bool w_pend = npend && lane == kEhPend, w_seq = npend && nq != 0;
    const bool w_pr = drops_all && lane == kEhPruned, w_err = lane == kEhErr && (err & ~e.head);
    uint32_t* const base = w_pend ? s.p_cnt : w_seq ? s.q_next_seq : w_pr ? s.q_pruned : s.err;
    const uint64_t idx = w_seq ? l * 3 + qi : l;
    const uint32_t v = w_pend ? 0u : w_seq ? e.head + nq : w_pr ? e.head + drops_all : (e.head | err);
    if (w_pend || w_seq || w_pr || w_err) base[idx] = v;
  }

  EPROF_T(t4);
  EPROF_ADD(7, t3, t4);
  EPROF_ADD(5, t0, t4);
#if RSF_EMIT_PROF
  ep_acc[6] = 1;
  if (lane == 0)
    for (int i = 0; i < 8; ++i)
      if (ep_acc[i]) atomicAdd(&g_eprof[(blockIdx.x & 511) * 8 + i], (unsigned long long)ep_acc[i]);
  if (lane == 0)
    for (int i = 0; i < 5; ++i)
      if (g_eprof_sub[i]) atomicAdd(&g_eprof2[(blockIdx.x & 511) * 8 + i], (unsigned long long)g_eprof_sub[i]);
#endif
}

// emission for queues of 65..256 slots (gossip_queue4.h): emit_run's steps with four slots
// per lane; no prefetch of the next sender and no deferred re-rank
template <bool BKT>
__device__ __forceinline__ void emit_run4(const GCfg& c, const GState& s, const uint32_t* __restrict__ grp_key,
                                          const uint32_t* __restrict__ slot, uint64_t l, uint32_t lane,
                                          uint32_t* __restrict__ cnt_s, uint32_t* __restrict__ out_val,
                                          uint32_t* __restrict__ out_dec, const Buckets& bk, QLds4& row) {
  // one lane-distributed word (emit_load's `head`, lane 0 = the intent queue's slot 0)
  const uint32_t* hp = nullptr;
  if (lane < 3) hp = s.q_rumor + (l * 3 + lane) * c.qcap;
  else if (lane == kEhPend) hp = s.p_cnt + l;
  else if (lane >= kEhSeq && lane < kEhSeq + 3) hp = s.q_next_seq + l * 3 + (lane - kEhSeq);
  else if (lane == kEhPruned) hp = s.q_pruned + l;
  else if (lane == kEhErr) hp = s.err + l;
  const uint32_t head = hp ? *hp : kEmpty;
  const uint32_t gk = lane < c.fanout ? grp_key[l * c.fanout + lane] : kSentinel;
  const uint32_t gs = lane < c.fanout ? slot[l * c.fanout + lane] : 0u;
  const uint32_t np = (uint32_t)__popcll(ballot(gk != kSentinel));
  const uint32_t pc = shfl_u32(head, kEhPend), npend = pend_total(pc);
  const bool ne0 = shfl_u32(head, 0) != kEmpty || (pc & 0xFF), ne1 = shfl_u32(head, 1) != kEmpty || ((pc >> 8) & 0xFF),
             ne2 = shfl_u32(head, 2) != kEmpty || ((pc >> 16) & 0xFF);
  if (np == 0 || !(ne0 || ne1 || ne2)) {
    if (BKT) bkt_zero_counts(bk, lane, np, gs);
    return;
  }
  bool d0 = false, d1 = false, d2 = false;
  uint32_t err = 0;
  PendRegs pr;
  pend_load(s, l, lane, npend, pr);
  uint32_t wdst = 0;
  if (BKT && lane < np) wdst = gs >> kBktWShift;
  Q4 Q0, Q1, Q2;
#pragma unroll
  for (uint32_t k = 0; k < kQK; ++k) {
    Q0.r[k] = Q1.r[k] = Q2.r[k] = kEmpty;
    Q0.sq[k] = Q1.sq[k] = Q2.sq[k] = Q0.tl[k] = Q1.tl[k] = Q2.tl[k] = 0;
    Q0.dec[k] = 0;
    Q1.dec[k] = kDecQuery;
    Q2.dec[k] = kDecEvent;
  }
  if (ne0) q4_load(c, s, l, 0, lane, Q0);
  if (ne1) q4_load(c, s, l, 1, lane, Q1);
  if (ne2) q4_load(c, s, l, 2, lane, Q2);
  if (npend) {
    uint32_t drops = 0;
    if (pc & 0xFF) {
      drops += q4_pend_apply<true>(c, Q0, lane, 0, npend, pr, shfl_u32(head, kEhSeq), row);
      d0 = true;
    }
    if ((pc >> 8) & 0xFF) {
      drops += q4_pend_apply<false>(c, Q1, lane, 1, npend, pr, shfl_u32(head, kEhSeq + 1), row);
      d1 = true;
    }
    if ((pc >> 16) & 0xFF) {
      drops += q4_pend_apply<false>(c, Q2, lane, 2, npend, pr, shfl_u32(head, kEhSeq + 2), row);
      d2 = true;
    }
    if (lane == kEhPend) s.p_cnt[l] = 0;
    if (lane >= kEhSeq && lane < kEhSeq + 3) {
      const uint32_t nq = (pc >> (8 * (lane - kEhSeq))) & 0xFF;
      if (nq) s.q_next_seq[l * 3 + (lane - kEhSeq)] = head + nq;
    }
    if (drops) {
      if (lane == kEhPruned) s.q_pruned[l] = head + drops;
      err |= kErrQueue;
    }
  }
  {
    // queue-major, as emit_run: every peer's picks from each queue in one pass (q4_pick_peers)
    uint64_t off = ~0ull;
    uint32_t* ov = out_val;
    uint32_t* od = out_dec;
    uint32_t* oc = nullptr;
    if (lane < np) {
      if (BKT) {
        const uint32_t idx = gs & kBktIdxMask;
        if (idx < bk.gcap) {
          off = (uint64_t)wdst * bk.stride_u32 + bk.vals_off + (uint64_t)idx * c.cap_t;
          oc = bk.send + (uint64_t)wdst * bk.stride_u32 + bk.cnt_off + idx;
        }
      } else {
        off = (uint64_t)gs * c.cap_t;
        oc = cnt_s + gs;
      }
    }
    if (BKT) {
      ov = bk.send;
      od = bk.send + (bk.decs_off - bk.vals_off);
    }
    uint32_t used_v = 0, nrec_v = 0;
    if (ne0) q4_pick_peers<true>(c, Q0, lane, np, used_v, nrec_v, off, ov, od, err, d0, row);
    if (ne1) q4_pick_peers<false>(c, Q1, lane, np, used_v, nrec_v, off, ov, od, err, d1, row);
    if (ne2) q4_pick_peers<false>(c, Q2, lane, np, used_v, nrec_v, off, ov, od, err, d2, row);
    if (oc && (BKT || nrec_v)) *oc = min(nrec_v, c.cap_t);
  }
  if (d0) q4_store(c, s, l, 0, lane, Q0);
  if (d1) q4_store(c, s, l, 1, lane, Q1);
  if (d2) q4_store(c, s, l, 2, lane, Q2);
  if (lane == kEhErr && (err & ~head)) s.err[l] = head | err;
}

template <bool BKT>
__global__ void __launch_bounds__(64) emit4_kernel(GCfg c, GState s, const uint32_t* __restrict__ grp_key,
                                                   const uint32_t* __restrict__ slot, uint32_t* __restrict__ cnt_s,
                                                   uint32_t* __restrict__ out_val, uint32_t* __restrict__ out_dec,
                                                   Buckets bk) {
  __shared__ QLds4 row;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t l = blockIdx.x;
  if (l >= c.n_loc) return;
  emit_run4<BKT>(c, s, grp_key, slot, l, lane, cnt_s, out_val, out_dec, bk, row);
}

// FULL: queue_cap == 64 (one slot per lane of the wave), known at compile time -- every
// `lane < qcap` test and its branch fold away (the bench configuration)
#ifndef RSF_EMIT_DEEP_SGPR
#define RSF_EMIT_DEEP_SGPR 94  // SGPR cap for the deep emission: occupancy 8 instead of 7 (11 SGPRs spilled to VGPR lanes; 1.45 -> 1.40 ms at 1M, same box x2); 0: none
#endif
template <bool BKT, bool FULL, uint32_t DEEP>
__device__ __forceinline__ void emit_body(GCfg c, const GState& s, const uint32_t* __restrict__ grp_key,
                                          const uint32_t* __restrict__ slot, uint32_t* __restrict__ cnt_s,
                                          uint32_t* __restrict__ out_val, uint32_t* __restrict__ out_dec,
                                          const Buckets& bk) {
  if (FULL) c.qcap = kWave;
  __shared__ QLds rows[RSF_EMIT_WPB];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  QLds& row = rows[threadIdx.x / kWave];
  const uint64_t l = ((uint64_t)xcd_block(blockIdx.x, gridDim.x) * RSF_EMIT_WPB +
                      (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)) * RSF_EMIT_PER_WAVE;
  if (l >= c.n_loc) return;
  EmitIn cur, nxt;
  emit_load<DEEP>(c, s, grp_key, slot, l, lane, cur);
  if (RSF_EMIT_PER_WAVE == 1) {
    emit_run<BKT, DEEP>(c, s, l, lane, cur, cnt_s, out_val, out_dec, bk, row);
    return;
  }
  for (uint32_t k = 0; k < RSF_EMIT_PER_WAVE; ++k) {
    if (k + 1 < RSF_EMIT_PER_WAVE) emit_load<DEEP>(c, s, grp_key, slot, l + k + 1, lane, nxt);
    if (l + k < c.n_loc) emit_run<BKT, DEEP>(c, s, l + k, lane, cur, cnt_s, out_val, out_dec, bk, row);
    cur = nxt;
  }
}
template <bool BKT, bool FULL>
__global__ void __launch_bounds__(64 * RSF_EMIT_WPB) emit_kernel(GCfg c, GState s, const uint32_t* __restrict__ grp_key,
                                                                 const uint32_t* __restrict__ slot,
                                                                 uint32_t* __restrict__ cnt_s,
                                                                 uint32_t* __restrict__ out_val,
                                                                 uint32_t* __restrict__ out_dec, Buckets bk) {
  emit_body<BKT, FULL, 0>(c, s, grp_key, slot, cnt_s, out_val, out_dec, bk);
}
// deep queues (DEEP: the queues with a tail, bit q)
template <bool BKT, bool FULL, uint32_t DEEP>
__global__ void __launch_bounds__(64 * RSF_EMIT_WPB)
#if RSF_EMIT_DEEP_SGPR
    __attribute__((amdgpu_num_sgpr(RSF_EMIT_DEEP_SGPR)))
#endif
    emit_kernel_deep(GCfg c, GState s, const uint32_t* __restrict__ grp_key, const uint32_t* __restrict__ slot,
                     uint32_t* __restrict__ cnt_s, uint32_t* __restrict__ out_val, uint32_t* __restrict__ out_dec,
                     Buckets bk) {
  emit_body<BKT, FULL, DEEP>(c, s, grp_key, slot, cnt_s, out_val, out_dec, bk);
}


// Record decoration: what merge_kernel needs to address the view entry (the
// subject) and to pick the queue, written beside the sorted rumor ids so the
// merge issues its view-entry load in the same round trip as the rumor-body
// load instead of after it.
__device__ __forceinline__ uint32_t decorate(const rsf_rumor* __restrict__ rumors, uint32_t rid) {
  // subject and type share one aligned 8-B word (offset 16): one load, no dependent second one
  static_assert(offsetof(rsf_rumor, subject) == 16 && offsetof(rsf_rumor, type) == 20, "rumor layout");
  const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(rumors + rid) + 16);
  const uint8_t t = (uint8_t)w.y;
  if (t == RSF_MSG_QUERY) return kDecQuery;
  if (t == RSF_MSG_USER_EVENT) return kDecEvent;
  return w.x;
}

// The round's rumor block decorated once into a dense 4-B table (rdec): emission and the
// receive side look a record's decoration up there instead of in the 24-B rumor bodies,
// a table 6x denser in L2 / Infinity Cache.  Run after the block is complete (after the
// all-reduce on the multi-GPU path).
// The same pass keeps the rumor bodies without their 8-B key (only user events and
// queries need it) as aligned 16-B records for the merge kernel's gather.
__global__ void __launch_bounds__(256) dec_fill_kernel(const rsf_rumor* __restrict__ rumors, uint32_t* __restrict__ rdec,
                                                       uint4* __restrict__ rbody, uint64_t base, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rdec[base + i] = decorate(rumors, (uint32_t)(base + i));
  const uint2* w = reinterpret_cast<const uint2*>(rumors + base + i);  // ltime | key | subject..msg_len
  const uint2 lt = w[0], tail = w[2];
  rbody[base + i] = make_uint4(lt.x, lt.y, tail.x, tail.y);
}
// a rumor rebuilt from its 16-B body (+ the key when the record needs it)
// segment bounds per receiver + record decoration (keys == nullptr: decoration only)
__global__ void __launch_bounds__(256) segment_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint64_t lo,
                                                      uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_end,
                                                      const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ rdec,
                                                      uint32_t* __restrict__ dec, uint32_t rmask) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t k = keys[i];
  if (k == kSentinel) return;
  if (i == 0 || keys[i - 1] != k) seg_start[k - lo] = (uint32_t)i;
  if (i + 1 == n || keys[i + 1] != k) seg_end[k - lo] = (uint32_t)(i + 1);
  if (dec) dec[i] = rdec[vals[i] & rmask];
}

// ---- multi-GPU send side: the records of the receiver-sorted groups (cap_t slots each,
// cnt[i] used) compacted into one receiver-ordered record stream [end[i-1], end[i])
// (end = inclusive scan of cnt); the last valid group publishes the record count.
// kLanesPerGroup lanes per group, one record per lane.
constexpr uint32_t kLanesPerGroup = 16;
// The records go out packed as (receiver << 32 | rumor id): the exchange's send format.
__global__ void __launch_bounds__(256) grp_expand_kernel(const uint32_t* __restrict__ key_s,
                                                         const uint32_t* __restrict__ end, uint64_t n,
                                                         uint32_t cap_t, const uint32_t* __restrict__ slots,
                                                         uint64_t* __restrict__ out, unsigned long long* n_valid) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = t / kLanesPerGroup;
  const uint32_t sub = (uint32_t)t % kLanesPerGroup;
  if (i >= n) return;
  const uint32_t key = key_s[i];
  if (key == kSentinel) return;
  const uint32_t o = i ? end[i - 1] : 0u, e = end[i];
  const uint32_t* src = slots + i * cap_t;
  for (uint32_t k = sub; o + k < e; k += kLanesPerGroup) out[o + k] = ((uint64_t)key << 32) | src[k];
  if (sub == 0 && (i + 1 == n || key_s[i + 1] == kSentinel)) *n_valid = e;
}

template <bool RUNS>
__global__ void __launch_bounds__(256, RSF_MERGE_WAVES) merge_kernel(GCfg c, GState s, const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ dec,
                                                    const uint32_t* __restrict__ seg_start,
                                                    const uint32_t* __restrict__ seg_end,
                                                    const uint32_t* __restrict__ gcnt, uint32_t stride, Buckets bk,
                                                    BigList big) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  __shared__ uint32_t subj_bits[kWavesPerBlock][128];  // chain detection (zero between chunks)
  uint32_t* sbits = subj_bits[threadIdx.x / kWave];
  for (uint32_t i = threadIdx.x & (kWave - 1); i < 128; i += kWave) sbits[i] = 0u;
  const uint64_t l = ((uint64_t)xcd_block(blockIdx.x, gridDim.x) * kWavesPerBlock +
                      (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)) * RSF_MERGE_PER_WAVE;
  if (l >= c.n_loc) return;
  const MSetupLane sl = merge_setup_lane(c, s, seg_start, seg_end, lane, RUNS ? bk.n_runs : 0u);
  uint32_t cur = merge_setup(sl, l, lane);
  // every owned receiver's setup is in flight one receiver ahead of its merge
  for (uint32_t k = 0; k < RSF_MERGE_PER_WAVE && l + k < c.n_loc; ++k) {
    const uint32_t nxt = k + 1 < RSF_MERGE_PER_WAVE && l + k + 1 < c.n_loc ? merge_setup(sl, l + k + 1, lane) : 0u;
    merge_one<RUNS, false>(c, s, vals, dec, gcnt, stride, l + k, lane, cur, nullptr, sbits, bk, big);
    cur = nxt;
  }
}

// the receivers merge_kernel deferred (BigList), grid-stride over the list
template <bool RUNS>
__global__ void __launch_bounds__(256) merge_big_kernel(GCfg c, GState s, const uint32_t* __restrict__ vals,
                                                        const uint32_t* __restrict__ dec,
                                                        const uint32_t* __restrict__ seg_start,
                                                        const uint32_t* __restrict__ seg_end,
                                                        const uint32_t* __restrict__ gcnt, uint32_t stride, Buckets bk,
                                                        BigList big) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  __shared__ QLds4 qlds[kWavesPerBlock];  // scratch of a pending list applied here
  __shared__ uint32_t subj_bits[kWavesPerBlock][128];
  QLds4& ql = qlds[threadIdx.x / kWave];
  uint32_t* sbits = subj_bits[threadIdx.x / kWave];
  for (uint32_t i = lane; i < 128; i += kWave) sbits[i] = 0u;
  const uint64_t n = *big.n;
  const uint64_t nw = (uint64_t)gridDim.x * kWavesPerBlock;
  const MSetupLane sl = merge_setup_lane(c, s, seg_start, seg_end, lane, RUNS ? bk.n_runs : 0u);
  for (uint64_t i = (uint64_t)blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
       i < n; i += nw) {
    const uint64_t l = big.ids[i];
    merge_one<RUNS, true>(c, s, vals, dec, gcnt, stride, l, lane, merge_setup(sl, l, lane), &ql, sbits, bk, big);
  }
}

// ---- push/pull anti-entropy (M7): merge_remote_state of a sender's local_state
// (core/src/serf/delegate.rs:376-554).  Snapshot semantics: memberlist sends its
// local state before it merges the remote one, so every sender's state is copied
// to a slab first (streaming, one block per pair), then merged.

__global__ void __launch_bounds__(256) pp_snapshot_kernel(GCfg c, GState s, const rsf_pp_pair* __restrict__ pairs,
                                                          PPSlab sl) {
  const uint64_t p = blockIdx.x;
  const uint64_t l = pairs[p].sender - c.lo;
  const uint4* vsrc = reinterpret_cast<const uint4*>(vrow_of(s, c, l));
  uint4* vdst = reinterpret_cast<uint4*>(view_row(sl.view, c.vrow, p));
  for (uint32_t i = threadIdx.x; i < c.vrow / 16; i += blockDim.x) vdst[i] = vsrc[i];
  for (uint32_t i = threadIdx.x; i < c.ebuf; i += blockDim.x) {
    sl.eb_ltime[p * c.ebuf + i] = s.eb_ltime[l * c.ebuf + i];
    sl.eb_cnt[p * c.ebuf + i] = s.eb_cnt[l * c.ebuf + i];
  }
  const uint64_t nk = (uint64_t)c.ebuf * c.slot_k;
  for (uint64_t i = threadIdx.x; i < nk; i += blockDim.x) sl.eb_keys[p * nk + i] = s.eb_keys[l * nk + i];
  if (threadIdx.x == 0) {
    sl.clocks[p * 4 + 0] = s.clock[l];
    sl.clocks[p * 4 + 1] = s.eclock[l];
    sl.clocks[p * 4 + 2] = s.qclock[l];
  }
}

// One wave per pair (receiver).  Lanes walk the subject slots 64 at a time:
// left members run handle_node_leave_intent(status_time + 1), the other known
// entries handle_node_join_intent(status_time); subjects are distinct, so lanes
// are independent except for the Lamport clock, whose value at each leave is an
// inclusive prefix max over the left members before it (all leaves precede all
// joins, delegate.rs:477-511).  The event buffer is walked the same way: sender
// slot i holds events of ltime = i (mod B), so it lands in receiver slot i and
// lanes touch distinct slots; the event clock is again a prefix max.  Member
// events, refutations and deliveries are digested serially in order.
__global__ void __launch_bounds__(256) pp_merge_kernel(GCfg c, GState s, const rsf_pp_pair* __restrict__ pairs,
                                                       uint64_t n_pairs, PPSlab sl, uint32_t flags) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (p >= n_pairs) return;
  const uint32_t m = pairs[p].receiver;
  const uint64_t l = m - c.lo;
  if (!s.alive[m]) return;
  MRegs r;
  load_regs(s, l, r);
  const uint64_t pl = sl.clocks[p * 4 + 0], pel = sl.clocks[p * 4 + 1], pql = sl.clocks[p * 4 + 2];
  if (pl > 0) witness(r.clock, pl - 1);
  if (pel > 0) witness(r.eclock, pel - 1);
  if (pql > 0) witness(r.qclock, pql - 1);
  // ---- status_ltimes / left_members
  const ViewS* sv = view_row(sl.view, c.vrow, p);
  ViewS* vrow = vrow_of(s, c, l);
  uint64_t c_leave = r.clock, c_join = r.clock;
  for (uint32_t base = 0; base < c.S; base += kWave) {
    const uint32_t subj = base + lane;
    const bool valid = subj < c.S;
    ViewE se{};
    if (valid) se = *view_at(sv, subj);
    const bool known = valid && vkind(se.meta) == RSF_KIND_KNOWN;
    const bool left = known && vstatus(se.meta) == RSF_STATUS_LEFT;
    const bool join = known && !left;
    ViewE v{};
    if (known) v = *view_at(vrow, subj);
    const uint64_t L = left ? se.ltime + 1 : se.ltime;
    const uint64_t incl = wave_inclusive_max_u64(left ? L + 1 : 0);
    const uint64_t excl = wave_shr1_u64(incl);
    int f = 0;
    uint64_t ref = 0;
    if (known) {
      MRegs rr = r;
      rr.clock = excl > c_leave ? excl : c_leave;
      rr.digest = 0;
      const uint64_t lt0 = v.ltime;
      const uint32_t mt0 = v.meta;
      const uint32_t t0 = v.t;
      if (left) f = hv_leave_intent(v, rr, subj, L, false, ref, c.now);
      else f = hv_join_intent(v, rr, L, c.now);
      if (v.ltime != lt0 || v.meta != mt0 || v.t != t0) *view_at(vrow, subj) = v;
    }
    const uint64_t lmax = lane63_u64(incl);
    if (lmax > c_leave) c_leave = lmax;
    const uint64_t jmax = wave_max_u64(join ? L + 1 : 0);
    if (jmax > c_join) c_join = jmax;
    uint64_t mm = ballot(f & (RSF_F_MEMBER_EVENT | RSF_F_REFUTE));
    while (mm) {
      const int i = __ffsll((long long)mm) - 1;
      mm &= mm - 1;
      const uint32_t fi = shfl_u32((uint32_t)f, i);
      if (fi & RSF_F_MEMBER_EVENT) {
        r.digest = digest_mix(r.digest, kDigMember | ((uint64_t)kEvLeave << 32) | (base + (uint32_t)i));
        if (lane == 0) mlog_put(c, s, l, r.err, kEvLeave, base + (uint32_t)i);
        r.err = shfl_u32(r.err, 0);
      }
      if (fi & RSF_F_REFUTE) {
        const uint64_t rf = shfl_u64(ref, i);
        if (lane == 0) push_refute(c, s, r, rf);
        r.err = shfl_u32(r.err, 0);
      }
    }
  }
  r.clock = c_leave > c_join ? c_leave : c_join;
  // ---- eventJoinIgnore (delegate.rs:513-521)
  if ((flags & 3) == 3 && pel > r.emin) r.emin = pel;
  // ---- the sender's event buffer, index order (delegate.rs:523-541)
  const uint64_t B = c.ebuf;
  uint64_t ec = r.eclock;
  for (uint32_t base = 0; base < c.ebuf; base += kWave) {
    const uint32_t i = base + lane;
    const bool valid = i < c.ebuf;
    const uint32_t cnt = valid ? sl.eb_cnt[p * c.ebuf + i] : 0u;
    const uint64_t L = cnt ? sl.eb_ltime[p * c.ebuf + i] : 0ull;
    const uint64_t incl = wave_inclusive_max_u64(cnt ? L + 1 : 0);
    const uint64_t excl = wave_shr1_u64(incl);
    uint64_t cur = excl > ec ? excl : ec;
    if (cnt && L + 1 > cur) cur = L + 1;  // witness(L) of this slot's events
    uint64_t dmask = 0;  // delivered keys of this slot (slot_k <= 64)
    uint32_t e_err = 0;
    if (cnt && !(L < r.emin) && !(cur > B && L < cur - B)) {
      const uint64_t rs = l * c.ebuf + (L % B);
      if ((L % B) != i) {
        e_err = kErrEvSlot;  // a ring slot not at ltime mod B: never produced by handle_user_event
      } else {
        uint64_t* rk = s.eb_keys + rs * c.slot_k;
        const uint64_t* sk = sl.eb_keys + (p * c.ebuf + i) * c.slot_k;
        uint32_t rc = s.eb_cnt[rs];
        const uint32_t rc0 = rc;
        for (uint32_t k = 0; k < cnt; ++k) {
          const uint64_t key = sk[k];
          bool dup = false;
          for (uint32_t j = 0; j < rc; ++j) dup |= rk[j] == key;
          if (dup) continue;
          if (rc == 0) {
            s.eb_ltime[rs] = L;
            rk[0] = key;
            rc = 1;
          } else if (rc < c.slot_k) {
            rk[rc++] = key;
          } else {
            e_err |= kErrEvSlot;
          }
          dmask |= 1ull << k;
        }
        if (rc != rc0) s.eb_cnt[rs] = rc;
      }
    }
    const uint64_t emax = lane63_u64(incl);
    if (emax > ec) ec = emax;
    uint64_t mm = ballot(dmask != 0 || e_err != 0);
    while (mm) {
      const int j = __ffsll((long long)mm) - 1;
      mm &= mm - 1;
      r.err |= shfl_u32(e_err, j);
      uint64_t dm = shfl_u64(dmask, j);
      const uint64_t Lj = shfl_u64(L, j);
      const uint64_t* skj = sl.eb_keys + (p * c.ebuf + base + (uint32_t)j) * c.slot_k;
      while (dm) {
        const int k = __ffsll((long long)dm) - 1;
        dm &= dm - 1;
        r.digest = digest_mix(digest_mix(r.digest, kDigUser ^ skj[k]), Lj);
        if (lane == 0) dlog_put(c, s, l, r, Lj, skj[k], false);
        r.err = shfl_u32(r.err, 0);
      }
    }
  }
  r.eclock = ec;
  if (lane == 0) {
    store_regs(s, l, r);
    s.emin[l] = r.emin;
  }
}


// QueueChecker tick (base.rs:703-760): one thread per (member, queue).  A sorted queue's
// live items are its leading slots, so num_queued is the first free slot; prune(max)
// drops the items past `max`, the last ones in send order (memberlist
// TransmitLimitedQueue::prune).  stats[q] = queued, stats[3 + q] = members at or above
// the warning depth, stats[6 + q] = pruned.
// Deep queues: numq counts the tail too, and a queue to prune is listed (s.deep_ids) for
// check_stream_kernel, which keeps the max smallest keys of head and tail.
// qmax (non-null when min_queue_depth > 0): each member's own get_queue_max (queue_max_kernel).
// One wave per member (lane = head slot; 65..256-slot queues in chunks of 64), a grid-stride
// loop over the phase's members: a queue's head count is its leading run of live slots, one
// ballot per chunk.  The counts and the occupancy histogram are summed per block in LDS and
// added to HBM once per block (one global atomic per member on the same few addresses took
// 0.25 ms for 6.7k members).
__global__ void __launch_bounds__(256) check_queues_kernel(GCfg c, GState s, uint32_t max_depth, uint32_t warn,
                                                           unsigned long long* __restrict__ stats,
                                                           const uint32_t* __restrict__ qmax,
                                                           uint32_t* __restrict__ hist, uint32_t period,
                                                           uint32_t phase) {
  __shared__ unsigned long long bst[9];
  __shared__ uint32_t bh[kOccHistWords];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  for (uint32_t i = threadIdx.x; i < kOccHistWords; i += blockDim.x) bh[i] = 0;
  if (threadIdx.x < 9) bst[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t l0 = phase_first(c, period, phase);
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / kWave);
  for (uint64_t wi = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;; wi += nw) {
    const uint64_t l = l0 + wi * period;
    if (l >= c.n_loc) break;
    const uint32_t mx = qmax ? qmax[l] : max_depth;
    uint32_t nq[3];
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) {
      const uint64_t base = (l * 3 + q) * c.qcap;
      uint32_t n = 0;
      for (uint32_t j = 0; j < c.qcap; j += kWave) {
        const bool live = j + lane < c.qcap && s.q_rumor[base + j + lane] != kEmpty;
        const uint64_t m = ballot(live);
        const uint32_t run = m == ~0ull ? kWave : (uint32_t)__builtin_ctzll(~m);
        n = j + run;
        if (run < kWave) break;
      }
      if (tcap_of(c, q)) n += s.tsum[l * 3 + q].x;
      nq[q] = n;
    }
    if (lane < 3) {
      const uint32_t q = lane, n = q == 0 ? nq[0] : q == 1 ? nq[1] : nq[2];
      atomicAdd(&bh[q * (kOccBins + 1) + min(n / kOccBin, kOccBins)], 1u);  // occupancy before the prune
      atomicMax(&bh[3 * (kOccBins + 1) + q], n);
      if (n) atomicAdd(&bst[q], (unsigned long long)n);
      if (n >= warn) atomicAdd(&bst[3 + q], 1ull);
      if (n > mx) atomicAdd(&bst[6 + q], (unsigned long long)(n - mx));
      // the deep queues' entries for check_stream_kernel at fixed places (kEmpty: under the
      // max): one atomic per listed queue on a single counter took most of this kernel's time
      if (tcap_of(c, q)) s.deep_ids[wi * deep_queues(c) + deep_rank(c, q)] = n > mx ? (uint32_t)(l * 3 + q) : kEmpty;
    }
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) {
      if (tcap_of(c, q) || nq[q] <= mx) continue;  // numq >= max -> prune(max): retain max
      const uint64_t base = (l * 3 + q) * c.qcap;
      for (uint32_t i = mx + lane; i < nq[q]; i += kWave) {
        s.q_rumor[base + i] = kEmpty;
        s.q_seq[base + i] = 0;
        s.q_txlen[base + i] = 0;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 9 && bst[threadIdx.x]) atomicAdd(stats + threadIdx.x, bst[threadIdx.x]);
  if (hist) {
    for (uint32_t i = threadIdx.x; i < 3 * (kOccBins + 1); i += blockDim.x)
      if (bh[i]) atomicAdd(hist + i, bh[i]);
    if (threadIdx.x < 3 && bh[3 * (kOccBins + 1) + threadIdx.x])
      atomicMax(hist + 3 * (kOccBins + 1) + threadIdx.x, bh[3 * (kOccBins + 1) + threadIdx.x]);
  }
}

// get_queue_max with min_queue_depth > 0 (base.rs:748-759): max(2 * members.states.len(),
// min_queue_depth), per member, since each node's checker reads its own member map.
// states.len() is every member the node knows, as the Reconnector counts it
// (reconnect_kernel): the N - S untracked members, the local node when it is a subject, and
// the tracked subjects whose entry is KNOWN.  One wave per member; out[l] saturates at 2^32-1.
__global__ void __launch_bounds__(256) queue_max_kernel(GCfg c, GState s, uint32_t min_depth,
                                                        uint32_t* __restrict__ out, uint32_t period, uint32_t phase) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t l = phase_first(c, period, phase) + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave * period;
  if (l >= c.n_loc) return;
  const int32_t own = s.member_subj[l];
  const ViewS* row = vrow_of(s, c, l);
  uint64_t known = (c.N - c.S) + (own >= 0 ? 1u : 0u);
  for (uint32_t j0 = 0; j0 < c.S; j0 += kWave) {
    const uint32_t j = j0 + lane;
    const bool kn = j < c.S && (int32_t)j != own && vkind(ViewE(*view_at(row, j)).meta) == RSF_KIND_KNOWN;
    known += (uint32_t)__popcll(ballot(kn));
  }
  uint64_t mx = 2 * known;
  if (mx < min_depth) mx = min_depth;
  if (lane == 0) out[l] = (uint32_t)(mx < 0xFFFFFFFFull ? mx : 0xFFFFFFFFull);
}

// Generations alive: gen and gen - 1 (modulo the generation count, even so that the
// parity alternates across the wrap).

// At the start of generation `gen` (the ring wrapped): every queue drops its items of
// generation gen - 2, whose table half this generation overwrites.  One wave per
// (member, queue), lane = queue slot; the survivors keep their sorted order.
__global__ void __launch_bounds__(256) expire_kernel(GCfg c, GState s, uint32_t gen) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (t >= c.n_loc * 3) return;
  const uint64_t l = t / 3;
  const uint32_t q = (uint32_t)(t % 3);
  const uint32_t G = rumor_generations(c);
  if (c.qcap > kWave) {
    __shared__ QLds4 rows[kWavesPerBlock];
    Q4 Q;
    q4_load(c, s, l, q, lane, Q);
    bool stale[kQK];
#pragma unroll
    for (uint32_t k = 0; k < kQK; ++k) stale[k] = (gen + G - (Q.r[k] >> c.rbits) % G) % G >= 2;
    const uint32_t x = q4_expire(c, Q, lane, stale, q == 0, rows[threadIdx.x / kWave]);
    if (!x) return;
    q4_store(c, s, l, q, lane, Q);
    if (lane == 0) atomicAdd(s.q_expired + l, x);
    return;
  }
  QRegs Q{kEmpty, 0, 0};
  q_load(c, s, l, q, lane, Q);
  const uint32_t age = (gen + G - (Q.r >> c.rbits) % G) % G;
  const uint32_t x = q_expire(c, Q, lane, age >= 2, q == 0);
  if (x) q_store(c, s, l, q, lane, Q, true);
  const uint32_t xt = tail_expire_wave(c, s, l, q, lane, gen, G);  // deep queues: the tail too
  if ((x + xt) && lane == 0) atomicAdd(s.q_expired + l, x + xt);
}

// ---- multi-GPU exchange buckets: the sorted groups split by destination shard.
// bounds: wstart[w] = first sorted group whose receiver is in shard w (sentinel groups,
// dead senders, sort last); each bucket's header = its group count (overflow flagged).
__global__ void bucket_bounds_kernel(const uint32_t* __restrict__ key_s, uint64_t n, uint64_t per, uint32_t world,
                                     uint32_t* __restrict__ wstart, uint32_t* __restrict__ send, uint64_t stride_u32,
                                     uint32_t gcap, unsigned long long* __restrict__ flags) {
  const uint32_t w = threadIdx.x;
  if (w > world) return;
  auto first_ge = [&](uint64_t target) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) / 2;
      if ((uint64_t)key_s[mid] < target) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const uint64_t a = first_ge((uint64_t)w * per);
  wstart[w] = (uint32_t)a;
  if (w == world) return;
  const uint64_t b = first_ge((uint64_t)(w + 1) * per), ng = b - a;
  send[(uint64_t)w * stride_u32] = (uint32_t)(ng < gcap ? ng : gcap);
  if (ng > gcap) atomicOr(flags, 1ull);
}

__global__ void __launch_bounds__(256) zero_spans_kernel(ZeroSpans z) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
#pragma unroll
  for (int k = 0; k < kZeroSpans; ++k)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < z.words[k]; i += stride) z.p[k][i] = 0u;
}

// counters[kCtrMergedTotal] (records merged since creation) += counters[from] (this round's)
__global__ void accumulate_kernel(unsigned long long* counters, uint32_t from) {
  if (threadIdx.x == 0 && blockIdx.x == 0) counters[kCtrMergedTotal] += counters[from];
}


}  // namespace

void rsf::mark(rsf_gossip* g, int k) {
  if (!g->profiling || g->prof_rounds >= rsf_gossip::kMaxProfRounds) return;
  hipEventRecord(g->ev[g->prof_rounds][k], g->stream);
  if (k == rsf_gossip::kMarks - 1) g->prof_rounds++;
}

// Every member's pending re-queues applied to its queues: before anything other than
// emission reads the queues, the queue-prune counters or the error flags.
int rsf::flush_pending(rsf_gossip* g, uint32_t period, uint32_t phase) {
  const uint64_t cnt = phase_count(g->c, period, phase);
  if (!cnt) return RSF_OK;
  hipLaunchKernelGGL(pend_flush_kernel, dim3(grid1(cnt, kWavesPerBlock)), dim3(kWave * kWavesPerBlock), 0,
                     g->stream, g->c, g->s, period, phase);
  RSF_HIP(hipGetLastError());
  return RSF_OK;
}

static int ensure_lists(rsf_gossip* g, uint32_t n_ml, uint32_t n_acts) {
  int rc;
  if (n_ml > g->cap_ml) {
    hipFree(g->d_ml);
    g->d_ml = nullptr;
    uint32_t cap = std::max<uint32_t>(n_ml, 64);
    if ((rc = dmalloc((void**)&g->d_ml, cap * sizeof(rsf_ml_event)))) return rc;
    g->cap_ml = cap;
  }
  if (n_acts > g->cap_acts) {
    hipFree(g->d_acts);
    hipFree(g->d_act_status);
    g->d_acts = nullptr;
    g->d_act_status = nullptr;
    g->cap_acts = 0;
    uint32_t cap = std::max<uint32_t>(n_acts, 1024);
    if ((rc = dmalloc((void**)&g->d_acts, (size_t)cap * sizeof(rsf_action)))) return rc;
    if ((rc = dmalloc((void**)&g->d_act_status, (size_t)cap * sizeof(int32_t)))) return rc;
    g->cap_acts = cap;
  }
  return RSF_OK;
}

// every radix sort sizes its own temporary storage (rsf::cub_run)
int rsf::sort_pairs(rsf_gossip* g, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                      uint64_t n, hipStream_t on) {
  const int end_bit = g->end_bit;
  hipStream_t st = on ? on : g->stream;
  return rsf::cub_run(
      g->sort_tmp, st,
      [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, kin, kout, vin, vout, (int)n, 0, end_bit, st);
      },
      "group/record radix sort");
}

// the peers-ahead work in flight (if any) is joined by the context stream and dropped: before
// anything changes liveness, or uses the group arrays / sort storage another way
int rsf::ahead_drop(rsf_gossip* g) {
  if (g->ahead_launched) RSF_HIP(hipStreamWaitEvent(g->stream, g->ev_ahead, 0));
  g->ahead_launched = g->ahead_valid = false;
  return RSF_OK;
}

// peer draw + stable sort of the groups by receiver, on stream `st`
static int peers_and_sort(rsf_gossip* g, uint32_t round, hipStream_t st) {
  const GCfg& c = g->c;
  hipLaunchKernelGGL(peers_kernel, dim3(grid1(c.n_loc)), dim3(256), 0, st, c, g->s, round, g->grp_key);
  RSF_HIP(hipGetLastError());
  RSF_DBG_SYNC(st, "peers_kernel");
  int rc = sort_pairs(g, g->grp_key, g->grp_key_s, g->grp_id, g->grp_id_s, g->n_groups, st);
  if (rc) return rc;
  RSF_DBG_SYNC(st, "group sort");
  return RSF_OK;
}


// merge_big_kernel, the deep emission classes and check_stream_kernel run as many blocks as
// stay resident: their grids, asked of the runtime once at creation
int rsf::resident_grids(rsf_gossip* g) {
  const GCfg& c = g->c;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, merge_kernel<false>, kWave * kWavesPerBlock, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess)
    return rsf::set_error(RSF_ERR_HIP, "occupancy query failed");
  g->merge_blocks = (unsigned)std::max(1, per_cu * cus);
  if (c.deep) {
    int dpc = 0, dpb = 0, dpk = 0, dpt = 0, dpm = 0;
    if (
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&dpc, emit_deep_wave_kernel<false, kDeepSmall>, kWave, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&dpt, emit_deep_wave_kernel<false, kDeepTiny>, kWave, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&dpm, emit_deep_block_kernel<false, kDeepMid>, kDeepBlkThreads, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&dpb, emit_deep_block_kernel<false, kDeepBig>, kDeepBlkThreads, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&dpk, check_stream_kernel, kDeepThreads, 0) != hipSuccess)
      return rsf::set_error(RSF_ERR_HIP, "occupancy query failed");
    g->deep_blocks = (unsigned)std::max(1, dpc * cus);
    g->deep_blocks_big = (unsigned)std::max(1, dpb * cus);
    g->deep_blocks_tiny = (unsigned)std::max(1, dpt * cus);
    g->deep_blocks_mid = (unsigned)std::max(1, dpm * cus);
    g->deep_check_blocks = (unsigned)std::max(1, dpk * cus);
  }
  return RSF_OK;
}

extern "C" {

// phases 1-3 (everything before emission)
int rsf_gossip_round_begin(rsf_gossip* g, uint32_t round, const rsf_ml_event* ml, uint32_t n_ml,
                           const rsf_action* acts, uint32_t n_acts) {
  if (!g || (n_ml && !ml) || (n_acts && !acts)) return gerr("null argument");
  const GCfg& c = g->c;
  for (uint32_t e = 0; e < n_ml; ++e)
    if (ml[e].subject >= c.S || (ml[e].kind != RSF_ML_JOIN && ml[e].kind != RSF_ML_LEAVE && ml[e].kind != RSF_ML_UPDATE) || ml[e].set_alive > 2)
      return gerr("bad memberlist event");
  // actions: known kinds, members in range, distinct members
  {
    std::vector<uint32_t> ms;
    ms.reserve(n_acts);
    for (uint32_t a = 0; a < n_acts; ++a) {
      const rsf_action& x = acts[a];
      if (x.member >= c.N || x.act < RSF_ACT_JOIN_SELF || x.act > RSF_ACT_QUERY) return gerr("bad action");
      if (x.act == RSF_ACT_FORCE_LEAVE && x.subject >= c.S) return gerr("force_leave subject out of range");
      if ((x.act == RSF_ACT_JOIN_SELF || x.act == RSF_ACT_LEAVE_SELF) &&
          !std::binary_search(g->subj_sorted.begin(), g->subj_sorted.end(), x.member))
        return gerr("join / leave of a member that is not a tracked subject");
      ms.push_back(x.member);
    }
    std::sort(ms.begin(), ms.end());
    if (std::adjacent_find(ms.begin(), ms.end()) != ms.end()) return gerr("actions of one round must name distinct members");
  }
  uint64_t need = (uint64_t)c.S * c.max_refute + n_acts;
  if (need > g->max_rumors) return rsf::set_error(RSF_ERR_OVERFLOW, "one round's rumors exceed the rumor ring");
  RSF_HIP(hipSetDevice(g->device));
  int rc = ensure_lists(g, n_ml, n_acts);
  if (rc) return rc;
  for (uint32_t e = 0; e < n_ml; ++e)  // liveness changes: peers drawn ahead are stale
    if (ml[e].set_alive != 2 && (rc = ahead_drop(g))) return rc;
  hipStream_t st = g->stream;
  mark(g, 0);
  g->cur_round = round;
  g->c.now = round;  // handlers stamp leave / intent times with the round
  if ((uint64_t)g->n_rumors + need > g->max_rumors) {  // the block restarts the ring, next generation
    g->n_rumors = 0;
    g->gen = (g->gen + 1) % rumor_generations(c);
    g->c.gen = g->gen;
    // this generation reuses the half of the table of generation gen - 2: queued ids of
    // that generation expire now, before anything reads or re-queues them
    if ((rc = flush_pending(g))) return rc;
    hipLaunchKernelGGL(expire_kernel, dim3(grid1(c.n_loc * 3, kWavesPerBlock)), dim3(kWave * kWavesPerBlock), 0,
                       g->stream, c, g->s, g->gen);
  }
  g->round_slot = g->n_rumors;
  g->round_base = (uint32_t)(((uint64_t)g->gen << c.rbits) | g->round_slot);
  g->round_abase = g->round_base + c.S * c.max_refute;
  g->round_need = (uint32_t)need;
  g->n_rumors += (uint32_t)need;
  const uint32_t round_pidx = g->round_base & c.rmask;  // physical index: generation parity | slot
  RSF_HIP(hipMemsetAsync(g->s.rumors + round_pidx, 0, need * sizeof(rsf_rumor), st));
  if (g->c.dcap) RSF_HIP(hipMemsetAsync(g->s.dcnt, 0, c.n_loc * 4, st));  // the round's delivery log
  const size_t b_ml = (size_t)n_ml * sizeof(rsf_ml_event), b_acts = (size_t)n_acts * sizeof(rsf_action);
  const char* pin_ml = nullptr;
  const char* pin_acts = nullptr;
  int pin_k = -1;
  if (!RSF_PIN_STAGING) {
    pin_ml = (const char*)ml;
    pin_acts = (const char*)acts;
  } else if (b_ml + b_acts) {
    const int k = pin_k = g->pin_next;
    g->pin_next ^= 1;
    if (g->pin_used[k]) RSF_HIP(hipEventSynchronize(g->pin_ev[k]));  // its previous copy has landed
    if (!g->pin_ev[k]) RSF_HIP(hipEventCreateWithFlags(&g->pin_ev[k], hipEventDisableTiming));
    if (b_ml + b_acts > g->pin_cap[k]) {
      if (g->pin[k]) RSF_HIP(hipHostFree(g->pin[k]));
      g->pin[k] = nullptr;
      g->pin_cap[k] = 0;
      const size_t cap = std::max<size_t>(b_ml + b_acts, 1 << 20);
      RSF_HIP(hipHostMalloc(&g->pin[k], cap, hipHostMallocDefault));
      g->pin_cap[k] = cap;
    }
    char* p = (char*)g->pin[k];
    if (b_ml) memcpy(p, ml, b_ml);
    if (b_acts) memcpy(p + b_ml, acts, b_acts);
    pin_ml = p;
    pin_acts = p + b_ml;
  }
  if (n_ml) {
    RSF_HIP(hipMemcpyAsync(g->d_ml, pin_ml, b_ml, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ml_kernel, dim3(grid1(c.n_loc)), dim3(256), 0, st, c, g->s, g->d_ml, n_ml);
    hipLaunchKernelGGL(ml_alive_kernel, dim3(1), dim3(64), 0, st, g->s, g->d_ml, n_ml);
  }
  hipLaunchKernelGGL(refute_kernel, dim3(grid1(c.S)), dim3(256), 0, st, c, g->s, g->round_base);
  RSF_DBG_SYNC(st, "refute_kernel");
  if (n_acts) {
    RSF_HIP(hipMemcpyAsync(g->d_acts, pin_acts, b_acts, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(originate_kernel, dim3(grid1(n_acts)), dim3(256), 0, st, c, g->s, g->d_acts, n_acts,
                       g->round_abase, g->d_act_status);
    RSF_DBG_SYNC(st, "originate_kernel");
  }
  g->last_n_acts = n_acts;
  if (pin_k >= 0) {  // the slot is free again once the stream has passed this point
    RSF_HIP(hipEventRecord(g->pin_ev[pin_k], st));
    g->pin_used[pin_k] = true;
  }
  RSF_HIP(hipGetLastError());
  mark(g, 1);
  return RSF_OK;
}

int rsf_gossip_rumor_block(rsf_gossip* g, void** p, uint64_t* bytes) {
  if (!g || !p || !bytes) return gerr("null argument");
  *p = g->s.rumors + (g->round_base & g->c.rmask);
  *bytes = (uint64_t)g->round_need * sizeof(rsf_rumor);
  return RSF_OK;
}

}  // extern "C"

// Emission in canonical order.  peers_kernel draws every sender's peers; a stable radix
// sort of the GROUPS (sender, peer) by receiver (n_loc * fanout keys, not records) fixes
// where each group's records go, so emit_kernel writes them in merge order directly:
// cap_t slots per group, in (receiver; sender, position) order, with the group's count.
// local: this context merges its own records (single context): also each receiver's
// range of groups for merge_kernel.  Otherwise the groups are compacted into one
// receiver-ordered record stream (packed into send_buf, n_valid) for the exchange.
// bucket mode (world > 0): emission straight into the destination shards' buckets
// emission by the queue layout: four slots per lane (65..256), one (64: FULL, or fewer); deep
// queues then run the members the heads could not decide through emit_deep_wave_kernel
template <bool BKT>
static int launch_emit(rsf_gossip* g, dim3 egrid, const Buckets& bk) {
  const GCfg& c = g->c;
  hipStream_t st = g->stream;
  const dim3 eb(kWave * RSF_EMIT_WPB);
  if (c.qcap > kWave) {
    hipLaunchKernelGGL(emit4_kernel<BKT>, dim3((unsigned)c.n_loc), dim3(kWave), 0, st, c, g->s, g->grp_key, g->grp_slot,
                       g->grp_cnt, g->stage_val, g->stage_dec, bk);
  } else if (c.deep) {
    // (the deferred-member lists were emptied by peers_kernel)
    // only the intent queue deep (the common configuration): the other queues' tail code is
    // compiled out of the emission
    const bool q0_only = c.tcap1 == 0 && c.tcap2 == 0;
#define RSF_EMIT_DEEP(FULL, M)                                                                                         \
  hipLaunchKernelGGL((emit_kernel_deep<BKT, FULL, M>), egrid, eb, 0, st, c, g->s, g->grp_key, g->grp_slot, g->grp_cnt, \
                     g->stage_val, g->stage_dec, bk)
    if (c.qcap == kWave) {
      if (q0_only) RSF_EMIT_DEEP(true, 1u);
      else RSF_EMIT_DEEP(true, 7u);
    } else {
      if (q0_only) RSF_EMIT_DEEP(false, 1u);
      else RSF_EMIT_DEEP(false, 7u);
    }
#undef RSF_EMIT_DEEP
    RSF_HIP(hipGetLastError());
    RSF_DBG_SYNC(st, "emit_kernel (deep)");
    // by capacity; the full depth last, with the members the smaller classes re-list (list 4)
    // after its own in the same launch.  (Run beside each other on two streams, the classes
    // were slower: a full-depth wave holds most of its CU's LDS, so the small classes' waves
    // could not share the CU.)
    hipLaunchKernelGGL((emit_deep_wave_kernel<BKT, kDeepTiny>), dim3(g->deep_blocks_tiny), dim3(kWave), 0, st, c, g->s,
                       g->grp_key, g->grp_slot, g->grp_cnt, g->stage_val, g->stage_dec, bk, 2u, g->d_counters + kCtrDeepTotal);
    hipLaunchKernelGGL((emit_deep_wave_kernel<BKT, kDeepSmall>), dim3(g->deep_blocks), dim3(kWave), 0, st, c, g->s,
                       g->grp_key, g->grp_slot, g->grp_cnt, g->stage_val, g->stage_dec, bk, 0u, g->d_counters + kCtrDeepTotal);
    hipLaunchKernelGGL((emit_deep_block_kernel<BKT, kDeepMid>), dim3(g->deep_blocks_mid), dim3(kDeepBlkThreads), 0, st, c,
                       g->s, g->grp_key, g->grp_slot, g->grp_cnt, g->stage_val, g->stage_dec, bk, 3u, g->d_counters + kCtrDeepTotal);
    hipLaunchKernelGGL((emit_deep_block_kernel<BKT, kDeepBig>), dim3(g->deep_blocks_big), dim3(kDeepBlkThreads), 0, st, c,
                       g->s, g->grp_key, g->grp_slot, g->grp_cnt, g->stage_val, g->stage_dec, bk, 1u, g->d_counters + kCtrDeepTotal);
  } else if (c.qcap == kWave) {
    hipLaunchKernelGGL((emit_kernel<BKT, true>), egrid, eb, 0, st, c, g->s, g->grp_key, g->grp_slot, g->grp_cnt,
                       g->stage_val, g->stage_dec, bk);
  } else {
    hipLaunchKernelGGL((emit_kernel<BKT, false>), egrid, eb, 0, st, c, g->s, g->grp_key, g->grp_slot, g->grp_cnt,
                       g->stage_val, g->stage_dec, bk);
  }
  RSF_HIP(hipGetLastError());
  return RSF_OK;
}

// after round t's emission (the last reader of grp_key / grp_slot): round t + 1's peers and
// group sort on the side stream
static int launch_ahead(rsf_gossip* g, uint32_t round) {
  if (!g->ahead_on) return RSF_OK;
  RSF_HIP(hipEventRecord(g->ev_emitted, g->stream));
  RSF_HIP(hipStreamWaitEvent(g->side, g->ev_emitted, 0));
  int rc = peers_and_sort(g, round + 1, g->side);
  // (also on an error: work already queued on the side stream may still write the group keys,
  // so the main stream must wait for it before their next use -- ahead_drop does)
  RSF_HIP(hipEventRecord(g->ev_ahead, g->side));
  g->ahead_launched = true;
  g->ahead_valid = rc == RSF_OK;
  if (rc) return rc;
  g->ahead_round = round + 1;
  return RSF_OK;
}

static int check_in_round(rsf_gossip* g, uint32_t round);
int rsf::emit_and_sort(rsf_gossip* g, uint32_t round, bool local, uint32_t world) {
  const GCfg& c = g->c;
  hipStream_t st = g->stream;
  const uint64_t ng = g->n_groups;
  if (g->round_need)
    hipLaunchKernelGGL(dec_fill_kernel, dim3(grid1(g->round_need)), dim3(256), 0, st, (const rsf_rumor*)g->s.rumors,
                       g->s.rdec, g->s.rbody, (uint64_t)(g->round_base & c.rmask), (uint64_t)g->round_need);
  RSF_DBG_SYNC(st, "dec_fill_kernel");
  // this round's peers and group order: drawn ahead under the previous round, or now
  const bool use_ahead = g->ahead_valid && g->ahead_round == round;
  if (g->ahead_launched) RSF_HIP(hipStreamWaitEvent(st, g->ev_ahead, 0));
  g->ahead_launched = g->ahead_valid = false;
  int rc;
  if (!use_ahead && (rc = peers_and_sort(g, round, st))) return rc;
  {
    // the emission's deferred-member lists, the group counts (buckets carry their own), the
    // segment bounds of the single-context merge: one launch
    ZeroSpans z{};
    int k = 0;
    if (c.deep) z.p[k] = g->s.deep_n, z.words[k++] = kDeepLists;
    if (!world) z.p[k] = g->grp_cnt, z.words[k++] = ng;
    if (local) {
      z.p[k] = g->seg_start, z.words[k++] = c.n_loc;
      z.p[k] = g->seg_end, z.words[k++] = c.n_loc;
    }
    uint64_t most = 0;
    for (int i = 0; i < k; ++i) most = std::max(most, z.words[i]);
    if (most) {
      hipLaunchKernelGGL(zero_spans_kernel, dim3((unsigned)std::min<uint64_t>(grid1(most), 2048)), dim3(256), 0, st, z);
      RSF_HIP(hipGetLastError());
    }
  }
  const dim3 egrid(grid1((c.n_loc + RSF_EMIT_PER_WAVE - 1) / RSF_EMIT_PER_WAVE, RSF_EMIT_WPB));
  if (world) {
    // buckets: the shard bounds first, then every group's slot word = (shard, place in bucket)
    // only a group's place inside its bucket must fit the slot word's index field
    if (g->bkt_gcap >= kBktIdxMask || world >= (1u << (32 - kBktWShift)))
      return gerr("bucket capacity too large for the slot encoding");
    const Buckets bk = send_buckets(g);
    hipLaunchKernelGGL(bucket_bounds_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)g->grp_key_s, ng, bk.per, world,
                       g->d_wstart, g->bkt_send, bk.stride_u32, bk.gcap, g->d_counters + kCtrBktBad);
    hipLaunchKernelGGL(grp_index_kernel, dim3(grid1(ng)), dim3(256), 0, st, g->grp_key_s, g->grp_id_s, ng, c.lo,
                       g->grp_slot, nullptr, nullptr, (const uint32_t*)g->d_wstart, (uint32_t)bk.per,
                       g->bkt_send + bk.keys_off, bk.stride_u32, bk.gcap);
    RSF_HIP(hipGetLastError());
    RSF_DBG_SYNC(st, "grp_index_kernel");
    mark(g, 2);
    if ((rc = launch_emit<true>(g, egrid, bk))) return rc;
    // the tick before the next round's peers start on the side stream: the prune's blocks
    // hold most of a CU's LDS and would only trade places with the sort's
    if ((rc = check_in_round(g, round))) return rc;
    if ((rc = launch_ahead(g, round))) return rc;
    mark(g, 3);
    return RSF_OK;
  }
  hipLaunchKernelGGL(grp_index_kernel, dim3(grid1(ng)), dim3(256), 0, st, g->grp_key_s, g->grp_id_s, ng, c.lo,
                     g->grp_slot, local ? g->seg_start : nullptr, local ? g->seg_end : nullptr);
  RSF_HIP(hipGetLastError());
  RSF_DBG_SYNC(st, "grp_index_kernel");
  mark(g, 2);
  if ((rc = launch_emit<false>(g, egrid, Buckets{}))) return rc;
  RSF_DBG_SYNC(st, "emit_kernel");
  // the counts path reads the sorted groups after the emission (grp_expand_kernel): no ahead
  if ((rc = check_in_round(g, round))) return rc;
  if (local && (rc = launch_ahead(g, round))) return rc;
  if (local) {
    unsigned long long* sum = (unsigned long long*)g->d_counters + kCtrSent;
    const uint32_t* cnt = g->grp_cnt;
    int rc2 = rsf::cub_run(
        g->grp_tmp, st,
        [&](void* t, size_t& b) { return hipcub::DeviceReduce::Sum(t, b, cnt, sum, (int)ng, st); },
        "group count reduce");
    if (rc2) return rc2;
    RSF_DBG_SYNC(st, "group count reduce");
  } else {
    const uint32_t* cnt = g->grp_cnt;
    uint32_t* off = g->grp_off;
    int rc2 = rsf::cub_run(
        g->grp_tmp, st, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveSum(t, b, cnt, off, (int)ng, st); },
        "group count scan");
    if (rc2) return rc2;
    RSF_DBG_SYNC(st, "group count scan");
    RSF_HIP(hipMemsetAsync(g->d_counters + kCtrSent, 0, 8, st));
    hipLaunchKernelGGL(grp_expand_kernel, dim3(grid1(ng * kLanesPerGroup)), dim3(256), 0, st, g->grp_key_s,
                       g->grp_off, ng, c.cap_t, g->stage_val, g->send_buf, g->d_counters + kCtrSent);
    RSF_HIP(hipGetLastError());
  }
  mark(g, 3);
  return RSF_OK;
}

// grouped: the records are emit_kernel's groups (stage_val / stage_dec, cap_t slots, grp_cnt);
// otherwise a flat record stream (vals, rec_dec)
static BigList big_list(rsf_gossip* g) { return BigList{g->big_ids, g->d_counters + kCtrBigCount}; }
// merge_kernel over every receiver, then merge_big_kernel over the ones it deferred
template <bool RUNS>
static int merge_launch(rsf_gossip* g, const uint32_t* vals, const uint32_t* dec, const uint32_t* start,
                        const uint32_t* end, const uint32_t* gcnt, uint32_t stride, const Buckets& bk) {
  const GCfg& c = g->c;
  const BigList big = big_list(g);
  RSF_HIP(hipMemsetAsync(big.n, 0, 8, g->stream));
  const unsigned blocks = grid1((c.n_loc + RSF_MERGE_PER_WAVE - 1) / RSF_MERGE_PER_WAVE, kWavesPerBlock);
  hipLaunchKernelGGL(merge_kernel<RUNS>, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, g->stream, c, g->s, vals, dec,
                     start, end, gcnt, stride, bk, big);
  RSF_DBG_SYNC(g->stream, "merge_kernel");
  hipLaunchKernelGGL(merge_big_kernel<RUNS>, dim3(std::min(g->merge_blocks, blocks)), dim3(kWave * kWavesPerBlock), 0,
                     g->stream, c, g->s, vals, dec, start, end, gcnt, stride, bk, big);
  RSF_HIP(hipGetLastError());
  RSF_DBG_SYNC(g->stream, "merge_big_kernel");
  return RSF_OK;
}

// grouped: the records are emit_kernel's groups (stage_val / stage_dec, cap_t slots, grp_cnt);
// otherwise a flat record stream (vals, rec_dec)
int rsf::launch_merge(rsf_gossip* g, const uint32_t* vals, bool grouped) {
  const GCfg& c = g->c;
  int rc = merge_launch<false>(g, grouped ? g->stage_val : vals, grouped ? g->stage_dec : (const uint32_t*)g->rec_dec,
                               g->seg_start, g->seg_end, grouped ? g->grp_cnt : nullptr, grouped ? c.cap_t : 1u,
                               Buckets{});
  if (rc) return rc;
  mark(g, 4);
  return RSF_OK;
}

// ---- what the other units need of this unit's kernels (declared in gossip_ctx.h)
int rsf::merge_runs(rsf_gossip* g) {
  return merge_launch<true>(g, nullptr, nullptr, g->d_rstart, g->d_rend, nullptr, g->c.cap_t, send_buckets(g));
}

int rsf::segment_bounds(rsf_gossip* g, const uint32_t* keys, uint64_t n, uint64_t lo, const uint32_t* vals,
                        const uint32_t* rdec, uint32_t* rec_dec, uint32_t rmask) {
  const GCfg& c = g->c;
  hipStream_t st = g->stream;
  RSF_HIP(hipMemsetAsync(g->seg_start, 0, c.n_loc * 4, st));
  RSF_HIP(hipMemsetAsync(g->seg_end, 0, c.n_loc * 4, st));
  if (n) {
    hipLaunchKernelGGL(segment_kernel, dim3(grid1(n)), dim3(256), 0, st, keys, n, lo, g->seg_start, g->seg_end, vals,
                       rdec, rec_dec, rmask);
  }
  return RSF_OK;
}

int rsf::zero_spans(rsf_gossip* g, uint32_t* const* p, const uint64_t* words, int n) {
  ZeroSpans z{};
  uint64_t most = 0;
  for (int k = 0; k < n && k < kZeroSpans; ++k) z.p[k] = p[k], z.words[k] = words[k], most = std::max(most, words[k]);
  hipLaunchKernelGGL(zero_spans_kernel, dim3((unsigned)std::min<uint64_t>(grid1(most), 2048)), dim3(256), 0, g->stream, z);
  RSF_HIP(hipGetLastError());
  return RSF_OK;
}

void rsf::accumulate(rsf_gossip* g, uint32_t from) {
  hipLaunchKernelGGL(accumulate_kernel, dim3(1), dim3(64), 0, g->stream, g->d_counters, from);
}

extern "C" {

int rsf_gossip_round(rsf_gossip* g, uint32_t round, const rsf_ml_event* ml, uint32_t n_ml, const rsf_action* acts,
                     uint32_t n_acts) {
  if (!g) return gerr("null context");
  if (g->c.n_loc != g->c.N) return gerr("sharded context: use round_begin / round_emit / round_merge");
  int rc = rsf_gossip_round_begin(g, round, ml, n_ml, acts, n_acts);
  if (rc) return rc;
  if ((rc = emit_and_sort(g, round, true))) return rc;
  g->merged_from_stage = true;
  g->merged_from_buckets = false;
  hipLaunchKernelGGL(accumulate_kernel, dim3(1), dim3(64), 0, g->stream, g->d_counters, (uint32_t)kCtrSent);
  return launch_merge(g, nullptr, true);
}

static size_t pp_bytes_per_pair(const GCfg& c) {
  return (size_t)c.vrow + (size_t)c.ebuf * 12 + (size_t)c.ebuf * c.slot_k * 8 + 32;
}

int rsf_gossip_push_pull_device(rsf_gossip* g, const rsf_pp_pair* pairs, uint64_t n, uint32_t flags) {
  if (!g || (n && !pairs)) return gerr("null argument");
  if (n == 0) return RSF_OK;
  const GCfg& c = g->c;
  RSF_HIP(hipSetDevice(g->device));
  if (n > g->pp_cap) {
    if (g->pp_buf) {
      RSF_HIP(hipStreamSynchronize(g->stream));
      hipFree(g->pp_buf);
    }
    g->pp_buf = nullptr;
    g->pp_cap = 0;
    int rc = rsf::dmalloc(&g->pp_buf, pp_bytes_per_pair(c) * n);
    if (rc) return rc;
    g->pp_cap = n;
  }
  // slab regions, each 16-byte aligned
  char* b = (char*)g->pp_buf;
  PPSlab sl;
  sl.view = (ViewS*)b;
  b += (size_t)c.vrow * n;
  sl.eb_keys = (uint64_t*)b;
  b += (size_t)c.ebuf * c.slot_k * 8 * n;
  sl.eb_ltime = (uint64_t*)b;
  b += (size_t)c.ebuf * 8 * n;
  sl.clocks = (uint64_t*)b;
  b += (size_t)32 * n;
  sl.eb_cnt = (uint32_t*)b;
  hipLaunchKernelGGL(pp_snapshot_kernel, dim3((unsigned)n), dim3(256), 0, g->stream, c, g->s, pairs, sl);
  hipLaunchKernelGGL(pp_merge_kernel, dim3(grid1(n, kWavesPerBlock)), dim3(kWave * kWavesPerBlock), 0, g->stream, c,
                     g->s, pairs, n, sl, flags);
  RSF_HIP(hipGetLastError());
  return RSF_OK;
}

int rsf_gossip_push_pull(rsf_gossip* g, const rsf_pp_pair* pairs, uint64_t n, uint32_t flags) {
  if (!g || (n && !pairs)) return gerr("null argument");
  if (n == 0) return RSF_OK;
  if (n > 0x7FFFFFFFull) return gerr("batch too large");
  const GCfg& c = g->c;
  std::vector<uint32_t> rs(n);
  for (uint64_t i = 0; i < n; ++i) {
    const rsf_pp_pair& x = pairs[i];
    if (x.receiver < c.lo || x.receiver >= c.lo + c.n_loc || x.sender < c.lo || x.sender >= c.lo + c.n_loc)
      return gerr("push/pull members must be in the shard");
    rs[i] = x.receiver;
  }
  std::sort(rs.begin(), rs.end());
  if (std::adjacent_find(rs.begin(), rs.end()) != rs.end()) return gerr("receivers of one push/pull batch must be distinct");
  RSF_HIP(hipSetDevice(g->device));
  size_t bytes[1] = {n * sizeof(rsf_pp_pair)};
  void* d[1];
  int rc = g->scratch.take(bytes, 1, d);
  if (rc) return rc;
  RSF_HIP(hipMemcpyAsync(d[0], pairs, bytes[0], hipMemcpyHostToDevice, g->stream));
  if ((rc = rsf_gossip_push_pull_device(g, (const rsf_pp_pair*)d[0], n, flags))) return rc;
  RSF_HIP(hipStreamSynchronize(g->stream));
  return RSF_OK;
}


// diagnostic only: device addresses of the context's main buffers and of a global in the
// library's code object (open issue: an address-dependent fault).  Order:
// view, p_ent, q_rumor, stage_val, stage_dec, grp_slot, grp_cnt, seg_start, rbody, rumors,
// rdec, clock, code-object global (0 without one), big_ids, sort_tmp, grp_tmp, d_counters,
// d_acts, grp_key, grp_key_s, grp_id, grp_id_s, grp_off, stage_key, sort_key, sort_val,
// send_buf, rec_dec, seg_end, p_cnt, err, member_subj.  Returns the count written.
int rsf_gossip_debug_ptrs(rsf_gossip* g, uint64_t* out, uint32_t n) {
  if (!g || !out) return gerr("null argument");
  const void* p[32] = {g->s.view, g->s.p_ent, g->s.q_rumor, g->stage_val, g->stage_dec, g->grp_slot, g->grp_cnt,
                       g->seg_start, g->s.rbody, g->s.rumors, g->s.rdec, g->s.clock, nullptr,
                       g->big_ids, g->sort_tmp.p, g->grp_tmp.p, g->d_counters, g->d_acts, g->grp_key, g->grp_key_s,
                       g->grp_id, g->grp_id_s, g->grp_off, g->stage_key, g->sort_key, g->sort_val, g->send_buf,
                       g->rec_dec, g->seg_end, g->s.p_cnt, g->s.err, g->s.member_subj};
#if RSF_MERGE_PROF || RSF_EMIT_PROF || RSF_CHECKS
  void* sym = nullptr;
  if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_merge_prof)) == hipSuccess) p[12] = sym;
#endif
  const uint32_t k = n < 32 ? n : 32;
  for (uint32_t i = 0; i < k; ++i) out[i] = (uint64_t)(uintptr_t)p[i];
  return (int)k;
}

// diagnostic only (experiments/deep_prof.py, builds with -DRSF_DEEP_PROF=1): reads and clears
// the deferral reasons, the deep wave kernel's phase totals and queue-size histogram (64 words);
// returns -1 in normal builds
int rsf_gossip_deep_prof(uint64_t* out64) {
#if RSF_DEEP_PROF
  RSF_HIP(hipDeviceSynchronize());
  RSF_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_deep_prof), 80 * sizeof(uint64_t)));
  unsigned long long z[80] = {};
  RSF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_deep_prof), z, sizeof(z)));
  return 0;
#else
  (void)out64;
  return -1;
#endif
}

// diagnostic only (experiments/merge_prof.py, builds with -DRSF_MERGE_PROF=1): reads and
// clears merge_kernel's per-phase shader-clock totals; returns -1 in normal builds
int rsf_gossip_merge_prof(uint64_t* out8) {
#if RSF_MERGE_PROF || RSF_EMIT_PROF || RSF_CHECKS
  RSF_HIP(hipDeviceSynchronize());
  RSF_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_merge_prof), 8 * sizeof(uint64_t)));
  unsigned long long z[8] = {};
  RSF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_merge_prof), z, sizeof(z)));
#if RSF_EMIT_PROF
  {
    std::vector<unsigned long long> w(512 * 8), zw(512 * 8, 0ull);
    RSF_HIP(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_eprof), w.size() * sizeof(unsigned long long)));
    RSF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_eprof), zw.data(), zw.size() * sizeof(unsigned long long)));
    for (int i = 0; i < 8; ++i) {
      out8[i] = 0;
      for (int r = 0; r < 512; ++r) out8[i] += w[r * 8 + i];
    }
    RSF_HIP(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_eprof2), w.size() * sizeof(unsigned long long)));
    RSF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_eprof2), zw.data(), zw.size() * sizeof(unsigned long long)));
    for (int i = 0; i < 5; ++i) {
      unsigned long long t = 0;
      for (int r = 0; r < 512; ++r) t += w[r * 8 + i];
      fprintf(stderr, "eprof2[%d] %llu\n", i, t);
    }
  }
#endif
  return RSF_OK;
#else
  (void)out8;
  return -1;
#endif
}


// one checker tick at the members whose global id is phase mod period (period 1: all), on
// the engine's stream; reset: the stats block and the occupancy histogram start from zero
static int check_launch(rsf_gossip* g, uint32_t max_queue_depth, uint32_t min_queue_depth, uint32_t depth_warning,
                        uint32_t period, uint32_t phase, bool reset) {
  hipStream_t rs = g->stream;
  const GCfg& c = g->c;
  // get_queue_max (base.rs:748-759): max_queue_depth, or (min_queue_depth > 0) per member
  // max(2 * members.states.len(), min_queue_depth) -- queue_max_kernel
  const uint32_t max_depth = max_queue_depth;
  RSF_HIP(hipSetDevice(g->device));
  int rc = flush_pending(g, period, phase);
  if (rc) return rc;
  if (min_queue_depth > 0) {
    if (!g->qmax && (rc = dmalloc((void**)&g->qmax, c.n_loc * 4))) return rc;
    hipLaunchKernelGGL(queue_max_kernel, dim3(grid1(std::max<uint64_t>(1, phase_count(c, period, phase)), 256 / kWave)),
                       dim3(256), 0, g->stream, c, g->s, min_queue_depth, g->qmax, period, phase);
    RSF_HIP(hipGetLastError());
  }
  const uint32_t* qmax = min_queue_depth > 0 ? g->qmax : nullptr;
  const size_t hist_words = kOccHistWords;
  if (!g->occ_hist) {
    if ((rc = dmalloc((void**)&g->occ_hist, hist_words * 4))) return rc;
    reset = true;
  }
  if (reset) {
    RSF_HIP(hipMemsetAsync(g->occ_hist, 0, hist_words * 4, rs));
    RSF_HIP(hipMemsetAsync(g->d_counters + kCtrCheckStats, 0, kCheckStatWords * 8, rs));
  }
  hipLaunchKernelGGL(check_queues_kernel,
                     dim3((unsigned)std::min<uint64_t>(1024, grid1(std::max<uint64_t>(1, phase_count(c, period, phase)),
                                                                   256 / kWave))),
                     dim3(256), 0, rs, c, g->s, max_depth, depth_warning, g->d_counters + kCtrCheckStats, qmax, g->occ_hist, period,
                     phase);
  RSF_HIP(hipGetLastError());
  if (c.deep) {  // the deep queues over the max: the smallest max keys of head and tail kept
    const uint64_t n_list = phase_count(c, period, phase) * deep_queues(c);
    hipLaunchKernelGGL(check_stream_kernel, dim3(g->deep_check_blocks), dim3(kDeepThreads), 0, rs, c, g->s, max_depth,
                       qmax, (uint32_t)n_list);
    RSF_HIP(hipGetLastError());
  }
  return RSF_OK;
}

// the in-round checker ticks (rsf_gossip_set_checker): after round `round`'s emission, before
// its merge.  (Run on a second stream beside the merge, the prune and the merge each took
// longer and the round did not shorten: the prune's blocks hold most of a CU's LDS.)
static int check_in_round(rsf_gossip* g, uint32_t round) {
  if (!g->chk_period) return RSF_OK;
  return check_launch(g, g->chk_max, g->chk_min, g->chk_warn, g->chk_period, round % g->chk_period, false);
}

int rsf_gossip_check_queues(rsf_gossip* g, uint32_t max_queue_depth, uint32_t min_queue_depth, uint32_t depth_warning,
                            uint64_t* num_queued, uint64_t* n_warn, uint64_t* n_pruned) {
  if (!g) return gerr("null context");
  int rc = check_launch(g, max_queue_depth, min_queue_depth, depth_warning, 1, 0, true);
  return rc ? rc : rsf_gossip_checker_stats(g, num_queued, n_warn, n_pruned, 0);
}

int rsf_gossip_check_queues_phase(rsf_gossip* g, uint32_t max_queue_depth, uint32_t min_queue_depth,
                                  uint32_t depth_warning, uint32_t period, uint32_t phase) {
  if (!g) return gerr("null context");
  if (!period || phase >= period) return gerr("phase must be below a non-zero period");
  return check_launch(g, max_queue_depth, min_queue_depth, depth_warning, period, phase, false);
}

}  // extern "C"
