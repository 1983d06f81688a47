// gossip_queue.h — the transmit-limited queues in registers, one slot per lane (queue_cap
// <= 64): load / store, insertion, expiry, re-ranking, get_broadcasts and the peer picks of
// the emission, the deep queues' spill into the HBM tail and its prune, and the pending
// re-queue lists.  The four-slots-per-lane layout (65..256) builds on this: gossip_queue4.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gossip_handlers.h"
#include "gossip_wave.h"

// why the emission deferred a member to the deep path: recorded only in the round unit's
// RSF_DEEP_PROF builds (gossip_diag.h, included before this header there)
#ifndef RSF_DEEP_WHY
#define RSF_DEEP_WHY(k) \
  do {                  \
  } while (0)
#endif

using namespace rsf;

namespace {

// record decoration (what merge_kernel needs to address the view entry before the rumor
// body arrives): the subject slot of an intent, or the queue of a query / user event
constexpr uint32_t kDecQuery = 0xFFFFFFFEu, kDecEvent = 0xFFFFFFFDu, kDecViewMax = 0xFFFFFFF0u;
// one transmit-limited queue held in registers: lane i owns slot i
struct QRegs {
  uint32_t r, sq, tl;  // rumor id (kEmpty = free), insertion seq, transmits | len << 16
  uint32_t dec = 0;    // emit only: the item's record decoration (subject / kDecQuery / kDecEvent)
};

#ifndef RSF_Q_NT
#define RSF_Q_NT 0  // broadcast queues (touched once by emit, once by merge per round) read / written non-temporally
#endif
// The intent queue also keeps each item's record decoration (its subject slot, q_dec);
// the query / event queues' decoration is the queue itself.
__device__ __forceinline__ void q_load(const GCfg& c, const GState& s, uint64_t l, uint32_t q, uint32_t lane,
                                       QRegs& Q) {
  Q.dec = q == 1 ? kDecQuery : kDecEvent;
  if (lane < c.qcap) {
    uint64_t i = (l * 3 + q) * c.qcap + lane;
#if RSF_Q_NT
    Q.r = __builtin_nontemporal_load(s.q_rumor + i);
    Q.sq = __builtin_nontemporal_load(s.q_seq + i);
    Q.tl = __builtin_nontemporal_load(s.q_txlen + i);
#else
    Q.r = s.q_rumor[i];
    Q.sq = s.q_seq[i];
    Q.tl = s.q_txlen[i];
#endif
    if (q == 0) Q.dec = s.q_dec[l * c.qcap + lane];
  } else {
    Q.r = kEmpty;
    Q.sq = 0;
    Q.tl = 0;
  }
}
__device__ __forceinline__ void q_store(const GCfg& c, const GState& s, uint64_t l, uint32_t q, uint32_t lane,
                                        const QRegs& Q, bool with_seq) {
  if (lane < c.qcap) {
    uint64_t i = (l * 3 + q) * c.qcap + lane;
#if RSF_Q_NT
    __builtin_nontemporal_store(Q.r, s.q_rumor + i);
    __builtin_nontemporal_store(Q.tl, s.q_txlen + i);
    if (with_seq) __builtin_nontemporal_store(Q.sq, s.q_seq + i);
#else
    s.q_rumor[i] = Q.r;
    s.q_txlen[i] = Q.tl;
    if (with_seq) s.q_seq[i] = Q.sq;
#endif
    if (q == 0) s.q_dec[l * c.qcap + lane] = Q.dec;
  }
}

// Queues are kept SORTED in send order: lane i of a queue holds the item with
// the i-th smallest key (transmits, ~len, ~seq); free slots (kEmpty) follow the
// live items.  The content is exactly the reference model's (first-free-slot /
// prune-the-last-item), only the slot order is canonical.

__device__ __forceinline__ uint64_t below_mask(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }
// popcount of m over the lanes below this one (v_mbcnt: two vector instructions, no mask build)
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// this lane's bit of a wave-uniform mask (the mask is used as the lane condition directly)
__device__ __forceinline__ bool lane_bit(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// popcount of m over the lanes above this one
__device__ __forceinline__ uint32_t mbcnt_above(uint64_t m) {
  return (uint32_t)__popcll(m) - mbcnt(m) - (lane_bit(m) ? 1u : 0u);
}

// insert: position = number of smaller live keys; lanes at/after it shift by
// one, so on a full queue the last lane (the largest key) falls off = memberlist
// Prune; a new item that would land past the end is itself the pruned one.
// Returns 1 when the queue was full (a live item, possibly the new one, was dropped).
__device__ __forceinline__ uint32_t q_insert_wave(const GCfg& c, QRegs& Q, uint32_t lane, uint32_t rid, uint32_t len,
                                                  uint32_t seq) {
  const bool valid = lane < c.qcap;
  const bool live = valid && Q.r != kEmpty;
  const uint64_t newkey = tlq_key(0, len, seq);
  const uint64_t k = live ? tlq_key(Q.tl & 0xFFFF, Q.tl >> 16, Q.sq) : ~0ull;
  const uint32_t full = (uint32_t)__popcll(ballot(live)) == c.qcap ? 1u : 0u;
  const uint32_t pos = (uint32_t)__popcll(ballot(live && k < newkey));
  if (pos >= c.qcap) return full;
  const int src = lane ? (int)lane - 1 : 0;
  const uint32_t pr = (uint32_t)__shfl((int)Q.r, src), ps = (uint32_t)__shfl((int)Q.sq, src),
                 pt = (uint32_t)__shfl((int)Q.tl, src);
  if (valid && lane > pos) {
    Q.r = pr;
    Q.sq = ps;
    Q.tl = pt;
  }
  if (lane == pos) {
    Q.r = rid;
    Q.sq = seq;
    Q.tl = len << 16;
  }
  return full;
}

// Batched insert of new items (transmits 0) into a sorted queue, equivalent to
// q_insert_wave on each of them in lane order (seq = seq0, seq0+1, ...):
// inserting into a bounded sorted queue and pruning the largest key keeps the
// qcap smallest keys of everything inserted so far, so the result is the qcap
// smallest of (queue items U new items).  Keys are distinct (seqs are unique).
//   existing item i (sorted lane i) lands at i + #(new keys below it);
//   new item j lands at #(existing keys below it) + #(new keys below it).
// One pass over the new items counts both, then every slot PULLS its item
// (ds_bpermute): slots taken by new items are marked in a 64-bit mask, the
// others take the existing items in order.  Returns the number of live items
// that did not fit (memberlist Prune of the queue's tail).
__device__ __forceinline__ uint32_t q_insert_batch(const GCfg& c, QRegs& Q, uint32_t lane, bool ins, uint32_t rid,
                                                   uint32_t len, uint32_t seq0, uint64_t newmask) {
  const bool valid = lane < c.qcap;
  const bool live = valid && Q.r != kEmpty;
  const uint32_t n_live = (uint32_t)__popcll(ballot(live));
  const uint32_t myseq = seq0 + mbcnt(newmask);
  const uint64_t nkey = ins ? tlq_key(0, len, myseq) : ~0ull;
  const uint64_t ekey = live ? tlq_key(Q.tl & 0xFFFF, Q.tl >> 16, Q.sq) : ~0ull;
  uint32_t n_rank = 0, e_less = 0;
  uint64_t mm = newmask;
  while (mm) {
    const int k = __ffsll((long long)mm) - 1;
    mm &= mm - 1;
    const uint64_t bk = shfl_u64(nkey, k);
    const bool eb = live && bk < ekey;
    n_rank += (ins && bk < nkey) ? 1u : 0u;
    const uint32_t el = n_live - (uint32_t)__popcll(ballot(eb));
    e_less = (int)lane == k ? el : e_less;
  }
  const uint32_t pos_n = e_less + n_rank;
  // destinations of the surviving new items and, per destination, its source lane
  uint64_t dm = 0;
  uint32_t srcn = 0;
  mm = ballot(ins && pos_n < c.qcap);
  while (mm) {
    const int k = __ffsll((long long)mm) - 1;
    mm &= mm - 1;
    const uint32_t d = shfl_u32(pos_n, k);
    dm |= 1ull << d;
    srcn = lane == d ? (uint32_t)k : srcn;
  }
  const bool is_new = lane_bit(dm);
  const uint32_t ei = lane - mbcnt(dm);
  const bool is_old = !is_new && valid && ei < n_live;
  const int a_new = (int)(srcn * 4), a_old = (int)((is_old ? ei : lane) * 4);
  const uint32_t nr = (uint32_t)__builtin_amdgcn_ds_bpermute(a_new, (int)rid);
  const uint32_t ns = (uint32_t)__builtin_amdgcn_ds_bpermute(a_new, (int)myseq);
  const uint32_t nl = (uint32_t)__builtin_amdgcn_ds_bpermute(a_new, (int)len);
  const uint32_t orr = (uint32_t)__builtin_amdgcn_ds_bpermute(a_old, (int)Q.r);
  const uint32_t os = (uint32_t)__builtin_amdgcn_ds_bpermute(a_old, (int)Q.sq);
  const uint32_t ot = (uint32_t)__builtin_amdgcn_ds_bpermute(a_old, (int)Q.tl);
  if (valid) {
    Q.r = is_new ? nr : (is_old ? orr : kEmpty);
    Q.sq = is_new ? ns : (is_old ? os : 0u);
    Q.tl = is_new ? (nl << 16) : (is_old ? ot : 0u);
  }
  const uint32_t total = n_live + (uint32_t)__popcll(newmask);
  return total > c.qcap ? total - c.qcap : 0u;
}

// Items whose rumor slot was recycled (the slot's generation is no longer the id's)
// expire: they are dropped and the survivors keep their sorted order at the front.
// Returns the number dropped (wave-uniform).
__device__ __forceinline__ uint32_t q_expire(const GCfg& c, QRegs& Q, uint32_t lane, bool stale, bool permute_dec) {
  const bool valid = lane < c.qcap;
  const bool live = valid && Q.r != kEmpty;
  const uint64_t sm = ballot(live && stale);
  if (!sm) return 0;
  const bool keep = live && !stale;
  const uint64_t km = ballot(keep), vm = ballot(valid);
  const uint32_t mb_k = mbcnt(km), mb_f = mbcnt(vm & ~km);
  const uint32_t pos = keep ? mb_k : (valid ? (uint32_t)__popcll(km) + mb_f : lane);
  if (valid && !keep) {
    Q.r = kEmpty;
    Q.sq = 0;
    Q.tl = 0;
  }
  const int addr = (int)(pos * 4);
  Q.r = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.r);
  Q.sq = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.sq);
  Q.tl = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.tl);
  if (permute_dec) Q.dec = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.dec);
  return (uint32_t)__popcll(sm);
}

// One LDS row per wave: scratch of the batched insert (q_insert_batch_lds) and of the
// re-rank after a pick (q_get_broadcasts).
struct alignas(16) QLds {
  uint32_t r[kWave], sq[kWave], tl[kWave], dec[kWave];
};

// Re-rank after picks: the unpicked keepers (np_m) and the bumped keepers (pk_m) are each
// still sorted in lane order; merge them, free lanes after.  Each list's keys go to the
// wave's LDS row in order, and every keeper counts the other list's keys below its own by a
// binary search there (keys are distinct), all lanes at once: a handful of LDS reads
// instead of a wave-wide pass per bumped item.
template <bool PERMUTE_DEC>
__device__ __forceinline__ void q_rerank(const GCfg& c, QRegs& Q, uint32_t lane, uint64_t pk_m, uint64_t np_m,
                                         QLds& row) {
  const bool valid = lane < c.qcap;
  const uint64_t kept_m = pk_m | np_m;
  const bool np = lane_bit(np_m), kept = lane_bit(kept_m);
  const uint64_t mykey = tlq_key(Q.tl & 0xFFFF, Q.tl >> 16, Q.sq);
  uint64_t* const keys_np = reinterpret_cast<uint64_t*>(row.r);  // r + sq: 64 keys
  uint64_t* const keys_pk = reinterpret_cast<uint64_t*>(row.tl);  // tl + dec: 64 keys
  // (mbcnt is convergent: computed outside any select arm, or the select becomes a branch)
  const uint32_t mb_np = mbcnt(np_m), mb_pk = mbcnt(pk_m), mb_free = mbcnt(~kept_m);
  const uint32_t r_own = np ? mb_np : mb_pk;
  // both lists padded with keys above every real one (LDS writes of a wave land in order, so
  // the real keys overwrite the padding): the search needs no bounds test
  keys_np[lane] = ~0ull;
  keys_pk[lane] = ~0ull;
  if (kept) (np ? keys_np : keys_pk)[r_own] = mykey;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // lower_bound of mykey in the other list, branchless: a keeper's other list holds at most 63
  // keys (both lists share the wave's 64 lanes), so steps 32 .. 1 reach every count, and the
  // probes stay inside the 64-key row
  const uint64_t* const other = np ? keys_pk : keys_np;
  const uint32_t n_pk = (uint32_t)__popcll(pk_m), n_np = (uint32_t)__popcll(np_m);
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = 32; step; step >>= 1) lo = other[lo + step - 1] < mykey ? lo + step : lo;
  const uint32_t pos_free = valid ? n_pk + n_np + mb_free : lane;
  const uint32_t pos = kept ? r_own + lo : pos_free;
  __builtin_amdgcn_wave_barrier();  // the row is free once every lane has searched it
  const int addr = (int)(pos * 4);
  Q.r = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.r);
  Q.sq = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.sq);
  Q.tl = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.tl);
  if (PERMUTE_DEC) Q.dec = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)Q.dec);
}

// one get_broadcasts call on a sorted register-resident queue; returns bytes used.
// The lowest unpicked lane that fits IS the reference's pick (lowest transmits, then
// longest fitting, then newest): every skipped lower lane did not fit and never will.
// Written over wave-uniform lane masks (live, picked, kept): the selection loops are
// scalar work on one 64-bit mask instead of per-lane flags under exec masking.
#ifndef RSF_EMIT_NT
#define RSF_EMIT_NT 0  // emit: records written non-temporally
#endif
// DEEP (a tail behind the head, its key / length lower bounds tmin / tminlen): the call is
// exact only if every pick's key is below tmin and every stop with budget left is one no tail
// item could fit; otherwise *unsafe is set and the caller abandons the emission (the member
// then takes emit_deep_wave_kernel's whole-queue path).  Picks are checked before they are bumped.
template <bool PERMUTE_DEC, bool DEEP = false>
__device__ __forceinline__ int64_t q_get_broadcasts(const GCfg& c, QRegs& Q, uint32_t lane, int64_t limit,
                                                    uint32_t* stage_val, uint32_t* stage_dec,
                                                    uint64_t out_base, uint32_t& nrec, uint32_t& err, bool& dirty,
                                                    QLds& row, uint64_t tmin = ~0ull, uint32_t tminlen = ~0u,
                                                    bool* unsafe = nullptr) {
  const bool valid = lane < c.qcap;
  const uint64_t live_m = ballot(valid && Q.r != kEmpty);  // a sorted queue: a prefix
  if (!live_m) {
    if (DEEP && tmin != ~0ull && limit - (int64_t)c.overhead >= (int64_t)tminlen) {
      *unsafe = true;
      RSF_DEEP_WHY(3);
    }
    return 0;
  }
  const bool live = lane_bit(live_m);
  const uint32_t len = Q.tl >> 16;
  // Live items are the sorted prefix.  If every earlier item was taken, item i fits iff
  // the inclusive prefix sum of (overhead + len) is <= limit, so the leading run of picks
  // comes out of one wave scan; the remaining budget is then offered to later (shorter)
  // items one by one, as the reference does.
  if (limit < 0) return 0;
  const uint32_t lim = (uint32_t)limit;  // 32-bit budget arithmetic below (used <= lim)
  const uint32_t incl = wave_inclusive_sum_u32(live ? c.overhead + len : 0u);
  uint64_t pick_m = ballot(incl <= lim) & live_m;
  uint32_t used = pick_m ? shfl_u32(incl, 63 - __clzll((long long)pick_m)) : 0u;
  for (;;) {
    const int32_t free_b = (int32_t)(lim - used - c.overhead);
    if (free_b <= 0) break;
    const uint64_t cand = ballot(len <= (uint32_t)free_b) & live_m & ~pick_m;
    if (!cand) {
      if (DEEP && tminlen <= (uint32_t)free_b) {  // a tail item might fit
        *unsafe = true;
        RSF_DEEP_WHY(4);
      }
      break;
    }
    const int win = __ffsll((long long)cand) - 1;
    pick_m |= 1ull << win;
    used += c.overhead + shfl_u32(len, win);
  }
  if (DEEP && pick_m) {  // the largest pick (the highest lane: the head is sorted) below the tail
    const int hl = 63 - __clzll((long long)pick_m);
    const uint32_t tl = shfl_u32(Q.tl, hl);
    if (tlq_key(tl & 0xFFFF, tl >> 16, shfl_u32(Q.sq, hl)) >= tmin) {
      *unsafe = true;
      RSF_DEEP_WHY(5);
#if RSF_DEEP_PROF
      {  // diagnostic: is the first pick past the tail bound in the leading run (24) or a later
         // fit (25); would "no tail item fits the budget left before it" have decided it (26)
        const uint64_t below = ballot(live && tlq_key(Q.tl & 0xFFFF, Q.tl >> 16, Q.sq) < tmin);
        const uint64_t cross = pick_m & ~below;
        const int fc = __ffsll((long long)cross) - 1;
        const uint64_t before = fc > 0 ? (~0ull >> (64 - fc)) : 0ull;
        RSF_DEEP_WHY((pick_m & before) == before ? 24 : 25);
        RSF_DEEP_WHY((shfl_u32(Q.tl, fc) & 0xFFFF) == 0 ? 27 : 28);  // the crossing pick's transmit class
        if ((tmin >> 48) == 0) RSF_DEEP_WHY(7);  // the tail's bound is a transmits-0 key
        const uint32_t ub = wave_inclusive_sum_u32(lane_bit(pick_m & before) ? c.overhead + len : 0u);
        const int32_t f0 = (int32_t)lim - (int32_t)shfl_u32(ub, 63) - (int32_t)c.overhead;
        if (f0 < (int32_t)tminlen) RSF_DEEP_WHY(26);
      }
#endif
    }
  }
  if (DEEP && *unsafe) return used;
  if (!pick_m) return used;
  // picks are in ascending lane (= send) order: record rank = picked lanes below
  const bool picked = lane_bit(pick_m);
  const uint32_t npick = (uint32_t)__popcll(pick_m);
  const uint32_t rank = mbcnt(pick_m);
  if (picked && nrec + rank < c.cap_t && stage_val) {
#if RSF_EMIT_NT
    __builtin_nontemporal_store(Q.r, stage_val + out_base + nrec + rank);
    if (stage_dec) __builtin_nontemporal_store(Q.dec, stage_dec + out_base + nrec + rank);
#else
    stage_val[out_base + nrec + rank] = Q.r;
    if (stage_dec) stage_dec[out_base + nrec + rank] = Q.dec;
#endif
  }
  if (nrec + npick > c.cap_t) err |= kErrStage;
  nrec += npick;
  dirty = true;
  // transmits+1, or retire at the retransmit limit
  const bool retire = picked && (Q.tl & 0xFFFF) + 1 >= c.tx_limit;
  const uint64_t ret_m = ballot(retire);
  Q.r = retire ? kEmpty : Q.r;
  Q.tl = (picked && !retire) ? Q.tl + 1 : Q.tl;
  q_rerank<PERMUTE_DEC>(c, Q, lane, pick_m & ~ret_m, live_m & ~pick_m, row);
  return used;
}

// All the fanout peers' get_broadcasts calls on ONE queue in one pass (queue-major emission).
// A peer's picks from queue q depend only on q's state after the earlier peers' picks from q
// and on what the peer's earlier queues left of its byte budget, so running queue 0 for every
// peer, then queue 1, then queue 2 picks exactly what the reference's peer-major
// broadcast_messages loop picks.  Within a queue, for every peer: while all picks come from the queue's lowest transmit class t0 (the leading run
// of the sorted queue), the send order is [unpicked class-t0 items in lane order] followed by
// everything else, so ONE prefix sum of the run's costs serves every peer (each peer's prefix
// is a further stretch of the same sums), the picked items are bumped in place and the re-rank
// runs once at the end.  Picks are recorded per lane (peer, slot in the peer's group) and
// written together after the last peer.  When a peer's next candidate could lie past the run,
// the deferred picks are written and re-ranked into place and the remaining peers run the
// exact q_get_broadcasts one by one.
// Per-peer state is lane-distributed: lane j (< np) holds peer j's bytes used so far (used_v),
// records written so far (nrec_v) and the element offset of its group's record slots from
// ov / od (off_v; ~0 = no output: a bucket over capacity).
// DEEP: as q_get_broadcasts -- abandoned (*unsafe) as soon as the head alone cannot decide.
template <bool PERMUTE_DEC, bool DEEP = false>
__device__ __forceinline__ void q_pick_peers(const GCfg& c, QRegs& Q, uint32_t lane, uint32_t np, uint32_t& used_v,
                                             uint32_t& nrec_v, uint64_t off_v, uint32_t* ov, uint32_t* od,
                                             uint32_t& err, bool& dirty, QLds& row, uint64_t* ep = nullptr,
                                             uint64_t tmin = ~0ull, uint32_t tminlen = ~0u, bool* unsafe = nullptr) {
  const bool valid = lane < c.qcap;
  const uint64_t live_m = ballot(valid && Q.r != kEmpty);  // a sorted queue: a prefix
  if (!live_m) {
    if (DEEP && tmin != ~0ull) {  // only the tail holds items
      *unsafe = true;
      RSF_DEEP_WHY(0);
    }
    return;
  }
#if RSF_EMIT_PROF
  const uint64_t pp0 = __builtin_amdgcn_s_memtime();
#endif
  const uint32_t t0 = shfl_u32(Q.tl, 0) & 0xFFFF;  // lane 0 holds the smallest key
  const uint32_t len = Q.tl >> 16;
  const uint64_t a_m = ballot((Q.tl & 0xFFFF) == t0) & live_m;
  const bool retire_all = t0 + 1 >= c.tx_limit;  // every pick of class t0 retires (or none does)
  uint32_t incl = wave_inclusive_sum_u32(lane_bit(a_m) ? c.overhead + len : 0u);
  uint32_t base = 0;      // the sums consumed by the picks so far (while they are a prefix of the run)
  bool prefix = true;     // the picks so far are a prefix of the class-t0 run
  uint64_t cons = 0;      // picked so far (all of class t0), bumped in place, not yet written
  uint64_t gone = 0;      // picked and retiring: no longer candidates
  uint32_t pk_peer = 0, pk_pos = 0;  // a picked lane: its peer and its slot in the peer's group
  uint32_t j = 0;
  bool exact = false;
  for (; j < np; ++j) {
    // 32-bit budget arithmetic (a peer's bytes used never exceed the limit): scalar 32-bit
    // operations instead of 64-bit pairs in the loop the emission spends most of its scalar
    // issue on
    const uint32_t limit = c.limit - shfl_u32(used_v, j);
    const uint64_t rem = a_m & ~cons;
    if (!prefix) {  // a skip broke the run's prefix: sums of what is left of it
      incl = wave_inclusive_sum_u32(lane_bit(rem) ? c.overhead + len : 0u);
      base = 0;
      prefix = true;
    }
    // (lanes before the consumed prefix wrap to huge sums and fail the compare; masked anyway)
    uint64_t pick = ballot(incl - base <= limit) & rem;
    const uint32_t top = pick ? shfl_u32(incl, 63 - __clzll((long long)pick)) : base;
    uint32_t used = top - base;
    bool skipped = false;
    const uint64_t avail = live_m & ~gone;
    for (;;) {
      const int32_t free_b = (int32_t)(limit - used - c.overhead);
      if (free_b <= 0) break;
      const uint64_t fit = ballot(len <= (uint32_t)free_b) & avail & ~pick;
      if (!fit) {
        if (DEEP && tminlen <= (uint32_t)free_b) {  // a tail item might fit
          *unsafe = true;
          RSF_DEEP_WHY(1);
        }
        break;
      }
      const uint64_t cand = fit & rem;
      if (!cand) {  // the next candidate lies past the class-t0 run (or is a bumped pick)
        exact = true;
        break;
      }
      const int win = __ffsll((long long)cand) - 1;
      pick |= 1ull << win;
      used += c.overhead + shfl_u32(len, win);
      skipped = true;
    }
    if (exact) break;
    if (DEEP && *unsafe) return;
    if (pick) {
      const uint32_t npick = (uint32_t)__popcll(pick);
      const uint32_t nrec = shfl_u32(nrec_v, j);
      const bool pb = lane_bit(pick);
      const uint32_t mb = mbcnt(pick);
      pk_peer = pb ? j : pk_peer;
      pk_pos = pb ? nrec + mb : pk_pos;  // picks in ascending lane (= send) order
      if (nrec + npick > c.cap_t) err |= kErrStage;
      nrec_v = lane == j ? nrec + npick : nrec_v;
      cons |= pick;
      if (retire_all) gone |= pick;
      dirty = true;
      if (skipped) prefix = false;
      else base = top;
    }
    used_v += lane == j ? used : 0u;
  }
#if RSF_EMIT_PROF
  const uint64_t pp1 = __builtin_amdgcn_s_memtime();
  ep[0] += pp1 - pp0;  // picks (prefix sums, fit loops)
  if (exact) ep[4] += 1;  // emissions that needed the exact path
#endif
  if (DEEP && cons) {  // the largest deferred pick (highest lane) below the tail
    const int hl = 63 - __clzll((long long)cons);
    const uint32_t tl = shfl_u32(Q.tl, hl);
    if (tlq_key(tl & 0xFFFF, tl >> 16, shfl_u32(Q.sq, hl)) >= tmin) {
      *unsafe = true;
      RSF_DEEP_WHY(2);
      RSF_DEEP_WHY((tl & 0xFFFF) == 0 ? 27 : 28);  // (diagnostic) the crossing pick's transmit class
      return;
    }
  }
  if (cons) {
    // the deferred picks: records to their groups, then transmits + 1 or retired
    const bool picked = lane_bit(cons);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)off_v, (int)pk_peer);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(off_v >> 32), (int)pk_peer);
    const uint64_t off = ((uint64_t)hi << 32) | lo;
    if (picked && pk_pos < c.cap_t && off != ~0ull) {
#if RSF_EMIT_NT
      __builtin_nontemporal_store(Q.r, ov + off + pk_pos);
      if (od) __builtin_nontemporal_store(Q.dec, od + off + pk_pos);
#else
      ov[off + pk_pos] = Q.r;
      if (od) od[off + pk_pos] = Q.dec;
#endif
    }
    Q.r = (picked && retire_all) ? kEmpty : Q.r;
    Q.tl = (picked && !retire_all) ? Q.tl + 1 : Q.tl;
#if RSF_EMIT_PROF
    const uint64_t pp2 = __builtin_amdgcn_s_memtime();
    ep[1] += pp2 - pp1;  // deferred stores + bumps
#endif
    q_rerank<PERMUTE_DEC>(c, Q, lane, cons & ~gone, live_m & ~cons, row);
#if RSF_EMIT_PROF
    ep[2] += __builtin_amdgcn_s_memtime() - pp2;  // re-rank
#endif
  }
#if RSF_EMIT_PROF
  const uint64_t pp3 = __builtin_amdgcn_s_memtime();
#endif
  // the remaining peers exactly, one re-rank after each
  for (; j < np; ++j) {
    const int64_t limit = (int64_t)c.limit - (int64_t)shfl_u32(used_v, j);
    uint32_t nrec = shfl_u32(nrec_v, j);
    const uint64_t off = shfl_u64(off_v, j);
    const bool out = off != ~0ull;
    const int64_t used = q_get_broadcasts<PERMUTE_DEC, DEEP>(c, Q, lane, limit, out ? ov : nullptr, out ? od : nullptr,
                                                             out ? off : 0ull, nrec, err, dirty, row, tmin, tminlen,
                                                             unsafe);
    if (DEEP && *unsafe) return;
    used_v += lane == j ? (uint32_t)used : 0u;
    nrec_v = lane == j ? nrec : nrec_v;
  }
#if RSF_EMIT_PROF
  ep[3] += __builtin_amdgcn_s_memtime() - pp3;  // exact tail
#endif
}

// Deep queues: the running tail of one (member, queue) while a wave works on its head.  cnt,
// minlen, minkey mirror tsum (wave-uniform); spills are written at t[cnt ...] (the row has
// kTailSlack slots past the capacity) and counted in only by the caller's commit.
struct Spill {
  uint4* t = nullptr;      // the query / event queues' 16-B items
  uint64_t* t8 = nullptr;  // the intent queue's packed items (tail_pack)
  uint32_t cnt = 0, minlen = 0xFFFFFFFFu;
  uint64_t minkey = ~0ull;
};
__device__ __forceinline__ void spill_row(const GCfg& c, const GState& s, uint64_t l, uint32_t q, Spill& sp) {
  if (q == 0) sp.t8 = tail8(s, c, l);
  else sp.t = tail16(s, q) + l * tstride_of(c, q);
}
__device__ __forceinline__ void spill_put(const GCfg& c, const Spill& sp, uint32_t i, uint32_t rid, uint32_t seq,
                                          uint32_t tl, uint32_t dec) {
  if (sp.t8) sp.t8[i] = tail_pack(c, rid, seq, tl);
  else sp.t[i] = make_uint4(rid, seq, tl, dec);
}
__device__ __forceinline__ Spill spill_of(const GCfg& c, const GState& s, uint64_t l, uint32_t q, uint4 sm) {
  Spill sp;
  spill_row(c, s, l, q, sp);
  sp.cnt = sm.x;
  sp.minlen = sm.y;
  sp.minkey = ((uint64_t)sm.w << 32) | sm.z;
  return sp;
}
__device__ __forceinline__ uint4 spill_sum(const Spill& sp) {
  return make_uint4(sp.cnt, sp.minlen, (uint32_t)sp.minkey, (uint32_t)(sp.minkey >> 32));
}
constexpr uint4 kTSumEmpty = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};

// Batched insert of new items (transmits 0, seqs seq0, seq0 + 1, ... in lane order over
// `newmask`) into a sorted register-resident queue: the result is the qcap smallest keys of
// (queue items U new items), exactly memberlist's insert-then-prune one at a time.  Done
// over the DISTINCT LENGTHS of the new items instead of the items.  New items all have
// transmits 0 and newer seqs than anything queued, so:
//   new j lands at  #{queued: tx 0, len > len_j} + #{new: len > len_j} + #{new: len == len_j, later lane}
//   queued i (lane i) lands at  i + (tx_i > 0 ? n_new : #{new: len >= len_i})
// -- one pass per distinct new length (the message-length model has a handful), then
// every item is written to its place in the wave's LDS row and read back in order.
// DEC: the items' record decorations (Q.dec / dec) move with them.
// Returns the number of live items that did not fit (memberlist Prune of the tail).
// SPILL (deep queues): the items that do not fit the head go to the tail instead (sp), and
// the return value is 0; the caller checks the tail's capacity.
template <bool DEC, bool SPILL = false>
__device__ __forceinline__ uint32_t q_insert_batch_lds(const GCfg& c, QRegs& Q, uint32_t lane, bool ins, uint32_t rid,
                                                       uint32_t dec, uint32_t len, uint32_t seq0, uint64_t newmask,
                                                       QLds& row, Spill* sp = nullptr) {
  const bool valid = lane < c.qcap;
  const uint64_t live_m = ballot(valid && Q.r != kEmpty);
  const bool live = lane_bit(live_m);
  const uint32_t n_live = (uint32_t)__popcll(live_m);
  const uint32_t n_new = (uint32_t)__popcll(newmask);
  const uint32_t myseq = seq0 + mbcnt(newmask);
  const uint64_t etx0_m = ballot((Q.tl & 0xFFFF) == 0) & live_m;  // queued items of transmits 0
  const uint32_t elen = Q.tl >> 16;
  uint32_t pos_n = 0, pos_e = lane + (lane_bit(live_m & ~etx0_m) ? n_new : 0u);
  // one pass per distinct new length, over wave-uniform masks (ins == this lane's bit of newmask)
  uint64_t rem = newmask;
  while (rem) {
    const uint32_t L = shfl_u32(len, __ffsll((long long)rem) - 1);
    const uint64_t same = ballot(len == L) & newmask;
    rem &= ~same;
    const uint64_t gt_old_m = ballot(elen > L) & etx0_m;
    const uint32_t base = (uint32_t)__popcll(ballot(len > L) & newmask) + (uint32_t)__popcll(gt_old_m);
    const uint32_t ab = mbcnt_above(same);
    pos_n = lane_bit(same) ? base + ab : pos_n;
    pos_e += lane_bit(etx0_m & ~gt_old_m) ? (uint32_t)__popcll(same) : 0u;
  }
  if (SPILL && n_live + n_new > c.qcap) {
    // positions past the head are the largest keys, in order: they go to the tail, the one at
    // position qcap being the smallest of them
    const bool sn = ins && pos_n >= c.qcap, se = live && pos_e >= c.qcap;
    // (ordinary stores: non-temporal ones measured 1.37 -> 2.24 ms of emission, later spills
    // landing in the same partly written sectors)
    if (sn) spill_put(c, *sp, sp->cnt + (pos_n - c.qcap), rid, myseq, len << 16, DEC ? dec : 0u);
    if (se) spill_put(c, *sp, sp->cnt + (pos_e - c.qcap), Q.r, Q.sq, Q.tl, DEC ? Q.dec : 0u);
    const uint64_t at_n = ballot(ins && pos_n == c.qcap), at_e = ballot(live && pos_e == c.qcap);
    const int w = __ffsll((long long)(at_n | at_e)) - 1;
    const uint32_t tl_w = at_n ? (shfl_u32(len, w) << 16) : shfl_u32(Q.tl, w);
    const uint32_t sq_w = at_n ? shfl_u32(myseq, w) : shfl_u32(Q.sq, w);
    const uint64_t kmin = tlq_key(tl_w & 0xFFFF, tl_w >> 16, sq_w);
    const uint32_t lmin = wave_min_u32(min(sn ? len : 0xFFFFFFFFu, se ? elen : 0xFFFFFFFFu));
    sp->cnt += n_live + n_new - c.qcap;
    sp->minkey = kmin < sp->minkey ? kmin : sp->minkey;
    sp->minlen = lmin < sp->minlen ? lmin : sp->minlen;
  }
  if (ins && pos_n < c.qcap) {
    row.r[pos_n] = rid;
    row.sq[pos_n] = myseq;
    row.tl[pos_n] = len << 16;
    if (DEC) row.dec[pos_n] = dec;
  }
  if (live && pos_e < c.qcap) {
    row.r[pos_e] = Q.r;
    row.sq[pos_e] = Q.sq;
    row.tl[pos_e] = Q.tl;
    if (DEC) row.dec[pos_e] = Q.dec;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t total = n_live + n_new;
  {
    // every lane reads its slot; lanes past the items (or the queue) select the free value
    const bool take = valid && lane < total;
    const uint32_t r = row.r[lane], sq = row.sq[lane], tl = row.tl[lane];
    const uint32_t fr = valid ? kEmpty : Q.r, fs = valid ? 0u : Q.sq, ft = valid ? 0u : Q.tl;
    Q.r = take ? r : fr;
    Q.sq = take ? sq : fs;
    Q.tl = take ? tl : ft;
    if (DEC) {
      const uint32_t d = row.dec[lane];
      Q.dec = take ? d : Q.dec;
    }
  }
  __builtin_amdgcn_wave_barrier();  // the row is free once every lane has read it
  return (!SPILL && total > c.qcap) ? total - c.qcap : 0u;
}

// A member's pending re-queues (pc: their packed counts, which the caller may hold in
// registers) applied to its queues by one wave (lane = slot / entry):
// per queue, its entries in insertion order take the next seqs and go in as one batch.
// Adds the live items dropped to q_pruned and returns their number (the caller flags
// kErrQueue).  merge_kernel calls it only when a list would overflow.
// The entries of one queue from the wave's two batches of the list (lanes 0..63 hold
// entries lane and 64 + lane) go in as one batch after the other, seqs continuing.
struct PendRegs {
  uint32_t rid[2], dec[2], lq[2];
};
__device__ __forceinline__ void pend_load(const GState& s, uint64_t l, uint32_t lane, uint32_t n, PendRegs& p) {
#pragma unroll
  for (uint32_t b = 0; b < 2; ++b) {
    p.rid[b] = p.dec[b] = p.lq[b] = 0;
    if (b * kWave + lane < n) {
      const GState::PendE e = s.p_ent[l * kPend + b * kWave + lane];
      p.rid[b] = e.rid;
      p.dec[b] = e.dec;
      p.lq[b] = e.lq;
    }
  }
}
template <bool DEC, bool SPILL = false>
__device__ __forceinline__ uint32_t pend_apply(const GCfg& c, QRegs& Q, uint32_t lane, uint32_t q, uint32_t n,
                                               const PendRegs& p, uint32_t seq0, QLds& row, Spill* sp = nullptr) {
  uint32_t drops = 0, seq = seq0;
#pragma unroll
  for (uint32_t b = 0; b < 2; ++b) {
    if (b * kWave >= n) break;
    const bool ins = b * kWave + lane < n && (p.lq[b] >> 16) == q;
    const uint64_t m = ballot(ins);
    if (!m) continue;
    drops += q_insert_batch_lds<DEC, SPILL>(c, Q, lane, ins, p.rid[b], p.dec[b], p.lq[b] & 0xFFFF, seq, m, row, sp);
    seq += (uint32_t)__popcll(m);
  }
  return drops;
}

// Deep queues: while the tail holds more than its capacity (head + tail over the queue's
// depth), drop the largest key of the two -- the bounded queue's prune, rare (a queue at its
// full depth).  That key is always in the tail: the tail only goes past its capacity by this
// call's spills, and a spilled item is, by construction, at least every key left in the
// head (the items whose sorted position among head and new items is >= queue_cap).  So one
// pass over the tail finds it.  One wave; returns the number dropped.
// nseq: the queue's next seq after the spills (every tail item is older)
__device__ __forceinline__ uint32_t deep_prune_wave(const GCfg& c, QRegs& Q, uint32_t lane, uint32_t q, Spill& sp,
                                                    uint32_t nseq) {
  (void)Q;
  uint32_t drops = 0;
  while (sp.cnt > tcap_of(c, q)) {
    uint64_t tk = 0;
    uint32_t ti = 0;
    for (uint32_t b = 0; b < sp.cnt; b += kWave) {  // the tail holds items (cnt > tcap >= 1)
      const bool in = b + lane < sp.cnt;
      uint64_t k = 0ull;
      if (sp.t8) {
        const uint64_t x = in ? sp.t8[b + lane] : 0ull;
        const uint32_t tl = tail_tl(x);
        k = in ? tlq_key(tl & 0xFFFF, tl >> 16, tail_seq(x, nseq)) : 0ull;
      } else {
        const uint4 e = in ? sp.t[b + lane] : make_uint4(0u, 0u, 0u, 0u);
        k = in ? tlq_key(e.z & 0xFFFF, e.z >> 16, e.y) : 0ull;
      }
      const uint64_t m = wave_max_u64(k);
      const uint64_t at = ballot(in && k == m);
      if (at && (b == 0 || m > tk)) {
        tk = m;
        ti = b + (uint32_t)(__ffsll((long long)at) - 1);
      }
    }
    if (sp.t8) {
      const uint64_t last = sp.t8[sp.cnt - 1];
      if (lane == 0) sp.t8[ti] = last;
    } else {
      const uint4 last = sp.t[sp.cnt - 1];
      if (lane == 0) sp.t[ti] = last;
    }
    __threadfence_block();  // the next pass reads the moved item
    sp.cnt--;
    drops++;
  }
  return drops;
}

__device__ __forceinline__ uint32_t pend_flush_wave(const GCfg& c, const GState& s, uint64_t l, uint32_t lane,
                                                    uint32_t pc, QLds& row) {
  const uint32_t n = pend_total(pc);
  if (n == 0) return 0;
  PendRegs p;
  pend_load(s, l, lane, n, p);
  uint32_t drops = 0;
#pragma unroll
  for (uint32_t q = 0; q < 3; ++q) {
    const uint32_t nq = (pc >> (8 * q)) & 0xFF;
    if (!nq) continue;
    QRegs Q{kEmpty, 0, 0};
    q_load(c, s, l, q, lane, Q);
    const uint32_t seq0 = s.q_next_seq[l * 3 + q];
    if (tcap_of(c, q)) {  // deep queue: the head's overflow spills into the tail
      Spill sp = spill_of(c, s, l, q, s.tsum[l * 3 + q]);
      pend_apply<true, true>(c, Q, lane, q, n, p, seq0, row, &sp);
      const uint32_t pd = deep_prune_wave(c, Q, lane, q, sp, seq0 + nq);
      drops += pd;
      if (lane == 0) {
        s.tsum[l * 3 + q] = spill_sum(sp);
        if (pd) s.tseal[l * 3 + q].x = 0u;  // the prune moved items inside the tail: no seal
      }
    } else {
      drops += pend_apply<true>(c, Q, lane, q, n, p, seq0, row);
    }
    q_store(c, s, l, q, lane, Q, true);
    if (lane == 0) s.q_next_seq[l * 3 + q] = seq0 + nq;
  }
  if (lane == 0) {
    s.p_cnt[l] = 0;
    if (drops) s.q_pruned[l] += drops;
  }
  return drops;
}

// period > 1: only the members whose global id is phase mod period (a staggered checker tick);
// the grids run over those members only: local ids phase_first + i * period
__host__ __device__ inline uint64_t phase_first(const GCfg& c, uint32_t period, uint32_t phase) {
  return (phase + period - (uint32_t)(c.lo % period)) % period;
}
__host__ __device__ inline uint64_t phase_count(const GCfg& c, uint32_t period, uint32_t phase) {
  const uint64_t l0 = phase_first(c, period, phase);
  return c.n_loc > l0 ? (c.n_loc - l0 + period - 1) / period : 0;
}

}  // namespace
