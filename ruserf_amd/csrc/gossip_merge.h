// gossip_merge.h — one receiver's merge (merge_one) and its setup: the body of merge_kernel and
// merge_big_kernel (and push_refute, which the originating and push/pull kernels share with it).  Part of the round unit (gossip.hip defines the kernels; the range guards
// and the phase profile here write the diagnostics globals of gossip_diag.h).
#pragma once
#include "gossip_ctx.h"
#include "gossip_diag.h"
#include "gossip_queue4.h"

namespace {

// a refutation spawned by a handler: broadcast by refute_kernel next round
__device__ __forceinline__ void push_refute(const GCfg& c, const GState& s, MRegs& r, uint64_t ltime) {
  if (r.subj < 0) return;
  if (RSF_BAD2(11, (uint32_t)r.subj >= c.S, r.subj)) return;
  uint32_t cnt = s.refute_cnt[r.subj];
  if (cnt < c.max_refute) {
    s.refute_ltime[(uint64_t)r.subj * c.max_refute + cnt] = ltime;
    s.refute_cnt[r.subj] = cnt + 1;
  } else {
    r.err |= kErrRefute;
  }
}

__device__ __forceinline__ rsf_rumor rumor_from_body(uint4 b, uint64_t key) {
  rsf_rumor ru;
  ru.ltime = ((uint64_t)b.y << 32) | b.x;
  ru.key = key;
  ru.subject = b.z;
  ru.type = (uint8_t)(b.w & 0xFF);
  ru.flags = (uint8_t)((b.w >> 8) & 0xFF);
  ru.msg_len = (uint16_t)(b.w >> 16);
  return ru;
}

// One wave per receiver, lane = record.  Records arrive in canonical
// (sender, position) order in [seg_start, seg_end); a chunk of up to 64 is
// prefetched lane-parallel (rumor id, rumor body, the receiver's view entry of
// the subject).  The intent handlers then run IN PARALLEL across lanes:
//   * LamportClock::witness(t) is c = max(c, t+1), associative, so the clock a
//     record sees is an exclusive prefix max over earlier intents (DPP scan);
//   * records about the same subject form a chain (prev/next lane); chains are
//     walked in depth order, each link taking its predecessor's output entry;
//   * digest contributions (member events, deliveries), refutations and
//     re-queues are then applied serially in record order.
// User events / queries (dedup rings in HBM) run serially in lane 0.
// the merge's record streams are read once per round
__device__ __forceinline__ uint32_t rec_ld(const uint32_t* p) {
  return *p;
}
#ifndef RSF_MERGE_WAVES
#define RSF_MERGE_WAVES 7  // min waves/SIMD for merge_kernel (register cap; 7 measured fastest with 8 receivers per wave, 8 before)
#endif
#ifndef RSF_MERGE_CHAIN_BY_SUBJECT
#define RSF_MERGE_CHAIN_BY_SUBJECT 1  // 1: chain detection loops over distinct subjects, not records
#endif
// What a receiver's merge needs before its records: segment bounds, liveness, the pending
// re-queue counts and the member's registers, issued a receiver AHEAD (merge_kernel)
// as ONE lane-distributed load: lane j fetches dword j of the setup (kSu* below) from its
// own array, so the prefetch holds one vector register until merge_one reads the fields
// out with readlane.
enum : uint32_t {
  kSuStart, kSuEnd, kSuAlive, kSuPend, kSuClock, kSuEClock = kSuClock + 2,
  kSuQClock = kSuEClock + 2, kSuEMin = kSuQClock + 2, kSuQMin = kSuEMin + 2, kSuDigest = kSuQMin + 2,
  kSuErr = kSuDigest + 2, kSuSerf, kSuSubj, kSuRun,  // kSuRun + 2r, + 2r + 1: run r's groups
  kSuLanes = kSuRun + 2 * kMaxRuns
};
// per-lane source: byte address = base + l * mult + off (alive / serf_state: the aligned
// dword holding the byte)
struct MSetupLane {
  const char* base;
  uint32_t mult, off;
};
__device__ __forceinline__ MSetupLane merge_setup_lane(const GCfg& c, const GState& s,
                                                       const uint32_t* __restrict__ seg_start,
                                                       const uint32_t* __restrict__ seg_end, uint32_t lane,
                                                       uint32_t n_runs) {
  const char* b = (const char*)seg_start;
  uint32_t mult = 4, off = 0;
  if (lane == kSuEnd) b = (const char*)seg_end;
  // bucket input: seg_start / seg_end are [run][n_loc] group ranges
  if (lane >= kSuRun && lane < kSuRun + 2 * n_runs) {
    const uint32_t r = (lane - kSuRun) >> 1;
    b = (const char*)((lane - kSuRun) & 1 ? seg_end : seg_start);
    off = (uint32_t)(r * c.n_loc * 4);
  }
  if (lane == kSuAlive) b = (const char*)s.alive + c.lo, mult = 1;
  if (lane == kSuPend) b = (const char*)s.p_cnt;
  const uint64_t* u64s[6] = {s.clock, s.eclock, s.qclock, s.emin, s.qmin, s.digest};
#pragma unroll
  for (uint32_t k = 0; k < 6; ++k)
    if (lane == kSuClock + 2 * k || lane == kSuClock + 2 * k + 1)
      b = (const char*)u64s[k], mult = 8, off = 4 * (lane - kSuClock - 2 * k);
  if (lane == kSuErr) b = (const char*)s.err;
  if (lane == kSuSerf) b = (const char*)s.serf_state, mult = 1;
  if (lane == kSuSubj) b = (const char*)s.member_subj;
  return MSetupLane{b, mult, off};
}
__device__ __forceinline__ uint32_t merge_setup(const MSetupLane& sl, uint64_t l, uint32_t lane) {
  uint32_t v = 0;
  if (lane < kSuLanes && sl.base) {
    const uintptr_t a = (uintptr_t)(sl.base + l * sl.mult + sl.off);
    // a global (not flat) load: flat loads also count on lgkmcnt, which every ds_bpermute
    // wait of the current receiver would then drain
    v = *(const __attribute__((address_space(1))) uint32_t*)(a & ~(uintptr_t)3);
    v >>= 8 * (uint32_t)(a & 3);  // byte fields: shift the byte down
  }
  return v;
}
__device__ __forceinline__ uint64_t su64(uint32_t v, uint32_t k) {
  return ((uint64_t)shfl_u32(v, k + 1) << 32) | shfl_u32(v, k);
}

// One receiver (one wave).  Input layouts: flat (gcnt == nullptr, stride 1): records
// [seg_start, seg_end) in canonical order; grouped (emit_kernel's): groups [seg_start,
// seg_end) of `stride` slots each, group g holding gcnt[g] records, so lane = slot and the
// empty slots of a group are holes (invalid lanes) in an otherwise canonical lane order.
// Re-queues go to the member's pending list (applied at its next emission); the merge
// never reads or writes the queues themselves, except to apply a list that would overflow.
// Receivers whose pending list might overflow during the merge (pending + slots > kPend)
// are not merged by merge_kernel: they go to a list that merge_big_kernel works through
// afterwards with the in-merge list application compiled in (BIG), which the common path
// then need not carry (its registers).  Receivers are independent, so the order is free.
template <bool RUNS, bool BIG>
__device__ __forceinline__ void merge_one(const GCfg& c, const GState& s, const uint32_t* __restrict__ vals,
                                          const uint32_t* __restrict__ dec, const uint32_t* __restrict__ gcnt,
                                          uint32_t stride, uint64_t l, uint32_t lane, uint32_t su, QLds4* row,
                                          uint32_t* __restrict__ sbits, const Buckets& bk, const BigList& big) {
  MPROF_T(t_start);
  uint32_t st = 0, en = 0, total;
  uint32_t rcum[kMaxRuns + 1], rst[kMaxRuns];  // runs: cumulative slots, first group per run
  if (RUNS) {
    rcum[0] = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMaxRuns; ++r) {
      const uint32_t a = r < bk.n_runs ? shfl_u32(su, kSuRun + 2 * r) : 0u;
      const uint32_t b = r < bk.n_runs ? shfl_u32(su, kSuRun + 2 * r + 1) : 0u;
      rst[r] = a;
      rcum[r + 1] = rcum[r] + (b - a) * stride;
    }
    total = rcum[kMaxRuns];
  } else {
    st = shfl_u32(su, kSuStart);
    en = shfl_u32(su, kSuEnd);
    if (RSF_BAD2(10, st > en || en > c.n_loc * c.fanout, ((uint64_t)st << 32) | en)) return;
    total = st < en ? (en - st) * stride : 0u;
  }
  if (total == 0 || (shfl_u32(su, kSuAlive) & 0xFF) == 0) return;
  // pending re-queues: packed per-queue counts and their total (wave-uniform)
  const uint32_t pc0 = shfl_u32(su, kSuPend);
  uint32_t pc = pc0, pn = pend_total(pc0);
  if (RSF_BAD2(12, pn > kPend || (pc0 >> 24) != 0, pc0)) return;
  if (!BIG && pn + total > kPendMerge) {  // at most one re-queue per record slot: might not fit
    if (lane == 0) big.ids[atomicAdd(big.n, 1ull)] = (uint32_t)l;
    return;
  }
  uint32_t qdrop = 0;  // live queue items dropped by full queues (a list applied here)
  GState::PendE* const p_ent = s.p_ent + l * kPend;
  MRegs r;
  r.clock = su64(su, kSuClock);
  r.eclock = su64(su, kSuEClock);
  r.qclock = su64(su, kSuQClock);
  r.emin = su64(su, kSuEMin);
  r.qmin = su64(su, kSuQMin);
  r.digest = su64(su, kSuDigest);
  r.err = shfl_u32(su, kSuErr);
  r.serf_state = (uint8_t)shfl_u32(su, kSuSerf);
  r.subj = (int32_t)shfl_u32(su, kSuSubj);
  ViewS* vrow = vrow_of(s, c, l);
  MPROF_T(t_setup);
  MPROF_ADD(0, t_start, t_setup);
  const uint64_t vs = (uint64_t)st * stride;
  for (uint32_t vb = 0; vb < total; vb += kWave) {
    MPROF_T(t_c0);
    const uint32_t cnt = min((uint32_t)kWave, total - vb);  // lanes in this chunk
    if (BIG && pn + cnt > kPendMerge) {
      // the chunk's re-queues (at most one per record) might not fit the pending list:
      // apply the list to the queues first (rare: a receiver of many records)
      __threadfence_block();
      qdrop += pend_flush_any(c, s, l, lane, pc, *row);
      pc = pn = 0;
    }
    const bool in = lane < cnt;
    const uint32_t vi = vb + lane;  // this lane's slot in the receiver's slot list
    uint32_t rid0 = 0, dsub0 = kEmpty, gk = 1, gc = 1;
    if (RUNS) {
      // the run holding slot v, then its group and place in the group
      uint32_t r = 0;
#pragma unroll
      for (uint32_t q = 1; q < kMaxRuns; ++q) r = vi >= rcum[q] ? q : r;
      uint32_t cr = 0, sr = 0;
#pragma unroll
      for (uint32_t q = 0; q < kMaxRuns; ++q) {
        cr = q == r ? rcum[q] : cr;
        sr = q == r ? rst[q] : sr;
      }
      const uint32_t rel = vi - cr, gr = rel / stride;
      gk = rel - gr * stride;
      const uint64_t g = (uint64_t)sr + gr;
      const uint32_t* b = bk.run(r);
      if (in) {
        rid0 = rec_ld(b + bk.vals_off + g * stride + gk);
        dsub0 = rec_ld(b + bk.decs_off + g * stride + gk);
        gc = rec_ld(b + bk.cnt_off + g);
      }
    } else {
      // slot contents and the group's record count in one round trip (holes read stale ids)
      const uint64_t slot = vs + vi;
      if (RSF_BAD_W(6, in && slot >= (uint64_t)c.n_loc * c.fanout * c.cap_t, slot)) return;
      rid0 = in ? rec_ld(vals + slot) : 0;
      if (gcnt) {
        // group of the slot relative to the receiver's first group: a 32-bit division
        // (a receiver's slot range is small) instead of a 64-bit one
        const uint32_t gr = vi / stride;
        if (RSF_BAD2_W(9, in && (uint64_t)st + gr >= c.n_loc * c.fanout, st + gr)) return;
        if (in) {
          gk = vi - gr * stride;
          gc = rec_ld(gcnt + st + gr);
        }
      }
      // decoration (same round trip as the rumor ids): subject of an intent, or the
      // queue of an event / query; invalid lanes read as neither
      dsub0 = in ? rec_ld(dec + slot) : kEmpty;
    }
    const bool valid = in && (!(RUNS || gcnt) || gk < gc);
    const uint32_t rid = valid ? rid0 : 0;
    const uint32_t dsub = valid ? dsub0 : kEmpty;
    const bool is_view = dsub < kDecViewMax && !RSF_BAD(4, dsub < kDecViewMax && dsub >= c.S, dsub);
    rsf_rumor ru{};
    if (valid) {  // the key only for user events / queries (the decoration says which)
      const uint4 b = s.rbody[rid & c.rmask];
      const uint64_t key = (dsub == kDecQuery || dsub == kDecEvent) ? s.rumors[rid & c.rmask].key : 0ull;
      ru = rumor_from_body(b, key);
    }
    ViewE pre{};
    if (is_view) pre = *view_at(vrow, dsub);  // issued beside the rumor-body load (a non-temporal load measured far slower)
    const uint32_t my_subj = is_view ? dsub : 0xFFFFFFFFu;
    // chains: previous / next record of the same subject in this chunk
    int prev = -1, next = -1;
#if RSF_MERGE_CHAIN_BY_SUBJECT
    // fast path: chunk subjects hashed into the wave's 4096-bit LDS map; no clash means
    // every subject is distinct in the chunk, so there are no chains to link
    bool clash = false;
    if (is_view) {
      const uint32_t h = my_subj & 4095u;
      const uint32_t old = atomicOr(sbits + (h >> 5), 1u << (h & 31));
      clash = (old >> (h & 31)) & 1u;
      sbits[h >> 5] = 0u;  // LDS ops of a wave run in order: every lane's OR has returned
    }
    if (ballot(clash)) {
      // one pass per DISTINCT subject: the ballot of the lanes holding it is the chain,
      // each lane's neighbours are the nearest set bits below and above it
      uint64_t mm = ballot(is_view), same = 0;
      while (mm) {
        const uint32_t sj = shfl_u32(my_subj, __ffsll((long long)mm) - 1);
        const bool hit = my_subj == sj;  // non-view lanes hold 0xFFFFFFFF, never a subject
        const uint64_t grp = ballot(hit);
        if (hit) same = grp;
        mm &= ~grp;
      }
      const uint64_t below = same & ((1ull << lane) - 1), above = same & ~((2ull << lane) - 1);
      prev = below ? 63 - __clzll((long long)below) : -1;
      next = above ? __ffsll((long long)above) - 1 : -1;
    }
#else
    {
      const uint64_t vmask = ballot(is_view);
      uint64_t mm = vmask;
      while (mm) {
        const int j = __ffsll((long long)mm) - 1;
        mm &= mm - 1;
        const uint32_t sj = shfl_u32(my_subj, j);
        if (is_view && sj == my_subj) {
          if (j < (int)lane) prev = j;
          if (j > (int)lane && next < 0) next = j;
        }
      }
    }
#endif
    // Lamport clock each intent record witnesses against: exclusive prefix max
    const uint64_t wit = is_view ? ru.ltime + 1 : 0;
    const uint64_t incl = wave_inclusive_max_u64(wit);
    const uint64_t excl = wave_shr1_u64(incl);
    const uint64_t clock_before = excl > r.clock ? excl : r.clock;
    const uint64_t chunk_max = lane63_u64(incl);
    MPROF_T(t_c1);
    MPROF_ADD(1, t_c0, t_c1);
    // walk chains in depth order
    ViewE v = pre;
    int f = 0;
    uint64_t ref = 0, contrib = 0;  // digest word of a MemberEvent (Failed -> Left)
    bool done = !is_view, dirty = false;
    // bounded: a chain has at most cnt links, so cnt passes always finish it
    for (uint32_t pass = 0; pass < cnt; ++pass) {
      // every lane takes part in each ds_bpermute (an exec-masked source lane reads as 0)
      const int src = prev < 0 ? (int)lane : prev;
      const int pdone = __shfl((int)done, src);  // NOT inside `||`: short-circuit would exec-mask it
      const bool prev_done = prev < 0 || pdone != 0;
      const uint64_t pl = __shfl(v.ltime, src);
      // meta uses 16 bits: the predecessor's dirty flag rides in bit 31
      const uint32_t pmd = (uint32_t)__shfl((int)(v.meta | (dirty ? 0x80000000u : 0u)), src);
      const uint32_t pt = (uint32_t)__shfl((int)v.t, src);
      const bool go = !done && prev_done;
      if (go) {
        if (prev >= 0) {
          v.ltime = pl;
          v.meta = pmd & 0x7FFFFFFFu;
          v.t = pt;
          dirty = (pmd >> 31) != 0;
        }
        MRegs rr = r;
        rr.clock = clock_before;
        rr.digest = 0;
        const uint64_t lt0 = v.ltime;
        const uint32_t mt0 = v.meta, t0 = v.t;
        if (ru.type == RSF_MSG_JOIN) f = hv_join_intent(v, rr, ru.ltime, c.now);
        else f = hv_leave_intent<false>(v, rr, ru.subject, ru.ltime, ru.flags & 1, ref, c.now);
        if (f & RSF_F_MEMBER_EVENT) contrib = kDigMember | ((uint64_t)kEvLeave << 32) | ru.subject;
        dirty = dirty || v.ltime != lt0 || v.meta != mt0 || v.t != t0;
        done = true;
      }
      if (!ballot(!done)) break;
    }
    if (next < 0 && is_view && dirty) *view_at(vrow, my_subj) = v;  // last link writes the subject back
    if (chunk_max > r.clock) r.clock = chunk_max;
    MPROF_T(t_c2);
    MPROF_ADD(2, t_c1, t_c2);
    // intent re-queues of the chunk appended to the pending list in one batch (record order)
    const bool ins = is_view && (f & RSF_F_REBROADCAST);
    const uint64_t newmask = ballot(ins);
    if (newmask) {
      const uint32_t k = (uint32_t)__popcll(newmask);
      const uint32_t i = pn + mbcnt(newmask);
      if (RSF_BAD_W(5, ins && i >= kPend, i)) return;
      if (ins) p_ent[i] = GState::PendE{rid, dsub, ru.msg_len};  // queue 0
      pn += k;
      pc += k;
    }
    // serial part, record order: events/queries (lane 0 handlers), digest, refutes
    const uint64_t serial =
        ballot(valid && (!is_view || (f & (RSF_F_MEMBER_EVENT | RSF_F_REFUTE | RSF_F_PRUNE))));
    uint64_t mm = serial;
    while (mm) {
      const int i = __ffsll((long long)mm) - 1;
      mm &= mm - 1;
      const uint32_t tf = shfl_u32((uint32_t)ru.type | ((uint32_t)ru.flags << 8) | ((uint32_t)ru.msg_len << 16), i);
      const uint8_t type = (uint8_t)(tf & 0xFF);
      int fi;
      if (type == RSF_MSG_JOIN || type == RSF_MSG_LEAVE) {
        fi = (int)shfl_u32((uint32_t)f, i);
        if (fi & RSF_F_MEMBER_EVENT) r.digest = digest_mix(r.digest, shfl_u64(contrib, i));
        if (fi & RSF_F_PRUNE)  // handle_prune's Reap event, after the Leave event of a Failed member
          r.digest = digest_mix(r.digest, kDigMember | ((uint64_t)kEvReap << 32) | shfl_u32(ru.subject, i));
        if (c.dcap && (fi & (RSF_F_MEMBER_EVENT | RSF_F_PRUNE))) {
          const uint32_t sj = shfl_u32(ru.subject, i);
          if (lane == 0) mlog_intent(c, s, l, r.err, fi, sj);
          r.err = shfl_u32(r.err, 0);
        }
        if (fi & RSF_F_REFUTE) {
          const uint64_t rf = shfl_u64(ref, i);
          if (lane == 0) push_refute(c, s, r, rf);
          r.err = shfl_u32(r.err, 0);
        }
      } else {
        const uint64_t L = shfl_u64(ru.ltime, i);
        const uint64_t key = shfl_u64(ru.key, i);
        fi = 0;
        if (lane == 0) {
          if (type == RSF_MSG_USER_EVENT) fi = h_user_event(c, s, l, r, L, key, (tf >> 8) & 1);
          else if (type == RSF_MSG_QUERY) fi = h_query(c, s, l, r, L, (uint32_t)key, (tf >> 8) & 1);
        }
        fi = (int)shfl_u32((uint32_t)fi, 0);
        r.eclock = shfl_u64(r.eclock, 0);
        r.qclock = shfl_u64(r.qclock, 0);
        r.digest = shfl_u64(r.digest, 0);
        r.err = shfl_u32(r.err, 0);
      }
      const uint32_t q = queue_of(type);
      if ((fi & RSF_F_REBROADCAST) && q != kQIntent) {  // intents went in above, batched per chunk
        if (lane == 0) {
          p_ent[pn] = GState::PendE{shfl_u32(rid, i), q == kQQuery ? kDecQuery : kDecEvent, (tf >> 16) | (q << 16)};
        }
        pn++;
        pc += 1u << (8 * q);
      }
    }
    MPROF_T(t_c3);
    MPROF_ADD(3, t_c2, t_c3);
    if (vb + kWave < total) __threadfence_block();  // next chunk's prefetch must see this chunk's view stores
  }
  MPROF_T(t_st0);
  if (BIG && pn > kPendMerge) {  // leave the originations' headroom (kPendMerge)
    __threadfence_block();
    qdrop += pend_flush_any(c, s, l, lane, pc, *row);
    pc = pn = 0;
  }
  if (qdrop) r.err |= kErrQueue;
  // registers go back only where they changed (the setup lanes hold the old values)
  const bool w_clock = r.clock != su64(su, kSuClock), w_eclock = r.eclock != su64(su, kSuEClock),
             w_qclock = r.qclock != su64(su, kSuQClock), w_digest = r.digest != su64(su, kSuDigest),
             w_err = r.err != shfl_u32(su, kSuErr);
  if (lane == 0) {
    if (w_clock) s.clock[l] = r.clock;
    if (w_eclock) s.eclock[l] = r.eclock;
    if (w_qclock) s.qclock[l] = r.qclock;
    if (w_digest) s.digest[l] = r.digest;
    if (w_err) s.err[l] = r.err;
    if (pc != pc0 || qdrop) s.p_cnt[l] = pc;
  }
  MPROF_T(t_end);
  MPROF_ADD(4, t_st0, t_end);
  MPROF_ADD(5, t_start, t_end);
  if (lane == 0) { MPROF_ADD(6, 0, 1); }
}

}  // namespace
