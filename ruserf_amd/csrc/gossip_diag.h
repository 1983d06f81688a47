// gossip_diag.h — the diagnostics of the round kernels: the range guards (RSF_CHECKS,
// RSF_BAD*), the deferral reasons (RSF_DEEP_WHY) and the shader-clock phase profiles (MPROF_*,
// EPROF_*), with the __device__ globals they write.
//
// Included by gossip.hip (the round unit) ONLY, before gossip_queue.h.  The library is built
// without relocatable device code, so a __device__ global is one copy per translation unit:
// every kernel that writes g_merge_prof / g_deep_prof / g_eprof* and the host functions that
// read them (rsf_gossip_merge_prof, rsf_gossip_deep_prof, rsf_gossip_debug_ptrs) must be in the
// same unit, or the readers would see a copy nobody writes.  The queue code other units share
// (gossip_queue.h) uses only RSF_DEEP_WHY, and defines it away when this header is absent.
#pragma once
#include "gossip_wave.h"

#ifdef RSF_DEEP_WHY
#error "gossip_diag.h must come before gossip_queue.h (which defines RSF_DEEP_WHY away without it)"
#endif

namespace {

// Range guards on the round kernels' data-dependent indices (record slot, subject and
// pending-list index in the merge, sorted group ids): a violation is recorded
// (g_merge_prof[0] bit k, the value in [1 + k % 7], readable through rsf_gossip_merge_prof)
// and the access skipped.  They never fire on valid input; RSF_CHECKS=2 adds guards on every
// other data-dependent index (diagnostic builds; DESIGN.md §5, open issue at 1M x 4096).
#ifndef RSF_CHECKS
#define RSF_CHECKS 1
#endif
#if RSF_MERGE_PROF || RSF_EMIT_PROF || RSF_CHECKS
__device__ unsigned long long g_merge_prof[8];
#endif
// diagnostic build (experiments/deep_prof.py): why emit_run deferred members to the deep path
// ([0..7]), the deep wave kernel's per-phase shader-clock totals ([8..15]) and its queue sizes
// (a histogram by 128 items, [32..63]); read by rsf_gossip_deep_prof
#ifndef RSF_DEEP_PROF
#define RSF_DEEP_PROF 0
#endif
#if RSF_DEEP_PROF
__device__ unsigned long long g_deep_prof[80];
#define RSF_DEEP_WHY(k) \
  do {                  \
    if (lane == 0) atomicAdd(&g_deep_prof[(k)], 1ull); \
  } while (0)
#else
#define RSF_DEEP_WHY(k) \
  do {                  \
  } while (0)
#endif
#if RSF_CHECKS
#define RSF_BAD(k, cond, val) \
  ((cond) ? (atomicOr(&g_merge_prof[0], 1ull << (k)), g_merge_prof[1 + ((k) % 7)] = (unsigned long long)(val), true) : false)
#else
#define RSF_BAD(k, cond, val) false
#endif
// RSF_CHECKS >= 2 (diagnostic builds): further guards on every data-dependent index
#if RSF_CHECKS >= 2
#define RSF_BAD2(k, cond, val) RSF_BAD(k, cond, val)
#else
#define RSF_BAD2(k, cond, val) false
#endif
// wave-uniform forms for per-lane conditions: the whole wave records and skips together, so
// no lane leaves while the others go on through wave-wide ballots and shuffles.  Only in
// converged code (every lane of the wave active).
#if RSF_CHECKS
#define RSF_BAD_W(k, cond, val) (ballot(RSF_BAD(k, cond, val)) != 0)
#else
#define RSF_BAD_W(k, cond, val) false
#endif
#if RSF_CHECKS >= 2
#define RSF_BAD2_W(k, cond, val) RSF_BAD_W(k, cond, val)
#else
#define RSF_BAD2_W(k, cond, val) false
#endif

#ifndef RSF_MERGE_PROF
#define RSF_MERGE_PROF 0  // diagnostic build: per-phase shader-clock totals of merge_kernel
#endif
#ifndef RSF_EMIT_PROF
#define RSF_EMIT_PROF 0  // diagnostic build: per-phase shader-clock totals of emit_kernel (same counters)
#endif
#if RSF_MERGE_PROF
#define MPROF_T(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define MPROF_ADD(i, a, b) \
  if (lane == 0) atomicAdd(&g_merge_prof[i], (unsigned long long)((b) - (a)))
#else
#define MPROF_T(v)
#define MPROF_ADD(i, a, b)
#endif
#if RSF_EMIT_PROF
// phase times accumulate in the wave's own (scalar) registers and go out once at the end,
// spread over 512 counter rows: an atomic on one shared address per phase would make every
// following phase wait for that contended atomic (vmcnt also counts it)
__device__ unsigned long long g_eprof[512 * 8];
__device__ unsigned long long g_eprof2[512 * 8];  // q_pick_peers' own split
#define EPROF_T(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define EPROF_ADD(i, a, b) ep_acc[i] += (uint64_t)((b) - (a))
#else
#define EPROF_T(v)
#define EPROF_ADD(i, a, b)
#endif

}  // namespace
