// gossip_wave.h — wave-level primitives of the gossip kernels (gfx950, wave64): the block
// shape constants, the ballot, and the DPP / readlane reductions, scans and shuffles.
// Depends on nothing else of the engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;
#ifndef RSF_WPB
#define RSF_WPB 4  // waves per block of the merge and the other wave-per-member kernels
#endif
constexpr int kWavesPerBlock = RSF_WPB;
constexpr uint32_t kSentinel = 0xFFFFFFFFu;

// Ballot of a per-lane condition straight from its compare.  HIP's __ballot takes an int, so
// the condition is first materialised as 0/1 in a VGPR and compared again (two extra vector
// instructions per ballot, and the emission and merge kernels take dozens per member).
__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Wave-wide u64 min/max through DPP (row_ror inside 16-lane rows, then
// row_bcast15 / row_bcast31 across rows, result in lane 63): VALU-only data
// movement, no LDS permute round trips.  Every lane of the wave must be active.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROWMASK, 0xF, false);
  hi = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROWMASK, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t lane63_u64(uint64_t v) {
  uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}
#define RSF_DPP_STEP(OP, CTRL, RM)        \
  {                                       \
    uint64_t o_ = dpp64<CTRL, RM>(v);     \
    v = (o_ OP v) ? o_ : v;               \
  }
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
  RSF_DPP_STEP(<, 0xB1, 0xF)   // quad_perm [1,0,3,2]
  RSF_DPP_STEP(<, 0x4E, 0xF)   // quad_perm [2,3,0,1]
  RSF_DPP_STEP(<, 0x124, 0xF)  // row_ror:4
  RSF_DPP_STEP(<, 0x128, 0xF)  // row_ror:8
  RSF_DPP_STEP(<, 0x142, 0xA)  // row_bcast:15 into rows 1,3
  RSF_DPP_STEP(<, 0x143, 0xC)  // row_bcast:31 into rows 2,3
  return lane63_u64(v);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  RSF_DPP_STEP(>, 0xB1, 0xF)
  RSF_DPP_STEP(>, 0x4E, 0xF)
  RSF_DPP_STEP(>, 0x124, 0xF)
  RSF_DPP_STEP(>, 0x128, 0xF)
  RSF_DPP_STEP(>, 0x142, 0xA)
  RSF_DPP_STEP(>, 0x143, 0xC)
  return lane63_u64(v);
}
#undef RSF_DPP_STEP
#define RSF_DPP_STEP32(CTRL, RM)                                                               \
  {                                                                                            \
    const uint32_t o_ = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, RM, 0xF, false); \
    v = o_ < v ? o_ : v;                                                                       \
  }
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  RSF_DPP_STEP32(0xB1, 0xF)
  RSF_DPP_STEP32(0x4E, 0xF)
  RSF_DPP_STEP32(0x124, 0xF)
  RSF_DPP_STEP32(0x128, 0xF)
  RSF_DPP_STEP32(0x142, 0xA)
  RSF_DPP_STEP32(0x143, 0xC)
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
#undef RSF_DPP_STEP32

// inclusive prefix max over the wave (lane 0 first); identity 0
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint64_t dpp64_id0(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, ROWMASK, 0xF, false);
  hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, ROWMASK, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
#define RSF_SCAN_STEP(CTRL, RM)            \
  {                                        \
    uint64_t o_ = dpp64_id0<CTRL, RM>(v);  \
    v = o_ > v ? o_ : v;                   \
  }
__device__ __forceinline__ uint64_t wave_inclusive_max_u64(uint64_t v) {
  RSF_SCAN_STEP(0x111, 0xF)  // row_shr:1
  RSF_SCAN_STEP(0x112, 0xF)  // row_shr:2
  RSF_SCAN_STEP(0x114, 0xF)  // row_shr:4
  RSF_SCAN_STEP(0x118, 0xF)  // row_shr:8
  RSF_SCAN_STEP(0x142, 0xA)  // row_bcast:15
  RSF_SCAN_STEP(0x143, 0xC)  // row_bcast:31
  return v;
}
#undef RSF_SCAN_STEP
// inclusive prefix sum over the wave (u32, identity 0)
__device__ __forceinline__ uint32_t wave_inclusive_sum_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return v;
}

// value of the previous lane (lane 0 gets 0): wave_shr:1
__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v) { return dpp64_id0<0x138, 0xF>(v); }

__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int lane) {
  uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace
