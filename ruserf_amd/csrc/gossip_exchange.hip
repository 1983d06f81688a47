// gossip_exchange.hip — the multi-GPU paths of a round.  Three ways for the records of a
// sharded context to reach their receivers' shards:
//   counts   round_emit packs the receiver-ordered stream into send_buf and returns the count
//            per destination; round_merge re-sorts what arrived and merges it;
//   runs     as counts, but round_merge_runs merges the per-source runs (each already sorted)
//            without a second sort;
//   buckets  round_emit_buckets emits straight into per-destination buckets and
//            round_merge_buckets merges the received ones: no host synchronisation.
// The emission and the merge themselves are the round unit's (gossip.hip), called through the
// functions gossip_ctx.h declares; the kernels the emission launches for these paths
// (grp_expand_kernel, bucket_bounds_kernel) sit with it there.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gossip_ctx.h"

namespace {

__global__ void shard_bounds_kernel(const uint64_t* __restrict__ rec, const unsigned long long* n_valid,
                                    uint64_t per, uint32_t world, unsigned long long* __restrict__ bounds) {
  uint32_t w = threadIdx.x;
  if (w > world) return;
  uint64_t nv = *n_valid;
  uint64_t target = (uint64_t)w * per;  // first key >= target
  uint64_t lo = 0, hi = nv;
  while (lo < hi) {
    uint64_t mid = (lo + hi) / 2;
    if ((rec[mid] >> 32) < target) lo = mid + 1;
    else hi = mid;
  }
  bounds[w] = (w == world) ? nv : lo;
}

__global__ void unpack_kernel(const uint64_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ keys,
                              uint32_t* __restrict__ vals) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t x = in[i];
  keys[i] = (uint32_t)(x >> 32);
  vals[i] = (uint32_t)x;
}

// ---- multi-GPU receive side without a second sort.  The received buffer is n_runs
// runs (one per source shard, concatenated in source-rank = ascending-sender order),
// each already sorted (stably) by receiver.  The canonical merge order is (receiver,
// run, position in run); it is built from run boundaries, per-(run, receiver) counts,
// one scan over receivers and an ordered scatter.
__device__ __forceinline__ uint32_t run_of(const uint64_t* __restrict__ off, uint32_t n_runs, uint64_t i) {
  uint32_t lo = 0, hi = n_runs;  // largest r with off[r] <= i (an empty run is never chosen)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) runs_bounds_kernel(const uint64_t* __restrict__ rec, uint64_t n,
                                                          const uint64_t* __restrict__ off, uint32_t n_runs,
                                                          uint64_t lo, uint64_t n_loc, uint32_t* __restrict__ rstart,
                                                          uint32_t* __restrict__ rend,
                                                          unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = run_of(off, n_runs, i);
  const uint32_t k = (uint32_t)(rec[i] >> 32);
  const uint64_t l = (uint64_t)k - lo;
  const bool first = i == off[r] || (uint32_t)(rec[i - 1] >> 32) != k;
  const bool last = i + 1 == off[r + 1] || (uint32_t)(rec[i + 1] >> 32) != k;
  if (l >= n_loc || (i > off[r] && (uint32_t)(rec[i - 1] >> 32) > k)) {  // not ours / run not sorted
    atomicOr(bad, 1ull);
    return;
  }
  if (first) rstart[r * n_loc + l] = (uint32_t)i;
  if (last) rend[r * n_loc + l] = (uint32_t)(i + 1);
}

__global__ void __launch_bounds__(256) runs_base_kernel(uint32_t n_runs, uint64_t n_loc,
                                                        const uint32_t* __restrict__ rstart,
                                                        const uint32_t* __restrict__ rend, uint32_t* __restrict__ rbase,
                                                        uint32_t* __restrict__ total) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_loc) return;
  uint32_t acc = 0;
  for (uint32_t r = 0; r < n_runs; ++r) {
    const uint64_t idx = r * n_loc + l;
    rbase[idx] = acc;
    acc += rend[idx] - rstart[idx];
  }
  total[l] = acc;
}

__global__ void __launch_bounds__(256) runs_scatter_kernel(const uint64_t* __restrict__ rec, uint64_t n,
                                                           const uint64_t* __restrict__ off, uint32_t n_runs,
                                                           uint64_t lo, uint64_t n_loc,
                                                           const uint32_t* __restrict__ rstart,
                                                           const uint32_t* __restrict__ rbase,
                                                           const uint32_t* __restrict__ seg_start,
                                                           uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ rdec,
                                                           uint32_t* __restrict__ dec, uint32_t rmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = run_of(off, n_runs, i);
  const uint64_t x = rec[i];
  const uint64_t l = (uint64_t)(uint32_t)(x >> 32) - lo;
  if (l >= n_loc) return;
  const uint64_t idx = r * n_loc + l;
  const uint32_t pos = seg_start[l] + rbase[idx] + (uint32_t)(i - rstart[idx]);
  vals[pos] = (uint32_t)x;
  dec[pos] = rdec[(uint32_t)x & rmask];
}

__global__ void __launch_bounds__(256) seg_end_kernel(uint64_t n_loc, const uint32_t* __restrict__ seg_start,
                                                      const uint32_t* __restrict__ total,
                                                      uint32_t* __restrict__ seg_end) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l < n_loc) seg_end[l] = seg_start[l] + total[l];
}

// receive side: per (run r, receiver) the range of its groups in bucket r; the records
// merged (group counts) summed for the statistics; a receiver outside the shard or an
// unsorted bucket is flagged.  Grid-stride over a bounded grid: one atomic per block (an
// atomic per 256 groups on one address serialised into ~0.25 ms at 6M groups).
constexpr unsigned kBucketIndexBlocks = 1024;
__global__ void __launch_bounds__(256) bucket_index_kernel(Buckets bk, uint64_t lo, uint64_t n_loc,
                                                           uint32_t* __restrict__ rstart, uint32_t* __restrict__ rend,
                                                           unsigned long long* __restrict__ merged,
                                                           unsigned long long* __restrict__ flags) {
  // 32-bit indices: n_runs <= 8 buckets of < 2^26 groups (checked at rsf_gossip_bucket_buffers);
  // the 64-bit division per group was most of this kernel's time
  const uint32_t n = bk.n_runs * bk.gcap;
  uint64_t sum = 0;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const uint32_t r = t / bk.gcap, i = t - r * bk.gcap;
    const uint32_t* b = bk.run(r);
    const uint32_t ng = b[0];
    if (i >= ng) continue;
    const uint32_t key = b[bk.keys_off + i];
    const uint64_t l = (uint64_t)key - lo;
    if (l >= n_loc || (i > 0 && b[bk.keys_off + i - 1] > key)) {
      atomicOr(flags, 2ull);
      continue;
    }
    const uint32_t cnt = b[bk.cnt_off + i];
    sum += cnt;
    if (i == 0 || b[bk.keys_off + i - 1] != key) rstart[(uint64_t)r * n_loc + l] = i;
    if (i + 1 == ng || b[bk.keys_off + i + 1] != key) rend[(uint64_t)r * n_loc + l] = i + 1;
  }
  __shared__ uint64_t part[4];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long tot = part[0] + part[1] + part[2] + part[3];
    if (tot) atomicAdd(merged, tot);
  }
}

}  // namespace

static int segment_and_merge(rsf_gossip* g, const uint32_t* keys, const uint32_t* vals, uint64_t n) {
  const GCfg& c = g->c;
  int rc = segment_bounds(g, keys, n, c.lo, vals, (const uint32_t*)g->s.rdec, g->rec_dec, c.rmask);
  if (rc) return rc;
  return launch_merge(g, vals);
}


extern "C" {

int rsf_gossip_bucket_buffers(rsf_gossip* g, uint32_t world, void** send, void** recv, uint64_t* bucket_bytes) {
  if (!g || !send || !recv || !bucket_bytes || world == 0 || world > kMaxRuns) return gerr("bad argument");
  const GCfg& c = g->c;
  if (c.N % world || c.n_loc != c.N / world) return gerr("shards must be equal contiguous ranges of n_members");
  if (world != g->bkt_world) {
    RSF_HIP(hipSetDevice(g->device));
    RSF_HIP(hipStreamSynchronize(g->stream));
    for (void* p : {(void*)g->bkt_send, (void*)g->bkt_recv, (void*)g->d_rstart, (void*)g->d_rend})
      if (p) hipFree(p);
    g->bkt_send = g->bkt_recv = g->d_rstart = g->d_rend = nullptr;
    g->bkt_world = 0;
    // groups per destination: n_loc * fanout / world for uniform peers; the capacity holds
    // 1/8 more plus 4096 (overflow is flagged, rsf_gossip_bucket_status)
    const uint64_t expect = (c.n_loc * c.fanout + world - 1) / world;
    const uint64_t gcap = std::min<uint64_t>(expect + expect / 8 + 4096, c.n_loc * c.fanout);
    if (gcap >= kBktIdxMask) return gerr("bucket capacity exceeds the slot word's 26-bit place field");
    if (gcap * (2 * c.cap_t + 2) + 64 >= (1ull << 32)) return gerr("a bucket exceeds 32-bit word offsets");
    g->bkt_gcap = (uint32_t)gcap;
    const Buckets b = bucket_layout(g, world);
    const size_t bytes = (size_t)b.stride_u32 * 4 * world;
    int rc;
    if ((rc = rsf::dmalloc((void**)&g->bkt_send, bytes)) || (rc = rsf::dmalloc((void**)&g->bkt_recv, bytes)) ||
        (rc = rsf::dmalloc((void**)&g->d_rstart, (size_t)world * c.n_loc * 4)) ||
        (rc = rsf::dmalloc((void**)&g->d_rend, (size_t)world * c.n_loc * 4)))
      return rc;
    if (!g->d_wstart && (rc = rsf::dmalloc((void**)&g->d_wstart, (kMaxRuns + 1) * 4))) return rc;
    RSF_HIP(hipMemset(g->bkt_send, 0, bytes));
    RSF_HIP(hipMemset(g->bkt_recv, 0, bytes));
    g->bkt_world = world;
  }
  *send = g->bkt_send;
  *recv = g->bkt_recv;
  *bucket_bytes = bucket_layout(g, world).stride_u32 * 4;
  return RSF_OK;
}

int rsf_gossip_round_emit_buckets(rsf_gossip* g, uint32_t world) {
  if (!g || world == 0 || world != g->bkt_world) return gerr("call rsf_gossip_bucket_buffers(world) first");
  RSF_HIP(hipSetDevice(g->device));
  int rc = emit_and_sort(g, g->cur_round, false, world);
  if (rc) return rc;
  g->merged_from_stage = false;
  g->merged_from_buckets = true;
  return RSF_OK;
}

int rsf_gossip_round_merge_buckets(rsf_gossip* g, uint32_t world) {
  if (!g || world == 0 || world != g->bkt_world) return gerr("call rsf_gossip_bucket_buffers(world) first");
  const GCfg& c = g->c;
  RSF_HIP(hipSetDevice(g->device));
  hipStream_t st = g->stream;
  const Buckets bk = send_buckets(g);
  {  // the runs' receiver ranges and the records-merged counter: one launch
    uint32_t* const p[3] = {g->d_rstart, g->d_rend, reinterpret_cast<uint32_t*>(g->d_counters + kCtrBktMerged)};
    const uint64_t words[3] = {(uint64_t)world * c.n_loc, (uint64_t)world * c.n_loc, 2};
    int rc = zero_spans(g, p, words, 3);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(bucket_index_kernel, dim3(std::min<uint64_t>(grid1((uint64_t)world * bk.gcap), kBucketIndexBlocks)),
                     dim3(256), 0, st, bk, c.lo, c.n_loc, g->d_rstart, g->d_rend, g->d_counters + kCtrBktMerged,
                     g->d_counters + kCtrBktBad);
  accumulate(g, kCtrBktMerged);
  if (g->profiling && g->prof_rounds < rsf_gossip::kMaxProfRounds)
    hipEventRecord(g->ev[g->prof_rounds][3], g->stream);  // exchange time lands in the sort slot
  int rc = merge_runs(g);
  if (rc) return rc;
  mark(g, 4);
  return RSF_OK;
}

int rsf_gossip_bucket_status(rsf_gossip* g, int* ok) {
  if (!g || !ok) return gerr("null argument");
  unsigned long long f = 0;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(&f, g->d_counters + kCtrBktBad, 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  *ok = f == 0;
  return RSF_OK;
}

int rsf_gossip_round_emit(rsf_gossip* g, uint32_t world, uint64_t* send_counts) {
  if (!g || !send_counts || world == 0 || world > 32) return gerr("bad argument");  // d_counters[kCtrShardBounds ..][world + 1]
  const GCfg& c = g->c;
  if (c.N % world || c.n_loc != c.N / world) return gerr("shards must be equal contiguous ranges of n_members");
  RSF_HIP(hipSetDevice(g->device));
  int rc = emit_and_sort(g, g->cur_round, false);
  if (rc) return rc;
  hipStream_t st = g->stream;
  // emit_and_sort left the stream packed in send_buf (grp_expand_kernel)
  hipLaunchKernelGGL(shard_bounds_kernel, dim3(1), dim3(64), 0, st, g->send_buf, g->d_counters + kCtrSent, c.N / world, world,
                     g->d_counters + kCtrShardBounds);
  RSF_HIP(hipGetLastError());
  unsigned long long b[64];
  RSF_HIP(hipMemcpyAsync(b, g->d_counters + kCtrSent, (world + 2) * 8, hipMemcpyDeviceToHost, st));
  RSF_HIP(hipStreamSynchronize(st));
  for (uint32_t w = 0; w < world; ++w) send_counts[w] = b[1 + w + 1] - b[1 + w];
  g->merged_from_stage = false;
  g->merged_from_buckets = false;
  return RSF_OK;
}

int rsf_gossip_send_buffer(rsf_gossip* g, void** p, uint64_t* cap) {
  if (!g || !p) return gerr("null argument");
  *p = g->send_buf;
  if (cap) *cap = std::max(g->stage_cap, g->recv_cap);
  return RSF_OK;
}

int rsf_gossip_round_merge(rsf_gossip* g, const uint64_t* recv, uint64_t n_recv) {
  if (!g || (n_recv && !recv)) return gerr("null argument");
  if (n_recv > g->recv_cap) return rsf::set_error(RSF_ERR_OVERFLOW, "receive buffer capacity exceeded");
  RSF_HIP(hipSetDevice(g->device));
  hipStream_t st = g->stream;
  if (n_recv) {
    hipLaunchKernelGGL(unpack_kernel, dim3(grid1(n_recv)), dim3(256), 0, st, recv, n_recv, g->stage_key, g->stage_val);
    int rc = sort_pairs(g, g->stage_key, g->sort_key, g->stage_val, g->sort_val, n_recv);
    if (rc) return rc;
  }
  g->last_merged = n_recv;
  g->total_merged_host += n_recv;
  if (!g->profiling) {
  } else if (g->prof_rounds < rsf_gossip::kMaxProfRounds) {
    hipEventRecord(g->ev[g->prof_rounds][3], g->stream);  // exchange time lands in the sort slot
  }
  return segment_and_merge(g, g->sort_key, g->sort_val, n_recv);
}

int rsf_gossip_round_merge_runs(rsf_gossip* g, const uint64_t* recv, const uint64_t* run_counts, uint32_t n_runs) {
  if (!g || (n_runs && !run_counts) || n_runs > 32) return gerr("bad argument");
  const GCfg& c = g->c;
  uint64_t off[63];
  off[0] = 0;
  for (uint32_t r = 0; r < n_runs; ++r) off[r + 1] = off[r] + run_counts[r];
  const uint64_t n = n_runs ? off[n_runs] : 0;
  if (n && !recv) return gerr("null argument");
  if (n > g->recv_cap) return rsf::set_error(RSF_ERR_OVERFLOW, "receive buffer capacity exceeded");
  RSF_HIP(hipSetDevice(g->device));
  hipStream_t st = g->stream;
  if (n_runs > g->run_cap) {
    for (void* p : {(void*)g->run_start, (void*)g->run_end, (void*)g->run_base})
      if (p) hipFree(p);
    g->run_start = g->run_end = g->run_base = nullptr;
    g->run_cap = 0;
    const size_t tab = (size_t)n_runs * c.n_loc * 4;
    int rc;
    if ((rc = rsf::dmalloc((void**)&g->run_start, tab)) || (rc = rsf::dmalloc((void**)&g->run_end, tab)) ||
        (rc = rsf::dmalloc((void**)&g->run_base, tab)))
      return rc;
    g->run_cap = n_runs;
  }
  if (!g->run_total) {
    int rc;
    if ((rc = rsf::dmalloc((void**)&g->run_total, c.n_loc * 4)) || (rc = rsf::dmalloc((void**)&g->d_run_off, 63 * 8)))
      return rc;
  }
  RSF_HIP(hipMemcpyAsync(g->d_run_off, off, (n_runs + 1) * 8, hipMemcpyHostToDevice, st));
  const size_t tab = (size_t)n_runs * c.n_loc * 4;
  RSF_HIP(hipMemsetAsync(g->run_start, 0, tab, st));
  RSF_HIP(hipMemsetAsync(g->run_end, 0, tab, st));
  RSF_HIP(hipMemsetAsync(g->d_counters + kCtrRunsBad, 0, 8, st));
  if (n)
    hipLaunchKernelGGL(runs_bounds_kernel, dim3(grid1(n)), dim3(256), 0, st, recv, n, g->d_run_off, n_runs, c.lo,
                       c.n_loc, g->run_start, g->run_end, g->d_counters + kCtrRunsBad);
  hipLaunchKernelGGL(runs_base_kernel, dim3(grid1(c.n_loc)), dim3(256), 0, st, n_runs, c.n_loc, g->run_start,
                     g->run_end, g->run_base, g->run_total);
  {
    const uint32_t* tot = g->run_total;
    uint32_t* seg = g->seg_start;
    const int nl = (int)c.n_loc;
    int rc = rsf::cub_run(
        g->scan_tmp, st, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, tot, seg, nl, st); },
        "run-merge segment scan");
    if (rc) return rc;
  }
  if (n)
    hipLaunchKernelGGL(runs_scatter_kernel, dim3(grid1(n)), dim3(256), 0, st, recv, n, g->d_run_off, n_runs, c.lo,
                       c.n_loc, g->run_start, g->run_base, g->seg_start, g->sort_val, (const uint32_t*)g->s.rdec,
                       g->rec_dec, c.rmask);
  hipLaunchKernelGGL(seg_end_kernel, dim3(grid1(c.n_loc)), dim3(256), 0, st, c.n_loc, g->seg_start, g->run_total,
                     g->seg_end);
  RSF_HIP(hipGetLastError());
  g->last_merged = n;
  g->total_merged_host += n;
  if (g->profiling && g->prof_rounds < rsf_gossip::kMaxProfRounds)
    hipEventRecord(g->ev[g->prof_rounds][3], g->stream);  // exchange time lands in the sort slot
  return launch_merge(g, g->sort_val);
}

int rsf_gossip_check_runs(rsf_gossip* g, int* ok) {
  if (!g || !ok) return gerr("null argument");
  unsigned long long bad = 0;
  RSF_HIP(hipSetDevice(g->device));
  RSF_HIP(hipMemcpyAsync(&bad, g->d_counters + kCtrRunsBad, 8, hipMemcpyDeviceToHost, g->stream));
  RSF_HIP(hipStreamSynchronize(g->stream));
  *ok = bad == 0;
  return RSF_OK;
}

}  // extern "C"
