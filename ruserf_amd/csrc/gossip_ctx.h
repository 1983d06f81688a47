// gossip_ctx.h — the gossip context (struct rsf_gossip) and what its translation units share
// on the host side: the kernel-argument structs the host fills, the layout of the device
// counter block, launch helpers, and the few host functions that cross units.
//
// Units: gossip.hip (the round: begin, emission, merge, QueueChecker ticks, push/pull, the
// diagnostics readers), gossip_ctx.hip (create / destroy / setters), gossip_exchange.hip
// (multi-GPU paths), gossip_state.hip (apply_batch, reaper), gossip_dump.hip (read-back),
// gossip_snapshot.hip (snapshot log, Reconnector).  Only gossip.hip is depended on by the
// others (the functions declared at the end); it depends on none of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <vector>

#include "../../include/ruserf_amd.h"
#include "common.h"
#include "gossip_handlers.h"
#include "rsf_internal.h"

#ifndef RSF_PIN_STAGING
#define RSF_PIN_STAGING 1  // the round's host lists go to the device from pinned staging (rsf_gossip::pin)
#endif

using namespace rsf;

namespace {

// ---- kernel-argument structs filled by the host
// a group's slot word on the bucket path: destination shard | place in its bucket (grp_index_kernel)
constexpr uint32_t kBktWShift = 26, kBktIdxMask = (1u << kBktWShift) - 1;

// Multi-GPU exchange buckets (rsf_gossip_round_emit_buckets): one bucket per destination
// shard, u32 layout [n_groups, 3 x pad | keys[gcap] | cnt[gcap] | vals[gcap * cap_t] |
// decs[gcap * cap_t]]; the groups of a bucket are sorted by receiver.  On the receive side the world's buckets arrive
// back to back in source-rank order = runs.  The bucket a shard addresses to itself never
// travels: the receive side reads run `self_run` from the send buffer (the receive buffer's
// slot for it is left as it is), so the exchange moves (world - 1) buckets per rank.
// Record decorations travel with the rumor ids (80 B per group of 9 slots instead of 44):
// emission has them in registers, while rebuilding them on the receive side from the
// replicated rumor table cost a random 64-B sector per record -- 0.24 ms per round at 1M
// members in the reference regime, whose picks span millions of rumor ids (the merge looking
// them up itself, a separate pass per slot or per group: all slower).
constexpr uint32_t kMaxRuns = 8;
struct Buckets {
  const uint32_t* base;  // receive buffer (RUNS merge); emission writes through `send`
  uint32_t* send;        // send buffer (emission into buckets)
  const uint32_t* wstart;  // emission: per destination shard, its first group in sorted order
  uint64_t per;            // members per shard
  uint64_t stride_u32;   // one bucket
  uint32_t keys_off, cnt_off, vals_off, decs_off, gcap, n_runs, self_run;
  // run r's bucket on the receive side
  __device__ __forceinline__ const uint32_t* run(uint32_t r) const {
    return (r == self_run ? (const uint32_t*)send : base) + (uint64_t)r * stride_u32;
  }
};

// receivers merge_kernel defers to merge_big_kernel (see merge_one)
struct BigList {
  uint32_t* ids;            // [n_loc]
  unsigned long long* n;    // count (reset before each merge)
};

// push/pull: the senders' states, copied to a slab before any is merged (pp_snapshot_kernel)
struct PPSlab {
  ViewS* view;        // [pair][S]
  uint64_t* eb_ltime; // [pair][ebuf]
  uint32_t* eb_cnt;   // [pair][ebuf]
  uint64_t* eb_keys;  // [pair][ebuf * slot_k]
  uint64_t* clocks;   // [pair][4]: clock, event clock, query clock, -
};

// several device buffers cleared by one launch (each hipMemsetAsync is a launch of its own,
// ~5 us on the stream however small the buffer): up to kZeroSpans spans of 4-B words
constexpr int kZeroSpans = 4;
struct ZeroSpans {
  uint32_t* p[kZeroSpans];
  uint64_t words[kZeroSpans];
};

// ---- QueueChecker occupancy histogram (check_queues_kernel -> rsf_gossip_checker_occupancy)
constexpr uint32_t kOccBin = 64, kOccBins = 160;  // occupancy histogram: 64-item bins up to 10240, then one overflow bin
constexpr uint32_t kOccHistWords = 3 * (kOccBins + 1) + 3;  // per queue the bins, then the three maxima

// The device counter block (rsf_gossip::d_counters, u64 words, zeroed at creation): who writes
// each slot and who reads it.
enum : uint32_t {
  // records emitted this round.  W: the group count reduce (single context) or
  // grp_expand_kernel (packed stream), both in emit_and_sort.  R: accumulate_kernel,
  // shard_bounds_kernel, rsf_gossip_last_round_stats
  kCtrSent = 0,
  // [world + 1] the packed stream's bounds by destination shard (world <= 32).
  // W: shard_bounds_kernel.  R: rsf_gossip_round_emit (with kCtrSent in front, one copy)
  kCtrShardBounds = 1,
  // [kCheckStatWords] QueueChecker totals: queued, at or above the warning depth, pruned, per
  // queue.  W: check_queues_kernel.  R: rsf_gossip_checker_stats; cleared there and by
  // check_launch
  kCtrCheckStats = 40,
  // [3] members deferred since creation to the deep lists 0 (small), 1 (full depth), 2 (tiny).
  // W: the deep emission kernels, at their `total` argument - kDeepClassOff + list.
  // R: rsf_gossip_deep_class_stats (one copy up to kCtrDeepMid)
  kCtrDeepClass = 49,
  // receivers merge_kernel deferred to merge_big_kernel this merge (BigList::n).
  // W: merge_kernel; cleared by merge_launch.  R: merge_big_kernel
  kCtrBigCount = 52,
  // members deferred to the deep emission since creation (the kernels' `total` argument).
  // W: the deep emission kernels.  R: rsf_gossip_deep_stats
  kCtrDeepTotal = 55,
  // list 3 (middle class) of the per-list deferral counters, at total + 1.  W / R as kCtrDeepClass
  kCtrDeepMid = 56,
  // records merged this round on the bucket path.  W: bucket_index_kernel (cleared by
  // rsf_gossip_round_merge_buckets).  R: accumulate_kernel, rsf_gossip_last_round_stats
  kCtrBktMerged = 57,
  // bucket path status, non-zero = a bucket overflowed or arrived unsorted / out of shard.
  // W: bucket_bounds_kernel, bucket_index_kernel.  R: rsf_gossip_bucket_status
  kCtrBktBad = 58,
  // records merged since creation (device-side part).  W: accumulate_kernel.  R: rsf_gossip_totals
  kCtrMergedTotal = 60,
  // runs path status, non-zero = a received run was not sorted by receiver.
  // W: runs_bounds_kernel (cleared by rsf_gossip_round_merge_runs).  R: rsf_gossip_check_runs
  kCtrRunsBad = 62,
  // GState::deep_n, as u32 words: the kDeepLists list lengths (W: emit_run / the deep kernels,
  // cleared before each emission; R: the deep kernels), then at u32 word kDeepFullItems the
  // full-depth class's item sum and max, two u64 (R: rsf_gossip_deep_full_items)
  kCtrDeepLists = 64,
  kCtrWords = 72
};
constexpr uint32_t kCheckStatWords = 9;
static_assert(kCtrDeepClass == kCtrDeepTotal - kDeepClassOff, "the per-list counters sit below the total");
static_assert(kCtrDeepLists * 2 + kDeepFullItems + 4 <= kCtrWords * 2, "deep_n and the two u64 fit the block");

// ---- launch helpers
inline unsigned grid1(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }
#ifndef RSF_SYNC_DEBUG
#define RSF_SYNC_DEBUG 0  // diagnostic build: synchronise after every launch of the round and name a failing one
#endif
#define RSF_DBG_SYNC(st, name)                                                                 \
  do {                                                                                         \
    if (RSF_SYNC_DEBUG) {                                                                      \
      const hipError_t e_ = hipStreamSynchronize(st);                                          \
      if (e_ != hipSuccess) {                                                                  \
        fprintf(stderr, "RSF_SYNC_DEBUG: after %s: %s\n", name, hipGetErrorString(e_));        \
        return rsf::set_hip_error(e_, name, __FILE__, __LINE__);                              \
      }                                                                                        \
    }                                                                                          \
  } while (0)
inline int bits_for(uint64_t n) {
  int b = 1;
  while (b < 32 && ((1ull << b) <= n)) ++b;
  return b;
}

#ifndef RSF_GUARD_ZONES
#define RSF_GUARD_ZONES 0  // diagnostic builds: 0xA5 zones around stage_dec and big_ids
#endif
constexpr size_t kZone = RSF_GUARD_ZONES ? (2u << 20) : 0;

}  // namespace

struct rsf_gossip {
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  GCfg c{};
  GState s{};
  // rumor ring: cursor (next free slot) and generation; the round's block is slots
  // [round_slot, round_slot + round_need), its ids round_base + i (gen << rbits | slot)
  uint32_t n_rumors = 0, max_rumors = 0, gen = 0;
  std::vector<uint32_t> subj_sorted;  // the tracked subjects' members, sorted (action checks)
  uint32_t round_slot = 0, round_base = 0, round_abase = 0, round_need = 0;
  // per-round device lists
  rsf_ml_event* d_ml = nullptr;
  rsf_action* d_acts = nullptr;
  int32_t* d_act_status = nullptr;  // [cap_acts] originate_kernel's per-action result
  uint32_t cap_ml = 0, cap_acts = 0, last_n_acts = 0;
  // the round's host lists go to the device from pinned staging (two slots, each reused
  // once the copy issued from it two rounds earlier has completed): a copy from pageable
  // memory would block the host until the stream drained, leaving the GPU idle while the
  // next round is prepared and launched
  void* pin[2] = {nullptr, nullptr};
  size_t pin_cap[2] = {0, 0};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_used[2] = {false, false};
  int pin_next = 0;
  // record pipeline
  uint64_t stage_cap = 0, recv_cap = 0;
  uint32_t *stage_key = nullptr, *stage_val = nullptr, *sort_key = nullptr, *sort_val = nullptr;
  uint32_t *seg_start = nullptr, *seg_end = nullptr;
  void* pp_buf = nullptr;  // push/pull snapshot slab (grow-only)
  uint64_t pp_cap = 0;
  uint32_t* rec_dec = nullptr;  // record decoration beside sort_val (segment_kernel / runs_scatter_kernel)
  // record groups (emit_kernel): [n_loc * fanout] receiver / count, sorted copies, ids, offsets
  uint64_t n_groups = 0;
  // record groups: [n_loc * fanout] peers (emit order) -> sorted by receiver (key_s, id_s);
  // slot[gid] = sorted position; cnt[sorted] = records; off = inclusive scan of cnt (multi-GPU)
  uint32_t *grp_key = nullptr, *grp_cnt = nullptr, *grp_key_s = nullptr, *grp_id = nullptr, *grp_id_s = nullptr,
           *grp_slot = nullptr, *grp_off = nullptr, *stage_dec = nullptr;
  rsf::CubTemp grp_tmp;  // the group count reduce / scan (each call sized by cub_run)
  unsigned merge_blocks = 1;  // merge_big_kernel's grid: merge_kernel's resident blocks per CU x CUs
  unsigned deep_blocks = 1;   // emit_deep_wave_kernel<kDeepSmall> grid (resident waves x CUs)
  unsigned deep_blocks_big = 1;  // emit_deep_wave_kernel<kDeepBig> grid
  unsigned deep_blocks_tiny = 1;  // emit_deep_wave_kernel<kDeepTiny> grid
  unsigned deep_blocks_mid = 1;   // emit_deep_wave_kernel<kDeepMid> grid
  unsigned deep_check_blocks = 1;  // check_stream_kernel grid
  uint64_t deep_last = 0;     // rsf_gossip_deep_stats' previous total
  uint32_t* big_ids = nullptr;  // receivers deferred to merge_big_kernel (count: d_counters[kCtrBigCount])
  uint32_t* qmax = nullptr;     // [n_loc] per-member get_queue_max (rsf_gossip_check_queues, min_queue_depth > 0)
  uint32_t* occ_hist = nullptr; // the last checker tick's occupancy histogram + maxima (check_queues_kernel)
  // RSF_GUARD_ZONES (diagnostic builds): 0xA5-filled zones before and after big_ids and
  // stage_dec and after the sort's storage; rsf_gossip_debug_zones counts changed bytes
  char *big_base = nullptr, *dec_base = nullptr;
  uint64_t* send_buf = nullptr;
  unsigned long long* d_counters = nullptr;  // [kCtrWords], the slots named above
  rsf::CubTemp sort_tmp;  // every radix sort of the round (sort_pairs)
  // Peers ahead: once round t's emission has consumed the groups, round t + 1's peer draw and
  // group sort (they depend on nothing but liveness and the round number) run on a second
  // stream, under round t's merge / bucket exchange.  Round t + 1 uses them if nothing changed
  // liveness in between (ahead_valid), else redraws.  RSF_PEERS_AHEAD=0 turns it off.
  hipStream_t side = nullptr;
  hipEvent_t ev_emitted = nullptr, ev_ahead = nullptr;
  // in-round checker ticks (rsf_gossip_set_checker): period 0 = off
  uint32_t chk_period = 0, chk_max = 0, chk_min = 0, chk_warn = 0;
  bool ahead_launched = false, ahead_valid = false, ahead_on = true;
  uint32_t ahead_round = 0;
  int end_bit = 32;
  uint64_t last_sent = 0, last_merged = 0;
  uint32_t cur_round = 0;
  bool merged_from_stage = true, merged_from_buckets = false;
  // bucket exchange: send / receive buffers (world buckets each), group ranges per run
  uint32_t *bkt_send = nullptr, *bkt_recv = nullptr, *d_rstart = nullptr, *d_rend = nullptr, *d_wstart = nullptr;
  uint32_t bkt_world = 0, bkt_gcap = 0;
  uint64_t total_merged_host = 0;  // multi-GPU merges (n_recv known on host)
  // run-merge tables of rsf_gossip_round_merge_runs: [run_cap][n_loc] u32 x3, [n_loc] u32
  uint32_t *run_start = nullptr, *run_end = nullptr, *run_base = nullptr, *run_total = nullptr;
  uint64_t* d_run_off = nullptr;
  uint32_t run_cap = 0;
  rsf::CubTemp scan_tmp;  // rsf_gossip_round_merge_runs' segment scan
  // phase profiling: marks per round [begin, after begin, after emit, after sort, after merge]
  bool profiling = false;
  static constexpr int kMarks = 5, kMaxProfRounds = 256;
  hipEvent_t ev[kMaxProfRounds][kMarks] = {};
  int prof_rounds = 0;
  bool events_made = false;
  DeviceScratch scratch;
};

static inline int gerr(const char* m) { return rsf::set_error(RSF_ERR_ARG, m); }

// ---- bucket exchange layout (multi-GPU without host synchronisation)
static inline Buckets bucket_layout(const rsf_gossip* g, uint32_t world) {
  const GCfg& c = g->c;
  Buckets b{};
  b.gcap = g->bkt_gcap;
  b.keys_off = 4;
  b.cnt_off = b.keys_off + b.gcap;
  b.vals_off = b.cnt_off + b.gcap;
  b.decs_off = b.vals_off + b.gcap * c.cap_t;
  b.stride_u32 = ((uint64_t)b.decs_off + (uint64_t)b.gcap * c.cap_t + 63) & ~63ull;  // 256-B aligned buckets
  b.per = world ? c.N / world : c.N;
  b.n_runs = world;
  b.self_run = (uint32_t)(c.lo / b.per);
  return b;
}
static inline Buckets send_buckets(rsf_gossip* g) {
  Buckets b = bucket_layout(g, g->bkt_world);
  b.send = g->bkt_send;
  b.wstart = g->d_wstart;
  b.base = g->bkt_recv;
  return b;
}

// ---- host functions of the round unit (gossip.hip) that the other units call
namespace rsf {
// phase-profiling mark k of the current round on the context stream
void mark(rsf_gossip* g, int k);
// Every member's pending re-queues applied to its queues: before anything other than
// emission reads the queues, the queue-prune counters or the error flags.
int flush_pending(rsf_gossip* g, uint32_t period = 1, uint32_t phase = 0);
// every radix sort of the round's key width, through the context's sort storage
int sort_pairs(rsf_gossip* g, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, uint64_t n,
               hipStream_t on = nullptr);
// joins and drops the peers-ahead work in flight: before anything changes liveness
int ahead_drop(rsf_gossip* g);
// rsf_gossip_create: the grids of the kernels launched as many blocks as stay resident
int resident_grids(rsf_gossip* g);
// the round's emission; world > 0: into the exchange buckets, !local: packed into send_buf
int emit_and_sort(rsf_gossip* g, uint32_t round, bool local, uint32_t world = 0);
// seg_start / seg_end of a receiver-sorted key stream (and, with vals, the records' decorations)
int segment_bounds(rsf_gossip* g, const uint32_t* keys, uint64_t n, uint64_t lo, const uint32_t* vals,
                   const uint32_t* rdec, uint32_t* rec_dec, uint32_t rmask);
// merge of [seg_start, seg_end): the emission's groups (grouped) or a flat record stream
int launch_merge(rsf_gossip* g, const uint32_t* vals, bool grouped = false);
// merge of the received buckets' runs (send_buckets(g), d_rstart / d_rend)
int merge_runs(rsf_gossip* g);
// the round unit's two utility kernels on the context stream: n <= kZeroSpans spans of 4-B
// words cleared by one launch; counters[kCtrMergedTotal] += counters[from]
int zero_spans(rsf_gossip* g, uint32_t* const* p, const uint64_t* words, int n);
void accumulate(rsf_gossip* g, uint32_t from);
}  // namespace rsf
