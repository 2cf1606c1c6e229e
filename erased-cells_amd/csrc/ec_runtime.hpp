// ec_runtime.hpp — process-wide state shared by the translation units of
// liberased_cells_hip.so: error reporting, launch-shape knobs, reduction scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <string>

#include "ec_launch_split.hpp"  // kMaxGroups, part
#include "ec_reduce_plan.hpp"  // kReduceU, kMaxReduceBlocks
#include "ec_refusal.hpp"
#include "erased_cells.h"

namespace ecd {

// Compile-time launch shape of the binary-arithmetic kernels; chosen from the
// A/B runs recorded in profiles/ (tools/tune_binop.hip).
constexpr int kBinopU = 2;         // chunks of 128 cells per wave per tile (U = 2 beats 8 by ≈6 %: tune_binop_v4/v5.log)

struct Tuning;
Tuning& tuning();
// Process-wide knobs (ec_tune_set).  Each field is an atomic word: a knob may be turned while other host threads
// launch — a launch sees the old or the new value of each knob, never a torn one; both are valid launch shapes.
struct Tuning {
    std::atomic<int> binop_variant{-1};  // -1 = by rule (ec_binop_tu.hpp: LDS-staged for an 8-byte operand against one of <= 4 bytes), 0 = always direct narrow loads, 1 = LDS-staged wherever an operand can be staged
    std::atomic<int> reduce_bpc{0};     // workgroups per CU for reductions; 0 = each launch shape's own default (4 x 512 threads)
    std::atomic<int> reduce_shape{0};   // min_max launch shape A/B (ec_abi.hip launch_min_max): 0 = 512 thr x 8 loads (default)
    std::atomic<int> map_u{2};          // 16-B groups per lane per tile for the map kernels (1, 2 or 4)
    std::atomic<int> peel{1};              // leading-cell peel of the binop/fused kernels: 0 off, 1 for 1-byte operands, 2 also for 2-byte ones
    std::atomic<int> unaligned_vector{1};  // 1 = vector kernels at any cell offset (gfx950 unaligned global access);
                                           // 0 = pointers that are not 16-byte aligned run the cell-wise kernels
    std::atomic<int> fused_mixed{1};       // 1 = one-pass typed-load kernels for fused chains over mixed cell types; 0 = convert, then fuse
    std::atomic<int64_t> mall_mb{256};     // Infinity Cache budget of cache_plan(): operand streams that fit it together are loaded with
                                           // the default cache policy, all others non-temporal; 0 = every stream non-temporal
    std::atomic<int> inject_shard_failure{0};  // test hook: shard index + 1 whose NEXT fire-and-forget job of a shard group reports
                                               // EC_ERR_HIP instead of launching (exercises the deferred-error path); 0 = off
    std::atomic<int> inject_pin_refusal{0};    // test hook: 1 = PinSet::pin_all treats every hipHostRegister as refused, so the
                                               // pageable fallback of the host-to-host pipelines is exercised
    std::atomic<int> expr_jit{1};  // expression programs compiled at run time (ec_expr_jit.hpp): 0 never, 1 in the background once a
                                   // program has interpreted 2^31 cell-steps, 2 on the calling thread at first sight
    std::atomic<int> expr_fixed{1};  // 1 (default): a program of the ahead-of-time catalogue (ec_expr_fixed.hpp) runs as its built-in straight-line
                                     // kernel; 0: never (the interpreter / the compiled form serve it — the comparison path of the tests)
    std::atomic<int> write_lds_kb{64};  // LDS reserved per workgroup of a PURE-WRITE launch (ec_fill): caps the workgroups resident
                                        // per CU (64 KiB: two of 160 KiB).  A write-only stream runs faster from few resident waves — 0.85 of the HBM
                                        // peak at full occupancy, 0.88-0.90 at 2-3 workgroups per CU, 0.93 with write-through stores on top
                                        // (profiles/r04/tune_store_v2.log); any launch that also loads needs its occupancy and gets none.  0 = no cap
    // Occupancy caps (unused LDS reserved per workgroup) for kernels that load with 16 bytes per lane: such loads keep enough bytes in flight
    // from fewer waves, and the store stream likes fewer (profiles/r04/write_heavy_caps.md, rotating sets, 16384²): f64 ∘ f64 0.778 -> 0.793 at
    // 48 KiB (3 workgroups per CU), f64 ∘ scalar 0.806 -> 0.828 at 32 KiB (5).  Every kernel with a NARROW operand loses under any cap
    // (u8 ∘ scalar 0.75 -> 0.52 at 32 KiB) and takes none.  -1 = that rule; >= 0 forces the reservation for every launch of the family.
    std::atomic<int> binop_lds_kb{-1};
    std::atomic<int> scalar_lds_kb{-1};
    std::atomic<int> map_lds_kb{0};     // experiment knob for the map launches that load (convert, neg, mask_select …): no rule adopted
    std::atomic<int> fused_lds_kb{0};   // the same reservation for the one-pass kernels (k_fused_any, k_expr, k_expr_fixed): an experiment knob (profiles/r04/fused_caps.md)
    std::atomic<int> counts_one_launch{1};  // Mask::counts in ONE launch: every workgroup adds (1 << 40 | its count) to one 64-bit word of the stream's
                                            // scratch with a returning atomic, the workgroup that reads grid - 1 in the upper bits owns the total,
                                            // writes the result and zeroes the word — one device-scope round trip behind the last load instead of a
                                            // second launch (0: partials + finalize kernel, the form of rounds 1-3; 1: below 2^29 cells; 2: always)
    std::atomic<int> cache_force{-1};  // A/B hook: >= 0 replaces cache_plan()'s answer by these bits for every launch (profiles/r04/cache_plan_ab.md)
    std::atomic<int64_t> pool_keep_mb{32768};  // release threshold of the library's stream-ordered pool (per device)
};

int device_cus();      // CU count of the device bound by the last ensure_ready() on this thread
int current_device();  // that device's index

ec_status ensure_ready();  // EC_ERR_NOT_INITIALIZED unless ec_init ran; binds the calling thread to its library device
ec_status set_error(ec_status code, const char* fmt, ...);
ec_status set_error_text(ec_status code, const std::string& text);
const std::string& last_error_text();
ec_status set_narrowing(int src, int dst);
std::atomic<int64_t>& lds_rule_launches();  // binop launches that took the LDS-staged variant by rule (ec_stat_get "binop_lds_rule_launches")
// The status and text of a call that `r` refuses (r.why not null): EC_ERR_UNSUPPORTED_TYPE for a bad type, else EC_ERR_ARG, and
// "<who>: <r.why> <about>", `about` being the family's own words on the call's arguments, printf-style.
ec_status refused(const ecv::Refusal& r, const char* who, const char* about_fmt, ...) __attribute__((format(printf, 3, 4)));
ec_status check_launch(const char* what);
ec_status check_hip(hipError_t e, const char* what);
// `otherwise` of a dispatch (ec_dispatch.hpp) whose entry point refused a bad dtype with its own text before: never returned
constexpr ec_status kTypeChecked = EC_ERR_UNSUPPORTED_TYPE;
inline hipStream_t S(ec_stream s) { return static_cast<hipStream_t>(s); }  // the C ABI's stream handle as HIP's

// Work on other devices from a thread that may have one of its own: remembers the calling thread's library device, if it has
// one, and puts it back on destruction if it changed — on every path out of the scope, and without touching the thread's last
// error text, so a failure inside the scope is still the one the caller reads.
class DeviceScope {
    int32_t before_ = -1;
    const bool had_;

public:
    DeviceScope() : had_(ec_get_device(&before_) == EC_OK) {}
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    ~DeviceScope() {
        if (!had_ || current_device() == before_) return;
        const std::string keep = last_error_text();
        (void)ec_set_device(before_);
        (void)set_error_text(EC_OK, keep);
    }
};

// May the vector kernels run on these pointers?  Their loads and stores are declared under-aligned
// (ec_device.hpp nt_load/nt_store), so the answer is yes at any cell offset unless the
// "unaligned_vector" knob is turned off.
inline bool aligned16(const void* a, const void* b, const void* c) {
    return tuning().unaligned_vector ||
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}
inline bool aligned_to(const void* a, size_t bytes) {
    return tuning().unaligned_vector || reinterpret_cast<uintptr_t>(a) % bytes == 0;
}

// Leading cells (0 or 1) the direct binop / fused kernels peel so that the 2-cell loads of 1-byte operands start
// on even addresses: a u8x2 load at an odd address costs ≈6 % of the kernel, more than the 8-byte shift of the
// f64 pair stores the peel causes (u8∘u16 at an odd offset: 0.75 of peak unpeeled, 0.78–0.80 peeled).  Pair
// loads of 2-byte cells at 2 mod 4 cost nothing, so they are left alone — peeling for them only misaligns the
// output (u16∘u16: 0.78 unpeeled, 0.70–0.73 peeled; profiles/r01/peel_ab.md).
inline unsigned peel_cost(const void* p, size_t size, unsigned h) {
    const bool counts = size == 1 || (size == 2 && tuning().peel >= 2);
    return counts ? static_cast<unsigned>(size) * static_cast<unsigned>(((reinterpret_cast<uintptr_t>(p) / size) + h) & 1) : 0u;
}
// One operand stream of a launch as the host set-up sees it: its first cell and cell width (size 0: the slot loads nothing), and
// `same_as`, an earlier stream of the launch that reads the same buffer (-1: none).
struct LoadedStream {
    const void* p = nullptr;
    size_t size = 0;
    int same_as = -1;
};
// peel one leading cell when that puts more of the loaded streams' bytes on even addresses (every stream counts, a buffer loaded
// under two names twice)
inline unsigned peel_head(const LoadedStream* st, int count, size_t n) {
    if (n < 2 || !tuning().peel) return 0;
    unsigned c0 = 0, c1 = 0;
    for (int k = 0; k < count; ++k) {
        c0 += peel_cost(st[k].p, st[k].size, 0);
        c1 += peel_cost(st[k].p, st[k].size, 1);
    }
    return c1 < c0 ? 1u : 0u;
}

// Load policy of a launch (policy_arms(), ec_device.hpp): bit k set = operand stream k is loaded with the default cache
// policy because it may still be — or is worth leaving — in the 256 MiB Infinity Cache; clear = non-temporal.  Streams
// are admitted smallest first while they fit the budget TOGETHER (two 256 MiB operands would only evict each other); a
// stream bigger than the cache is always streamed.  The figures behind the rule (MI355X, 16384² cells, profiles/r03/
// tune_nt_width_rotating.log): the u8 ÷ u16 divide with its 256 MiB u8 operand cacheable runs at 0.856 of the HBM peak
// when that operand was touched by the previous launch and 0.792 when it was not; with every load nt, 0.80 either way.
// Big streams want nt: a 2 GiB read-only stream reaches 0.865 nt against 0.76 cacheable.
//
// `value_out_bytes` (round 4): the f64 result the launch streams out, for the kernels that write one (binop, fused, expr).  With it
// a second rule applies: if a stream is LEFT OUT that is no bigger than one that was admitted — two equal operands of which only one
// fits — nothing is admitted.  Measured (profiles/r04/cache_plan_ab.md): u8 ∘ u8 → f64 at 16384² with one of its two 256 MiB operands
// cacheable runs 1.5 % (add) to 7 % (divide) SLOWER in the one-set loop than with every load nt — at any relative placement of the
// two buffers (tools/cache_conflict_probe.py), with either one admitted — while u8 ∘ u16 with its u8 operand cacheable runs 5-8 %
// faster, and the 1 B/cell kernels (mask_and with one of two masks cacheable: 0.93 against 0.80) keep their gain: they pass 0 here.
// An operand that is never read again costs at most 0.6 % under either rule (the rotating-set column of the same table).
inline unsigned cache_plan(const size_t* bytes, int n, size_t value_out_bytes = 0) {
    const int forced = tuning().cache_force.load();
    if (forced >= 0) return static_cast<unsigned>(forced) & ((1u << (n < 8 ? n : 8)) - 1u);
    const size_t budget = static_cast<size_t>(tuning().mall_mb.load()) << 20;
    unsigned plan = 0;
    size_t used = 0, largest_taken = 0;
    bool taken[8] = {false, false, false, false, false, false, false, false};
    for (int round = 0; round < n && n <= 8; ++round) {
        int best = -1;
        for (int k = 0; k < n; ++k)
            if (!taken[k] && bytes[k] > 0 && (best < 0 || bytes[k] < bytes[best])) best = k;
        if (best < 0 || used + bytes[best] > budget) break;
        taken[best] = true;
        used += bytes[best];
        if (bytes[best] > largest_taken) largest_taken = bytes[best];
        plan |= 1u << best;
    }
    if (value_out_bytes > 0 && plan != 0)
        for (int k = 0; k < n && n <= 8; ++k)
            if (!taken[k] && bytes[k] > 0 && bytes[k] <= largest_taken) return 0;  // an equal (or smaller) peer does not fit: admit none
    return plan;
}

// cache_plan of a one-pass launch (ec_stream_tile.hpp): the four stream slots `st` (bit k) and the `nmask` distinct masks (bit 4 + j) of
// n cells.  A stream that reads the buffer of an earlier one counts its bytes once and takes that stream's bit: one buffer, one policy.
inline unsigned stream_policy(const LoadedStream (&st)[4], int nmask, size_t n) {
    size_t bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) bytes[k] = st[k].same_as < 0 ? n * st[k].size : 0;
    for (int j = 0; j < nmask; ++j) bytes[4 + j] = n;
    unsigned policy = cache_plan(bytes, 8, n * sizeof(double));
    for (int k = 0; k < 4; ++k)
        if (st[k].same_as >= 0) policy = (policy & ~(1u << k)) | (((policy >> st[k].same_as) & 1u) << k);
    return policy;
}

// Adds the mask of buffer operand `k` to a launch's distinct masks ms[0 .. *nmask) unless it is there already (one mask shared by
// several operands is ANDed once), and ANDs its 16-byte alignment test into *aligned.  A null mask is refused.
inline ec_status add_mask(const uint8_t* m, int k, const char* what, const uint8_t** ms, int8_t* nmask, bool* aligned) {
    if (!m) return set_error(EC_ERR_ARG, "%s: null mask %d", what, k);
    for (int j = 0; j < *nmask; ++j)
        if (ms[j] == m) return EC_OK;
    ms[(*nmask)++] = m;
    *aligned = *aligned && aligned_to(m, 16);
    return EC_OK;
}

// Element-wise kernels: one workgroup per tile.  A job of more than ecs::kMaxGroups tiles does not fit one launch
// (ec_launch_split.hpp): its caller has refused it (check_groups) or cut it (split_launch) before it comes here.  The answer for
// one that comes all the same is 0, a grid the runtime refuses (check_launch then reports it) — never a smaller grid that would
// run and leave tiles unwritten.
inline unsigned grid_for(size_t tiles) {
    if (tiles < 1) tiles = 1;
    return tiles <= size_t(ecs::kMaxGroups) ? static_cast<unsigned>(tiles) : 0u;
}
// The refusal of the streaming families (binops, maps, one-pass trees), before any device work: EC_ERR_ARG and nothing written
// for a call whose tiles do not fit one launch.
inline ec_status check_groups(const char* what, size_t tiles) {
    if (tiles <= size_t(ecs::kMaxGroups)) return EC_OK;
    return set_error(EC_ERR_ARG, "%s: %zu tiles of %d lanes do not fit one launch (at most %llu workgroups: a grid's work-items are a 32-bit count); "
                     "run it over shards of the buffer", what, tiles, int(ecs::kLanes), static_cast<unsigned long long>(ecs::kMaxGroups));
}
// The launches of a one-workgroup-per-tile job of any size up to the families' 2^31 - 1 tiles: launch(first tile, workgroups) once
// per part of ecs::part, in order, on the caller's stream.  No allocation, no synchronisation; capturable.
template <typename F>
inline ec_status split_launch(size_t tiles, const char* what, F&& launch) {
    if (tiles < 1) tiles = 1;
    for (uint64_t k = 0, parts = ecs::launches(tiles); k < parts; ++k) {
        const ecs::Part p = ecs::part(tiles, k);
        launch(static_cast<size_t>(p.first), static_cast<unsigned>(p.count));
        const ec_status st = check_launch(what);
        if (st != EC_OK) return st;
    }
    return EC_OK;
}
// Grid-stride kernels (cell-wise fallbacks, reductions): at most bpc workgroups per CU.
inline unsigned grid_capped(size_t blocks, int bpc) {
    if (blocks < 1) blocks = 1;
    const size_t cap = size_t(device_cus()) * size_t(bpc > 0 ? bpc : 8);
    return static_cast<unsigned>(blocks < cap ? blocks : cap);
}

// f(workspace) on the caller's block `own`, or — own null — on `bytes` bytes of the library's stream-ordered pool that go back to
// it behind f's launches on the same stream: the call stays asynchronous.  f's status first, then the hand-back's.
template <typename F>
inline ec_status with_workspace(void* own, size_t bytes, ec_stream stream, F&& f) {
    if (own) return f(own);
    void* block = nullptr;
    ec_status st = ec_alloc_async(&block, bytes, stream);
    if (st != EC_OK) return st;
    st = f(block);
    const ec_status freed = ec_free_async(block, stream);
    return st != EC_OK ? st : freed;
}

// Per-(device, stream) scratch for reduction partials (device) and results (pinned host).  The stream orders the LAUNCHES
// that use a slot, not the CALLS that make them: a two-launch reduction queues a partials kernel and then a finalize kernel
// that reads the same slot, and a second host thread on the same stream could queue its own partials between the two.  `mu`
// is therefore the stream's turn at its scratch (ScratchTurn below): every call that queues more than one launch on a slot —
// launch_reduction, the two-launch ec_mask_counts_device — holds it while it queues them, and the synchronous-result entry
// points (sync_result, ec_reduce_launch.hpp) hold it until they have read their result words.  Host threads that share a
// stream take turns; threads on streams of their own never meet.
//
// The layout of Scratch::dev, in 64-bit words: every slot is named here and nowhere else.
constexpr int kStatsRecordWords = 8;  // one ec_moments (64 bytes); a Moments partial (ec_reduce_kernels.hpp) is no larger
struct ScratchSlot { size_t word, words; constexpr size_t end() const { return word + words; } };  // first word, length
constexpr ScratchSlot kScratchPartials = {0, 2 * size_t(kMaxReduceBlocks)};    // min/max: a key pair per workgroup; first difference, counts: a word
constexpr ScratchSlot kScratchResult = {kScratchPartials.end(), 2};           // min/max, counts, first difference without the pinned mapping
constexpr ScratchSlot kScratchExprKeys = {kScratchResult.end(), 2};           // ec_expr_min_max's key pair
constexpr ScratchSlot kScratchAcc = {kScratchExprKeys.end(), 4};              // the one-launch counts' accumulator word (zero between kernels)
constexpr ScratchSlot kScratchStatsPartials = {kScratchAcc.end(), size_t(kStatsRecordWords) * kMaxReduceBlocks};  // a Moments per workgroup
constexpr ScratchSlot kScratchStatsRecord = {kScratchStatsPartials.end(), kStatsRecordWords};                     // ec_stats_compute's record
constexpr size_t kScratchWords = kScratchStatsRecord.end();
static_assert(kScratchPartials.end() <= kScratchResult.word && kScratchResult.end() <= kScratchExprKeys.word && kScratchExprKeys.end() <= kScratchAcc.word &&
              kScratchAcc.end() <= kScratchStatsPartials.word && kScratchStatsPartials.end() <= kScratchStatsRecord.word, "two slots of the stream's scratch overlap");
static_assert(kScratchStatsPartials.word % 8 == 0 && kScratchStatsRecord.word % 8 == 0, "the stats area is 64-byte aligned: hipMalloc's alignment + whole 64-byte lines");
struct ScratchOwner;  // frees the three allocations when the last Scratch copy that names them is gone (ec_runtime.hip)
struct Scratch {
    std::shared_ptr<ScratchOwner> owner;  // every copy handed out by get_scratch() shares ownership: releasing or recycling a
                                          // stream's entry only drops the TABLE's reference, so a host thread that is
                                          // inside a synchronous-result call with this scratch (its `mu` locked, its
                                          // kernels queued) keeps valid memory until it returns
    int64_t* dev = nullptr;    // kScratchWords words, laid out as above
    int64_t* host = nullptr;   // 4 words, pinned (coherent): the calls whose result is one or two words let the last kernel
                               // write it straight into them — no device-to-host copy is queued behind the kernel
    int64_t* host_dev = nullptr;  // the same words as the device addresses them
    std::mutex* mu = nullptr;
    int64_t* at(const ScratchSlot& slot) const { return dev + slot.word; }
};
ec_status get_scratch(hipStream_t s, Scratch* out);

// The calling thread's turn at a stream's scratch: locks sc.mu for the guard's lifetime, unless this thread holds that very
// mutex already — sync_result calls the asynchronous entry points under it, and std::mutex is not recursive.  No allocation,
// no synchronisation with the device: a turn lasts as long as queueing the call's launches does (capturable).
inline thread_local const std::mutex* t_scratch_turn = nullptr;  // the mutex this thread holds through a ScratchTurn, if any
class ScratchTurn {
  public:
    explicit ScratchTurn(const Scratch& sc) {
        if (t_scratch_turn == sc.mu) return;  // the caller up the stack has the turn
        sc.mu->lock();
        mu_ = sc.mu;
        outer_ = t_scratch_turn;
        t_scratch_turn = sc.mu;
    }
    ~ScratchTurn() {
        if (!mu_) return;
        t_scratch_turn = outer_;
        mu_->unlock();
    }
    ScratchTurn(const ScratchTurn&) = delete;
    ScratchTurn& operator=(const ScratchTurn&) = delete;

  private:
    std::mutex* mu_ = nullptr;
    const std::mutex* outer_ = nullptr;
};

// Workgroups of `kernel` (BLOCK threads, no dynamic LDS) that fit on one CU at a time, at most `want`.
template <typename K>
inline int resident_per_cu(K kernel, int block, int want) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess || nb < 1) {
        (void)hipGetLastError();
        return want;
    }
    return nb < want ? nb : want;
}

// reduce_plan (ec_reduce_plan.hpp) of a launch on this thread's device under the current knobs.  `p0`: stream 0's first cell;
// `residue1`: see reduce_plan; `stream_bytes`: what cache_plan() decides the load policy from.
inline unsigned residue(const void* p, size_t mod) { return static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) % mod); }
inline ReducePlan plan_reduction(const void* p0, unsigned residue1, size_t cell_size, size_t n, const ReduceShape& shape,
                                 const size_t* stream_bytes, int nstreams) {
    return reduce_plan(residue(p0, 16), residue1, cell_size, n, shape, device_cus(), tuning().reduce_bpc, tuning().unaligned_vector != 0,
                       cache_plan(stream_bytes, nstreams));
}

// The cells one exact stats record may cover (stats_max_cells, ec_stats_fold.hpp), checked for a whole buffer (shard < 0) or
// for shard `shard` of a group; `advice` closes the refusal's text.  ec_stats.hip.
ec_status check_stats_cells(const char* who, int shard, int t, size_t n, const char* advice);

// The zonal statistics' forms with a workspace of the library's own (ec_zonal.hip), for ec_sharded.hip: the refusals of
// ec_zonal_stats_compute, and the n_zones ec_moments of one launch downloaded to HOST address recs (synchronous).
ec_status check_zonal_host_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n,
                                int32_t n_zones, const void* stats_out);
ec_status zonal_records_host(ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n, int32_t n_zones,
                             ec_moments* recs, ec_stream stream);
// The same two of the table family (ec_zonal_table.hip): ec_zonal_table_compute's refusals and its records on the host.
ec_status check_zonal_table_host_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n,
                                      int32_t n_zones, const void* stats_out);
ec_status zonal_table_records_host(ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n, int32_t n_zones,
                                   ec_moments* recs, ec_stream stream);

// binary arithmetic, one translation unit per op
template <int OP>
ec_status dispatch_binop(int lt, const void* l, int rt, const void* r, size_t n, double* out, hipStream_t s);
template <int OP>
ec_status dispatch_masked_binop(int lt, const void* l, const uint8_t* lm, int rt, const void* r, const uint8_t* rm,
                                size_t n, double* out, uint8_t* om, hipStream_t s);
template <int OP>
ec_status dispatch_binop_scalar(int lt, const void* l, double rhs, size_t n, double* out, hipStream_t s);

}  // namespace ecd
