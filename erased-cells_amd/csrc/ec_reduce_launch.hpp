// ec_reduce_launch.hpp — the host side of a reduction, written once: the launch sequence of a partials kernel and its finalize
// step (launch_reduction), and the hand-over of a result to a caller that waits for it (sync_result).  Host code for the .hip
// units that launch reductions (ec_abi.hip, ec_stats.hip) or wait for one (ec_expr.hip); what is decided per launch is
// ec_reduce_plan.hpp's, the slots of the stream's scratch are ec_runtime.hpp's.
#pragma once

#include <cstring>
#include <mutex>
#include <type_traits>

#include "ec_tile.hpp"  // kBlock, the cell-wise kernels' workgroup
#include "ec_runtime.hpp"

namespace ecd {

// A reduction of one cell stream under an optional mask describes itself to launch_reduction with a family struct R:
//   Cell, Partial, Out              the cell type, what a workgroup leaves in the scratch, what the result is written as
//   kPartials                       the ScratchSlot of the partials
//   vector_kernel<MASKED, U, BLOCK>()   (cells, mask, n, partials, head | policy << 8, direct): BLOCK threads, U loads in flight;
//                                       direct != nullptr (one-workgroup grid): the workgroup writes the result itself
//   cellwise_kernel<MASKED>()       (cells, mask, n, partials): kBlock threads, any alignment
//   finalize(partials, nparts, first_cell_or_null, out, stream)   launches the one-workgroup finalize kernel
//   kSingle, kPartialsName, kFinalizeName   what check_launch reports
//
// The sequence: as many workgroups per CU as are resident at once, at most PER_CU (the masked kernels of some types need more
// than 64 VGPRs and fit 3, not 4, workgroups of 512 threads on a CU), so that the grid runs as ONE round — probed once per
// family, cell type and shape, also when the plan then picks the cell-wise kernel ("unaligned_vector" off), which has no use
// for the answer; the plan; the partials kernel; then the finalize launch unless one workgroup has written the result.  The call
// holds the stream's turn at its scratch (ScratchTurn) while it queues the two, so host threads that share a stream cannot
// interleave their launches on the partials slot.
template <typename R, int U, int BLOCK, int PER_CU>
ec_status launch_reduction(const void* p, const uint8_t* mask, size_t n, typename R::Out* out, hipStream_t s) {
    using T = typename R::Cell;
    Scratch sc;
    ec_status st = get_scratch(s, &sc);
    if (st != EC_OK) return st;
    const ScratchTurn turn(sc);  // partials and finalize are one unit: no other host thread's partials land between them
    const T* tp = static_cast<const T*>(p);
    auto* partials = reinterpret_cast<typename R::Partial*>(sc.at(R::kPartials));
    unsigned grid = 0;
    if (n > 0) {
        static const int resident[2] = {resident_per_cu(R::template vector_kernel<false, U, BLOCK>(), BLOCK, PER_CU),
                                        resident_per_cu(R::template vector_kernel<true, U, BLOCK>(), BLOCK, PER_CU)};
        const size_t stream_bytes[2] = {n * sizeof(T), mask ? n : 0};
        const ReduceShape shape = {BLOCK, U, resident[mask ? 1 : 0], kBlock, 8};  // the cell-wise kernel: 256-thread workgroups
        const ReducePlan pl = plan_reduction(p, mask ? residue(mask, 16 / sizeof(T)) : 0u, sizeof(T), n, shape, stream_bytes, 2);
        grid = pl.grid;
        typename R::Out* direct = pl.aligned && pl.single ? out : nullptr;  // one workgroup: it writes the result itself
        auto launch = [&](auto masked) {
            constexpr bool MASKED = decltype(masked)::value;
            if (pl.aligned) R::template vector_kernel<MASKED, U, BLOCK>()<<<grid, BLOCK, 0, s>>>(tp, mask, n, partials, pl.head_policy, direct);
            else R::template cellwise_kernel<MASKED>()<<<grid, kBlock, 0, s>>>(tp, mask, n, partials);
        };
        if (mask) launch(std::true_type{});
        else launch(std::false_type{});
        if (direct) return check_launch(R::kSingle);
        st = check_launch(R::kPartialsName);
        if (st != EC_OK) return st;
    }
    R::finalize(partials, static_cast<int>(grid), n > 0 ? tp : nullptr, out, s);
    return check_launch(R::kFinalizeName);
}

// Where the last kernel of a synchronous-result call leaves its result, and how it reaches the caller.
//   mapped: the stream's pinned host words as the device sees them (zero-copy: the result is on the host when the stream has
//           drained); `slot` serves when the mapping is unavailable, with a copy to the pinned words first.  At most 4 words.
//   else:   `slot`, and a copy from it to the caller's memory.
struct ResultSlot {
    ScratchSlot slot;
    bool mapped;
    const char* copy_name;  // what check_hip reports for the copy
};
constexpr ResultSlot kResultWords = {kScratchResult, true, "hipMemcpyAsync"};  // ec_min_max, ec_mask_counts, ec_first_difference
constexpr ResultSlot kResultExprKeys = {kScratchExprKeys, false, "hipMemcpyAsync(keys)"};
constexpr ResultSlot kResultStatsRecord = {kScratchStatsRecord, false, "hipMemcpyAsync(stats record)"};

// The one hand-over of the synchronous-result entry points: takes the stream's turn at its scratch (host threads that share a
// stream take turns, so no call sees another's result words), has `run(sc, where)` queue the kernels whose last one writes
// `bytes` bytes at `where`, waits for the stream and leaves them in `out`.  Nothing of the call is in flight on return.  The
// asynchronous entry points that `run` calls find the turn taken by their own thread and do not take it again (ScratchTurn).
// (Polling the stream with hipStreamQuery before blocking was tried for the 5 µs kernels of fixture-sized rasters: 19.5 µs per
// ec_min_max call against 15.1 µs — hipStreamSynchronize's own wait is the faster one; profiles/r04/sync_result_latency.txt.)
template <typename Run>
ec_status sync_result(hipStream_t s, const ResultSlot& rs, void* out, size_t bytes, Run run) {
    Scratch sc;
    ec_status st = get_scratch(s, &sc);
    if (st != EC_OK) return st;
    const ScratchTurn turn(sc);
    const bool zero_copy = rs.mapped && sc.host_dev;
    int64_t* where = zero_copy ? sc.host_dev : sc.at(rs.slot);
    st = run(sc, where);
    if (st == EC_OK && !zero_copy) st = check_hip(hipMemcpyAsync(rs.mapped ? static_cast<void*>(sc.host) : out, where, bytes, hipMemcpyDeviceToHost, s), rs.copy_name);
    if (st == EC_OK) st = check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (st == EC_OK && rs.mapped) std::memcpy(out, sc.host, bytes);
    return st;
}

}  // namespace ecd
