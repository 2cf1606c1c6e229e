// ec_map_launch.hpp — host-side launch of the k_map family (ec_map_kernels.hpp): one workgroup per tile of U 16-byte groups per
// lane, the cell-wise kernel when a pointer is not 16-byte aligned and the "unaligned_vector" knob is off.
#pragma once

#include <type_traits>

#include "ec_map_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

template <typename Fn> struct pure_store : std::false_type {};
template <typename W> struct pure_store<FillFn<W>> : std::true_type {};

// A job whose tiles do not fit one launch is refused before anything is launched (check_groups); EC_OK means "launched".
template <typename Fn, int U>
static ec_status launch_map_u(const Fn& fn, size_t n, hipStream_t s, const char* what) {
    const size_t groups = n / Fn::CPL;
    const size_t tiles = (groups + size_t(kBlock) * U - 1) / (size_t(kBlock) * U);
    if (const ec_status st = check_groups(what, tiles)) return st;
    const size_t stream_bytes[2] = {n * Fn::kIn0, n * Fn::kIn1};
    // ec_fill is a pure write stream with nothing to compute: unused dynamic LDS caps its resident workgroups per CU (the generators
    // load nothing either, but hash every cell — they need their occupancy: 576 -> 879 µs for 2^28 u8 cells under the same cap)
    const unsigned lds = (pure_store<Fn>::value ? static_cast<unsigned>(tuning().write_lds_kb.load())
                                                : (Fn::kIn0 != 0 ? static_cast<unsigned>(tuning().map_lds_kb.load()) : 0u)) << 10;
    k_map<Fn, U><<<grid_for(tiles), kBlock, lds, s>>>(fn, n, cache_plan(stream_bytes, 2));
    return EC_OK;
}

// KNOB_U = false: the default tile shape only ("map_u" = 2, whatever the knob says) — for the kernel families with many type
// pairs (ec_compare.hip, ec_cast.hip), which would otherwise triple their instantiation count over the knob.
template <bool KNOB_U = true, typename Fn>
static ec_status launch_map(const Fn& fn, size_t n, bool aligned, hipStream_t s, const char* what) {
    if (n == 0) return EC_OK;
    ec_status refused = EC_OK;
    if (!aligned) {
        k_map_cellwise<Fn><<<grid_capped((n + kBlock - 1) / kBlock, 8), kBlock, 0, s>>>(fn, n);
    } else if constexpr (KNOB_U) {
        switch (tuning().map_u) {  // groups of 16 B per lane per tile
            case 1: refused = launch_map_u<Fn, 1>(fn, n, s, what); break;
            case 4: refused = launch_map_u<Fn, 4>(fn, n, s, what); break;
            default: refused = launch_map_u<Fn, 2>(fn, n, s, what); break;
        }
    } else {
        refused = launch_map_u<Fn, 2>(fn, n, s, what);
    }
    return refused != EC_OK ? refused : check_launch(what);
}
constexpr bool kDefaultU = false;  // launch_map<kDefaultU>(fn, ...)

}  // namespace ecd
