// ec_stream_tile.hpp — the streaming frame of the one-pass kernels (k_fused_any, k_expr, k_expr_fixed): up to four operand streams
// in, one f64 value stream (and the AND of the operands' masks) out.  The families differ only in their arithmetic; the frame owns
// everything else, so a change of the streaming policy is made here once:
//   * the pair grid: `head` (0/1) peeled leading cells (peel_head, ec_runtime.hpp), then pairs of cells, kBlock * U pairs per tile, one
//     workgroup per tile, two fronts (two_front_tile);
//   * the loads of the streams by compile-time load class, under the launch's load policy (policy_arms, ec_device.hpp), and the
//     guarded nt loads of the last, partial tile;
//   * the nt stores of the value pairs, the peeled head cell and the odd tail cell, and the mask phase.
#pragma once

#include "ec_tile.hpp"
#include "ec_runtime.hpp"

namespace ecd {

using D2 = vec<double, 2>;

// what a lane loads for one PAIR of cells of byte width C — always unsigned words (1-byte cells as <2 x i8> would
// lose the non-temporal flag, ec_device.hpp)
struct no_stream {};
template <int C> struct raw_pair;
template <> struct raw_pair<0> { using type = no_stream; };
template <> struct raw_pair<1> { using type = uint16_t; };
template <> struct raw_pair<2> { using type = uint32_t; };
template <> struct raw_pair<4> { using type = vec<uint32_t, 2>; };
template <> struct raw_pair<8> { using type = vec<uint32_t, 4>; };

// The AND of a launch's distinct masks (A::m[0 .. A::nmask)) at cell i: nt loads in the mask phase, plain ones in the cell-wise
// comparison kernels.
template <bool NT, typename A>
__device__ __forceinline__ uint8_t mask_and_cell(const A& a, size_t i) {
    if constexpr (NT) {
        uint8_t acc = ld_cell(a.m[0] + i);
        for (int k = 1; k < a.nmask; ++k) acc &= ld_cell(a.m[k] + i);
        return acc;
    } else {
        uint8_t acc = a.m[0][i];
        for (int k = 1; k < a.nmask; ++k) acc &= a.m[k][i];
        return acc;
    }
}

// mask phase: AND of the distinct operand masks (src/masked/masked_buffer.rs:333 applied at every step of the eager chain),
// 16 mask bytes per lane; a mask's load policy is bit 4 + j of A::cacheable (cache_plan, ec_runtime.hpp)
template <typename A>
__device__ __forceinline__ void mask_phase(const A& a, uint8_t* __restrict__ out_mask, size_t n) {
    if (a.nmask > 0) {
        const size_t ngroups = n / 16;
        const size_t stride = size_t(gridDim.x) * kBlock;
        u32x4* __restrict__ om = reinterpret_cast<u32x4*>(out_mask);
        for (size_t g = size_t(blockIdx.x) * kBlock + threadIdx.x; g < ngroups; g += stride) {
            u32x4 acc = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
            for (int k = 0; k < a.nmask; ++k) {
                const u32x4* mk = reinterpret_cast<const u32x4*>(a.m[k]) + g;
                u32x4 x;
                policy_arms<1>(a.cacheable >> (4 + k), [&](auto bits) { x = load_vec<!(decltype(bits)::value & 1u)>(mk); });  // launch-uniform
                acc &= x;
            }
            mask_store(acc, om + g);
        }
        if (blockIdx.x == 0)
            for (size_t i = ngroups * 16 + threadIdx.x; i < n; i += kBlock) st_cell(mask_and_cell<true>(a, i), out_mask + i);
    }
}

// One tile of a one-pass kernel.  The caller names the streams it loads: load classes C0..C3 (cell bytes; 0 = the slot loads nothing),
// their first cells p[k], and `policy`, the load-policy bits of the loaded streams packed in slot order (bit 0 = the first loaded
// stream).  `body(np, r0, r1, r2, r3, o)` turns NP = decltype(np)::value raw pairs per stream (raw_pair<Ck>::type[NP]) into the 2 NP
// values o[]; the frame hands it the tile's U pairs in chunks of NP — U: the whole tile at once; 1: chunk by chunk, each chunk's store
// right behind it.  `one_cell(i)` is the value of cell i alone (the peeled head cell, the odd tail cell).  A::head, A::m, A::nmask and
// A::cacheable are read by name.
template <int U, int NP, int C0, int C1, int C2, int C3, typename A, typename Body, typename OneCell>
__device__ __forceinline__ void stream_tile(const A& a, const void* const (&p)[4], unsigned policy, Body&& body, OneCell&& one_cell,
                                            double* __restrict__ out, uint8_t* __restrict__ out_mask, size_t n) {
    static_assert(U % NP == 0, "chunks of the tile");
    using R0 = typename raw_pair<C0>::type;
    using R1 = typename raw_pair<C1>::type;
    using R2 = typename raw_pair<C2>::type;
    using R3 = typename raw_pair<C3>::type;
    const unsigned head = a.head;
    const size_t npairs = (n - head) >> 1;
    constexpr size_t TILE = size_t(kBlock) * U;
    const size_t tile = two_front_tile();
    const size_t base = tile * TILE + threadIdx.x;
    const bool full = tile * TILE + TILE <= npairs;
    D2* __restrict__ op = reinterpret_cast<D2*>(out + head);
    // first pair of the pair grid of each stream
    const R0* b0 = reinterpret_cast<const R0*>(static_cast<const char*>(p[0]) + size_t(head) * C0);
    const R1* b1 = reinterpret_cast<const R1*>(static_cast<const char*>(p[1]) + size_t(head) * C1);
    const R2* b2 = reinterpret_cast<const R2*>(static_cast<const char*>(p[2]) + size_t(head) * C2);
    const R3* b3 = reinterpret_cast<const R3*>(static_cast<const char*>(p[3]) + size_t(head) * C3);

    R0 q0[U] = {};
    R1 q1[U] = {};
    R2 q2[U] = {};
    R3 q3[U] = {};
    if (full) {
        constexpr int kStreams = (C0 != 0) + (C1 != 0) + (C2 != 0) + (C3 != 0);
        constexpr int kBit1 = (C0 != 0), kBit2 = kBit1 + (C1 != 0), kBit3 = kBit2 + (C2 != 0);
        policy_arms<kStreams>(policy, [&](auto bits) {
            constexpr unsigned B = decltype(bits)::value;
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const size_t pr = base + size_t(j) * kBlock;
                if constexpr (C0 != 0) q0[j] = load_vec<!(B & 1u)>(b0 + pr);
                if constexpr (C1 != 0) q1[j] = load_vec<!((B >> kBit1) & 1u)>(b1 + pr);
                if constexpr (C2 != 0) q2[j] = load_vec<!((B >> kBit2) & 1u)>(b2 + pr);
                if constexpr (C3 != 0) q3[j] = load_vec<!((B >> kBit3) & 1u)>(b3 + pr);
            }
        });
    } else {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const size_t pr = base + size_t(j) * kBlock;
            if (pr < npairs) {
                if constexpr (C0 != 0) q0[j] = nt_load(b0 + pr);
                if constexpr (C1 != 0) q1[j] = nt_load(b1 + pr);
                if constexpr (C2 != 0) q2[j] = nt_load(b2 + pr);
                if constexpr (C3 != 0) q3[j] = nt_load(b3 + pr);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < U; c += NP) {
        R0 r0[NP];
        R1 r1[NP];
        R2 r2[NP];
        R3 r3[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            r0[j] = q0[c + j];
            r1[j] = q1[c + j];
            r2[j] = q2[c + j];
            r3[j] = q3[c + j];
        }
        double o[2 * NP];
        body(std::integral_constant<int, NP>{}, r0, r1, r2, r3, o);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const size_t pr = base + size_t(c + j) * kBlock;
            if (full || pr < npairs) nt_store(D2{o[2 * j], o[2 * j + 1]}, op + pr);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {  // the peeled head cell (lane 0) and the odd tail cell (lane 1)
        const bool do_it = threadIdx.x == 0 ? head != 0 : ((n - head) & 1) != 0;
        const size_t i = threadIdx.x == 0 ? 0 : n - 1;
        if (do_it) st_cell(one_cell(i), out + i);
    }
    mask_phase(a, out_mask, n);
}

// Launch of a one-pass kernel of U pairs per lane per tile: one workgroup per tile behind the `head` peeled cells, and the LDS the
// fused_lds_kb knob reserves per workgroup (an occupancy cap: profiles/r04/fused_caps.md).  A job whose tiles do not fit one launch
// is refused before anything is launched (check_groups); EC_OK means "launched": the caller reads the launch's own status.
template <int U, typename... KArgs, typename... Args>
ec_status launch_stream_tile(const char* what, void (*kern)(KArgs...), unsigned head, size_t n, hipStream_t s, const Args&... args) {
    const size_t per_tile = size_t(kBlock) * U, tiles = (((n - head) >> 1) + per_tile - 1) / per_tile;
    if (const ec_status st = check_groups(what, tiles)) return st;
    hipLaunchKernelGGL(kern, dim3(grid_for(tiles)), dim3(kBlock), static_cast<unsigned>(tuning().fused_lds_kb.load()) << 10, s, args...);
    return EC_OK;
}

}  // namespace ecd
