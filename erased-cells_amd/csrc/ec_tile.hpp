// ec_tile.hpp — what every tiled kernel of the library shares (gfx950), and nothing that belongs to one family: the workgroup, the
// workgroup -> tile map, a vector load under the launch's load policy, and the 16-BYTE SLOT — the unit a lane moves, 16 / W cells of
// W bytes as four dwords at every width (1-byte cells as <16 x i8> would lose `nt`, ec_device.hpp) — with its cells, its validity
// bytes and its stores.  The families' kernels include this header, not one another's.
#pragma once

#include "ec_device.hpp"

namespace ecd {

constexpr int kBlock = 256;          // 4 waves
constexpr int kWave = 64;

// a vector load in one arm of its launch's load policy (policy_arms, ec_device.hpp): NT = the stream is not kept cacheable
template <bool NT, typename V>
__device__ __forceinline__ V load_vec(const V* p) {
    if constexpr (NT) return nt_load(p);
    else return plain_load(p);
}

// Workgroup -> tile map: even workgroups walk the buffer from the front, odd ones from the back, so
// two streaming fronts are live at once (measured +1…5 % over a single front, tune_binop_v4/v5.log).
// A bijection on [0, gridDim.x) for any grid size.
__device__ __forceinline__ size_t two_front_tile() {
    const size_t b = blockIdx.x;
    return (b & 1) ? size_t(gridDim.x) - 1 - (b >> 1) : (b >> 1);
}
// The same map inside one launch of a job cut into several (split_launch, ec_runtime.hpp): this launch covers the tiles
// [first, first + gridDim.x).  `first_group(first)` names the workgroup that does a job's once-only work (ragged tails).
__device__ __forceinline__ size_t two_front_tile(size_t first) { return first + two_front_tile(); }
__device__ __forceinline__ bool first_group(size_t first) { return first == 0 && blockIdx.x == 0; }

using u32x4 = vec<uint32_t, 4>;

template <int W> struct width_cell;
template <> struct width_cell<1> { using type = uint8_t; };
template <> struct width_cell<2> { using type = uint16_t; };
template <> struct width_cell<4> { using type = uint32_t; };
template <> struct width_cell<8> { using type = uint64_t; };

// cell k of a slot's four dwords (k is a constant after unrolling)
template <int W>
__device__ __forceinline__ void slot_put(u32x4& v, int k, typename width_cell<W>::type c) {
    if constexpr (W == 1) v[k >> 2] |= uint32_t(c) << (8 * (k & 3));
    else if constexpr (W == 2) v[k >> 1] |= uint32_t(c) << (16 * (k & 1));
    else if constexpr (W == 4) v[k] = c;
    else {
        v[2 * k] = uint32_t(c);
        v[2 * k + 1] = uint32_t(c >> 32);
    }
}
template <int W>
__device__ __forceinline__ typename width_cell<W>::type slot_get(const u32x4& v, int k) {
    using C = typename width_cell<W>::type;
    if constexpr (W == 1) return C((v[k >> 2] >> (8 * (k & 3))) & 0xffu);
    else if constexpr (W == 2) return C((v[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    else if constexpr (W == 4) return v[k];
    else return uint64_t(v[2 * k]) | (uint64_t(v[2 * k + 1]) << 32);
}

// the 16-byte store of a value stream (write-through) or of a mask stream (nt_store / mask_store, ec_device.hpp)
template <bool MASK_ST>
__device__ __forceinline__ void slot_store(u32x4 v, void* p) {
    if constexpr (MASK_ST) mask_store(v, static_cast<u32x4*>(p));
    else nt_store(v, static_cast<u32x4*>(p));
}

// The validity bytes of a slot's cells, 0 or 1 each, at most 16: gathered cell by cell (k a constant or a loop counter — no array, so
// nothing goes to scratch) and handed over as the word that ONE mask_store of 16 / W bytes writes beside the slot.
struct SlotMask {
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ void put(uint32_t k, bool valid) {
        if (k < 8) lo |= uint64_t(valid) << (8 * k);
        else hi |= uint64_t(valid) << (8 * (k & 7u));
    }
    template <int CPL>
    __device__ __forceinline__ typename byte_words<CPL>::type word() const {
        using M = typename byte_words<CPL>::type;
        if constexpr (CPL == 16) return M{uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32)};
        else if constexpr (CPL == 8) return M{uint32_t(lo), uint32_t(lo >> 32)};
        else return static_cast<M>(lo);
    }
};
// the inverse: byte k of the CPL bytes a lane read as one such word
template <int CPL>
__device__ __forceinline__ uint32_t mask_word_byte(const typename byte_words<CPL>::type& m, int k) {
    if constexpr (CPL <= 4) return (uint32_t(m) >> (8 * k)) & 0xffu;
    else return (m[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

// A whole slot — the one whose first cell is cell `at` of the value stream `dst` — leaves as one nt_store of its 16 value bytes and,
// where the launch writes a mask (`dmask`, the mask stream over the same cells, is not null: a launch-uniform test), one mask_store
// of its CPL validity bytes beside it: neighbouring lanes write neighbouring bytes of both streams.
template <int CPL, typename C>
__device__ __forceinline__ void slot_store_pair(u32x4 v, const SlotMask& m, C* dst, uint8_t* dmask, uint64_t at) {
    using M = typename byte_words<CPL>::type;
    nt_store(v, reinterpret_cast<u32x4*>(dst + at));
    if (dmask) mask_store(m.word<CPL>(), reinterpret_cast<M*>(dmask + at));
}

}  // namespace ecd
