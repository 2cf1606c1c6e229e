// ec_stack_plan.hpp — what ec_composite and ec_composite_rank (include/erased_cells.h) share on the host: the refusals of a stack of
// K co-registered layers, the head of the kernels' argument block (StackArgs) and how it is filled and checked for alignment.
//
// A refusal's text carries numbers, so the functions write it, behind `what` (the entry point's name), into a buffer on the caller's
// stack (Message: no call allocates) and return it, or null for a call that passes.  Three functions, the runs that the two entry
// points order differently around their own checks; the tile count is the caller's (composite_tile_shape, rank_group):
//   ec_composite       op, count_refusal, min_count_refusal, dtype, n == 0, pointer_refusal
//   ec_composite_rank  count_refusal, q, method, min_count_refusal, dtype, n == 0, pointer_refusal
//
// Self-contained: no HIP include, so host/test_stack_plan.cpp runs these very functions under the address and undefined-behaviour
// sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

namespace ecs {

constexpr int32_t kMaxLayers = 64;             // EC_COMPOSITE_MAX_LAYERS
constexpr uint64_t kMaxTiles = 0x7fffffffull;  // one workgroup per tile, a grid of at most 2^31 - 1

typedef char Message[160];

inline const char* count_refusal(Message& msg, const char* what, int32_t n_layers) {
    if (n_layers >= 1 && n_layers <= kMaxLayers) return nullptr;
    return snprintf(msg, sizeof msg, "%s: %d layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (%d)", what, int(n_layers), int(kMaxLayers)), msg;
}

// behind count_refusal: n_layers is positive
inline const char* min_count_refusal(Message& msg, const char* what, uint32_t min_count, int32_t n_layers) {
    if (min_count >= 1 && min_count <= uint32_t(n_layers)) return nullptr;
    return snprintf(msg, sizeof msg, "%s: min_count %u is not within 1 .. %d, the number of layers", what, min_count, int(n_layers)), msg;
}

// behind the two above, for a stack that is not empty: the pointers, the tile count and every aliasing rule
inline const char* pointer_refusal(Message& msg, const char* what, const void* const* layers, const uint8_t* const* masks, int32_t n_layers,
                                   size_t n, uint64_t tiles, const void* dst, const uint8_t* dst_mask, const uint8_t* aux) {
    const auto say = [&](const char* text) { return snprintf(msg, sizeof msg, "%s: %s", what, text), msg; };
    if (!layers || !dst) return say("null pointer");
    bool masked = false;
    for (int k = 0; k < n_layers; ++k) {
        if (!layers[k]) return snprintf(msg, sizeof msg, "%s: layer %d is a null pointer", what, k), msg;
        masked = masked || (masks && masks[k]);
    }
    if (masked && !dst_mask) return say("a layer has a mask, so the result needs dst_mask");
    if (tiles > kMaxTiles) return snprintf(msg, sizeof msg, "%s: %zu cells are more than 2^31 - 1 tiles", what, n), msg;
    for (int k = 0; k < n_layers; ++k)
        if (layers[k] == dst) return snprintf(msg, sizeof msg, "%s: dst is layer %d (the operation is not in-place)", what, k), msg;
    for (int k = 0; k < n_layers; ++k) {
        const uint8_t* m = masks ? masks[k] : nullptr;
        if (m && (m == dst_mask || m == aux)) return snprintf(msg, sizeof msg, "%s: dst_mask or aux is the mask of layer %d", what, k), msg;
    }
    if (dst_mask && dst_mask == dst) return say("dst_mask is dst");
    if (aux && (aux == dst || aux == dst_mask)) return say("aux is dst or dst_mask");
    return nullptr;
}

// The head of CompositeArgs and CompositeRankArgs (ec_composite_kernels.hpp, ec_composite_rank_kernels.hpp), which travel to the
// kernels by value: the kernels read the block by scalar loads at constant offsets, so this layout is part of them.
struct StackArgs {
    const void* p[kMaxLayers];
    const uint8_t* m[kMaxLayers];  // null: every cell of the layer is valid
    void* dst;
    uint8_t* dst_mask;  // may be null
    uint8_t* aux;       // may be null
    size_t n;
    int32_t layers;
    uint32_t min_count;
};
static_assert(sizeof(StackArgs) == 2 * 8 * kMaxLayers + 40 && offsetof(StackArgs, dst) == 2 * 8 * kMaxLayers, "the head has no padding");

// *a, a StackArgs or a block that starts with one, is all zeroes but for the head: for a call that pointer_refusal passed
template <typename A>
inline void fill(A* a, const void* const* layers, const uint8_t* const* masks, int32_t n_layers, size_t n, uint32_t min_count, void* dst,
                 uint8_t* dst_mask, uint8_t* aux) {
    static_assert(std::is_base_of<StackArgs, A>::value && std::is_trivially_copyable<A>::value, "a kernel argument block");
    memset(static_cast<void*>(a), 0, sizeof(A));
    for (int k = 0; k < n_layers; ++k) {  // read now: the caller's arrays may go when the call returns
        a->p[k] = layers[k];
        a->m[k] = masks ? masks[k] : nullptr;
    }
    a->dst = dst;
    a->dst_mask = dst_mask;
    a->aux = aux;
    a->n = n;
    a->layers = n_layers;
    a->min_count = min_count;
}

// every stream of the stack starts on a group of `group` cells: layers of `cell` bytes, results of `out` bytes, one byte per mask
// cell.  What the launchers ask unless the "unaligned_vector" knob lets the vector kernels run at any cell offset.
inline bool stack_aligned(const StackArgs& a, size_t group, size_t cell, size_t out) {
    const auto on = [](const void* q, size_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; };
    bool aligned = on(a.dst, group * out) && (!a.dst_mask || on(a.dst_mask, group)) && (!a.aux || on(a.aux, group));
    for (int k = 0; k < a.layers; ++k) aligned = aligned && on(a.p[k], group * cell) && (!a.m[k] || on(a.m[k], group));
    return aligned;
}

}  // namespace ecs
