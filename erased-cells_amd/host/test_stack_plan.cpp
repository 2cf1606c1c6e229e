// test_stack_plan.cpp — csrc/ec_stack_plan.hpp alone, under a plain C++ compiler: the refusals that ec_composite and
// ec_composite_rank share, in the order of either entry point and with their exact texts, the head of the kernels' argument block
// and its alignment test — the very functions the library's host side runs.  Built a second time with the address and
// undefined-behaviour sanitizers (test_stack_plan_san).  Needs no device: every pointer is a made-up address that is never
// dereferenced.  The op, q and method checks are the entry points' own (tests/test_composite_args.py, test_composite_rank_args.py
// hold their texts through the library); here they are the predicates of the cell headers, so that the order around them is checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ec_composite_rank_cell.hpp"
#include "ec_stack_plan.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using namespace ecs;

static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }
static uint8_t* byte_at(uintptr_t a) { return reinterpret_cast<uint8_t*>(a); }
static const uintptr_t L0 = 0x10000, L1 = 0x20000, L2 = 0x30000, DST = 0x40000, M0 = 0x50000, M1 = 0x60000, DMASK = 0x70000;

struct Call {
    int op = 0, t_valid = 1;
    std::vector<const void*> layers{at(L0), at(L1), at(L2)};
    std::vector<const uint8_t*> masks;  // empty: no mask array
    bool null_layers = false;
    int k = -100;  // -100: layers.size()
    size_t n = 1000;
    uint64_t tiles = 1;
    uint32_t num = 1, den = 2, min_count = 1;
    int method = 0;
    uintptr_t dst = DST, dmask = 0, aux = 0;

    int count() const { return k == -100 ? int(layers.size()) : k; }
    const void* const* lp() const { return null_layers ? nullptr : layers.data(); }
    const uint8_t* const* mp() const { return masks.empty() ? nullptr : masks.data(); }
};

static const char* const kOk = "";  // a call that passes, or has nothing to do

// ec_composite's order: op, layer count, min_count, dtype, n == 0, the pointers
static std::string as_composite(const Call& c) {
    Message why;
    if (!ecd::valid_composite_op(c.op)) return "op";
    if (count_refusal(why, "ec_composite", c.count()) || min_count_refusal(why, "ec_composite", c.min_count, c.count())) return why;
    if (!c.t_valid) return "dtype";
    if (c.n == 0) return kOk;
    const char* r = pointer_refusal(why, "ec_composite", c.lp(), c.mp(), c.count(), c.n, c.tiles, at(c.dst), byte_at(c.dmask), byte_at(c.aux));
    CHECK(r == nullptr || r == why);
    return r ? r : kOk;
}

// ec_composite_rank's order: layer count, q, method, min_count, dtype, n == 0, the pointers
static std::string as_rank(const Call& c) {
    Message why;
    if (count_refusal(why, "ec_composite_rank", c.count())) return why;
    if (!ecd::valid_rank_fraction(c.num, c.den)) return "q";
    if (!ecd::valid_rank_method(c.method)) return "method";
    if (min_count_refusal(why, "ec_composite_rank", c.min_count, c.count())) return why;
    if (!c.t_valid) return "dtype";
    if (c.n == 0) return kOk;
    const char* r = pointer_refusal(why, "ec_composite_rank", c.lp(), c.mp(), c.count(), c.n, c.tiles, at(c.dst), byte_at(c.dmask), byte_at(c.aux));
    return r ? r : kOk;
}

// the text both entry points give, each behind its own name
static void both(const Call& c, const char* text) {
    CHECK(as_composite(c) == std::string("ec_composite: ") + text);
    CHECK(as_rank(c) == std::string("ec_composite_rank: ") + text);
}

static std::vector<const uint8_t*> masks3(uintptr_t a, uintptr_t b, uintptr_t c) { return {byte_at(a), byte_at(b), byte_at(c)}; }

// REFUSALS of tests/test_composite_args.py and tests/test_composite_rank_args.py, the stack's own
static void every_refusal() {
    Call c;
    c = Call(); c.layers = {at(L0)}; c.k = 0;
    both(c, "0 layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (64)");
    c = Call(); c.k = -1;
    both(c, "-1 layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (64)");
    c = Call(); c.layers.clear();
    for (int i = 0; i < 65; ++i) c.layers.push_back(at(0x100000 + 0x1000 * uintptr_t(i)));
    both(c, "65 layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (64)");
    c = Call(); c.min_count = 0;
    both(c, "min_count 0 is not within 1 .. 3, the number of layers");
    c = Call(); c.min_count = 4;
    both(c, "min_count 4 is not within 1 .. 3, the number of layers");
    c = Call(); c.min_count = 0xffffffffu;
    both(c, "min_count 4294967295 is not within 1 .. 3, the number of layers");
    c = Call(); c.null_layers = true; c.k = 3;
    both(c, "null pointer");
    c = Call(); c.layers[1] = nullptr;
    both(c, "layer 1 is a null pointer");
    c = Call(); c.dst = 0;
    both(c, "null pointer");
    c = Call(); c.masks = masks3(0, M0, 0);
    both(c, "a layer has a mask, so the result needs dst_mask");
    c = Call(); c.dst = L2;
    both(c, "dst is layer 2 (the operation is not in-place)");
    c = Call(); c.masks = masks3(M0, 0, M1); c.dmask = M1;
    both(c, "dst_mask or aux is the mask of layer 2");
    c = Call(); c.masks = masks3(M0, 0, M1); c.dmask = DMASK; c.aux = M0;
    both(c, "dst_mask or aux is the mask of layer 0");
    c = Call(); c.dmask = DST;
    both(c, "dst_mask is dst");
    c = Call(); c.aux = DST;
    both(c, "aux is dst or dst_mask");
    c = Call(); c.dmask = DMASK; c.aux = DMASK;
    both(c, "aux is dst or dst_mask");
    // the rank family's own, between the layer count and min_count
    c = Call(); c.num = 0; c.den = 0; CHECK(as_rank(c) == "q");
    c = Call(); c.den = 65536; CHECK(as_rank(c) == "q");
    c = Call(); c.num = 3; CHECK(as_rank(c) == "q");
    c = Call(); c.num = 0xffffffffu; c.den = 65535; CHECK(as_rank(c) == "q");
    c = Call(); c.method = 2; CHECK(as_rank(c) == "method");
    c = Call(); c.method = -1; CHECK(as_rank(c) == "method");
    for (int op : {-1, 6, 255}) { c = Call(); c.op = op; CHECK(as_composite(c) == "op"); }
    // and calls that pass
    c = Call(); CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
    c.masks = masks3(M0, 0, M1); c.dmask = DMASK; c.aux = 0x80000;
    CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
}

// test_the_order_of_the_refusals of both files: each call has every later fault too
static void the_order() {
    const uint64_t many = uint64_t(1) << 40;  // tiles of 2^62 cells, whatever the shape
    Call c;
    c.op = 9; c.k = 0; c.min_count = 0; c.t_valid = 0; c.dst = 0;
    CHECK(as_composite(c) == "op");
    c.op = 0;
    CHECK(as_composite(c) == "ec_composite: 0 layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (64)");
    c.den = 0; c.method = 7;
    CHECK(as_rank(c) == "ec_composite_rank: 0 layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (64)");
    c.k = -100;
    CHECK(as_rank(c) == "q");
    c.num = 3; c.den = 2;
    CHECK(as_rank(c) == "q");
    c.num = 1;
    CHECK(as_rank(c) == "method");
    c.method = 0;
    both(c, "min_count 0 is not within 1 .. 3, the number of layers");
    c.min_count = 1;
    CHECK(as_composite(c) == "dtype" && as_rank(c) == "dtype");
    c = Call(); c.dst = 0; c.masks = masks3(M0, M0, M0); c.n = size_t(1) << 62; c.tiles = many;
    both(c, "null pointer");
    c.dst = L0;
    both(c, "a layer has a mask, so the result needs dst_mask");
    c.masks.clear();
    both(c, "4611686018427387904 cells are more than 2^31 - 1 tiles");
    c = Call(); c.dst = L0; c.masks = masks3(M0, M0, M0); c.dmask = M0;
    both(c, "dst is layer 0 (the operation is not in-place)");
    c.dst = DST; c.aux = DST;
    both(c, "dst_mask or aux is the mask of layer 0");
    c.masks.clear(); c.dmask = DST;
    both(c, "dst_mask is dst");
}

// 1, 3 and 64 layers; 2^31 - 1 tiles pass and 2^31 do not; an empty stack with null pointers; 2^62 cells
static void heights_and_limits() {
    for (int k : {1, 3, 64}) {
        Call c;
        c.layers.clear();
        for (int i = 0; i < k; ++i) c.layers.push_back(at(0x100000 + 0x1000 * uintptr_t(i)));
        CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
        c.min_count = uint32_t(k);
        CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
        c.min_count = uint32_t(k) + 1;
        char text[96];
        std::snprintf(text, sizeof text, "min_count %d is not within 1 .. %d, the number of layers", k + 1, k);
        both(c, text);
        c.min_count = 1;
        c.tiles = kMaxTiles;            // exactly 2^31 - 1: passes this check, so the next one refuses
        c.dst = 0x100000 + 0x1000 * uintptr_t(k - 1);
        std::snprintf(text, sizeof text, "dst is layer %d (the operation is not in-place)", k - 1);
        both(c, text);
        c.tiles = kMaxTiles + 1;        // 2^31
        both(c, "1000 cells are more than 2^31 - 1 tiles");
        c.dst = DST;
        both(c, "1000 cells are more than 2^31 - 1 tiles");
        c.tiles = kMaxTiles;
        CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
        c.layers[size_t(k) - 1] = nullptr;
        std::snprintf(text, sizeof text, "layer %d is a null pointer", k - 1);
        both(c, text);
        // the form the sharded entry points check with: no cells, no pointers
        c = Call(); c.null_layers = true; c.k = k; c.n = 0; c.dst = 0;
        CHECK(as_composite(c) == kOk && as_rank(c) == kOk);
        c.min_count = uint32_t(k) + 1;  // the checks come first
        CHECK(as_composite(c) != kOk && as_rank(c) != kOk);
    }
    Call c;
    c.n = size_t(1) << 62;
    c.tiles = (c.n / 16 + 511) / 512;   // as the widest tile of either family counts them
    CHECK(c.tiles > kMaxTiles);
    both(c, "4611686018427387904 cells are more than 2^31 - 1 tiles");
    Message why;                        // the longest text fits the buffer with room to spare
    CHECK(pointer_refusal(why, "ec_composite_rank", c.lp(), nullptr, 3, SIZE_MAX, UINT64_MAX, at(DST), nullptr, nullptr) == why);
    CHECK(std::strlen(why) + 32 < sizeof why);
}

struct Block : StackArgs {
    uint32_t tail[5];
};

// fill zeroes the whole block and copies the caller's arrays; stack_aligned looks at every stream of the stack and at no other
static void the_argument_block() {
    for (int k : {1, 3, 64}) {
        std::vector<const void*> layers;
        std::vector<const uint8_t*> masks;
        for (int i = 0; i < k; ++i) {
            layers.push_back(at(0x100000 + 0x1000 * uintptr_t(i)));
            masks.push_back(i % 2 ? byte_at(0x200000 + 0x1000 * uintptr_t(i)) : nullptr);
        }
        Block b;
        std::memset(static_cast<void*>(&b), 0xff, sizeof b);
        fill(&b, layers.data(), masks.data(), k, 12345, 2, const_cast<void*>(at(DST)), byte_at(DMASK), nullptr);
        for (int i = 0; i < kMaxLayers; ++i) {
            CHECK(b.p[i] == (i < k ? layers[size_t(i)] : nullptr));
            CHECK(b.m[i] == (i < k ? masks[size_t(i)] : nullptr));
        }
        CHECK(b.dst == at(DST) && b.dst_mask == byte_at(DMASK) && b.aux == nullptr && b.n == 12345 && b.layers == k && b.min_count == 2);
        for (uint32_t w : b.tail) CHECK(w == 0);
        StackArgs a;
        fill(&a, layers.data(), nullptr, k, 7, 1, const_cast<void*>(at(DST)), nullptr, nullptr);
        for (int i = 0; i < kMaxLayers; ++i) CHECK(a.m[i] == nullptr);
        CHECK(stack_aligned(b, 16, 1, 8) && stack_aligned(b, 4, 4, 4));
        b.p[k - 1] = at(0x100000 + 0x1000 * uintptr_t(k - 1) + 8);
        CHECK(!stack_aligned(b, 4, 4, 4) && stack_aligned(b, 2, 4, 4) && stack_aligned(b, 8, 1, 1));
        b.p[k - 1] = layers[size_t(k) - 1];
        b.p[kMaxLayers - 1] = k < kMaxLayers ? at(1) : b.p[kMaxLayers - 1];  // past the stack: not looked at
        CHECK(stack_aligned(b, 16, 1, 8));
        if (k > 1) {
            b.m[1] = byte_at(0x201000 + 4);
            CHECK(!stack_aligned(b, 8, 1, 1) && stack_aligned(b, 4, 1, 1));
            b.m[1] = masks[1];
        }
        b.aux = byte_at(0x90000 + 2);
        CHECK(!stack_aligned(b, 4, 1, 1) && stack_aligned(b, 2, 1, 1));
        b.aux = nullptr;
        b.dst = const_cast<void*>(at(DST + 16));
        CHECK(!stack_aligned(b, 4, 1, 8) && stack_aligned(b, 4, 1, 4));
    }
}

int main() {
    every_refusal();
    the_order();
    heights_and_limits();
    the_argument_block();
    std::printf("test_stack_plan: %d checks passed\n", g_checks);
    return 0;
}
