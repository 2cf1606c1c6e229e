// test_launch_split.cpp — the cut of a one-workgroup-per-tile job into launches (csrc/ec_launch_split.hpp) on its own: for tile
// counts around every multiple of the cap up to the families' limit of 2^31 - 1 tiles, the launches cover every tile exactly
// once, in order, none is empty and none holds more workgroups than one dispatch can (work-items in 32 bits).  The two-front
// numbering of the kernels (ec_binop_kernels.hpp) is restated here and checked to be a bijection of each launch onto its part.
// A stand-alone program; built plain and under the address and undefined-behaviour sanitizers (Makefile).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ec_launch_split.hpp"

static int failures = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            if (++failures <= 20) {             \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);       \
                std::printf("\n");              \
            }                                   \
        }                                       \
    } while (0)

// the tile workgroup `group` of a launch of `groups` workgroups takes when the launch starts at tile `first`
static uint64_t two_front_tile(uint64_t first, uint64_t group, uint64_t groups) {
    return first + ((group & 1) ? groups - 1 - (group >> 1) : (group >> 1));
}

// arithmetic only: the parts tile [0, tiles) in order, each within the cap
static void check_parts(uint64_t tiles, uint64_t cap) {
    const uint64_t parts = ecs::launches(tiles, cap);
    CHECK((tiles == 0) == (parts == 0), "tiles %llu parts %llu", (unsigned long long)tiles, (unsigned long long)parts);
    uint64_t next = 0;
    for (uint64_t k = 0; k < parts; ++k) {
        const ecs::Part p = ecs::part(tiles, k, cap);
        CHECK(p.first == next, "tiles %llu launch %llu starts at %llu, not %llu", (unsigned long long)tiles, (unsigned long long)k,
              (unsigned long long)p.first, (unsigned long long)next);
        CHECK(p.count >= 1 && p.count <= cap, "tiles %llu launch %llu holds %llu", (unsigned long long)tiles, (unsigned long long)k, (unsigned long long)p.count);
        CHECK(k + 1 == parts || p.count == cap, "tiles %llu launch %llu is not the last and not full", (unsigned long long)tiles, (unsigned long long)k);
        CHECK(p.count * ecs::kLanes <= 0xFFFFFFFFull || cap != ecs::kMaxGroups, "launch of %llu workgroups: work-items past 32 bits", (unsigned long long)p.count);
        next = p.first + p.count;
    }
    CHECK(next == tiles, "tiles %llu: the launches end at %llu", (unsigned long long)tiles, (unsigned long long)next);
}

// every tile exactly once, counted: each workgroup of each launch marks its tile
static void check_cover(uint64_t tiles, uint64_t cap, std::vector<uint8_t>& seen) {
    seen.assign(tiles, 0);
    for (uint64_t k = 0, parts = ecs::launches(tiles, cap); k < parts; ++k) {
        const ecs::Part p = ecs::part(tiles, k, cap);
        for (uint64_t g = 0; g < p.count; ++g) {
            const uint64_t t = two_front_tile(p.first, g, p.count);
            CHECK(t < tiles, "tiles %llu: workgroup %llu of launch %llu takes tile %llu", (unsigned long long)tiles, (unsigned long long)g,
                  (unsigned long long)k, (unsigned long long)t);
            if (t < tiles) {
                CHECK(seen[t] == 0, "tiles %llu: tile %llu taken twice", (unsigned long long)tiles, (unsigned long long)t);
                seen[t] = 1;
            }
        }
    }
    uint64_t missing = 0;
    for (uint64_t t = 0; t < tiles; ++t) missing += seen[t] == 0;
    CHECK(missing == 0, "tiles %llu: %llu tiles taken by no workgroup", (unsigned long long)tiles, (unsigned long long)missing);
}

int main() {
    const uint64_t cap = ecs::kMaxGroups, two24 = 1ull << 24, two25 = 1ull << 25, limit = 0x7fffffffull;
    CHECK(cap == two24 - 1, "cap %llu", (unsigned long long)cap);
    // the arithmetic at the real cap, around every count the issue names and every multiple of the cap up to the limit
    std::vector<uint64_t> counts = {0, 1, 2, 255, 256, 257};
    for (uint64_t c : {cap, two24, 2 * cap, two25, 3 * cap, uint64_t(1) << 30, 128 * cap, limit})
        for (int64_t d = -3; d <= 3; ++d)
            if (int64_t(c) + d >= 0 && uint64_t(int64_t(c) + d) <= limit) counts.push_back(uint64_t(int64_t(c) + d));
    for (uint64_t m = 1; m * cap <= limit; ++m)
        for (int64_t d = -1; d <= 1; ++d) counts.push_back(uint64_t(int64_t(m * cap) + d));
    for (uint64_t tiles : counts) check_parts(tiles, cap);
    CHECK(ecs::launches(limit) == 129, "2^31 - 1 tiles take %llu launches", (unsigned long long)ecs::launches(limit));
    // every tile exactly once at the real cap, around 2^24 and 2^25 (one byte per tile: 32 MiB at the most) …
    std::vector<uint8_t> seen;
    for (uint64_t tiles : {cap - 1, cap, two24, two24 + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1, two25 - 1, two25, two25 + 1}) check_cover(tiles, cap, seen);
    // … and with small caps, where every count up to several launches is walked, the limit's 129 launches among them
    for (uint64_t small : {1ull, 2ull, 3ull, 7ull, 8ull})
        for (uint64_t tiles = 0; tiles <= 130 * small + 3; ++tiles) {
            check_parts(tiles, small);
            check_cover(tiles, small, seen);
        }
    // the limit itself, counted without a byte per tile: the parts' sizes add up and the last tile belongs to the last launch
    {
        uint64_t total = 0;
        for (uint64_t k = 0; k < ecs::launches(limit); ++k) total += ecs::part(limit, k).count;
        CHECK(total == limit, "the parts of 2^31 - 1 tiles add up to %llu", (unsigned long long)total);
        const ecs::Part last = ecs::part(limit, ecs::launches(limit) - 1);
        CHECK(last.first + last.count == limit && last.count == limit - 128 * cap, "last launch of the limit: %llu + %llu", (unsigned long long)last.first,
              (unsigned long long)last.count);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
