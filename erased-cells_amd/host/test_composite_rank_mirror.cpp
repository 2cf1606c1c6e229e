// test_composite_rank_mirror.cpp — composite_rank() and composite_median() of the C++ host mirror, whole-buffer and sharded (needs an
// MI355X), on cells whose answer can be worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "erased_cells.hpp"

using namespace erased_cells;

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using Bits = std::vector<bool>;
using U8 = std::vector<uint8_t>;
using U16 = std::vector<uint16_t>;
using CB = std::vector<const CellBuffer*>;  // named: a braced list of two pointers would also be an iterator pair
using MB = std::vector<const MaskedCellBuffer*>;

int main() {
    try {
        init(0);
        {  // four unmasked scenes: the two medians, a quartile, the ends, and where each cell came from
            const CellBuffer a = CellBuffer::from_vec<uint16_t>({7, 1, 9, 4}), b = CellBuffer::from_vec<uint16_t>({9, 1, 2, 4}),
                             c = CellBuffer::from_vec<uint16_t>({8, 0, 9, 5}), d = CellBuffer::from_vec<uint16_t>({60000, 1, 3, 4});
            const CB stack = {&a, &b, &c, &d};
            CellBuffer aux(CellType::UInt8, 0);
            // sorted by (cell, k):  cell 0: 7a 8c 9b 60000d   cell 1: 0c 1a 1b 1d   cell 2: 2b 3d 9a 9c   cell 3: 4a 4b 4d 5c
            CHECK(composite_median(stack, EC_RANK_LOWER, &aux).to_vec<uint16_t>() == U16({8, 1, 3, 4}) && aux.to_vec<uint8_t>() == U8({2, 0, 3, 1}));
            CHECK(composite_median(stack, EC_RANK_UPPER, &aux).to_vec<uint16_t>() == U16({9, 1, 9, 4}) && aux.to_vec<uint8_t>() == U8({1, 1, 0, 3}));
            CHECK(composite_rank(stack, {1, 4}, EC_RANK_LOWER, &aux).to_vec<uint16_t>() == U16({7, 0, 2, 4}) && aux.to_vec<uint8_t>() == U8({0, 2, 1, 0}));
            CHECK(composite_rank(stack, {1, 4}, EC_RANK_UPPER, &aux).to_vec<uint16_t>() == U16({8, 1, 3, 4}) && aux.to_vec<uint8_t>() == U8({2, 0, 3, 1}));
            CHECK(composite_rank(stack, {0, 1}, EC_RANK_UPPER, &aux) == composite(stack, EC_COMPOSITE_MIN) && aux.to_vec<uint8_t>() == U8({0, 2, 1, 0}));
            CHECK(composite_rank(stack, {1, 1}, EC_RANK_LOWER, &aux) == composite(stack, EC_COMPOSITE_MAX));
            CHECK(aux.to_vec<uint8_t>() == U8({3, 3, 2, 2}));  // the greatest k among equal keys, where MAX reports the least
            CHECK(composite_rank(CB{&a, &b, &c}).to_vec<uint16_t>() == U16({8, 1, 9, 4}));  // three layers: one median
            CHECK(composite_rank(CB{&a, &b, &c}, {1, 2}, EC_RANK_UPPER).to_vec<uint16_t>() == U16({8, 1, 9, 4}));
        }
        {  // three dates with clouds: the median of the clear observations survives the NaN under a cleared mask byte
            const MaskedCellBuffer d0(CellBuffer::from_vec<float>({1.f, NAN, 3.f, 4.f}), Mask::new_({true, false, true, false}));
            const MaskedCellBuffer d1(CellBuffer::from_vec<float>({10.f, 20.f, NAN, 40.f}), Mask::new_({true, true, false, false}));
            const MaskedCellBuffer d2(CellBuffer::from_vec<float>({-0.f, 200.f, 0.f, NAN}), Mask::new_({true, true, true, false}));
            const MB stack = {&d0, &d1, &d2};
            CellBuffer aux(CellType::UInt8, 0);
            const MaskedCellBuffer lo = composite_median(stack, EC_RANK_LOWER, 1, &aux);
            CHECK(lo.to_vec<float>() == std::vector<float>({1.f, 20.f, 0.f, 0.f}) && lo.mask().to_vec() == Bits({true, true, true, false}));
            CHECK(aux.to_vec<uint8_t>() == U8({0, 1, 2, EC_COMPOSITE_NONE}));
            const MaskedCellBuffer hi = composite_median(stack, EC_RANK_UPPER, 1, &aux);
            CHECK(hi.to_vec<float>() == std::vector<float>({1.f, 200.f, 3.f, 0.f}) && aux.to_vec<uint8_t>() == U8({0, 2, 0, EC_COMPOSITE_NONE}));
            const MaskedCellBuffer three = composite_rank(stack, {0, 1}, EC_RANK_LOWER, 3, &aux);
            CHECK(three.mask().to_vec() == Bits({true, false, false, false}) && std::signbit(three.to_vec<float>()[0]));  // -0.0 is the least cell
            CHECK(three.to_vec<float>()[1] == 0.f && aux.to_vec<uint8_t>() == U8({2, EC_COMPOSITE_NONE, EC_COMPOSITE_NONE, EC_COMPOSITE_NONE}));
            CHECK(composite_median(MB{&d2, &d0, &d2}).to_vec<float>() == std::vector<float>({-0.f, 200.f, 0.f, 0.f}));  // the same layer twice
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1}), w = CellBuffer::from_vec<uint16_t>({1}), l = CellBuffer::from_vec<uint8_t>({1, 2});
            int threw = 0;
            try { composite_rank(CB{}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &w}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &l}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB(65, &a)); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &a}, {2, 1}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &a}, {0, 0}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &a}, {1, 65536}); } catch (const Error&) { ++threw; }
            try { composite_rank(CB{&a, &a}, {1, 2}, static_cast<ec_rank_method>(2)); } catch (const Error&) { ++threw; }
            const MaskedCellBuffer m(CellBuffer::from_vec<uint8_t>({1}), Mask::new_({true}));
            try { composite_rank(MB{&m, &m}, {1, 2}, EC_RANK_LOWER, 3); } catch (const Error&) { ++threw; }
            CHECK(threw == 9);
            CHECK(composite_rank(CB(64, &a), {65535, 65535}).to_vec<uint8_t>() == U8({1}));
        }
        {  // sharded over the one GPU listed three times, against the whole-raster call
            std::vector<int16_t> v(3 * 7 * 11), w(v.size()), x(v.size());
            std::vector<uint8_t> mv(v.size()), mw(v.size());
            for (size_t i = 0; i < v.size(); ++i) {
                v[i] = static_cast<int16_t>((i * 2654435761u) >> 16);
                w[i] = static_cast<int16_t>((i * 40503u) & 0xffff);
                x[i] = static_cast<int16_t>(i);
                mv[i] = (i * 7) % 3 != 0;
                mw[i] = (i * 5) % 4 != 0;
            }
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            using SB = sharded::ShardedCellBuffer;
            const SB sv = SB::scatter(group, v, 21, 11), sw = SB::scatter(group, w, 21, 11), sx = SB::scatter(group, x, 21, 11);
            const SB smv = SB::scatter(group, mv, 21, 11), smw = SB::scatter(group, mw, 21, 11);
            const CellBuffer bv = CellBuffer::from_vec(v), bw = CellBuffer::from_vec(w), bx = CellBuffer::from_vec(x);
            CHECK(SB::composite_rank({&sv, &sw, &sx}).to_vec<int16_t>() == composite_median(CB{&bv, &bw, &bx}).to_vec<int16_t>());
            std::vector<bool> bmv(mv.begin(), mv.end()), bmw(mw.begin(), mw.end());
            const MaskedCellBuffer qv(bv.clone(), Mask::new_(bmv)), qw(bw.clone(), Mask::new_(bmw));
            std::optional<SB> om, aux;
            const SB up = SB::composite_rank({&sv, &sw}, {1, 2}, EC_RANK_UPPER, 2, {&smv, &smw}, &om, &aux);
            CellBuffer whole_aux(CellType::UInt8, 0);
            const MaskedCellBuffer whole = composite_median(MB{&qv, &qw}, EC_RANK_UPPER, 2, &whole_aux);
            CHECK(up.to_vec<int16_t>() == whole.to_vec<int16_t>() && aux->to_vec<uint8_t>() == whole_aux.to_vec<uint8_t>());
            const U8 cut = om->to_vec<uint8_t>();
            CHECK(Bits(cut.begin(), cut.end()) == whole.mask().to_vec());
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
