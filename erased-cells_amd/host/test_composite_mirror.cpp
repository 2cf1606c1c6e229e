// test_composite_mirror.cpp — composite() of the C++ host mirror, whole-buffer and sharded (needs an MI355X), on cells whose
// answer can be worked out by hand.
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
using CB = std::vector<const CellBuffer*>;  // named: a braced list of two pointers would also be an iterator pair
using MB = std::vector<const MaskedCellBuffer*>;

int main() {
    try {
        init(0);
        {  // three unmasked scenes: every pick, the sum and the mean, and where each cell came from
            const CellBuffer a = CellBuffer::from_vec<uint16_t>({7, 1, 9, 4}), b = CellBuffer::from_vec<uint16_t>({9, 1, 2, 4}),
                             c = CellBuffer::from_vec<uint16_t>({8, 0, 9, 5});
            const std::vector<const CellBuffer*> stack = {&a, &b, &c};
            CellBuffer aux(CellType::UInt8, 0);
            CHECK(composite(stack) == a && composite(stack, EC_COMPOSITE_LAST) == c);
            CHECK(composite(stack, EC_COMPOSITE_MAX, &aux).to_vec<uint16_t>() == std::vector<uint16_t>({9, 1, 9, 5}));
            CHECK(aux.to_vec<uint8_t>() == U8({1, 0, 0, 2}));  // a tie keeps the least k
            CHECK(composite(stack, EC_COMPOSITE_MIN, &aux).to_vec<uint16_t>() == std::vector<uint16_t>({7, 0, 2, 4}));
            CHECK(aux.to_vec<uint8_t>() == U8({0, 2, 1, 0}));
            const CellBuffer s = composite(stack, EC_COMPOSITE_SUM, &aux);
            CHECK(s.cell_type() == CellType::Float64 && s.to_vec<double>() == std::vector<double>({24, 2, 20, 13}) && aux.to_vec<uint8_t>() == U8({3, 3, 3, 3}));
            CHECK(composite(stack, EC_COMPOSITE_MEAN).to_vec<double>() == std::vector<double>({8, 2.0 / 3.0, 20.0 / 3.0, 13.0 / 3.0}));
        }
        {  // cloud fill over three dates: the first clear observation, at least two clear ones, the mean of the clear ones
            const MaskedCellBuffer d0(CellBuffer::from_vec<float>({1.f, NAN, 3.f, 4.f}), Mask::new_({true, false, false, false}));
            const MaskedCellBuffer d1(CellBuffer::from_vec<float>({10.f, 20.f, NAN, 40.f}), Mask::new_({true, true, false, false}));
            const MaskedCellBuffer d2(CellBuffer::from_vec<float>({-0.f, 200.f, 300.f, NAN}), Mask::new_({true, true, true, false}));
            const std::vector<const MaskedCellBuffer*> stack = {&d0, &d1, &d2};
            CellBuffer aux(CellType::UInt8, 0);
            const MaskedCellBuffer first = composite(stack, EC_COMPOSITE_FIRST, 1, &aux);
            CHECK(first.to_vec<float>() == std::vector<float>({1.f, 20.f, 300.f, 0.f}) && first.mask().to_vec() == Bits({true, true, true, false}));
            CHECK(aux.to_vec<uint8_t>() == U8({0, 1, 2, EC_COMPOSITE_NONE}));
            const MaskedCellBuffer two = composite(stack, EC_COMPOSITE_MIN, 2, &aux);
            CHECK(two.to_vec<float>() == std::vector<float>({-0.f, 20.f, 0.f, 0.f}) && two.mask().to_vec() == Bits({true, true, false, false}));
            CHECK(std::signbit(two.to_vec<float>()[0]) && aux.to_vec<uint8_t>() == U8({2, 1, EC_COMPOSITE_NONE, EC_COMPOSITE_NONE}));
            const MaskedCellBuffer mean = composite(stack, EC_COMPOSITE_MEAN, 1, &aux);
            CHECK(mean.cell_type() == CellType::Float64 && mean.to_vec<double>() == std::vector<double>({11.0 / 3.0, 110.0, 300.0, 0.0}));
            CHECK(aux.to_vec<uint8_t>() == U8({3, 2, 1, 0}) && mean.mask().to_vec() == Bits({true, true, true, false}));
            // the same layer may appear twice; the chain of or_else is the FIRST composite
            CHECK(composite(MB{&d2, &d0, &d2}, EC_COMPOSITE_LAST).to_vec<float>() == std::vector<float>({-0.f, 200.f, 300.f, 0.f}));
            const MaskedCellBuffer chain = d0.or_else(d1).or_else(d2);
            CHECK(chain.mask().to_vec() == first.mask().to_vec() && chain.to_vec<float>()[1] == 20.f && chain.to_vec<float>()[2] == 300.f);
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1}), w = CellBuffer::from_vec<uint16_t>({1}), l = CellBuffer::from_vec<uint8_t>({1, 2});
            int threw = 0;
            try { composite(CB{}); } catch (const Error&) { ++threw; }
            try { composite(CB{&a, &w}); } catch (const Error&) { ++threw; }
            try { composite(CB{&a, &l}); } catch (const Error&) { ++threw; }
            try { composite(CB(65, &a)); } catch (const Error&) { ++threw; }
            try { composite(CB{&a, &a}, static_cast<ec_composite_op>(6)); } catch (const Error&) { ++threw; }
            const MaskedCellBuffer m(CellBuffer::from_vec<uint8_t>({1}), Mask::new_({true}));
            try { composite(MB{&m, &m}, EC_COMPOSITE_FIRST, 3); } catch (const Error&) { ++threw; }
            CHECK(threw == 6);
            CHECK(composite(CB(64, &a), EC_COMPOSITE_SUM).to_vec<double>() == std::vector<double>({64.0}));
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
            CHECK(SB::composite({&sv, &sw, &sx}, EC_COMPOSITE_MAX).to_vec<int16_t>() == composite(CB{&bv, &bw, &bx}, EC_COMPOSITE_MAX).to_vec<int16_t>());
            std::vector<bool> bmv(mv.begin(), mv.end()), bmw(mw.begin(), mw.end());
            const MaskedCellBuffer qv(bv.clone(), Mask::new_(bmv)), qw(bw.clone(), Mask::new_(bmw));
            std::optional<SB> om, aux;
            const SB mean = SB::composite({&sv, &sw}, EC_COMPOSITE_MEAN, 2, {&smv, &smw}, &om, &aux);
            CellBuffer whole_aux(CellType::UInt8, 0);
            const MaskedCellBuffer whole = composite(MB{&qv, &qw}, EC_COMPOSITE_MEAN, 2, &whole_aux);
            CHECK(mean.to_vec<double>() == whole.to_vec<double>() && aux->to_vec<uint8_t>() == whole_aux.to_vec<uint8_t>());
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
