// ec_zonal_host.hpp — what the host sides of the two zonal families (ec_zonal.hip, ec_zonal_table.hip) share: the dispatch over
// the zone raster's cell type.  Host code only; the kernels are each family's own.
#pragma once

#include "ec_dispatch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_U8 == 0 && EC_U16 == 1 && EC_I32 == 6, "ec_zonal_plan.hpp names the zone types by their codes");

// f(cell_tag<ZT>) for the zone type zt (checked before: one of the three)
template <typename F>
static ec_status with_zone_type(int zt, F&& f) {
    switch (zt) {
        case EC_U8: return f(ecl::cell_tag<uint8_t>{});
        case EC_U16: return f(ecl::cell_tag<uint16_t>{});
        case EC_I32: return f(ecl::cell_tag<int32_t>{});
    }
    return kTypeChecked;
}

}  // namespace ecd
