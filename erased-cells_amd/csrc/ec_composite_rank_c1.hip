// ec_composite_rank kernels for the cell types of 1 byte (see ec_composite_rank_tu.hpp).
#define EC_RANK_WIDTH 1
#include "ec_composite_rank_tu.hpp"
