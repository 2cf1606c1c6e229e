// ec_composite_rank kernels for the cell types of 2 bytes (see ec_composite_rank_tu.hpp).
#define EC_RANK_WIDTH 2
#include "ec_composite_rank_tu.hpp"
