// ec_focal_rank / ec_focal_majority kernels for the cell types of 1 byte (see ec_focal_rank_tu.hpp).
#define EC_FOCAL_RANK_WIDTH 1
#include "ec_focal_rank_tu.hpp"
