// ec_focal_rank / ec_focal_majority kernels for the cell types of 8 bytes (see ec_focal_rank_tu.hpp).
#define EC_FOCAL_RANK_WIDTH 8
#include "ec_focal_rank_tu.hpp"
