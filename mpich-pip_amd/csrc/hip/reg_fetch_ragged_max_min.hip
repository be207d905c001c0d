// reg_fetch_ragged_max_min.hip -- k_reduce_fetch_ragged for the pairs of MPIR_PAIRS_MAX_MIN (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_fetch_ragged, MPIR_PAIRS_MAX_MIN)
