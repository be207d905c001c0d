// reg_subarray_max_min.hip -- k_reduce_subarray for the pairs of MPIR_PAIRS_MAX_MIN (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_subarray, MPIR_PAIRS_MAX_MIN)
