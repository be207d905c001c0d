// reg_subarray_sum_prod.hip -- k_reduce_subarray for the pairs of MPIR_PAIRS_SUM_PROD (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_subarray, MPIR_PAIRS_SUM_PROD)
