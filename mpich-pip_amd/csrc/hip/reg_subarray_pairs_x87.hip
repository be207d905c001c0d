// reg_subarray_pairs_x87.hip -- k_reduce_subarray for the pairs of MPIR_PAIRS_PAIRS_X87 (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_subarray, MPIR_PAIRS_PAIRS_X87)
