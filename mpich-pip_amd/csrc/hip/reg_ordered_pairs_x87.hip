// reg_ordered_pairs_x87.hip -- k_reduce_indexed_ordered for the pairs of MPIR_PAIRS_PAIRS_X87 (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_ordered, MPIR_PAIRS_PAIRS_X87)
