// reg_fetch_ordered_pairs_x87.hip -- k_reduce_fetch_indexed_ordered for the pairs of MPIR_PAIRS_PAIRS_X87 (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_fetch_ordered, MPIR_PAIRS_PAIRS_X87)
