// reg_fetch_sum_prod.hip -- k_reduce_fetch for the pairs of MPIR_PAIRS_SUM_PROD (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_fetch, MPIR_PAIRS_SUM_PROD)
