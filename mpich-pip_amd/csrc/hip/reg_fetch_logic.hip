// reg_fetch_logic.hip -- k_reduce_fetch for the pairs of MPIR_PAIRS_LOGIC (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_fetch, MPIR_PAIRS_LOGIC)
