// reg_strided_logic.hip -- k_reduce_strided for the pairs of MPIR_PAIRS_LOGIC (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_strided, MPIR_PAIRS_LOGIC)
