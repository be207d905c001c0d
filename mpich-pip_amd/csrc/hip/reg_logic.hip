// reg_logic.hip -- the single call's kernels for the pairs of MPIR_PAIRS_LOGIC (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_UNIT(reg, reg_wide, MPIR_PAIRS_LOGIC)
