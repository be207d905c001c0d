// reg_pairs_x87.hip -- the single call's kernels for the pairs of MPIR_PAIRS_PAIRS_X87
// (kernel_table.hpp), and REPLACE (a byte copy for every class, MPIR_Localcopy of a basic type).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_UNIT(reg, reg_wide, MPIR_PAIRS_PAIRS_X87)
namespace {
struct InitReplace {
    InitReplace() {
        for (int e = 1; e < MPIR_HIP_NELEMS; ++e) reg<OpReplace, uint8_t>(MPIR_HIP_OP_REPLACE, e);
    }
} init_replace;
}  // namespace
