// reg_strided_pairs_x87.hip -- k_reduce_strided for reg_pairs_x87.hip's pairs
// but REPLACE: MAXLOC / MINLOC on the pair types, and the long double rows.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_strided<OpMaxloc, T>(MPIR_HIP_OP_MAXLOC, E); reg_strided<OpMinloc, T>(MPIR_HIP_OP_MINLOC, E);
        FOR_PAIRS(X)
#undef X
        reg_strided<OpSum, x80>(MPIR_HIP_OP_SUM, MPIR_HIP_F80);
        reg_strided<OpProd, x80>(MPIR_HIP_OP_PROD, MPIR_HIP_F80);
        reg_strided<OpMax, x80>(MPIR_HIP_OP_MAX, MPIR_HIP_F80);
        reg_strided<OpMin, x80>(MPIR_HIP_OP_MIN, MPIR_HIP_F80);
        reg_strided<OpLxor, x80>(MPIR_HIP_OP_LXOR, MPIR_HIP_F80);
        reg_strided<OpSum, cx80>(MPIR_HIP_OP_SUM, MPIR_HIP_CF80);
        reg_strided<OpProd, cx80>(MPIR_HIP_OP_PROD, MPIR_HIP_CF80);
        reg_strided<OpMaxloc, pldint>(MPIR_HIP_OP_MAXLOC, MPIR_HIP_PLDOUBLEINT);
        reg_strided<OpMinloc, pldint>(MPIR_HIP_OP_MINLOC, MPIR_HIP_PLDOUBLEINT);
    }
} init;
}  // namespace
