// reg_fetch_ordered_pairs_x87.hip -- k_reduce_fetch_indexed_ordered for
// reg_pairs_x87.hip's pairs but REPLACE: MAXLOC / MINLOC on the pair types, and the
// long double rows.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_fetch_ordered<OpMaxloc, T>(MPIR_HIP_OP_MAXLOC, E); reg_fetch_ordered<OpMinloc, T>(MPIR_HIP_OP_MINLOC, E);
        FOR_PAIRS(X)
#undef X
        reg_fetch_ordered<OpSum, x80>(MPIR_HIP_OP_SUM, MPIR_HIP_F80);
        reg_fetch_ordered<OpProd, x80>(MPIR_HIP_OP_PROD, MPIR_HIP_F80);
        reg_fetch_ordered<OpMax, x80>(MPIR_HIP_OP_MAX, MPIR_HIP_F80);
        reg_fetch_ordered<OpMin, x80>(MPIR_HIP_OP_MIN, MPIR_HIP_F80);
        reg_fetch_ordered<OpLxor, x80>(MPIR_HIP_OP_LXOR, MPIR_HIP_F80);
        reg_fetch_ordered<OpSum, cx80>(MPIR_HIP_OP_SUM, MPIR_HIP_CF80);
        reg_fetch_ordered<OpProd, cx80>(MPIR_HIP_OP_PROD, MPIR_HIP_CF80);
        reg_fetch_ordered<OpMaxloc, pldint>(MPIR_HIP_OP_MAXLOC, MPIR_HIP_PLDOUBLEINT);
        reg_fetch_ordered<OpMinloc, pldint>(MPIR_HIP_OP_MINLOC, MPIR_HIP_PLDOUBLEINT);
    }
} init;
}  // namespace
