// reg_fetch_ordered_sum_prod.hip -- k_reduce_fetch_indexed_ordered for
// reg_sum_prod.hip's pairs: MPI_SUM / MPI_PROD on integers, reals and complex.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_fetch_ordered<OpSum, T>(MPIR_HIP_OP_SUM, E); reg_fetch_ordered<OpProd, T>(MPIR_HIP_OP_PROD, E);
        FOR_INTS(X) FOR_REALS(X) FOR_CPLX(X)
#undef X
    }
} init;
}  // namespace
