// reg_fetch_ordered_max_min.hip -- k_reduce_fetch_indexed_ordered for
// reg_max_min.hip's pairs: MPI_MAX / MPI_MIN on integers and reals.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_fetch_ordered<OpMax, T>(MPIR_HIP_OP_MAX, E); reg_fetch_ordered<OpMin, T>(MPIR_HIP_OP_MIN, E);
        FOR_INTS(X) FOR_REALS(X)
#undef X
    }
} init;
}  // namespace
