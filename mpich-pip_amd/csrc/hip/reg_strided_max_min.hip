// reg_strided_max_min.hip -- k_reduce_strided for reg_max_min.hip's pairs:
// MPI_MAX / MPI_MIN on integers and reals.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_strided<OpMax, T>(MPIR_HIP_OP_MAX, E); reg_strided<OpMin, T>(MPIR_HIP_OP_MIN, E);
        FOR_INTS(X) FOR_REALS(X)
#undef X
    }
} init;
}  // namespace
