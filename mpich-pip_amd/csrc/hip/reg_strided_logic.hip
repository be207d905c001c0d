// reg_strided_logic.hip -- k_reduce_strided for reg_logic.hip's pairs: LAND /
// LOR / LXOR on integers, LXOR on the reals, BAND / BOR / BXOR on integers.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_strided<OpLand, T>(MPIR_HIP_OP_LAND, E); reg_strided<OpLor, T>(MPIR_HIP_OP_LOR, E); \
                reg_strided<OpLxor, T>(MPIR_HIP_OP_LXOR, E);
        FOR_INTS(X)
#undef X
#define X(E, T) reg_strided<OpLxor, T>(MPIR_HIP_OP_LXOR, E);
        FOR_REALS(X)
#undef X
#define X(E, T) reg_strided<OpBand, T>(MPIR_HIP_OP_BAND, E); reg_strided<OpBor, T>(MPIR_HIP_OP_BOR, E); \
                reg_strided<OpBxor, T>(MPIR_HIP_OP_BXOR, E);
        FOR_INTS(X)
#undef X
    }
} init;
}  // namespace
