// reg_fetch_ordered_logic.hip -- k_reduce_fetch_indexed_ordered for reg_logic.hip's
// pairs: LAND / LOR / LXOR on integers, LXOR on the reals, BAND / BOR / BXOR on
// integers.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
#define X(E, T) reg_fetch_ordered<OpLand, T>(MPIR_HIP_OP_LAND, E); reg_fetch_ordered<OpLor, T>(MPIR_HIP_OP_LOR, E); \
                reg_fetch_ordered<OpLxor, T>(MPIR_HIP_OP_LXOR, E);
        FOR_INTS(X)
#undef X
#define X(E, T) reg_fetch_ordered<OpLxor, T>(MPIR_HIP_OP_LXOR, E);
        FOR_REALS(X)
#undef X
#define X(E, T) reg_fetch_ordered<OpBand, T>(MPIR_HIP_OP_BAND, E); reg_fetch_ordered<OpBor, T>(MPIR_HIP_OP_BOR, E); \
                reg_fetch_ordered<OpBxor, T>(MPIR_HIP_OP_BXOR, E);
        FOR_INTS(X)
#undef X
    }
} init;
}  // namespace
