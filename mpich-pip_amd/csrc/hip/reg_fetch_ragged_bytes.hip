// reg_fetch_ragged_bytes.hip -- k_reduce_fetch_ragged for MPI_NO_OP (a pack of
// the pieces) and MPI_REPLACE (a swap): byte operations, one kernel per element
// size from 1 to 32 bytes, whatever the element class.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
        reg_fetch_ragged_bytes<0>();
        reg_fetch_ragged_bytes<1>();
        reg_fetch_ragged_bytes<2>();
        reg_fetch_ragged_bytes<3>();
        reg_fetch_ragged_bytes<4>();
        reg_fetch_ragged_bytes<5>();
    }
} init;
}  // namespace
