// reg_fetch_ordered_bytes.hip -- k_reduce_fetch_indexed_ordered for MPI_NO_OP (every
// block of a run receives the old target) and MPI_REPLACE (a chain of swaps): byte
// operations, one kernel per element size from 1 to 32 bytes, whatever the element
// class.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
        reg_fetch_ordered_bytes<0>();
        reg_fetch_ordered_bytes<1>();
        reg_fetch_ordered_bytes<2>();
        reg_fetch_ordered_bytes<3>();
        reg_fetch_ordered_bytes<4>();
        reg_fetch_ordered_bytes<5>();
    }
} init;
}  // namespace
