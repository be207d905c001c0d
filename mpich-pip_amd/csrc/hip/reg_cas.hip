// reg_cas.hip -- k_cas_indexed_ordered and k_cas_contig (MPIR_Hip_cas_indexed_ordered,
// the ordered compare-and-swap): byte comparisons, one pair of kernels per element
// size from 1 to 8 bytes, whatever the element class.
#include "kernel_table.hpp"

using namespace mpir_hip;

namespace {
struct Init {
    Init() {
        reg_cas<0>();
        reg_cas<1>();
        reg_cas<2>();
        reg_cas<3>();
    }
} init;
}  // namespace
