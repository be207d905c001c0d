// reg_chunked_pairs_x87.hip -- k_chunk_partials and k_fold_partials for the pairs of MPIR_PAIRS_PAIRS_X87 (kernel_table.hpp).
#include "kernel_table.hpp"
using namespace mpir_hip;
MPIR_REG_FAMILY_UNIT(reg_chunked, MPIR_PAIRS_PAIRS_X87)
