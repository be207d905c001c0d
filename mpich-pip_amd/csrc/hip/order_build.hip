// order_build.hip -- the device sort behind MPIR_Hip_order_build: a stable sort
// of (displacement, block number) pairs by the signed 64-bit displacement, whose
// sorted block numbers are the order table of MPIR_Hip_reduce_indexed_ordered.
// rocPRIM's radix_sort_pairs (an LSD radix sort, or its merge sort for small
// tables: both stable, signed keys handled) with a counting iterator as the
// values' input, so no table of block numbers is written first.  A unit of its
// own: rocPRIM's headers are the slowest to compile in the library, and nothing
// else here includes them.  (<rocprim/rocprim.hpp>, the umbrella, is not used:
// the radix sort's own header is all this needs.)  The kernel behind
// MPIR_Hip_runs_build sits here too, beside the table it reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

// (declared in shim_ctx.hpp, which this unit leaves out: it needs none of the
// kernel templates)
namespace mpir_hip {
size_t order_worksize(uint64_t n);
hipError_t order_sort(const int64_t *displs, uint64_t n, int *order, void *work, size_t work_bytes, hipStream_t s,
                      size_t *need);
hipError_t runs_build(const int64_t *displs, const int *order, uint64_t n, int *runstart, hipStream_t s);

namespace {
constexpr size_t kOrderAlign = 256;
size_t order_keys_bytes(uint64_t n) { return ((size_t)n * sizeof(int64_t) + kOrderAlign - 1) & ~(kOrderAlign - 1); }
}  // namespace

// What order_sort may use of `work`, from n alone (host arithmetic, no GPU):
// room to align the caller's pointer, the sorted keys (rocPRIM wants an output
// for them), and a bound on rocPRIM's own temporary storage, which depends on
// the sort it picks and the tuning of the device it runs on and cannot be asked
// without one: the double buffers of keys and values (12 n), the one-sweep
// sort's look-back states (at most 8 bytes x 256 digits per 256 items, 8 n, with
// any tuning), its histograms and alignment (1 MiB covers them).  order_sort
// asks rocPRIM for the true figure and refuses to run past the bound.
size_t order_worksize(uint64_t n) {
    return kOrderAlign + order_keys_bytes(n) + (size_t)n * 20 + ((size_t)1 << 20);
}

// Enqueue on `s` the sort of displs[0..n) (device memory) into order[0..n)
// (device memory), n > 0.  hipErrorInvalidValue where work_bytes is less than
// the sort needs (*need: what it needs), which order_worksize(n) always covers.
hipError_t order_sort(const int64_t *displs, uint64_t n, int *order, void *work, size_t work_bytes, hipStream_t s,
                      size_t *need) {
    const uintptr_t w = (reinterpret_cast<uintptr_t>(work) + kOrderAlign - 1) & ~(uintptr_t)(kOrderAlign - 1);
    const size_t lead = w - reinterpret_cast<uintptr_t>(work);
    int64_t *keys_out = reinterpret_cast<int64_t *>(w);
    void *tmp = reinterpret_cast<void *>(w + order_keys_bytes(n));
    size_t tmp_bytes = 0;
    const rocprim::counting_iterator<int> blocks(0);
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, displs, keys_out, blocks, order, (size_t)n, 0, 64, s);
    if (e != hipSuccess) return e;
    *need = lead + order_keys_bytes(n) + tmp_bytes;
    if (*need > work_bytes) return hipErrorInvalidValue;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, displs, keys_out, blocks, order, (size_t)n, 0, 64, s);
}


// The runstart table behind MPIR_Hip_runs_build: runstart[p] = the smallest
// sorted position q with displs[order[q]] == displs[order[p]].  One kernel, a
// lane per position: a lower-bound binary search over displs[order[.]] in
// [0, p], which is non-decreasing where `order` is what it must be.  Every order
// entry is clamped into [0, n), so a wrong device table gives wrong entries (all
// in [0, p]) but no read outside the tables.  No scratch, nothing asked of the
// runtime: the launch can be captured into a graph.
namespace {
__global__ __launch_bounds__(256) void k_runs_build(const int64_t *displs, const int *order, uint32_t n, int *runstart) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    auto at = [&](uint32_t q) {
        const uint32_t k = (uint32_t)order[q];
        return displs[k < n ? k : n - 1];
    };
    const int64_t d = at((uint32_t)p);
    uint32_t lo = 0, hi = (uint32_t)p;          // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (at(mid) < d) lo = mid + 1;
        else hi = mid;
    }
    runstart[p] = (int)lo;
}
}  // namespace

// Enqueue on `s` the build of runstart[0..n) from displs and order (all device memory), 0 < n <= INT32_MAX
hipError_t runs_build(const int64_t *displs, const int *order, uint64_t n, int *runstart, hipStream_t s) {
    hipLaunchKernelGGL(k_runs_build, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, displs, order, (uint32_t)n, runstart);
    return hipGetLastError();
}

}  // namespace mpir_hip
