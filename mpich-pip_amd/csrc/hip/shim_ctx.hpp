// shim_ctx.hpp -- what the units of the C-ABI shim share (hip_reduce.hip: the
// tables, knobs, the single call's routes and the combine; table_calls.hip: the
// calls on many blocks at once; classify.hip: the pointer classifier): the
// per-thread context pool with its streams, events and buffers, the error text,
// DeviceScope, the operand classes, the classifier's and direct_dispatch.hip's
// interfaces and what hip_reduce.hip lends table_calls.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>

#include "mpir_hip_reduce.h"
#include "kernel_table.hpp"

namespace mpir_hip {

// direct_dispatch.hip
int direct_reduce(int dev, int op, int elem, const ReducePlan &p, int *rc);
uint64_t direct_calls();
void direct_profile(int on);
uint64_t direct_last_kernel_ns();
int direct_state(int dev);
int direct_prepare(int dev);
void direct_last_split(uint64_t out[4]);
uint64_t direct_busy_skips();
uint64_t direct_kernarg_writes();
uint32_t direct_test_write_delay_us(uint32_t us);
void direct_test_fail_probe();
void direct_placement(int dev, int out[5]);

// order_build.hip (the sort of MPIR_Hip_order_build: see there)
size_t order_worksize(uint64_t n);
hipError_t order_sort(const int64_t *displs, uint64_t n, int *order, void *work, size_t work_bytes, hipStream_t s,
                      size_t *need);
hipError_t runs_build(const int64_t *displs, const int *order, uint64_t n, int *runstart, hipStream_t s);

// hip_reduce.hip, for table_calls.hip (the library does not export them): an
// element class's bytes, the range check of (op, elem), and a synchronous call's wait
#pragma GCC visibility push(hidden)
extern const size_t g_elem_size[MPIR_HIP_NELEMS];
bool pair_in_range(int op, int elem);
int wait_stream(int dev, hipStream_t s);
#pragma GCC visibility pop

// ------------------------------------------------------------ per-thread state
constexpr int kMaxDev = 64;
constexpr int kMaxStageSlots = 8;

enum { S_MAIN = 0, S_UP = 1, S_COMP = 2, S_DOWN = 3, S_NSTREAMS = 4 };

struct DevCtx {
    hipStream_t stream[S_NSTREAMS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_up[kMaxStageSlots] = {}, ev_comp[kMaxStageSlots] = {}, ev_free[kMaxStageSlots] = {};
    volatile uint32_t *flag = nullptr;   // pinned completion word (wait mode "flag")
    uint32_t seq = 0;
    bool main_pending = false;   // work enqueued on stream[S_MAIN] without a wait (stream variant)
    char *scratch = nullptr;     // staging slots x (in, inout) x chunk, or multi-operand temporaries
    size_t scratch_bytes = 0;
    char *bounce = nullptr;      // pinned host bounce slots x (in, inout) x chunk (pageable operands)
    size_t bounce_bytes = 0;
    char *zc = nullptr;          // pinned, device-mapped slot for small mixed-residency calls
    size_t zc_bytes = 0;
    char *tables = nullptr;      // device copy of a synchronous indexed / ragged call's host tables
    size_t tables_bytes = 0;
};

// HIP's verdict on host pages the HSA query does not know (classify below)
struct HostVerdict {
    uintptr_t page = ~(uintptr_t)0;
    int loc = 0;
    int dev = 0;
};
constexpr int kVerdicts = 16;

struct ThreadCtx {
    DevCtx dev[kMaxDev];
    char err[256] = {0};
    HostVerdict verdict[kVerdicts];
    ThreadCtx *next = nullptr;
};

// Per-thread contexts (streams, events, completion word, scratch) come from a
// process-wide pool: a thread takes one at its first call and hands it back
// when it exits, so an application that starts and ends many threads reuses
// a bounded set of HIP streams instead of leaking one set per thread.  A
// handed-back context keeps its streams (work still queued on them stays in
// order for the next owner); thread exit makes no HIP call, so it is safe at
// process teardown too.
inline std::mutex g_pool_mu;
inline ThreadCtx *g_pool = nullptr;
inline int g_ctx_created = 0;

struct CtxHolder {
    ThreadCtx *c = nullptr;
    ThreadCtx &get() {
        if (!c) {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            if (g_pool) {
                c = g_pool;
                g_pool = c->next;
                c->next = nullptr;
                c->err[0] = 0;
                for (HostVerdict &v : c->verdict) v = HostVerdict();    // a new thread's own verdicts
            } else {
                c = new ThreadCtx();
                ++g_ctx_created;
            }
        }
        return *c;
    }
    ~CtxHolder() {
        if (!c) return;
        std::lock_guard<std::mutex> lk(g_pool_mu);
        c->next = g_pool;
        g_pool = c;
        c = nullptr;
    }
};

inline thread_local CtxHolder t_holder;
inline ThreadCtx &ctx() { return t_holder.get(); }

inline int set_err(hipError_t e, const char *what) {
    snprintf(ctx().err, sizeof(ctx().err), "%s: %s", what, hipGetErrorString(e));
    return MPIR_HIP_ERUNTIME;
}

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return set_err(e_, #call); } while (0)

// `dev` is the calling thread's current device while the scope lives: the
// current one is recorded, changed only if it differs, and put back (an error
// there is ignored) when the scope ends.  A query or a change that failed is
// reported as HIPCHK would:  DeviceScope on(dev);  if (!on.ok()) return on.err();
class DeviceScope {
  public:
    explicit DeviceScope(int dev) {
        if ((e_ = hipGetDevice(&cur_)) != hipSuccess) {
            what_ = "hipGetDevice(&cur)";
        } else if (cur_ != dev) {
            if ((e_ = hipSetDevice(dev)) != hipSuccess) what_ = "hipSetDevice(dev)";
            else back_ = true;
        }
    }
    ~DeviceScope() {
        if (back_) (void)hipSetDevice(cur_);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    bool ok() const { return e_ == hipSuccess; }
    int err() const { return set_err(e_, what_); }

  private:
    int cur_ = 0;
    bool back_ = false;
    hipError_t e_ = hipSuccess;
    const char *what_ = "";
};

inline int get_stream(int dev, int slot, hipStream_t *out) {
    DevCtx &d = ctx().dev[dev];
    if (!d.stream[slot]) {
        // Blocking stream (not hipStreamNonBlocking): it orders after work the
        // caller queued on the legacy null stream for these buffers.
        HIPCHK(hipStreamCreate(&d.stream[slot]));
    }
    *out = d.stream[slot];
    return MPIR_HIP_OK;
}

inline int get_stage_events(int dev, int nslots) {
    DevCtx &d = ctx().dev[dev];
    for (int k = 0; k < nslots; ++k) {
        if (!d.ev_up[k]) HIPCHK(hipEventCreateWithFlags(&d.ev_up[k], hipEventDisableTiming));
        if (!d.ev_comp[k]) HIPCHK(hipEventCreateWithFlags(&d.ev_comp[k], hipEventDisableTiming));
        if (!d.ev_free[k]) HIPCHK(hipEventCreateWithFlags(&d.ev_free[k], hipEventDisableTiming));
    }
    return MPIR_HIP_OK;
}

inline int get_scratch(int dev, size_t bytes, char **out) {
    DevCtx &d = ctx().dev[dev];
    if (d.scratch_bytes < bytes) {
        // stream-ordered users of the old scratch may still be in flight
        if (d.scratch) HIPCHK(hipDeviceSynchronize());
        if (d.scratch) HIPCHK(hipFree(d.scratch));
        d.scratch = nullptr;
        d.scratch_bytes = 0;
        HIPCHK(hipMalloc(&d.scratch, bytes));
        d.scratch_bytes = bytes;
    }
    *out = d.scratch;
    return MPIR_HIP_OK;
}

inline int get_bounce(int dev, size_t bytes, char **out) {
    DevCtx &d = ctx().dev[dev];
    if (d.bounce_bytes < bytes) {
        if (d.bounce) HIPCHK(hipDeviceSynchronize());   // in-flight copies may still read it
        if (d.bounce) HIPCHK(hipHostFree(d.bounce));
        d.bounce = nullptr;
        d.bounce_bytes = 0;
        HIPCHK(hipHostMalloc(&d.bounce, bytes, hipHostMallocDefault));
        d.bounce_bytes = bytes;
    }
    *out = d.bounce;
    return MPIR_HIP_OK;
}

// the calling thread's small pinned slot (fine-grained: kernel stores land in
// host memory without a cache flush)
inline int get_zc(int dev, size_t bytes, char **out) {
    DevCtx &d = ctx().dev[dev];
    if (d.zc_bytes < bytes) {
        // a synchronous call's kernel is done with the old slot when it returned
        if (d.zc) HIPCHK(hipHostFree(d.zc));
        d.zc = nullptr;
        d.zc_bytes = 0;
        const size_t want = bytes < ((size_t)64 << 10) ? ((size_t)64 << 10) : bytes;
        HIPCHK(hipHostMalloc(&d.zc, want, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
        d.zc_bytes = want;
    }
    *out = d.zc;
    return MPIR_HIP_OK;
}

// the calling thread's table buffer on `dev`: one call's host tables side by
// side in `bytes` (MPIR_Hip_reduce_indexed's two displacement tables,
// MPIR_Hip_reduce_ragged's two and its starts, MPIR_Hip_reduce_indexed_ordered's
// two and its order; a synchronous MPIR_Hip_order_build's host side and, where
// the caller gave none, its work).  Not `scratch`: stream-variant work may still be reading that,
// while this buffer's only readers are synchronous calls, complete when they
// returned -- but for one that failed after it enqueued, hence the wait.
inline int get_tables(int dev, size_t bytes, char **out) {
    DevCtx &d = ctx().dev[dev];
    if (d.tables_bytes < bytes) {
        if (d.tables) HIPCHK(hipDeviceSynchronize());
        if (d.tables) HIPCHK(hipFree(d.tables));
        d.tables = nullptr;
        d.tables_bytes = 0;
        const size_t want = bytes < ((size_t)64 << 10) ? ((size_t)64 << 10) : bytes;
        HIPCHK(hipMalloc(&d.tables, want));
        d.tables_bytes = want;
    }
    *out = d.tables;
    return MPIR_HIP_OK;
}

// ------------------------------------------------- operand classes (classify.hip)
// LOC_HOST: pageable (or unknown to HIP); LOC_PINNED: page-locked host memory
// (hipHostMalloc / hipHostRegister), which DMA copies and kernels may still be
// writing when the caller hands it over
enum Loc { LOC_HOST = 0, LOC_DEVICE = 1, LOC_PINNED = 2 };

// the limits a kept verdict depends on (verdict_reusable; hip_reduce.hip)
uint64_t host_max_bytes();
uint64_t mixed_max_bytes();

bool gpu_runtime_started();
Loc classify(const void *p, int *dev, bool reuse = true, bool *kept = nullptr);
// the device allocation that answered last (classify_in_span)
struct DeviceSpan {
    uintptr_t lo = 0, hi = 0;
    int dev = -1;
};
Loc classify_in_span(const void *p, int *dev, DeviceSpan &span);
bool verdict_reusable(uint64_t bytes);
int device_count();

}  // namespace mpir_hip
