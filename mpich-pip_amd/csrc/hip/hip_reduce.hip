// hip_reduce.hip -- C-ABI shim: the kernel tables, the knobs, the routes of a
// call (host combine, device, mixed pinned slot, staged pipeline) and the
// MPIR_Hip_* entry points.  The per-thread streams and buffers are in
// shim_ctx.hpp, pointer classification in classify.hip, the host's thread
// pools and CPU share in host_env.hip.
//
// Replaces the scalar loop body the reference runs inside each MPIR_<OP>
// (src/mpi/coll/op/op*.c via MPIR_OP_TYPE_REDUCE_CASE,
// src/include/mpir_op_util.h:48-55).  Declared in include/mpir_hip_reduce.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>

#include "mpir_hip_reduce.h"
#include "kernel_table.hpp"
#include "host_env.hpp"
#include "shim_ctx.hpp"

using namespace mpir_hip;

namespace mpir_hip {
// Kernel tables (kernel_table.hpp), filled by the registration units
// reg_*.hip at static-initialisation time; zero-initialised storage here.
Entry g_table[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
multi_fn g_multi[MPIR_HIP_NOPS][MPIR_HIP_NELEMS][2][kMultiMaxP - 1];
BatchEntry g_batch[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
StridedEntry g_strided[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
IndexedEntry g_indexed[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
OrderedEntry g_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
RaggedEntry g_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchEntry g_fetch[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchRaggedEntry g_fetch_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchRaggedEntry g_fetch_ragged_bytes[2][kFetchRaggedSizes];
FetchOrderedEntry g_fetch_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchOrderedEntry g_fetch_ordered_bytes[2][kFetchRaggedSizes];
CasEntry g_cas[kCasSizes];

// Strided rows of at least this many bytes take the wide form (one row's tiles
// per G workgroups), shorter ones the narrow form (rows flattened into units):
// MPIR_CVAR_REDUCE_LOCAL_STRIDED_WIDE_KB, default 16, one tile (DESIGN.md §Strided
// reductions has the sweep behind it); MPIR_Hip_set_strided_wide_bytes() at run
// time.  At most 1 GiB, so that a narrow row's units fit 32 bits.
constexpr uint64_t kStridedWideMax = (uint64_t)1 << 30;
std::atomic<uint64_t> g_strided_wide{(uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_STRIDED_WIDE_KB", 0, 1L << 20, 16) << 10};
// MPIR_Hip_strided_test_max_groups: the calling thread's per-launch workgroup cap (0: kBatchMaxGroups)
thread_local uint64_t t_strided_cap = 0;

// Results of at most this many bytes are stored sc1 (into the Infinity Cache)
// rather than nt: MPIR_CVAR_REDUCE_LOCAL_KEEP_MB (0 = every store nt), default
// 64 (reduce_kernels.hpp, kKeepBytes); MPIR_Hip_set_keep_bytes() changes it at
// run time (an MPI_T-style cvar write).
static_assert(kKeepBytes == (uint64_t)64 << 20, "the knob's default below is kKeepBytes");
std::atomic<uint64_t> g_keep{(uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_KEEP_MB", 0, 4096, 64) << 20};
uint64_t keep_bytes() { return g_keep.load(std::memory_order_relaxed); }

// ... and results of at most this many bytes are stored nt again: below it the
// sc1 stores cost the call more at the kernel's end than a next reader gains
// from finding the result in the Infinity Cache (tools/keep_small_ab.py,
// profiles/r06/keep_small_r06z.log: nt ahead by 0.3-1.0 us per call from 16 KiB
// to 16 MiB whether or not the next call re-reads the result; sc1 ahead by
// 0.6-1.7 us at 32-64 MiB when it does).  MPIR_CVAR_REDUCE_LOCAL_KEEP_MIN_MB,
// default 16; MPIR_Hip_set_keep_min_bytes() at run time.
std::atomic<uint64_t> g_keep_min{(uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_KEEP_MIN_MB", 0, 4096, 16) << 20};

uint64_t keep_for(uint64_t vbytes) {
    return vbytes > g_keep_min.load(std::memory_order_relaxed) && vbytes <= keep_bytes() ? vbytes : 0;
}

// MPIR_Hip_combine_set_flags: the calling thread's combine flags
thread_local int t_combine_flags = 0;
bool multi_uncapped() { return (t_combine_flags & MPIR_HIP_COMBINE_UNCAPPED) != 0; }

// Both operands in host memory and at most this many bytes each: the combine
// runs on the host (host_loop, the same functors as the kernels; split over
// the copy pool's threads from host_split_bytes()) instead of a staged GPU
// round trip -- SURVEY.md §8b's dispatch rule ("both host -> CPU").  Measured
// on the MI355X host, fp32 SUM (tools/host_latency.py, tools/host_crossover.py,
// profiles/archive/r02/host_latency*.log, host_crossover.log): the host combine wins at
// every size -- 0.4 us against 48 us staged at 4 B, 35 against 125-194 us at
// 1 MiB, 108 against 299-466 us at 4 MiB, 5.6-5.7 against 10.7-13.9 ms at 256 MiB
// (staging is PCIe-bound, ~50 GB/s up).  MPIR_CVAR_REDUCE_LOCAL_HOST_MAX_KB:
// unset or negative = no limit (default), 0 = always stage through the GPU;
// MPIR_Hip_set_host_max_bytes() changes it at run time (as an MPI_T cvar write).
// (this limit and the next are also what classify.hip's verdict_reusable reads)
std::atomic<uint64_t> g_host_max{[] {
    const char *e = getenv("MPIR_CVAR_REDUCE_LOCAL_HOST_MAX_KB");
    if (!e) return ~(uint64_t)0;
    const long long kb = atoll(e);
    return kb < 0 ? ~(uint64_t)0 : ((uint64_t)kb << 10);
}()};
uint64_t host_max_bytes() { return g_host_max.load(std::memory_order_relaxed); }

// One operand in host memory, the other on a device, at most this many bytes:
// the host operand is copied into a pinned, device-mapped slot and the kernel
// reads (and for a host inoutbuf writes) it there over PCIe -- one dispatch, no
// DMA copies, no staging pipeline.  Measured fp32 SUM host -> device at count 1:
// 33 us through the staged pipeline (profiles/archive/r02/host_latency.log).
// MPIR_CVAR_REDUCE_LOCAL_MIXED_MAX_KB (default 1024; 0 = always stage).
uint64_t mixed_max_bytes() {
    static const uint64_t v = (uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_MIXED_MAX_KB", 0, 1L << 20, 1024) << 10;
    return v;
}
}  // namespace mpir_hip

namespace {

const size_t g_elem_size[MPIR_HIP_NELEMS] = {
    0, 1, 1, 2, 2, 4, 4, 8, 8, 2, 4, 8, 8, 16, 8, 8, 16, 8, 16, 16, 32, 32,
};
static_assert(sizeof(g_elem_size) / sizeof(g_elem_size[0]) == MPIR_HIP_NELEMS, "one size per element class");

bool pair_in_range(int op, int elem) { return op > 0 && op < MPIR_HIP_NOPS && elem > 0 && elem < MPIR_HIP_NELEMS; }

// Staging of host (or other-device) operands: chunks of `stage_chunk()` bytes
// per operand flow through a three-stage pipeline -- H2D copies on stream
// "up", the kernel on "comp", the D2H copy-back on "down" -- over
// `stage_slots()` device scratch slots, so host->device and device->host
// transfers run at the same time (PCIe is full duplex).  Events order the
// stages of one chunk and stop a slot from being refilled before its
// copy-back has read it.  Defaults 16 MiB x 3 slots (tools/archive/stage_sweep.py,
// profiles/archive/r01s3_stage_sweep.log: pinned 71.8 GiB/s, pageable 66.3 with the
// bounce path below; 32 MiB chunks leave a longer tail of copy-outs).
// MPIR_CVAR_REDUCE_LOCAL_STAGE_CHUNK_MB / MPIR_CVAR_REDUCE_LOCAL_STAGE_SLOTS override.
// (function-local statics: initialised once, thread-safe)
uint64_t stage_chunk() {
    static const uint64_t v = (uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_STAGE_CHUNK_MB", 1, 1024, 16) << 20;
    return v;
}
int stage_slots() {
    static const int v = (int)cvar_long("MPIR_CVAR_REDUCE_LOCAL_STAGE_SLOTS", 2, kMaxStageSlots, 3);
    return v;
}

// copies into / out of the mixed path's slot of at least this many bytes go
// through the copy pool (MPIR_CVAR_REDUCE_LOCAL_MIXED_SPLIT_KB, default 512: the
// pool's wake-up costs ~10 us, more than it saves at 256 KiB, less at 1 MiB --
// device -> host 135 -> 72-85 us; profiles/archive/r02/mixed_split_ab.log)
size_t zc_split_bytes() {
    static const size_t v = (size_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_MIXED_SPLIT_KB", 1, 1L << 20, 512) << 10;
    return v;
}

// host combines of at least this many bytes per operand are split over the
// copy pool's threads (MPIR_CVAR_REDUCE_LOCAL_HOST_SPLIT_KB, default 512)
uint64_t host_split_bytes() {
    static const uint64_t v = (uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_HOST_SPLIT_KB", 1, 1L << 22, 512) << 10;
    return v;
}

// A pinned host operand may be the target of work the caller queued on the
// legacy null stream (a hipMemcpyAsync D2H, a kernel writing mapped memory):
// the host reads it only after that work, the ordering the device path keeps
// for device operands (direct_reduce) and the blocking library streams keep for
// staged ones.  hipStreamQuery(NULL) keeps answering "not ready" for finished
// work until the host synchronises (profiles/archive/r02/direct_probe.log), so "not
// ready" is followed by hipStreamSynchronize(NULL).  Pageable operands need
// nothing: HIP's copies into pageable memory complete before they return.
int order_after_null_stream() {
    if (hipStreamQuery(nullptr) == hipSuccess) return MPIR_HIP_OK;
    (void)hipGetLastError();
    HIPCHK(hipStreamSynchronize(nullptr));
    return MPIR_HIP_OK;
}

// the same for a pinned operand of device `dev`'s context, which the caller may
// have filled through that device's null stream while another was current
// (ADVICE r3): that device's null stream, then the caller's device back
int order_after_null_stream_of(int dev) {
    if (dev < 0) return order_after_null_stream();      // the caller's current device
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    return order_after_null_stream();
}

// Both operands in host memory: g_table's host loop (the kernels' functors
// compiled for x86) over n units of `unit` bytes, on the calling thread, or
// from host_split_bytes() split over a pool's threads (combine_pool: the
// operands' NUMA node) in parts on 64-byte boundaries.
int host_combine(int op, int elem, const void *inbuf, void *inoutbuf, uint64_t n, uint64_t unit) {
    const host_fn fn = g_table[op][elem].host;
    if (!fn) return MPIR_HIP_ENOKERNEL;
    if (n * unit < host_split_bytes() || pool_threads() <= 1) {
        fn(inbuf, inoutbuf, n);
        return MPIR_HIP_OK;
    }
    CopyPool &pool = combine_pool(inbuf, inoutbuf, (size_t)(n * unit));
    struct H {
        host_fn fn;
        const char *in;
        char *io;
        uint64_t n, part, unit;
    } h{fn, static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf), n, 0, unit};
    // four parts per thread, handed out one at a time (a slower thread takes
    // fewer), of at least 256 KiB: a worker's wake-up costs a few us
    const uint64_t per = std::max<uint64_t>((n + 4 * (uint64_t)pool.threads() - 1) / (4 * (uint64_t)pool.threads()),
                                            ((uint64_t)256 << 10) / unit);
    const uint64_t grain = unit >= 64 ? 1 : 64 / unit;
    h.part = (per + grain - 1) / grain * grain;
    pool.run((size_t)((n + h.part - 1) / h.part), [](void *p, size_t k) {
        const H *h = static_cast<const H *>(p);
        const uint64_t b = k * h->part, e = std::min(h->n, b + h->part);
        h->fn(h->in + b * h->unit, h->io + b * h->unit, e - b);
    }, &h);
    return MPIR_HIP_OK;
}

// How the synchronous entry points wait for their launch.
//   MPIR_CVAR_REDUCE_LOCAL_WAIT=flag  (default): after the kernel, the stream
//       writes a per-thread sequence number into pinned host memory
//       (hipStreamWriteValue32, executed by the command processor in stream
//       order) and the caller spins on that word.  Measured on MI355X: an empty
//       launch + wait costs 7.2 us this way vs 11.5 us with
//       hipStreamSynchronize, 17.3 us polling hipStreamQuery (tools/latency.hip).
//   MPIR_CVAR_REDUCE_LOCAL_WAIT=block : hipStreamSynchronize.
// The spin re-checks hipStreamQuery every 64Ki polls so a faulted stream
// returns an error instead of spinning forever.
int wait_mode() {
    static const int mode = [] {
        const char *v = getenv("MPIR_CVAR_REDUCE_LOCAL_WAIT");
        return (v && !strcmp(v, "block")) ? 0 : 1;
    }();
    return mode;
}

int wait_stream_block(hipStream_t s) {
    HIPCHK(hipStreamSynchronize(s));
    return MPIR_HIP_OK;
}

int wait_stream(int dev, hipStream_t s) {
    if (wait_mode() == 0) return wait_stream_block(s);
    DevCtx &d = ctx().dev[dev];
    if (!d.flag) {
        void *p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return wait_stream_block(s);
        }
        d.flag = static_cast<volatile uint32_t *>(p);
        *d.flag = 0;
    }
    const uint32_t seq = ++d.seq ? d.seq : ++d.seq;
    if (hipStreamWriteValue32(s, (void *)d.flag, seq, 0) != hipSuccess) {
        (void)hipGetLastError();
        return wait_stream_block(s);
    }
    for (uint64_t it = 1; *d.flag != seq; ++it) {
        if ((it & 0xFFFF) == 0) {
            hipError_t e = hipStreamQuery(s);
            if (e != hipSuccess && e != hipErrorNotReady) return set_err(e, "stream fault while waiting");
        }
        __builtin_ia32_pause();
    }
    return MPIR_HIP_OK;
}

// Both operands reachable by device `dev`'s kernels (device memory, or the
// pinned slot of the mixed path): direct AQL dispatch of plan_reduce's kernel
// for a synchronous call on the library stream (any count, any alignment) when
// nothing queued on the library stream is still pending; otherwise -- REPLACE,
// the 32-byte classes, the stream variant -- the HIP launch (then the wait,
// for a synchronous call).
int device_call(int dev, const void *inbuf, void *inoutbuf, uint64_t count, int op, int elem, hipStream_t user_s,
                int sync) {
    launch_fn fn = g_table[op][elem].fn;
    const size_t esz = g_elem_size[elem];
    // REPLACE is registered as a byte copy: its launcher counts bytes
    const uint64_t unit = (op == MPIR_HIP_OP_REPLACE) ? 1 : esz;
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = user_s;
    int rc = MPIR_HIP_OK;
    DevCtx &d = ctx().dev[dev];
    if (sync && !s && g_table[op][elem].plan) {
        ReducePlan plan;
        g_table[op][elem].plan(inbuf, inoutbuf, count, &plan);
        bool idle = !d.main_pending;
        if (!idle && d.stream[S_MAIN] && hipStreamQuery(d.stream[S_MAIN]) == hipSuccess) {
            d.main_pending = false;
            idle = true;
        }
        (void)hipGetLastError();
        if (idle && direct_reduce(dev, op, elem, plan, &rc)) {
            if (rc != MPIR_HIP_OK) snprintf(ctx().err, sizeof(ctx().err), "direct dispatch: queue error");
            return rc;
        }
    }
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc == MPIR_HIP_OK) {
        hipError_t e = fn(inbuf, inoutbuf, count * esz / unit, s);
        if (e != hipSuccess) rc = set_err(e, "kernel launch");
        else if (sync) rc = wait_stream(dev, s);
        else if (!user_s) d.main_pending = true;
    }
    return rc;
}

// The operands of one MPIR_Hip_reduce call as classify() found them
struct Operand {
    Loc loc = LOC_HOST;
    int dev = -1;
    bool kept = false;
    // a host operand the host reads waits for the null stream if it is
    // pinned, or if its verdict was a kept one (classify: it may be stale)
    bool ordered() const { return loc == LOC_PINNED || (loc == LOC_HOST && kept); }
    // the device whose null stream that is: the pinned buffer's, else the caller's
    int order_dev() const { return loc == LOC_PINNED ? dev : -1; }
};
struct Operands {
    Operand in, io;
};

// Small, one operand host memory and the other on a device: the host operand
// goes through the thread's pinned slot, which the kernel reads (writes)
// directly; the slot copy keeps the device operand's offset mod 256 so the
// aligned tile kernels still apply.
int mixed_call(const Operands &ops, const void *inbuf, void *inoutbuf, uint64_t count, int op, int elem) {
    const uint64_t bytes = count * g_elem_size[elem];
    const bool in_dev = ops.in.loc == LOC_DEVICE;
    const Operand &host = in_dev ? ops.io : ops.in;
    const int dev = in_dev ? ops.in.dev : ops.io.dev;
    const uintptr_t adev = reinterpret_cast<uintptr_t>(in_dev ? inbuf : (const void *)inoutbuf);
    char *slot = nullptr;
    int rc = MPIR_HIP_OK;
    if (host.ordered()) {
        // the host operand is read (copied into the slot) before device_call's
        // own null-stream check: order it first, after the null stream of the
        // device that owns the pinned buffer (the caller's for a
        // kept pageable verdict) and of the device the kernel runs on
        const int pdev = host.order_dev();
        rc = order_after_null_stream_of(pdev);
        if (rc == MPIR_HIP_OK && pdev >= 0 && pdev != dev) rc = order_after_null_stream_of(dev);
        if (rc != MPIR_HIP_OK) return rc;
    }
    rc = get_zc(dev, (size_t)bytes + 256, &slot);
    if (rc != MPIR_HIP_OK) return rc;
    slot += adev & 255;
    // host <-> slot copies: split over the copy pool from zc_split_bytes() up
    auto hcopy = [&](void *dst, const void *src) {
        if (bytes >= zc_split_bytes())
            copy_pool().copy(static_cast<char *>(dst), static_cast<const char *>(src), bytes, zc_split_bytes());
        else
            memcpy(dst, src, bytes);
    };
    if (ops.io.loc == LOC_DEVICE) {
        hcopy(slot, inbuf);
        return device_call(dev, slot, inoutbuf, count, op, elem, nullptr, 1);
    }
    hcopy(slot, inoutbuf);
    rc = device_call(dev, inbuf, slot, count, op, elem, nullptr, 1);
    if (rc == MPIR_HIP_OK) hcopy(inoutbuf, slot);
    return rc;
}

// At least one operand is host memory (or the two operands live on different
// devices): the up / comp / down pipeline described at stage_chunk().
int staged_call(const Operands &ops, const void *inbuf, void *inoutbuf, uint64_t count, int op, int elem) {
    const launch_fn fn = g_table[op][elem].fn;
    const size_t esz = g_elem_size[elem];
    // REPLACE is registered as a byte copy: its launcher counts bytes
    const uint64_t unit = (op == MPIR_HIP_OP_REPLACE) ? 1 : esz;
    const Loc lin = ops.in.loc, lio = ops.io.loc;
    int dev = 0;
    if (lio == LOC_DEVICE) dev = ops.io.dev;
    else if (lin == LOC_DEVICE) dev = ops.in.dev;
    else {
        if (device_count() == 0) return MPIR_HIP_ENODEV;
        HIPCHK(hipGetDevice(&dev));
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();

    int rc = MPIR_HIP_OK;
    DevCtx &d = ctx().dev[dev];
    const bool stage_in = !(lin == LOC_DEVICE && ops.in.dev == dev);
    const bool stage_io = !(lio == LOC_DEVICE && ops.io.dev == dev);
    const uint64_t total = count * esz;
    uint64_t chunk_elems = stage_chunk() / esz;
    if (chunk_elems > count) chunk_elems = count;
    const uint64_t chunk_bytes = chunk_elems * esz;
    const uint64_t slot_bytes = (chunk_bytes + 255) & ~(uint64_t)255;
    const int nslots = stage_slots();
    char *scratch = nullptr;
    hipStream_t up = nullptr, comp = nullptr, down = nullptr;
    rc = get_scratch(dev, (size_t)(2 * nslots) * slot_bytes, &scratch);
    if (rc == MPIR_HIP_OK) rc = get_stream(dev, S_UP, &up);
    if (rc == MPIR_HIP_OK) rc = get_stream(dev, S_COMP, &comp);
    if (rc == MPIR_HIP_OK) rc = get_stream(dev, S_DOWN, &down);
    if (rc == MPIR_HIP_OK) rc = get_stage_events(dev, nslots);
    const char *cin = static_cast<const char *>(inbuf);
    char *cio = static_cast<char *>(inoutbuf);
    // Pageable host operands go through pinned bounce slots that the copy pool
    // fills and drains while the GPU works on earlier chunks (HIP's own
    // pageable path uploads ~36 GB/s; pinned memory is DMA'd directly).
    const bool bounce_in = stage_in && lin == LOC_HOST;
    const bool bounce_io = stage_io && lio == LOC_HOST;
    char *bounce = nullptr;
    if (rc == MPIR_HIP_OK && (bounce_in || bounce_io))
        rc = get_bounce(dev, (size_t)(2 * nslots) * slot_bytes, &bounce);
    CopyPool *pool = (bounce_in || bounce_io) ? &copy_pool() : nullptr;   // threads only when needed
    const uint64_t nchunks = (total + chunk_bytes - 1) / chunk_bytes;
    // chunk j's result: from its bounce slot to the caller's inoutbuf, once its
    // copy-back (recorded as ev_free of its slot) has landed
    auto drain = [&](uint64_t j) -> int {
        const int sl = (int)(j % (uint64_t)nslots);
        const uint64_t o = j * chunk_bytes, n = (total - o < chunk_bytes) ? total - o : chunk_bytes;
        hipError_t e = hipEventSynchronize(d.ev_free[sl]);
        if (e != hipSuccess) return set_err(e, "staged reduce");
        pool->copy(cio + o, bounce + (2 * sl + 1) * slot_bytes, n);
        return MPIR_HIP_OK;
    };
    for (uint64_t off = 0, k = 0; rc == MPIR_HIP_OK && off < total; off += chunk_bytes, ++k) {
        const uint64_t nb = (total - off < chunk_bytes) ? total - off : chunk_bytes;
        const int slot = (int)(k % (uint64_t)nslots);
        char *sin = scratch + (2 * slot) * slot_bytes;
        char *sio = scratch + (2 * slot + 1) * slot_bytes;
        char *bin = bounce ? bounce + (2 * slot) * slot_bytes : nullptr;
        char *bio = bounce ? bounce + (2 * slot + 1) * slot_bytes : nullptr;
        const void *kin = stage_in ? (const void *)sin : (const void *)(cin + off);
        void *kio = stage_io ? (void *)sio : (void *)(cio + off);
        hipError_t e = hipSuccess;
        // the slot's previous chunk must be fully consumed (kernel read, copy-back done)
        if (k >= (uint64_t)nslots) {
            if (bounce_io) {
                if ((rc = drain(k - nslots)) != MPIR_HIP_OK) break;
            } else if (bounce_in) {
                e = hipEventSynchronize(d.ev_free[slot]);   // the host rewrites bin
            }
            if (e == hipSuccess) e = hipStreamWaitEvent(up, d.ev_free[slot], 0);
        }
        if (e == hipSuccess && bounce_in) pool->copy(bin, cin + off, nb);
        if (e == hipSuccess && bounce_io) pool->copy(bio, cio + off, nb);
        if (e == hipSuccess && stage_in)
            e = hipMemcpyAsync(sin, bounce_in ? (const void *)bin : (const void *)(cin + off), nb, hipMemcpyDefault, up);
        if (e == hipSuccess && stage_io)
            e = hipMemcpyAsync(sio, bounce_io ? (const void *)bio : (const void *)(cio + off), nb, hipMemcpyDefault, up);
        if (e == hipSuccess) e = hipEventRecord(d.ev_up[slot], up);
        if (e == hipSuccess) e = hipStreamWaitEvent(comp, d.ev_up[slot], 0);
        if (e == hipSuccess) e = fn(kin, kio, nb / unit, comp);
        if (e == hipSuccess) e = hipEventRecord(d.ev_comp[slot], comp);
        if (stage_io) {
            if (e == hipSuccess) e = hipStreamWaitEvent(down, d.ev_comp[slot], 0);
            if (e == hipSuccess) e = hipMemcpyAsync(bounce_io ? (void *)bio : (void *)(cio + off), sio, nb, hipMemcpyDefault, down);
            if (e == hipSuccess) e = hipEventRecord(d.ev_free[slot], down);
        } else if (e == hipSuccess) {
            e = hipEventRecord(d.ev_free[slot], comp);
        }
        if (e != hipSuccess) rc = set_err(e, "staged reduce");
    }
    if (rc == MPIR_HIP_OK && bounce_io)
        for (uint64_t j = nchunks > (uint64_t)nslots ? nchunks - nslots : 0; rc == MPIR_HIP_OK && j < nchunks; ++j)
            rc = drain(j);
    if (rc == MPIR_HIP_OK) rc = wait_stream_block(comp);
    if (rc == MPIR_HIP_OK) rc = wait_stream_block(down);
    return rc;
}

// Which branch of MPIR_Hip_combine a fold of n operands takes, in its order
// (MPIR_Hip_combine launches it, MPIR_Hip_combine_plan_info reports it)
enum CombineRoute { ROUTE_COPY_FIRST, ROUTE_COPY_LAST, ROUTE_FUSED_TREE, ROUTE_FUSED_CHAIN, ROUTE_ANY, ROUTE_NONE };
CombineRoute combine_route(int n, int op, int elem, int order) {
    const bool fused = g_multi[op][elem][0][0] != nullptr;
    if (n == 1) return ROUTE_COPY_FIRST;
    // a fold of REPLACE in either order is the last operand
    if (op == MPIR_HIP_OP_REPLACE) return ROUTE_COPY_LAST;
    if (order == MPIR_HIP_ORDER_TREE && fused && n <= 8) return ROUTE_FUSED_TREE;
    if (order == MPIR_HIP_ORDER_CHAIN && fused) return ROUTE_FUSED_CHAIN;
    if (g_table[op][elem].any) return ROUTE_ANY;
    return ROUTE_NONE;
}

// the argument checks MPIR_Hip_combine makes before it looks at a pointer
bool combine_args_ok(int n, int op, int elem, int order) {
    if (n < 1 || n > 64 || (order != MPIR_HIP_ORDER_TREE && order != MPIR_HIP_ORDER_CHAIN)) return false;
    if (!pair_in_range(op, elem)) return false;
    return !(order == MPIR_HIP_ORDER_TREE && (n & (n - 1)));
}

// CHAIN beyond 8 operands: chunks of up to 8, each chunk's first operand the
// running acc (the output after the first pass).  fn(ops, P) per pass, until it
// returns false; returns the passes made.
template <class F>
int chain_passes(const void *const *inbufs, int n, const void *outbuf, F fn) {
    const void *acc = inbufs[0];
    int passes = 0;
    for (int i = 1; i < n;) {
        const int P = std::min(kMultiMaxP, n - i + 1);
        const void *ops[kMultiMaxP];
        ops[0] = acc;
        for (int j = 1; j < P; ++j) ops[j] = inbufs[i + j - 1];
        ++passes;
        if (!fn(ops, P)) break;
        i += P - 1;
        acc = outbuf;
    }
    return passes;
}

// The launches of a batch (MPIR_Hip_reduce_batch makes them,
// MPIR_Hip_batch_plan_info counts them): the non-empty segments in order, each
// at the first workgroup its predecessors leave it; a launch closes at
// kBatchMaxSegs descriptors or before its workgroups pass kBatchMaxGroups.
// emit(args, groups) per launch, until it returns false.  seg_kind / seg_groups
// (or null): every segment's path and workgroups.  totals = {launches,
// workgroups, tile segments, element segments, empty segments}.
template <class F>
void batch_launches(const BatchEntry &en, const MPIR_Hip_seg *segs, int nsegs, uint32_t *seg_kind, uint32_t *seg_groups,
                    uint64_t totals[5], F emit) {
    BatchArgs a;
    memset(&a, 0, sizeof a);
    uint64_t groups = 0;
    for (int k = 0; k < 5; ++k) totals[k] = 0;
    auto flush = [&]() {
        if (!a.nsegs) return true;
        ++totals[0];
        totals[1] += groups;
        const bool go = emit(a, groups);
        memset(&a, 0, sizeof a);
        groups = 0;
        return go;
    };
    for (int i = 0; i < nsegs; ++i) {
        if (segs[i].count == 0) {
            ++totals[4];
            if (seg_kind) seg_kind[i] = MPIR_HIP_BATCH_SEG_EMPTY;
            if (seg_groups) seg_groups[i] = 0;
            continue;
        }
        int tile = 0;
        const uint64_t g = en.groups(segs[i].in, segs[i].io, segs[i].count, &tile);
        ++totals[tile ? 2 : 3];
        if (seg_kind) seg_kind[i] = tile ? MPIR_HIP_BATCH_SEG_TILE : MPIR_HIP_BATCH_SEG_ELEMS;
        if (seg_groups) seg_groups[i] = (uint32_t)g;
        if ((a.nsegs == (uint32_t)kBatchMaxSegs || groups + g > kBatchMaxGroups) && !flush()) return;
        a.seg[a.nsegs++] = BatchSeg{static_cast<const char *>(segs[i].in), static_cast<char *>(segs[i].io),
                                    segs[i].count, groups};
        groups += g;
    }
    flush();
}

// the batch's only non-empty segment, or -1 if it has none or several
int batch_single(const MPIR_Hip_seg *segs, int nsegs) {
    int one = -1;
    for (int i = 0; i < nsegs; ++i)
        if (segs[i].count) {
            if (one >= 0) return -1;
            one = i;
        }
    return one;
}

bool batch_args_ok(const MPIR_Hip_seg *segs, int nsegs, int op, int elem) {
    if (nsegs < 0 || (nsegs > 0 && !segs)) return false;
    if (!pair_in_range(op, elem)) return false;
    return g_batch[op][elem].launch && g_batch[op][elem].groups;
}

// The plan of a strided call (MPIR_Hip_reduce_strided launches it,
// MPIR_Hip_strided_plan_info reports it): the form, what a workgroup covers and
// how many rows a launch takes, all O(1) in the number of rows.
struct StridedPlan {
    int form;                   // MPIR_HIP_STRIDED_*
    uint64_t threshold;         // the wide / narrow threshold in force
    uint64_t row_bytes;
    uint64_t per;               // WIDE: G, workgroups per row; NARROW: units per workgroup
    uint64_t upr;               // NARROW: units per row
    uint64_t rows_per_launch;
    uint64_t launches, groups;  // over the whole call
};

// workgroups of one launch of n rows
uint64_t strided_launch_groups(const StridedPlan &p, uint64_t n) {
    return p.form == MPIR_HIP_STRIDED_WIDE ? n * p.per : (n * p.upr + p.per - 1) / p.per;
}

// the argument checks MPIR_Hip_reduce_strided makes before it looks at a
// pointer; MPIR_HIP_OK with *form EMPTY or SINGLE where that settles the call
int strided_args(uint64_t in_stride, uint64_t io_stride, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                 int *form) {
    if (!pair_in_range(op, elem) || !g_strided[op][elem].launch || !g_batch[op][elem].groups) return MPIR_HIP_ENOKERNEL;
    *form = MPIR_HIP_STRIDED_EMPTY;
    if (!nblocks || !blocklen) return MPIR_HIP_OK;
    const uint64_t esz = g_elem_size[elem];
    if (blocklen > (~(uint64_t)0 >> 1) / esz) return MPIR_HIP_EARG;
    const uint64_t row_bytes = blocklen * esz, top = ~(uint64_t)0 - row_bytes;
    if (nblocks > 1) {
        if (io_stride < row_bytes) return MPIR_HIP_EARG;                    // output rows would overlap
        if (io_stride > top / (nblocks - 1) || (in_stride && in_stride > top / (nblocks - 1))) return MPIR_HIP_EARG;
    }
    *form = nblocks == 1 || (in_stride == row_bytes && io_stride == row_bytes) ? MPIR_HIP_STRIDED_SINGLE
                                                                              : MPIR_HIP_STRIDED_WIDE;
    return MPIR_HIP_OK;
}

// (for a call strided_args left as WIDE: more than one row, not contiguous)
void strided_plan(const void *in, uint64_t in_stride, const void *io, uint64_t io_stride, uint64_t nblocks,
                  uint64_t blocklen, int elem, StridedPlan &p) {
    const uint64_t esz = g_elem_size[elem];
    const uint64_t cap = t_strided_cap && t_strided_cap < kBatchMaxGroups ? t_strided_cap : kBatchMaxGroups;
    p.row_bytes = blocklen * esz;
    p.threshold = g_strided_wide.load(std::memory_order_relaxed);
    if (p.row_bytes >= p.threshold) {
        p.form = MPIR_HIP_STRIDED_WIDE;
        p.per = strided_row_groups_max(p.row_bytes, esz, io, io_stride);
        p.upr = 0;
        p.rows_per_launch = cap / p.per;                // a row is never split between launches
    } else {
        const uint64_t all = p.row_bytes | in_stride | io_stride | reinterpret_cast<uintptr_t>(in) |
                             reinterpret_cast<uintptr_t>(io);
        const bool vec = esz <= 16 && (all & 15) == 0;
        const uint64_t unit = vec ? 16 : esz;
        p.form = vec ? MPIR_HIP_STRIDED_NARROW_VEC : MPIR_HIP_STRIDED_NARROW_ELEMS;
        p.per = kTileBytes / unit;
        p.upr = p.row_bytes / unit;
        // the kernel's per-lane division is 32-bit: a launch's rows stay below 2^32
        p.rows_per_launch = std::min<uint64_t>(cap * p.per / p.upr, 0xFFFFFFFFull);
    }
    p.rows_per_launch = std::min(std::max<uint64_t>(p.rows_per_launch, 1), nblocks);
    const uint64_t full = nblocks / p.rows_per_launch, rest = nblocks % p.rows_per_launch;
    p.launches = full + (rest != 0);
    p.groups = full * strided_launch_groups(p, p.rows_per_launch) + (rest ? strided_launch_groups(p, rest) : 0);
}

// The launches of a plan: later row ranges with the base pointers advanced.
// emit(args, groups) per launch, until it returns false.
template <class F>
void strided_launches(const StridedPlan &p, const void *in, uint64_t in_stride, void *io, uint64_t io_stride,
                      uint64_t nblocks, uint64_t blocklen, F emit) {
    for (uint64_t row0 = 0; row0 < nblocks; row0 += p.rows_per_launch) {
        const uint64_t n = std::min(p.rows_per_launch, nblocks - row0);
        const StridedArgs a{static_cast<const char *>(in) + row0 * in_stride, static_cast<char *>(io) + row0 * io_stride,
                            in_stride, io_stride, blocklen, (uint32_t)n, (uint32_t)p.form,
                            (uint32_t)(p.form == MPIR_HIP_STRIDED_WIDE ? p.per : p.upr), 0};
        if (!emit(a, strided_launch_groups(p, n))) return;
    }
}

// ---- indexed calls: the strided call's plan with a table where the stride was.
// The forms carry the strided call's numbers, so StridedPlan and
// strided_launch_groups serve both.
static_assert(MPIR_HIP_INDEXED_EMPTY == MPIR_HIP_STRIDED_EMPTY && MPIR_HIP_INDEXED_SINGLE == MPIR_HIP_STRIDED_SINGLE &&
                  MPIR_HIP_INDEXED_WIDE == MPIR_HIP_STRIDED_WIDE &&
                  MPIR_HIP_INDEXED_NARROW_VEC == MPIR_HIP_STRIDED_NARROW_VEC &&
                  MPIR_HIP_INDEXED_NARROW_ELEMS == MPIR_HIP_STRIDED_NARROW_ELEMS,
              "the indexed forms are the strided forms");

// the argument checks MPIR_Hip_reduce_indexed makes before it looks at a
// pointer; MPIR_HIP_OK with *form EMPTY or SINGLE where that settles the call
int indexed_args(const void *in_displs, const void *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                 int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_indexed[op][elem].launch || !g_batch[op][elem].groups) return MPIR_HIP_ENOKERNEL;
    // (before the counts, as the MPIX entry checks it: the two layers answer alike)
    if (!disp_unit || disp_unit > (~(uint64_t)0 >> 1)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_INDEXED_EMPTY;
    if (!nblocks || !blocklen) return MPIR_HIP_OK;
    const uint64_t esz = g_elem_size[elem];
    if (blocklen > (~(uint64_t)0 >> 1) / esz) return MPIR_HIP_EARG;
    // a packed side's span, and the single call's count
    if (nblocks > (~(uint64_t)0 >> 1) / (blocklen * esz)) return MPIR_HIP_EARG;
    *form = !in_displs && !io_displs ? MPIR_HIP_INDEXED_SINGLE : MPIR_HIP_INDEXED_WIDE;
    return MPIR_HIP_OK;
}

// (for a call indexed_args left as WIDE: at least one table).  The tables are
// compared with null, never read: what a device table holds the host cannot see,
// so G is the worst case and the vector form needs disp_unit's word for it.
// `fetch` (the fetching ordered call's packed output, else null) joins the
// vector form's alignment test: its blocks sit at multiples of the block's bytes.
void indexed_plan(const void *in, const void *in_displs, const void *io, const void *io_displs, uint64_t disp_unit,
                  uint64_t nblocks, uint64_t blocklen, int elem, StridedPlan &p, const void *fetch = nullptr) {
    const uint64_t esz = g_elem_size[elem];
    const uint64_t cap = t_strided_cap && t_strided_cap < kBatchMaxGroups ? t_strided_cap : kBatchMaxGroups;
    p.row_bytes = blocklen * esz;
    p.threshold = g_strided_wide.load(std::memory_order_relaxed);
    if (p.row_bytes >= p.threshold) {
        p.form = MPIR_HIP_INDEXED_WIDE;
        p.per = indexed_row_groups_max(p.row_bytes, esz);
        p.upr = 0;
        p.rows_per_launch = cap / p.per;                // a block is never split between launches
    } else {
        const uint64_t all = p.row_bytes | reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(io) |
                             reinterpret_cast<uintptr_t>(fetch) | (in_displs || io_displs ? disp_unit : 0);
        const bool vec = esz <= 16 && (all & 15) == 0;
        const uint64_t unit = vec ? 16 : esz;
        p.form = vec ? MPIR_HIP_INDEXED_NARROW_VEC : MPIR_HIP_INDEXED_NARROW_ELEMS;
        p.per = kTileBytes / unit;
        p.upr = p.row_bytes / unit;
        // the kernel's per-lane division is 32-bit: a launch's blocks stay below 2^32
        p.rows_per_launch = std::min<uint64_t>(cap * p.per / p.upr, 0xFFFFFFFFull);
    }
    p.rows_per_launch = std::min(std::max<uint64_t>(p.rows_per_launch, 1), nblocks);
    const uint64_t full = nblocks / p.rows_per_launch, rest = nblocks % p.rows_per_launch;
    p.launches = full + (rest != 0);
    p.groups = full * strided_launch_groups(p, p.rows_per_launch) + (rest ? strided_launch_groups(p, rest) : 0);
}

// The launches of a plan: later block ranges, the table pointers advanced by
// the blocks before them and a packed side's base by those blocks' bytes.
// emit(args, groups) per launch, until it returns false.
template <class F>
void indexed_launches(const StridedPlan &p, const void *in, const int64_t *in_displs, void *io,
                      const int64_t *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, F emit) {
    for (uint64_t row0 = 0; row0 < nblocks; row0 += p.rows_per_launch) {
        const uint64_t n = std::min(p.rows_per_launch, nblocks - row0);
        const IndexedArgs a{static_cast<const char *>(in) + (in_displs ? 0 : row0 * p.row_bytes),
                            static_cast<char *>(io) + (io_displs ? 0 : row0 * p.row_bytes),
                            in_displs ? in_displs + row0 : nullptr, io_displs ? io_displs + row0 : nullptr,
                            disp_unit, blocklen, (uint32_t)n, (uint32_t)p.form,
                            (uint32_t)(p.form == MPIR_HIP_INDEXED_WIDE ? p.per : p.upr), 0};
        if (!emit(a, strided_launch_groups(p, n))) return;
    }
}

// A host displacement table, read before anything is enqueued: every
// displs[k] * disp_unit must fit 64 signed bits (MPIR_HIP_EARG), and the first
// byte of the lowest block and the last byte of the highest must be device
// memory on `dev` (MPIR_HIP_EBUFFER).  *first / *last (where asked for): those
// two bytes' addresses.
int indexed_host_table(const char *base, const int64_t *displs, uint64_t disp_unit, uint64_t nblocks,
                       uint64_t row_bytes, int dev, const char **first = nullptr, const char **last = nullptr) {
    int64_t lo = displs[0], hi = displs[0];
    for (uint64_t k = 1; k < nblocks; ++k) {
        lo = std::min(lo, displs[k]);
        hi = std::max(hi, displs[k]);
    }
    int64_t off_lo, off_hi;
    if (__builtin_mul_overflow(lo, (int64_t)disp_unit, &off_lo) || __builtin_mul_overflow(hi, (int64_t)disp_unit, &off_hi))
        return MPIR_HIP_EARG;
    if (off_hi > (int64_t)((~(uint64_t)0 >> 1) - row_bytes)) return MPIR_HIP_EARG;
    const void *ends[2] = {base + off_lo, base + off_hi + (row_bytes - 1)};
    DeviceSpan span;
    for (int k = 0; k < 2; ++k) {
        int d = -1;
        if (classify_in_span(ends[k], &d, span) != LOC_DEVICE || d != dev) return MPIR_HIP_EBUFFER;
    }
    if (first) *first = static_cast<const char *>(ends[0]);
    if (last) *last = static_cast<const char *>(ends[1]);
    return MPIR_HIP_OK;
}

// ---- ordered indexed calls: the indexed call's plan over sorted positions.
// the argument checks MPIR_Hip_reduce_indexed_ordered makes before it looks at
// a pointer, for a call with an order table: the indexed call's, then the two of
// its own (an order table needs an output table to sort, and holds ints)
int ordered_args(const void *in_displs, const void *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                 int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_ordered[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    const int rc = indexed_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, form);
    if (rc != MPIR_HIP_OK || *form == MPIR_HIP_INDEXED_EMPTY) return rc;
    if (!io_displs || nblocks > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    return MPIR_HIP_OK;
}

// The launches of an ordered plan: later ranges of sorted positions.  The bases
// and the tables are the call's in every launch (a head test looks back and a
// run goes on across a launch boundary); the range is in pos0 and nrows.
template <class F>
void ordered_launches(const StridedPlan &p, const void *in, const int64_t *in_displs, void *io,
                      const int64_t *io_displs, const int *order, uint64_t disp_unit, uint64_t nblocks,
                      uint64_t blocklen, F emit) {
    for (uint64_t pos0 = 0; pos0 < nblocks; pos0 += p.rows_per_launch) {
        const uint64_t n = std::min(p.rows_per_launch, nblocks - pos0);
        const OrderedArgs a{static_cast<const char *>(in), static_cast<char *>(io), in_displs, io_displs, order,
                            disp_unit, blocklen, (uint32_t)nblocks, (uint32_t)pos0, (uint32_t)n, (uint32_t)p.form,
                            (uint32_t)(p.form == MPIR_HIP_INDEXED_WIDE ? p.per : p.upr), 0};
        if (!emit(a, strided_launch_groups(p, n))) return;
    }
}

// A host order table, read before anything is enqueued: a permutation of
// [0, nblocks), and, where the output table is host memory too (else null), its
// displacements non-decreasing along it with ties in ascending block number.
// MPIR_HIP_EARG otherwise.
int ordered_host_order(const int *order, const int64_t *io_displs, uint64_t nblocks) {
    std::unique_ptr<uint8_t[]> seen(new (std::nothrow) uint8_t[nblocks]());
    if (!seen) {
        snprintf(ctx().err, sizeof(ctx().err), "no memory to check an order table of %llu entries",
                 (unsigned long long)nblocks);
        return MPIR_HIP_ERUNTIME;
    }
    for (uint64_t p = 0; p < nblocks; ++p) {
        const int k = order[p];
        if (k < 0 || (uint64_t)k >= nblocks || seen[k]) return MPIR_HIP_EARG;
        seen[k] = 1;
    }
    if (io_displs)
        for (uint64_t p = 1; p < nblocks; ++p) {
            const int64_t a = io_displs[order[p - 1]], b = io_displs[order[p]];
            if (a > b || (a == b && order[p - 1] > order[p])) return MPIR_HIP_EARG;
        }
    return MPIR_HIP_OK;
}

// both ends of a table of `bytes` at t: device memory on `dev` (*dev < 0: any
// device, which it then names)?  false: host memory; MPIR_HIP_EBUFFER in *rc
// where it starts on a device and is not all on the one
bool table_on_device(const void *t, uint64_t bytes, int *dev, int *rc) {
    DeviceSpan ts;
    int d = -1, d2 = -1;
    *rc = MPIR_HIP_OK;
    if (classify_in_span(t, &d, ts) != LOC_DEVICE) return false;
    if ((*dev >= 0 && d != *dev) ||
        classify_in_span(static_cast<const char *>(t) + (bytes - 1), &d2, ts) != LOC_DEVICE || d2 != d)
        *rc = MPIR_HIP_EBUFFER;
    *dev = d;
    return true;
}

// ---- ragged calls: unequal pieces from a table of packed element offsets.
// the argument checks MPIR_Hip_reduce_ragged makes before it looks at a pointer;
// MPIR_HIP_OK with *form EMPTY or SINGLE where that settles the call
int ragged_args(const void *in_displs, const void *io_displs, const void *starts, uint64_t disp_unit, uint64_t npieces,
                uint64_t count, int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_ragged[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    // (before the counts, as the MPIX entry checks it: the two layers answer alike)
    if (!disp_unit || disp_unit > (~(uint64_t)0 >> 1)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_EMPTY;
    if (!count) return MPIR_HIP_OK;
    // the kernel's piece indices and relative offsets are 32-bit: the public
    // entry point's ints
    if (!npieces || npieces > (uint64_t)INT32_MAX || count > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_SINGLE;
    if (!in_displs && !io_displs) return MPIR_HIP_OK;
    if (!starts) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_RAGGED;
    return MPIR_HIP_OK;
}

// The plan of a RAGGED call: one launch of ragged_groups workgroups, each a span
// of 16 KiB of packed elements; the rounds of the wave-wide search and the
// boundaries a workgroup holds in LDS come from the kernel's own constants.
// Host arithmetic on the counts alone: no table is read.
struct RaggedPlan {
    uint64_t groups, per, rounds, lds_entries;
};
void ragged_plan(uint64_t npieces, uint64_t count, int elem, RaggedPlan &p) {
    const uint64_t esz = g_elem_size[elem];
    p.groups = ragged_groups(count, esz);
    p.per = kTileBytes / esz;
    p.rounds = ragged_search_rounds(npieces);
    p.lds_entries = kRaggedLdsEntries;
}

// A host `starts`, read before anything is enqueued: starts[0] == 0, no entry
// below the one before it, starts[npieces] == count (else MPIR_HIP_EARG)
int ragged_host_starts(const int64_t *starts, uint64_t npieces, uint64_t count) {
    if (starts[0] != 0 || starts[npieces] != (int64_t)count) return MPIR_HIP_EARG;
    for (uint64_t k = 0; k < npieces; ++k)
        if (starts[k + 1] < starts[k]) return MPIR_HIP_EARG;
    return MPIR_HIP_OK;
}

// A host displacement table: every displs[k] * disp_unit must fit 64 signed
// bits (MPIR_HIP_EARG)
int ragged_host_products(const int64_t *displs, uint64_t disp_unit, uint64_t npieces) {
    for (uint64_t k = 0; k < npieces; ++k) {
        int64_t off;
        if (__builtin_mul_overflow(displs[k], (int64_t)disp_unit, &off)) return MPIR_HIP_EARG;
    }
    return MPIR_HIP_OK;
}

// ... and beside a host `starts` (both already checked) the pieces' lengths are
// known too: the first byte of the lowest non-empty piece and the last byte of
// the highest must be device memory on `dev` (MPIR_HIP_EBUFFER; an end past 64
// signed bits MPIR_HIP_EARG).  Beside a device `starts` the lengths are the
// kernel's to read, and only the products are checked.
int ragged_host_extremes(const char *base, const int64_t *displs, const int64_t *host_starts, uint64_t disp_unit,
                         uint64_t npieces, uint64_t esz, int dev, const char **first = nullptr,
                         const char **last = nullptr) {
    int64_t lo = INT64_MAX, hi = INT64_MIN;     // first byte of the lowest, last byte of the highest
    for (uint64_t k = 0; k < npieces; ++k) {
        if (host_starts[k + 1] == host_starts[k]) continue;
        const int64_t off = displs[k] * (int64_t)disp_unit;
        int64_t last;
        if (__builtin_add_overflow(off, (int64_t)((uint64_t)(host_starts[k + 1] - host_starts[k]) * esz - 1), &last))
            return MPIR_HIP_EARG;
        lo = std::min(lo, off);
        hi = std::max(hi, last);
    }
    const void *ends[2] = {base + lo, base + hi};   // (count > 0: some piece is not empty)
    DeviceSpan span;
    for (int k = 0; k < 2; ++k) {
        int d = -1;
        if (classify_in_span(ends[k], &d, span) != LOC_DEVICE || d != dev) return MPIR_HIP_EBUFFER;
    }
    if (first) *first = base + lo;
    if (last) *last = base + hi;
    return MPIR_HIP_OK;
}

// ---- fetching ragged calls.  The kernel of (op, elem): the pair's own, or for
// the two byte ops the one of the element's size (null: none)
fetch_ragged_fn fetch_ragged_kernel(int op, int elem) {
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return nullptr;
    if (op == MPIR_HIP_OP_NO_OP || op == MPIR_HIP_OP_REPLACE) {
        const uint64_t esz = g_elem_size[elem];
        int l = 0;
        while (l < kFetchRaggedSizes && ((uint64_t)1 << l) != esz) ++l;
        return l < kFetchRaggedSizes ? g_fetch_ragged_bytes[op == MPIR_HIP_OP_REPLACE][l].launch : nullptr;
    }
    return pair_in_range(op, elem) ? g_fetch_ragged[op][elem].launch : nullptr;
}

// the argument checks MPIR_Hip_reduce_fetch_ragged makes before it looks at a
// pointer: ragged_args' in ragged_args' order, with one table.  MPIR_HIP_OK with
// *form EMPTY or SINGLE where that settles the call.
int fetch_ragged_args(const void *io_displs, const void *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count,
                      int op, int elem, int *form) {
    if (!fetch_ragged_kernel(op, elem)) return MPIR_HIP_ENOKERNEL;
    if (!disp_unit || disp_unit > (~(uint64_t)0 >> 1)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_EMPTY;
    if (!count) return MPIR_HIP_OK;
    if (!npieces || npieces > (uint64_t)INT32_MAX || count > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_SINGLE;
    if (!io_displs) return MPIR_HIP_OK;
    if (!starts) return MPIR_HIP_EARG;
    *form = MPIR_HIP_RAGGED_RAGGED;
    return MPIR_HIP_OK;
}

// The two packed sides at multiples of 16 (NO_OP never looks at inbuf): what the
// kernel is told, since a chunk's packed addresses are the bases plus a multiple
// of 16 and need no table to know.
bool fetch_ragged_packed_aligned(const void *in, const void *fetch, int op) {
    const uintptr_t all = reinterpret_cast<uintptr_t>(fetch) | (op == MPIR_HIP_OP_NO_OP ? 0 : reinterpret_cast<uintptr_t>(in));
    return (all & 15) == 0;
}

// the argument checks MPIR_Hip_reduce_fetch makes before it looks at a pointer;
// MPIR_HIP_OK with *path EMPTY or COPY where that settles the call, else TILE
// (the plan then says which of the kernel's two paths)
int fetch_args(uint64_t count, int op, int elem, int *path) {
    const bool copy = op == MPIR_HIP_OP_NO_OP || op == MPIR_HIP_OP_REPLACE;
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return MPIR_HIP_ENOKERNEL;
    if (!copy && (!pair_in_range(op, elem) || !g_fetch[op][elem].launch || !g_fetch[op][elem].plan))
        return MPIR_HIP_ENOKERNEL;
    if (count > (~(uint64_t)0 >> 1) / g_elem_size[elem]) return MPIR_HIP_EARG;
    *path = !count ? MPIR_HIP_FETCH_EMPTY : copy ? MPIR_HIP_FETCH_COPY : MPIR_HIP_FETCH_TILE;
    return MPIR_HIP_OK;
}

// ---- fetching ordered indexed calls.  The kernel of (op, elem): the pair's own,
// or for the two byte ops the one of the element's size (null: none)
fetch_ordered_fn fetch_ordered_kernel(int op, int elem) {
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return nullptr;
    if (op == MPIR_HIP_OP_NO_OP || op == MPIR_HIP_OP_REPLACE) {
        const uint64_t esz = g_elem_size[elem];
        int l = 0;
        while (l < kFetchRaggedSizes && ((uint64_t)1 << l) != esz) ++l;
        return l < kFetchRaggedSizes ? g_fetch_ordered_bytes[op == MPIR_HIP_OP_REPLACE][l].launch : nullptr;
    }
    return pair_in_range(op, elem) ? g_fetch_ordered[op][elem].launch : nullptr;
}

// the argument checks MPIR_Hip_reduce_fetch_indexed_ordered makes before it
// looks at a pointer: the ordered call's in the ordered call's order, the op's
// kernel looked up as the fetching calls look it up.  MPIR_HIP_OK with *form
// EMPTY or SINGLE where that settles the call (SINGLE: no table at all).
int fetch_ordered_args(const void *in_displs, const void *io_displs, const void *order, uint64_t disp_unit,
                       uint64_t nblocks, uint64_t blocklen, int op, int elem, int *form) {
    if (!fetch_ordered_kernel(op, elem)) return MPIR_HIP_ENOKERNEL;
    if (!disp_unit || disp_unit > (~(uint64_t)0 >> 1)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_INDEXED_EMPTY;
    if (!nblocks || !blocklen) return MPIR_HIP_OK;
    const uint64_t esz = g_elem_size[elem];
    if (blocklen > (~(uint64_t)0 >> 1) / esz) return MPIR_HIP_EARG;
    if (nblocks > (~(uint64_t)0 >> 1) / (blocklen * esz)) return MPIR_HIP_EARG;
    if (!io_displs) {
        // a packed target has no repeats to order, and gathering the origin side is
        // not this call's job
        if (order || (in_displs && op != MPIR_HIP_OP_NO_OP)) return MPIR_HIP_EARG;
        *form = MPIR_HIP_INDEXED_SINGLE;
        return MPIR_HIP_OK;
    }
    if (nblocks > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    *form = MPIR_HIP_INDEXED_WIDE;
    return MPIR_HIP_OK;
}

// The launches of a fetching ordered plan: ordered_launches with fetch beside.
template <class F>
void fetch_ordered_launches(const StridedPlan &p, const void *in, const int64_t *in_displs, void *io,
                            const int64_t *io_displs, void *fetch, const int *order, uint64_t disp_unit,
                            uint64_t nblocks, uint64_t blocklen, F emit) {
    ordered_launches(p, in, in_displs, io, io_displs, order, disp_unit, nblocks, blocklen,
                     [&](const OrderedArgs &o, uint64_t groups) {
                         return emit(FetchOrderedArgs{o, static_cast<char *>(fetch)}, groups);
                     });
}

// A host output table beside no order table, read before anything is enqueued:
// the caller's promise that equal entries are adjacent.  An entry equal to an
// earlier one that is not its neighbour: MPIR_HIP_EARG.
int fetch_ordered_host_adjacent(const int64_t *io_displs, uint64_t nblocks) {
    std::unique_ptr<uint32_t[]> idx(new (std::nothrow) uint32_t[nblocks]);
    if (!idx) {
        snprintf(ctx().err, sizeof(ctx().err), "no memory to check a displacement table of %llu entries",
                 (unsigned long long)nblocks);
        return MPIR_HIP_ERUNTIME;
    }
    for (uint64_t k = 0; k < nblocks; ++k) idx[k] = (uint32_t)k;
    std::sort(idx.get(), idx.get() + nblocks, [&](uint32_t a, uint32_t b) {
        return io_displs[a] != io_displs[b] ? io_displs[a] < io_displs[b] : a < b;
    });
    for (uint64_t p = 1; p < nblocks; ++p)
        if (io_displs[idx[p - 1]] == io_displs[idx[p]] && idx[p] != idx[p - 1] + 1) return MPIR_HIP_EARG;
    return MPIR_HIP_OK;
}

// ---- ordered compare-and-swap.  The kernels of an element class: those of its
// size, 1 to 8 bytes (null: none)
const CasEntry *cas_kernels(int elem) {
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return nullptr;
    const uint64_t esz = g_elem_size[elem];
    int l = 0;
    while (l < kCasSizes && ((uint64_t)1 << l) != esz) ++l;
    return l < kCasSizes && g_cas[l].launch && g_cas[l].contig && g_cas[l].plan ? &g_cas[l] : nullptr;
}

// the argument checks MPIR_Hip_cas_indexed_ordered makes before it looks at a
// pointer, in the fetching ordered call's order.  MPIR_HIP_OK with *form EMPTY,
// INDEXED, or CONTIG_ELEMS for a call with no table (the plan then says which of
// the contiguous kernel's two paths).
int cas_args(const void *displs, const void *order, uint64_t disp_unit, uint64_t count, int elem, int *form) {
    if (!cas_kernels(elem)) return MPIR_HIP_ENOKERNEL;
    if (!disp_unit || disp_unit > (~(uint64_t)0 >> 1)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_CAS_EMPTY;
    if (!count) return MPIR_HIP_OK;
    if (count > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    if (!displs && order) return MPIR_HIP_EARG;             // a contiguous target has no repeats to order
    *form = displs ? MPIR_HIP_CAS_INDEXED : MPIR_HIP_CAS_CONTIG_ELEMS;
    return MPIR_HIP_OK;
}

// sorted positions of one launch of the indexed form: whole workgroups up to the
// per-launch cap (MPIR_Hip_strided_test_max_groups lowers it)
uint64_t cas_rows_per_launch(uint64_t count) {
    const uint64_t cap = t_strided_cap && t_strided_cap < kBatchMaxGroups ? t_strided_cap : kBatchMaxGroups;
    return std::min(cap * kCasPerGroup, count);
}

}  // namespace

extern "C" {

size_t MPIR_Hip_elem_size(int elem) {
    return (elem > 0 && elem < MPIR_HIP_NELEMS) ? g_elem_size[elem] : 0;
}

int MPIR_Hip_has_kernel(int op, int elem) {
    return pair_in_range(op, elem) && g_table[op][elem].fn != nullptr;
}

const char *MPIR_Hip_error_string(void) { return ctx().err; }

uint64_t MPIR_Hip_host_max_bytes(void) { return host_max_bytes(); }

uint64_t MPIR_Hip_set_host_max_bytes(uint64_t bytes) { return g_host_max.exchange(bytes); }

uint64_t MPIR_Hip_set_keep_bytes(uint64_t bytes) { return mpir_hip::g_keep.exchange(bytes); }

uint64_t MPIR_Hip_set_keep_min_bytes(uint64_t bytes) { return mpir_hip::g_keep_min.exchange(bytes); }

uint64_t MPIR_Hip_mixed_max_bytes(void) { return mixed_max_bytes(); }

uint64_t MPIR_Hip_direct_dispatches(void) { return direct_calls(); }

void MPIR_Hip_direct_profile(int on) { direct_profile(on); }

uint64_t MPIR_Hip_direct_last_kernel_ns(void) { return direct_last_kernel_ns(); }

int MPIR_Hip_direct_state(int dev) { return direct_state(dev); }

int MPIR_Hip_direct_prepare(int dev) { return direct_prepare(dev); }

void MPIR_Hip_direct_last_split(uint64_t out[4]) { direct_last_split(out); }

uint64_t MPIR_Hip_direct_busy_skips(void) { return direct_busy_skips(); }

uint64_t MPIR_Hip_direct_kernarg_writes(void) { return direct_kernarg_writes(); }
uint32_t MPIR_Hip_direct_test_write_delay_us(uint32_t us) { return direct_test_write_delay_us(us); }
void MPIR_Hip_direct_test_fail_probe(void) { direct_test_fail_probe(); }
void MPIR_Hip_direct_placement(int dev, int out[5]) { direct_placement(dev, out); }

int MPIR_Hip_set_local_ranks(int n) {
    return g_local_ranks.exchange(n > 0 ? n : 0);
}

int MPIR_Hip_host_threads(void) { return pool_threads(); }

int MPIR_Hip_combine_set_flags(int flags) {
    const int prev = mpir_hip::t_combine_flags;
    mpir_hip::t_combine_flags = flags & MPIR_HIP_COMBINE_UNCAPPED;
    return prev;
}

int MPIR_Hip_thread_contexts(void) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    return g_ctx_created;
}

int MPIR_Hip_device_count(void) { return device_count(); }

int MPIR_Hip_pointer_kind(const void *p, uint64_t bytes) {
    int dev = 0;
    return classify(p, &dev, verdict_reusable(bytes));
}

int MPIR_Hip_is_device_ptr(const void *p) {
    int dev = 0;
    return classify(p, &dev) == LOC_DEVICE;
}

int MPIR_Hip_memcpy(void *dst, const void *src, size_t bytes) {
    if (!bytes) return MPIR_HIP_OK;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return MPIR_HIP_OK;
}

int MPIR_Hip_combine(const void *const *inbufs, int n, void *outbuf, uint64_t count, int op, int elem,
                     int order, void *hip_stream, int sync) {
    ctx().err[0] = 0;
    if (!combine_args_ok(n, op, elem, order)) return MPIR_HIP_ENOKERNEL;
    const size_t esz = g_elem_size[elem];
    int dev = -1;
    if (classify(outbuf, &dev) != LOC_DEVICE) return MPIR_HIP_EBUFFER;
    for (int j = 0; j < n; ++j) {
        int d = -1;
        if (classify(inbufs[j], &d) != LOC_DEVICE || d != dev) return MPIR_HIP_EBUFFER;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    int rc = MPIR_HIP_OK;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    hipError_t e = hipSuccess;
    if (rc == MPIR_HIP_OK && count > 0) {
        switch (combine_route(n, op, elem, order)) {
        case ROUTE_COPY_FIRST:
            if (outbuf != inbufs[0]) e = hipMemcpyAsync(outbuf, inbufs[0], count * esz, hipMemcpyDeviceToDevice, s);
            break;
        case ROUTE_COPY_LAST:
            if (outbuf != inbufs[n - 1])
                e = hipMemcpyAsync(outbuf, inbufs[n - 1], count * esz, hipMemcpyDeviceToDevice, s);
            break;
        case ROUTE_FUSED_TREE:
            e = g_multi[op][elem][0][n - 2](inbufs, outbuf, count, s);
            break;
        case ROUTE_FUSED_CHAIN:
            // CHAIN: acc = y0; fold y1..y_{n-1} in order, one pass for n <= 8
            // (chain_passes beyond)
            chain_passes(inbufs, n, outbuf, [&](const void *const *ops, int P) {
                e = g_multi[op][elem][1][P - 2](ops, outbuf, count, s);
                return e == hipSuccess;
            });
            break;
        case ROUTE_ANY:
            // one pass, no temporaries (k_combine_any)
            e = g_table[op][elem].any(inbufs, n, order == MPIR_HIP_ORDER_TREE, outbuf, count, s);
            break;
        default:
            rc = MPIR_HIP_ENOKERNEL;
            break;
        }
        if (e != hipSuccess) rc = set_err(e, "combine launch");
        if (rc == MPIR_HIP_OK && sync) rc = wait_stream(dev, s);
    }
    return rc;
}

int MPIR_Hip_plan_info(const void *inbuf, const void *inoutbuf, uint64_t count, int op, int elem, uint64_t out[6]) {
    if (!pair_in_range(op, elem)) return MPIR_HIP_ENOKERNEL;
    const Entry &en = g_table[op][elem];
    const plan_fn fn = en.plan ? en.plan : en.wide;
    if (!en.fn || !fn) return MPIR_HIP_ENOKERNEL;
    ReducePlan p;
    fn(inbuf, const_cast<void *>(inoutbuf), count, &p);
    uint64_t nhead = 0, ntail = 0, vbytes = 0, keep = 0;
    switch (p.kind) {
    case kPlanLean:
    case kPlanWideTile: {
        LeanArgs a;
        memcpy(&a, p.args, sizeof a);
        vbytes = a.vbytes;
        keep = a.keep;
        break;
    }
    case kPlanFull:
    case kPlanShift: {
        // TileArgs<T> has one layout for every T (pointers and sizes); it leads ShiftArgs<T>
        TileArgs<char> a;
        memcpy(&a, p.args, sizeof a);
        nhead = a.nhead;
        ntail = a.ntail;
        vbytes = a.vbytes;
        keep = a.keep;
        break;
    }
    default:
        break;
    }
    out[0] = (uint64_t)p.kind;
    out[1] = p.groups;
    out[2] = nhead;
    out[3] = ntail;
    out[4] = vbytes;
    out[5] = keep;
    return MPIR_HIP_OK;
}

int MPIR_Hip_combine_plan_info(const void *const *inbufs, int n, const void *outbuf, uint64_t count, int op, int elem,
                               int order, uint64_t out[4]) {
    if (!combine_args_ok(n, op, elem, order)) return MPIR_HIP_ENOKERNEL;
    uint64_t path = MPIR_HIP_COMBINE_PATH_COPY, passes = 1, nhead = 0, ntail = 0;
    switch (combine_route(n, op, elem, order)) {
    case ROUTE_COPY_FIRST:
    case ROUTE_COPY_LAST:
        break;
    case ROUTE_FUSED_TREE:
    case ROUTE_FUSED_CHAIN: {
        const split_fn split = g_table[op][elem].split;
        if (!split) return MPIR_HIP_ENOKERNEL;
        path = MPIR_HIP_COMBINE_PATH_FUSED_VECTOR;
        auto pass = [&](const void *const *ops, int P) {
            CombineSplit c;
            split(ops, P, outbuf, count, &c);
            if (!c.vec_ok) path = MPIR_HIP_COMBINE_PATH_FUSED_ELEMENTS;
            nhead = c.nhead;        // the same in every vector pass: out and count alone set them
            ntail = c.ntail;
            return true;
        };
        if (order == MPIR_HIP_ORDER_TREE) pass(inbufs, n);
        else passes = (uint64_t)chain_passes(inbufs, n, outbuf, pass);
        if (path == MPIR_HIP_COMBINE_PATH_FUSED_ELEMENTS) nhead = ntail = 0;
        break;
    }
    case ROUTE_ANY:
        path = MPIR_HIP_COMBINE_PATH_ANY;
        break;
    default:
        return MPIR_HIP_ENOKERNEL;
    }
    out[0] = path;
    out[1] = passes;
    out[2] = nhead;
    out[3] = ntail;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce(const void *inbuf, void *inoutbuf, uint64_t count, int op, int elem, void *hip_stream,
                    int sync) {
    if (!MPIR_Hip_has_kernel(op, elem)) return MPIR_HIP_ENOKERNEL;
    if (count == 0) return MPIR_HIP_OK;
    const size_t esz = g_elem_size[elem];
    // REPLACE is registered as a byte copy: its launcher counts bytes
    const uint64_t unit = (op == MPIR_HIP_OP_REPLACE) ? 1 : esz;

    // no GPU runtime in this process: both operands are pageable host memory,
    // combined here with no HIP call (the reference's loop, opsum.c:21-76,
    // touches no device either)
    if (!gpu_runtime_started() && count * esz <= host_max_bytes()) {
        if (!sync) return MPIR_HIP_EBUFFER;
        return host_combine(op, elem, inbuf, inoutbuf, count * esz / unit, unit);
    }

    ctx().err[0] = 0;
    Operands o;
    const bool reuse = verdict_reusable(count * esz);
    o.in.loc = classify(inbuf, &o.in.dev, reuse, &o.in.kept);
    o.io.loc = classify(inoutbuf, &o.io.dev, reuse, &o.io.kept);

    // fast path: both operands device-resident on one device
    if (o.in.loc == LOC_DEVICE && o.io.loc == LOC_DEVICE && o.in.dev == o.io.dev)
        return device_call(o.io.dev, inbuf, inoutbuf, count, op, elem, (hipStream_t)hip_stream, sync);
    if (!sync) return MPIR_HIP_EBUFFER;  // the stream variant needs device buffers

    // both host-resident: combine on the host (no device needed)
    if (o.in.loc != LOC_DEVICE && o.io.loc != LOC_DEVICE &&
        (count * esz <= host_max_bytes() || device_count() == 0) && g_table[op][elem].host) {
        int rc = MPIR_HIP_OK;
        if (o.in.ordered()) rc = order_after_null_stream_of(o.in.order_dev());
        if (rc == MPIR_HIP_OK && o.io.ordered() && !(o.in.ordered() && o.in.order_dev() == o.io.order_dev()))
            rc = order_after_null_stream_of(o.io.order_dev());
        if (rc != MPIR_HIP_OK) return rc;
        return host_combine(op, elem, inbuf, inoutbuf, count * esz / unit, unit);
    }

    // small, one operand host memory and the other on a device: the pinned slot
    if ((o.in.loc == LOC_DEVICE) != (o.io.loc == LOC_DEVICE) && count * esz <= mixed_max_bytes())
        return mixed_call(o, inbuf, inoutbuf, count, op, elem);

    return staged_call(o, inbuf, inoutbuf, count, op, elem);
}

int MPIR_Hip_batch_plan_info(const MPIR_Hip_seg *segs, int nsegs, int op, int elem, uint64_t out[6],
                             uint32_t *seg_kind, uint32_t *seg_groups) {
    if (!batch_args_ok(segs, nsegs, op, elem)) return MPIR_HIP_ENOKERNEL;
    const BatchEntry &en = g_batch[op][elem];
    uint64_t totals[5];
    const int one = batch_single(segs, nsegs);
    if (one >= 0) {
        // the single call's own plan (MPIR_Hip_plan_info)
        const plan_fn fn = g_table[op][elem].plan ? g_table[op][elem].plan : g_table[op][elem].wide;
        if (!fn) return MPIR_HIP_ENOKERNEL;
        ReducePlan p;
        fn(segs[one].in, segs[one].io, segs[one].count, &p);
        for (int i = 0; i < nsegs; ++i) {
            if (seg_kind) seg_kind[i] = i == one ? MPIR_HIP_BATCH_SEG_SINGLE : MPIR_HIP_BATCH_SEG_EMPTY;
            if (seg_groups) seg_groups[i] = i == one ? (uint32_t)p.groups : 0;
        }
        totals[0] = 1;
        totals[1] = p.groups;
        totals[2] = totals[3] = 0;
        totals[4] = (uint64_t)nsegs - 1;
    } else {
        batch_launches(en, segs, nsegs, seg_kind, seg_groups, totals, [](const BatchArgs &, uint64_t) { return true; });
    }
    for (int k = 0; k < 5; ++k) out[k] = totals[k];
    out[5] = (uint64_t)kBatchMaxSegs;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_batch(const MPIR_Hip_seg *segs, int nsegs, int op, int elem, void *hip_stream, int sync) {
    if (!batch_args_ok(segs, nsegs, op, elem)) return MPIR_HIP_ENOKERNEL;
    const BatchEntry &en = g_batch[op][elem];
    ctx().err[0] = 0;
    // every pointer is classified, and every segment sized, before anything is
    // launched: a call that fails has written nothing
    int dev = -1, nonempty = 0;
    DeviceSpan span_in, span_io;
    for (int i = 0; i < nsegs; ++i) {
        if (!segs[i].count) continue;
        int din = -1, dio = -1, tile = 0;
        if (classify_in_span(segs[i].in, &din, span_in) != LOC_DEVICE ||
            classify_in_span(segs[i].io, &dio, span_io) != LOC_DEVICE || din != dio ||
            (nonempty && dio != dev))
            return MPIR_HIP_EBUFFER;
        dev = dio;
        ++nonempty;
        if (en.groups(segs[i].in, segs[i].io, segs[i].count, &tile) > kBatchMaxGroups) {
            snprintf(ctx().err, sizeof(ctx().err), "batch segment %d needs more workgroups than one launch holds", i);
            return MPIR_HIP_ERUNTIME;
        }
    }
    if (nonempty == 0) return MPIR_HIP_OK;
    if (nonempty == 1) {
        // the single call: the direct AQL dispatch when synchronous, every existing plan
        const MPIR_Hip_seg &s = segs[batch_single(segs, nsegs)];
        return MPIR_Hip_reduce(s.in, s.io, s.count, op, elem, hip_stream, sync);
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    int rc = MPIR_HIP_OK;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc == MPIR_HIP_OK) {
        hipError_t e = hipSuccess;
        uint64_t totals[5];
        batch_launches(en, segs, nsegs, nullptr, nullptr, totals, [&](const BatchArgs &a, uint64_t groups) {
            e = en.launch(&a, groups, s);
            return e == hipSuccess;
        });
        // (launches made before one that failed are still queued on the library stream)
        if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
        if (e != hipSuccess) rc = set_err(e, "batch launch");
        else if (sync) rc = wait_stream(dev, s);
    }
    return rc;
}

uint64_t MPIR_Hip_set_strided_wide_bytes(uint64_t bytes) {
    return mpir_hip::g_strided_wide.exchange(std::min(bytes, mpir_hip::kStridedWideMax));
}

uint64_t MPIR_Hip_strided_test_max_groups(uint64_t groups) {
    const uint64_t prev = mpir_hip::t_strided_cap;
    mpir_hip::t_strided_cap = groups;
    return prev;
}

int MPIR_Hip_strided_plan_info(const void *inbuf, uint64_t in_stride, const void *inoutbuf, uint64_t io_stride,
                               uint64_t nblocks, uint64_t blocklen, int op, int elem, uint64_t out[8]) {
    int form = 0;
    const int rc = strided_args(in_stride, io_stride, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[6] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    if (form == MPIR_HIP_STRIDED_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_STRIDED_SINGLE) {
        // the single call's own plan (MPIR_Hip_plan_info)
        const plan_fn fn = g_table[op][elem].plan ? g_table[op][elem].plan : g_table[op][elem].wide;
        if (!fn) return MPIR_HIP_ENOKERNEL;
        ReducePlan p;
        fn(inbuf, const_cast<void *>(inoutbuf), nblocks * blocklen, &p);
        out[1] = 1;
        out[2] = p.groups;
        out[7] = nblocks;
        return MPIR_HIP_OK;
    }
    StridedPlan p;
    strided_plan(inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen, elem, p);
    out[0] = (uint64_t)p.form;
    out[1] = p.launches;
    out[2] = p.groups;
    out[3] = p.per;
    out[7] = p.rows_per_launch;
    if (p.form == MPIR_HIP_STRIDED_WIDE) {
        // every row's path, from the function the batch's planner asks (a loop
        // over rows: this is the test tool, the launch makes none)
        const char *in = static_cast<const char *>(inbuf), *io = static_cast<const char *>(inoutbuf);
        for (uint64_t r = 0; r < nblocks; ++r) {
            int tile = 0;
            (void)g_batch[op][elem].groups(in + r * in_stride, io + r * io_stride, blocklen, &tile);
            ++out[tile ? 4 : 5];
        }
    }
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_strided(const void *inbuf, uint64_t in_stride, void *inoutbuf, uint64_t io_stride,
                            uint64_t nblocks, uint64_t blocklen, int op, int elem, void *hip_stream, int sync) {
    int form = 0;
    int rc = strided_args(in_stride, io_stride, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_STRIDED_EMPTY) return rc;
    ctx().err[0] = 0;
    // the first and the last byte of each operand's span, before anything is
    // launched: a call that fails has written nothing
    const uint64_t row_bytes = blocklen * g_elem_size[elem];
    const char *in = static_cast<const char *>(inbuf);
    char *io = static_cast<char *>(inoutbuf);
    const void *ends[4] = {in, in + (nblocks - 1) * in_stride + row_bytes - 1, io,
                           io + (nblocks - 1) * io_stride + row_bytes - 1};
    int dev = -1;
    DeviceSpan span_in, span_io;
    for (int k = 0; k < 4; ++k) {
        int d = -1;
        if (classify_in_span(ends[k], &d, k < 2 ? span_in : span_io) != LOC_DEVICE || (k && d != dev))
            return MPIR_HIP_EBUFFER;
        dev = d;
    }
    // one row, or contiguous rows: the single call -- the direct AQL dispatch
    // when synchronous, every existing plan
    if (form == MPIR_HIP_STRIDED_SINGLE)
        return MPIR_Hip_reduce(inbuf, inoutbuf, nblocks * blocklen, op, elem, hip_stream, sync);
    StridedPlan p;
    strided_plan(inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen, elem, p);
    if (p.form == MPIR_HIP_STRIDED_WIDE && p.per > kBatchMaxGroups) {
        snprintf(ctx().err, sizeof(ctx().err), "a strided row needs more workgroups than one launch holds");
        return MPIR_HIP_ERUNTIME;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc == MPIR_HIP_OK) {
        hipError_t e = hipSuccess;
        const strided_fn launch = g_strided[op][elem].launch;
        strided_launches(p, inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen,
                         [&](const StridedArgs &a, uint64_t groups) {
                             e = launch(&a, groups, s);
                             return e == hipSuccess;
                         });
        // (launches made before one that failed are still queued on the library stream)
        if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
        if (e != hipSuccess) rc = set_err(e, "strided launch");
        else if (sync) rc = wait_stream(dev, s);
    }
    return rc;
}

int MPIR_Hip_indexed_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                               const int64_t *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                               int op, int elem, uint64_t out[6]) {
    int form = 0;
    const int rc = indexed_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[4] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    if (form == MPIR_HIP_INDEXED_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_INDEXED_SINGLE) {
        // the single call's own plan (MPIR_Hip_plan_info)
        const plan_fn fn = g_table[op][elem].plan ? g_table[op][elem].plan : g_table[op][elem].wide;
        if (!fn) return MPIR_HIP_ENOKERNEL;
        ReducePlan p;
        fn(inbuf, const_cast<void *>(inoutbuf), nblocks * blocklen, &p);
        out[1] = 1;
        out[2] = p.groups;
        out[5] = nblocks;
        return MPIR_HIP_OK;
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    out[0] = (uint64_t)p.form;
    out[1] = p.launches;
    out[2] = p.groups;
    out[3] = p.per;
    out[5] = p.rows_per_launch;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_indexed(const void *inbuf, const int64_t *in_displs, void *inoutbuf, const int64_t *io_displs,
                            uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                            void *hip_stream, int sync) {
    int form = 0;
    int rc = indexed_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_INDEXED_EMPTY) return rc;
    ctx().err[0] = 0;
    // everything the call can classify, before anything is enqueued (a call that
    // fails has written nothing): both bases; the last byte of a packed side;
    // each table -- device memory on the operands' device, both its ends, or, in a
    // synchronous call on the library stream, host memory, which is then read for
    // the blocks' extremes
    const uint64_t row_bytes = blocklen * g_elem_size[elem];
    const char *in = static_cast<const char *>(inbuf);
    char *io = static_cast<char *>(inoutbuf);
    const int64_t *displs[2] = {in_displs, io_displs};
    const char *base[2] = {in, io};
    bool host_table[2] = {false, false};
    int dev = -1;
    DeviceSpan span[2];
    for (int k = 0; k < 2; ++k) {
        int d = -1;
        if (classify_in_span(base[k], &d, span[k]) != LOC_DEVICE || (k && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
        if (!displs[k] &&
            (classify_in_span(base[k] + (nblocks * row_bytes - 1), &d, span[k]) != LOC_DEVICE || d != dev))
            return MPIR_HIP_EBUFFER;
    }
    for (int k = 0; k < 2; ++k) {
        if (!displs[k]) continue;
        DeviceSpan ts;
        int d = -1;
        const Loc first = classify_in_span(displs[k], &d, ts);
        if (first == LOC_DEVICE) {
            int d2 = -1;
            if (d != dev ||
                classify_in_span(reinterpret_cast<const char *>(displs[k] + nblocks) - 1, &d2, ts) != LOC_DEVICE ||
                d2 != dev)
                return MPIR_HIP_EBUFFER;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        rc = indexed_host_table(base[k], displs[k], disp_unit, nblocks, row_bytes, dev);
        if (rc != MPIR_HIP_OK) return rc;
    }
    // both tables NULL: the single call -- the direct AQL dispatch when
    // synchronous, every existing plan
    if (form == MPIR_HIP_INDEXED_SINGLE)
        return MPIR_Hip_reduce(inbuf, inoutbuf, nblocks * blocklen, op, elem, hip_stream, sync);
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    if (p.form == MPIR_HIP_INDEXED_WIDE && p.per > kBatchMaxGroups) {
        snprintf(ctx().err, sizeof(ctx().err), "an indexed block needs more workgroups than one launch holds");
        return MPIR_HIP_ERUNTIME;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernels (the earlier synchronous call that read the buffer has returned)
        const size_t tbytes = (size_t)nblocks * sizeof(int64_t);
        char *buf = nullptr;
        rc = get_tables(dev, tbytes * ((size_t)host_table[0] + (size_t)host_table[1]), &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 2; ++k) {
            if (!host_table[k]) continue;
            const hipError_t ce = hipMemcpyAsync(buf, displs[k], tbytes, hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (the other table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "indexed table copy");
            }
            displs[k] = reinterpret_cast<const int64_t *>(buf);
            buf += tbytes;
        }
    }
    hipError_t e = hipSuccess;
    const indexed_fn launch = g_indexed[op][elem].launch;
    indexed_launches(p, inbuf, displs[0], inoutbuf, displs[1], disp_unit, nblocks, blocklen,
                     [&](const IndexedArgs &a, uint64_t groups) {
                         e = launch(&a, groups, s);
                         return e == hipSuccess;
                     });
    // (launches made before one that failed are still queued on the library stream)
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "indexed launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_indexed_ordered_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                       const int64_t *io_displs, const int *order, uint64_t disp_unit,
                                       uint64_t nblocks, uint64_t blocklen, int op, int elem, uint64_t out[6]) {
    if (!order)
        return MPIR_Hip_indexed_plan_info(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, op, elem,
                                          out);
    int form = 0;
    const int rc = ordered_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[4] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    if (form == MPIR_HIP_INDEXED_EMPTY) return MPIR_HIP_OK;
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    out[0] = (uint64_t)p.form;
    out[1] = p.launches;
    out[2] = p.groups;
    out[3] = p.per;
    out[5] = p.rows_per_launch;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_indexed_ordered(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                    const int64_t *io_displs, const int *order, uint64_t disp_unit, uint64_t nblocks,
                                    uint64_t blocklen, int op, int elem, void *hip_stream, int sync) {
    // no order table: a promise of no repeats, the indexed call unchanged
    if (!order)
        return MPIR_Hip_reduce_indexed(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, op, elem,
                                       hip_stream, sync);
    int form = 0;
    int rc = ordered_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_INDEXED_EMPTY) return rc;
    ctx().err[0] = 0;
    // everything classified before anything is enqueued, as the indexed call
    // does: both bases, the last byte of a packed input, and the three tables --
    // device memory on the operands' device or, in a synchronous call on the
    // library stream, host memory, which is then read and checked
    const uint64_t row_bytes = blocklen * g_elem_size[elem];
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    const void *table[3] = {in_displs, io_displs, order};
    const size_t tbytes[3] = {(size_t)nblocks * sizeof(int64_t), (size_t)nblocks * sizeof(int64_t),
                              (size_t)nblocks * sizeof(int)};
    bool host_table[3] = {false, false, false};
    int dev = -1;
    DeviceSpan span[2];
    for (int k = 0; k < 2; ++k) {
        int d = -1;
        if (classify_in_span(base[k], &d, span[k]) != LOC_DEVICE || (k && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
        if (!table[k] &&
            (classify_in_span(base[k] + (nblocks * row_bytes - 1), &d, span[k]) != LOC_DEVICE || d != dev))
            return MPIR_HIP_EBUFFER;
    }
    for (int k = 0; k < 3; ++k) {
        if (!table[k]) continue;
        if (table_on_device(table[k], tbytes[k], &dev, &rc)) {
            if (rc != MPIR_HIP_OK) return rc;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        if (k < 2) rc = indexed_host_table(base[k], static_cast<const int64_t *>(table[k]), disp_unit, nblocks, row_bytes, dev);
        else rc = ordered_host_order(order, host_table[1] ? io_displs : nullptr, nblocks);
        if (rc != MPIR_HIP_OK) return rc;
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    if (p.form == MPIR_HIP_INDEXED_WIDE && p.per > kBatchMaxGroups) {
        snprintf(ctx().err, sizeof(ctx().err), "an indexed block needs more workgroups than one launch holds");
        return MPIR_HIP_ERUNTIME;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1] || host_table[2]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernels; the order table's ints last, so the displacements stay 8-byte aligned
        size_t total = 0;
        for (int k = 0; k < 3; ++k) total += host_table[k] ? tbytes[k] : 0;
        char *buf = nullptr;
        rc = get_tables(dev, total, &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 3; ++k) {
            if (!host_table[k]) continue;
            const hipError_t ce = hipMemcpyAsync(buf, table[k], tbytes[k], hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (another table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "ordered indexed table copy");
            }
            table[k] = buf;
            buf += tbytes[k];
        }
    }
    hipError_t e = hipSuccess;
    const ordered_fn launch = g_ordered[op][elem].launch;
    ordered_launches(p, inbuf, static_cast<const int64_t *>(table[0]), inoutbuf, static_cast<const int64_t *>(table[1]),
                     static_cast<const int *>(table[2]), disp_unit, nblocks, blocklen,
                     [&](const OrderedArgs &a, uint64_t groups) {
                         e = launch(&a, groups, s);
                         return e == hipSuccess;
                     });
    // (launches made before one that failed are still queued on the library stream)
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "ordered indexed launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_order_worksize(uint64_t nblocks, uint64_t *work_bytes) {
    if (nblocks > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    *work_bytes = (uint64_t)order_worksize(nblocks);
    return MPIR_HIP_OK;
}

int MPIR_Hip_order_build(const int64_t *displs, uint64_t nblocks, int *order, void *work, uint64_t work_bytes,
                         void *hip_stream, int sync) {
    if (nblocks > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    if (!nblocks) return MPIR_HIP_OK;
    ctx().err[0] = 0;
    const size_t need = order_worksize(nblocks);
    if (work && work_bytes < need) return MPIR_HIP_EARG;
    const size_t dbytes = (size_t)nblocks * sizeof(int64_t), obytes = (size_t)nblocks * sizeof(int);
    int dev = -1, rc = MPIR_HIP_OK;
    const bool displs_dev = table_on_device(displs, dbytes, &dev, &rc);
    if (rc != MPIR_HIP_OK) return rc;
    const bool order_dev = table_on_device(order, obytes, &dev, &rc);
    if (rc != MPIR_HIP_OK) return rc;
    if ((!displs_dev || !order_dev) && (hip_stream || !sync)) return MPIR_HIP_EBUFFER;      // a host table with a stream
    if (!work && hip_stream) return MPIR_HIP_EBUFFER;
    if (!displs_dev && !order_dev) {
        // both tables on the host: a host sort, no GPU runtime needed
        for (uint64_t k = 0; k < nblocks; ++k) order[k] = (int)k;
        std::stable_sort(order, order + nblocks, [displs](int a, int b) { return displs[a] < displs[b]; });
        return MPIR_HIP_OK;
    }
    if (work) {
        int wrc = MPIR_HIP_OK;
        if (!table_on_device(work, need, &dev, &wrc) || wrc != MPIR_HIP_OK) return MPIR_HIP_EBUFFER;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    // what the caller did not give in device memory comes from the thread's table
    // buffer (a synchronous call: done with it on return): a host side's device
    // copy, and the scratch
    const size_t al = 256;
    const size_t part[3] = {displs_dev ? 0 : (dbytes + al - 1) & ~(al - 1), order_dev ? 0 : (obytes + al - 1) & ~(al - 1),
                            work ? 0 : need};
    const int64_t *d_displs = displs;
    int *d_order = order;
    if (part[0] + part[1] + part[2]) {
        char *buf = nullptr;
        rc = get_tables(dev, part[0] + part[1] + part[2], &buf);
        if (rc != MPIR_HIP_OK) return rc;
        if (part[0]) {
            const hipError_t ce = hipMemcpyAsync(buf, displs, dbytes, hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "order build table copy");
            }
            d_displs = reinterpret_cast<const int64_t *>(buf);
        }
        if (part[1]) d_order = reinterpret_cast<int *>(buf + part[0]);
        if (part[2]) {
            work = buf + part[0] + part[1];
            work_bytes = need;
        }
    }
    size_t wants = 0;
    // (never past the reported size, whatever the caller's buffer holds beyond it)
    work_bytes = need;
    hipError_t e = order_sort(d_displs, nblocks, d_order, work, need, s, &wants);
    if (e == hipSuccess && part[1]) e = hipMemcpyAsync(order, d_order, obytes, hipMemcpyDeviceToHost, s);
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) {
        if (wants > work_bytes) {
            snprintf(ctx().err, sizeof(ctx().err), "the order sort needs %zu bytes of work, MPIR_Hip_order_worksize gave %zu",
                     wants, need);
            return MPIR_HIP_ERUNTIME;
        }
        return set_err(e, "order build");
    }
    if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_ragged_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                              const int64_t *io_displs, const int64_t *starts, uint64_t disp_unit, uint64_t npieces,
                              uint64_t count, int op, int elem, uint64_t out[6]) {
    int form = 0;
    const int rc = ragged_args(in_displs, io_displs, starts, disp_unit, npieces, count, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    if (form == MPIR_HIP_RAGGED_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_RAGGED_SINGLE) {
        // the single call's own plan (MPIR_Hip_plan_info)
        const plan_fn fn = g_table[op][elem].plan ? g_table[op][elem].plan : g_table[op][elem].wide;
        if (!fn) return MPIR_HIP_ENOKERNEL;
        ReducePlan p;
        fn(inbuf, const_cast<void *>(inoutbuf), count, &p);
        out[1] = 1;
        out[2] = p.groups;
        return MPIR_HIP_OK;
    }
    RaggedPlan p;
    ragged_plan(npieces, count, elem, p);
    out[1] = 1;
    out[2] = p.groups;
    out[3] = p.per;
    out[4] = p.rounds;
    out[5] = p.lds_entries;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_ragged(const void *inbuf, const int64_t *in_displs, void *inoutbuf, const int64_t *io_displs,
                           const int64_t *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count, int op,
                           int elem, void *hip_stream, int sync) {
    int form = 0;
    int rc = ragged_args(in_displs, io_displs, starts, disp_unit, npieces, count, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_RAGGED_EMPTY) return rc;
    ctx().err[0] = 0;
    // Everything is settled before anything is enqueued (a call that fails has
    // written nothing).  First the tables: each is device memory, both its ends,
    // or, in a synchronous call on the library stream, host memory, which is
    // then read for what is wrong with it whatever the operands are -- starts
    // for its three conditions, a displacement table for its products
    // (MPIR_HIP_EARG).  Then residency: both bases on one device; the last byte
    // of a packed side; the device tables on that device; and, where starts is a
    // host table beside a host displacement table, the pieces' extremes.
    const uint64_t esz = g_elem_size[elem];
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    // both tables NULL: the single call, and starts is not looked at
    const bool single = form == MPIR_HIP_RAGGED_SINGLE;
    const int64_t *table[3] = {in_displs, io_displs, single ? nullptr : starts};
    const uint64_t entries[3] = {npieces, npieces, npieces + 1};
    bool host_table[3] = {false, false, false};
    int table_dev[3] = {-1, -1, -1};
    for (int k = 2; k >= 0; --k) {
        if (!table[k]) continue;
        DeviceSpan ts;
        if (classify_in_span(table[k], &table_dev[k], ts) == LOC_DEVICE) {
            int d2 = -1;
            if (classify_in_span(reinterpret_cast<const char *>(table[k] + entries[k]) - 1, &d2, ts) != LOC_DEVICE ||
                d2 != table_dev[k])
                return MPIR_HIP_EBUFFER;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        rc = k == 2 ? ragged_host_starts(starts, npieces, count) : ragged_host_products(table[k], disp_unit, npieces);
        if (rc != MPIR_HIP_OK) return rc;
    }
    int dev = -1;
    DeviceSpan span[2];
    for (int k = 0; k < 2; ++k) {
        int d = -1;
        if (classify_in_span(base[k], &d, span[k]) != LOC_DEVICE || (k && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
        if (!table[k] && (classify_in_span(base[k] + (count * esz - 1), &d, span[k]) != LOC_DEVICE || d != dev))
            return MPIR_HIP_EBUFFER;
    }
    if (single) return MPIR_Hip_reduce(inbuf, inoutbuf, count, op, elem, hip_stream, sync);
    for (int k = 0; k < 3; ++k) {
        if (!table[k]) continue;
        if (!host_table[k] && table_dev[k] != dev) return MPIR_HIP_EBUFFER;
        if (host_table[k] && k < 2 && host_table[2]) {
            rc = ragged_host_extremes(base[k], table[k], starts, disp_unit, npieces, esz, dev);
            if (rc != MPIR_HIP_OK) return rc;
        }
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1] || host_table[2]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernel (the earlier synchronous call that read the buffer has returned)
        size_t total = 0;
        for (int k = 0; k < 3; ++k) total += host_table[k] ? (size_t)entries[k] * sizeof(int64_t) : 0;
        char *buf = nullptr;
        rc = get_tables(dev, total, &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 3; ++k) {
            if (!host_table[k]) continue;
            const size_t tbytes = (size_t)entries[k] * sizeof(int64_t);
            const hipError_t ce = hipMemcpyAsync(buf, table[k], tbytes, hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (another table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "ragged table copy");
            }
            table[k] = reinterpret_cast<const int64_t *>(buf);
            buf += tbytes;
        }
    }
    const RaggedArgs a{base[0], static_cast<char *>(inoutbuf), table[0], table[1], table[2], disp_unit,
                       (uint32_t)npieces, (uint32_t)count};
    const hipError_t e = g_ragged[op][elem].launch(&a, s);
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "ragged launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_fetch_plan_info(const void *inbuf, const void *inoutbuf, const void *fetchbuf, uint64_t count, int op,
                             int elem, uint64_t out[4]) {
    int path = 0;
    const int rc = fetch_args(count, op, elem, &path);
    if (rc != MPIR_HIP_OK) return rc;
    out[0] = (uint64_t)path;
    out[1] = out[2] = out[3] = 0;
    if (path != MPIR_HIP_FETCH_TILE) return MPIR_HIP_OK;
    const FetchArgs a{static_cast<const char *>(inbuf), static_cast<char *>(const_cast<void *>(inoutbuf)),
                      static_cast<char *>(const_cast<void *>(fetchbuf)), count};
    FetchPlan p;
    g_fetch[op][elem].plan(&a, &p);
    out[0] = p.tile ? MPIR_HIP_FETCH_TILE : MPIR_HIP_FETCH_ELEMS;
    out[1] = p.groups;
    out[2] = p.nhead;
    out[3] = p.ntail;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_fetch(const void *inbuf, void *inoutbuf, void *fetchbuf, uint64_t count, int op, int elem,
                          void *hip_stream, int sync) {
    int path = 0;
    int rc = fetch_args(count, op, elem, &path);
    if (rc != MPIR_HIP_OK || path == MPIR_HIP_FETCH_EMPTY) return rc;
    ctx().err[0] = 0;
    // the first and the last byte of every buffer the call looks at (NO_OP never
    // looks at inbuf), and the kernel's plan, before anything is enqueued: a call
    // that fails has written nothing
    const uint64_t bytes = count * g_elem_size[elem];
    const char *in = static_cast<const char *>(inbuf);
    char *io = static_cast<char *>(inoutbuf), *fe = static_cast<char *>(fetchbuf);
    const void *ends[6] = {io, io + bytes - 1, fe, fe + bytes - 1, in, in ? in + bytes - 1 : in};
    DeviceSpan span[3];
    int dev = -1;
    for (int k = 0; k < (op == MPIR_HIP_OP_NO_OP ? 4 : 6); ++k) {
        int d = -1;
        if (classify_in_span(ends[k], &d, span[k / 2]) != LOC_DEVICE || (k && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
    }
    const FetchArgs a{in, io, fe, count};
    if (path == MPIR_HIP_FETCH_TILE) {
        FetchPlan p;
        g_fetch[op][elem].plan(&a, &p);
        if (p.groups > kBatchMaxGroups) {
            snprintf(ctx().err, sizeof(ctx().err), "a fetching reduction of this size needs more workgroups than one launch holds");
            return MPIR_HIP_ERUNTIME;
        }
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc == MPIR_HIP_OK) {
        hipError_t e;
        if (path == MPIR_HIP_FETCH_COPY) {
            // stream-ordered device copies: the old bytes out, then (REPLACE) the new ones in
            e = hipMemcpyAsync(fe, io, bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && op == MPIR_HIP_OP_REPLACE && in != io)
                e = hipMemcpyAsync(io, in, bytes, hipMemcpyDeviceToDevice, s);
        } else {
            e = g_fetch[op][elem].launch(&a, s);
        }
        // (a copy enqueued before one that failed is still queued on the library stream)
        if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
        if (e != hipSuccess) rc = set_err(e, "fetch launch");
        else if (sync) rc = wait_stream(dev, s);
    }
    return rc;
}

int MPIR_Hip_fetch_ragged_plan_info(const void *inbuf, const void *inoutbuf, const int64_t *io_displs,
                                    const void *fetchbuf, const int64_t *starts, uint64_t disp_unit, uint64_t npieces,
                                    uint64_t count, int op, int elem, uint64_t out[7]) {
    int form = 0;
    const int rc = fetch_ragged_args(io_displs, starts, disp_unit, npieces, count, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 7; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    if (form == MPIR_HIP_RAGGED_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_RAGGED_SINGLE) {
        // the fetch call's own plan (MPIR_Hip_fetch_plan_info)
        uint64_t f[4];
        const int frc = MPIR_Hip_fetch_plan_info(inbuf, inoutbuf, fetchbuf, count, op, elem, f);
        if (frc != MPIR_HIP_OK) return frc;
        out[1] = f[0] == MPIR_HIP_FETCH_COPY && op == MPIR_HIP_OP_REPLACE ? 2 : 1;
        out[2] = f[1];
        return MPIR_HIP_OK;
    }
    RaggedPlan p;
    ragged_plan(npieces, count, elem, p);
    out[1] = 1;
    out[2] = p.groups;
    out[3] = p.per;
    out[4] = p.rounds;
    out[5] = p.lds_entries;
    out[6] = fetch_ragged_packed_aligned(inbuf, fetchbuf, op);
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_fetch_ragged(const void *inbuf, void *inoutbuf, const int64_t *io_displs, void *fetchbuf,
                                 const int64_t *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count, int op,
                                 int elem, void *hip_stream, int sync) {
    int form = 0;
    int rc = fetch_ragged_args(io_displs, starts, disp_unit, npieces, count, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_RAGGED_EMPTY) return rc;
    // no table: the fetch call, which makes its own checks; starts is not looked at
    if (form == MPIR_HIP_RAGGED_SINGLE)
        return MPIR_Hip_reduce_fetch(inbuf, inoutbuf, fetchbuf, count, op, elem, hip_stream, sync);
    ctx().err[0] = 0;
    // Everything is settled before anything is enqueued (a call that fails has
    // written nothing), in MPIR_Hip_reduce_ragged's order.  First the tables:
    // device memory, both ends, or, in a synchronous call on the library stream,
    // host memory, which is then read for what is wrong with it (MPIR_HIP_EARG).
    // Then residency: the three bases on one device (NO_OP never looks at inbuf),
    // the last byte of the two packed sides, the device tables on that device;
    // and, where both tables are host tables, the pieces' extremes and fetchbuf's
    // range against the extent between them.
    const uint64_t esz = g_elem_size[elem];
    const bool no_op = op == MPIR_HIP_OP_NO_OP;
    const int64_t *table[2] = {io_displs, starts};
    const uint64_t entries[2] = {npieces, npieces + 1};
    bool host_table[2] = {false, false};
    int table_dev[2] = {-1, -1};
    for (int k = 1; k >= 0; --k) {
        DeviceSpan ts;
        if (classify_in_span(table[k], &table_dev[k], ts) == LOC_DEVICE) {
            int d2 = -1;
            if (classify_in_span(reinterpret_cast<const char *>(table[k] + entries[k]) - 1, &d2, ts) != LOC_DEVICE ||
                d2 != table_dev[k])
                return MPIR_HIP_EBUFFER;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        rc = k == 1 ? ragged_host_starts(starts, npieces, count) : ragged_host_products(io_displs, disp_unit, npieces);
        if (rc != MPIR_HIP_OK) return rc;
    }
    const char *in = static_cast<const char *>(inbuf);
    char *io = static_cast<char *>(inoutbuf), *fe = static_cast<char *>(fetchbuf);
    const uint64_t bytes = count * esz;
    int dev = -1;
    {
        // io's base, then the packed sides' first and last bytes
        const void *ends[5] = {io, fe, fe + (bytes - 1), in, in ? in + (bytes - 1) : in};
        DeviceSpan span[3];
        const int which[5] = {0, 1, 1, 2, 2};
        for (int k = 0; k < (no_op ? 3 : 5); ++k) {
            int d = -1;
            if (classify_in_span(ends[k], &d, span[which[k]]) != LOC_DEVICE || (k && d != dev)) return MPIR_HIP_EBUFFER;
            dev = d;
        }
    }
    for (int k = 0; k < 2; ++k)
        if (!host_table[k] && table_dev[k] != dev) return MPIR_HIP_EBUFFER;
    if (host_table[0] && host_table[1]) {
        const char *first = nullptr, *last = nullptr;
        rc = ragged_host_extremes(io, io_displs, starts, disp_unit, npieces, esz, dev, &first, &last);
        if (rc != MPIR_HIP_OK) return rc;
        // the old bytes must not land on a piece: anywhere in the pieces' extent is refused
        const uintptr_t f0 = reinterpret_cast<uintptr_t>(fe), f1 = f0 + (bytes - 1);
        if (f0 <= reinterpret_cast<uintptr_t>(last) && reinterpret_cast<uintptr_t>(first) <= f1) return MPIR_HIP_EBUFFER;
    }
    const fetch_ragged_fn launch = fetch_ragged_kernel(op, elem);
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernel (the earlier synchronous call that read the buffer has returned)
        size_t total = 0;
        for (int k = 0; k < 2; ++k) total += host_table[k] ? (size_t)entries[k] * sizeof(int64_t) : 0;
        char *buf = nullptr;
        rc = get_tables(dev, total, &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 2; ++k) {
            if (!host_table[k]) continue;
            const size_t tbytes = (size_t)entries[k] * sizeof(int64_t);
            const hipError_t ce = hipMemcpyAsync(buf, table[k], tbytes, hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (another table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "fetch ragged table copy");
            }
            table[k] = reinterpret_cast<const int64_t *>(buf);
            buf += tbytes;
        }
    }
    const FetchRaggedArgs a{in, io, fe, table[0], table[1], disp_unit, (uint32_t)npieces, (uint32_t)count,
                            (uint32_t)fetch_ragged_packed_aligned(in, fe, op), 0};
    const hipError_t e = launch(&a, s);
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "fetch ragged launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_fetch_indexed_ordered_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                             const int64_t *io_displs, const void *fetchbuf, const int *order,
                                             uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                             uint64_t out[6]) {
    int form = 0;
    const int rc = fetch_ordered_args(in_displs, io_displs, order, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[4] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    if (form == MPIR_HIP_INDEXED_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_INDEXED_SINGLE) {
        // the fetch call's own plan (MPIR_Hip_fetch_plan_info)
        uint64_t f[4];
        const int frc = MPIR_Hip_fetch_plan_info(inbuf, inoutbuf, fetchbuf, nblocks * blocklen, op, elem, f);
        if (frc != MPIR_HIP_OK) return frc;
        out[1] = f[0] == MPIR_HIP_FETCH_COPY && op == MPIR_HIP_OP_REPLACE ? 2 : 1;
        out[2] = f[1];
        return MPIR_HIP_OK;
    }
    const bool no_op = op == MPIR_HIP_OP_NO_OP;
    StridedPlan p;
    indexed_plan(no_op ? nullptr : inbuf, no_op ? nullptr : in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen,
                 elem, p, fetchbuf);
    out[0] = (uint64_t)p.form;
    out[1] = p.launches;
    out[2] = p.groups;
    out[3] = p.per;
    out[5] = p.rows_per_launch;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_fetch_indexed_ordered(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                          const int64_t *io_displs, void *fetchbuf, const int *order, uint64_t disp_unit,
                                          uint64_t nblocks, uint64_t blocklen, int op, int elem, void *hip_stream,
                                          int sync) {
    int form = 0;
    int rc = fetch_ordered_args(in_displs, io_displs, order, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_INDEXED_EMPTY) return rc;
    // no table at all: the fetch call, which makes its own checks
    if (form == MPIR_HIP_INDEXED_SINGLE)
        return MPIR_Hip_reduce_fetch(inbuf, inoutbuf, fetchbuf, nblocks * blocklen, op, elem, hip_stream, sync);
    ctx().err[0] = 0;
    // Everything classified before anything is enqueued, in the ordered call's
    // order: the bases (NO_OP never looks at inbuf or in_displs), the last byte of
    // a packed input and of fetchbuf, then the three tables -- device memory on
    // the operands' device or, in a synchronous call on the library stream, host
    // memory, which is then read and checked.  A host output table also gives the
    // target's extent, which fetchbuf must not meet, and beside no order table is
    // held to the promise that equal entries are adjacent.
    const bool no_op = op == MPIR_HIP_OP_NO_OP;
    if (no_op) {
        inbuf = nullptr;
        in_displs = nullptr;
    }
    const uint64_t row_bytes = blocklen * g_elem_size[elem];
    const uint64_t bytes = nblocks * row_bytes;
    const char *base[3] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf), static_cast<char *>(fetchbuf)};
    const void *table[3] = {in_displs, io_displs, order};
    const size_t tbytes[3] = {(size_t)nblocks * sizeof(int64_t), (size_t)nblocks * sizeof(int64_t),
                              (size_t)nblocks * sizeof(int)};
    bool host_table[3] = {false, false, false};
    int dev = -1;
    DeviceSpan span[3];
    for (int k = no_op ? 1 : 0; k < 3; ++k) {
        int d = -1;
        if (classify_in_span(base[k], &d, span[k]) != LOC_DEVICE || (dev >= 0 && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
        if ((k == 2 || !table[k]) && (classify_in_span(base[k] + (bytes - 1), &d, span[k]) != LOC_DEVICE || d != dev))
            return MPIR_HIP_EBUFFER;
    }
    for (int k = 0; k < 3; ++k) {
        if (!table[k]) continue;
        if (table_on_device(table[k], tbytes[k], &dev, &rc)) {
            if (rc != MPIR_HIP_OK) return rc;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        if (k == 0) {
            rc = indexed_host_table(base[0], in_displs, disp_unit, nblocks, row_bytes, dev);
        } else if (k == 1) {
            const char *first = nullptr, *last = nullptr;
            rc = indexed_host_table(base[1], io_displs, disp_unit, nblocks, row_bytes, dev, &first, &last);
            if (rc != MPIR_HIP_OK) return rc;
            // the fetched bytes must not land on a target block: anywhere in the blocks' extent is refused
            const uintptr_t f0 = reinterpret_cast<uintptr_t>(fetchbuf), f1 = f0 + (bytes - 1);
            if (f0 <= reinterpret_cast<uintptr_t>(last) && reinterpret_cast<uintptr_t>(first) <= f1) return MPIR_HIP_EBUFFER;
            if (!order) rc = fetch_ordered_host_adjacent(io_displs, nblocks);
        } else {
            rc = ordered_host_order(order, host_table[1] ? io_displs : nullptr, nblocks);
        }
        if (rc != MPIR_HIP_OK) return rc;
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p, fetchbuf);
    if (p.form == MPIR_HIP_INDEXED_WIDE && p.per > kBatchMaxGroups) {
        snprintf(ctx().err, sizeof(ctx().err), "an indexed block needs more workgroups than one launch holds");
        return MPIR_HIP_ERUNTIME;
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1] || host_table[2]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernels; the order table's ints last, so the displacements stay 8-byte aligned
        size_t total = 0;
        for (int k = 0; k < 3; ++k) total += host_table[k] ? tbytes[k] : 0;
        char *buf = nullptr;
        rc = get_tables(dev, total, &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 3; ++k) {
            if (!host_table[k]) continue;
            const hipError_t ce = hipMemcpyAsync(buf, table[k], tbytes[k], hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (another table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "fetching ordered indexed table copy");
            }
            table[k] = buf;
            buf += tbytes[k];
        }
    }
    hipError_t e = hipSuccess;
    const fetch_ordered_fn launch = fetch_ordered_kernel(op, elem);
    fetch_ordered_launches(p, inbuf, static_cast<const int64_t *>(table[0]), inoutbuf,
                           static_cast<const int64_t *>(table[1]), fetchbuf, static_cast<const int *>(table[2]), disp_unit,
                           nblocks, blocklen, [&](const FetchOrderedArgs &a, uint64_t groups) {
                               e = launch(&a, groups, s);
                               return e == hipSuccess;
                           });
    // (launches made before one that failed are still queued on the library stream)
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "fetching ordered indexed launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

int MPIR_Hip_cas_plan_info(const void *origin, const void *compare, const void *target, const int64_t *displs,
                           const void *result, const int *order, uint64_t disp_unit, uint64_t count, int elem,
                           uint64_t out[8]) {
    int form = 0;
    const int rc = cas_args(displs, order, disp_unit, count, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[5] = (uint64_t)kCasAhead;
    if (form == MPIR_HIP_CAS_EMPTY) return MPIR_HIP_OK;
    if (form == MPIR_HIP_CAS_INDEXED) {
        const uint64_t rpl = cas_rows_per_launch(count);
        out[1] = (count + rpl - 1) / rpl;
        // (a launch's positions are whole workgroups but the last launch's)
        out[2] = (count / rpl) * ((rpl + kCasPerGroup - 1) / kCasPerGroup) + (count % rpl + kCasPerGroup - 1) / kCasPerGroup;
        out[3] = rpl;
        out[4] = kCasPerGroup;
        return MPIR_HIP_OK;
    }
    const CasContigArgs a{static_cast<const char *>(origin), static_cast<const char *>(compare),
                          static_cast<char *>(const_cast<void *>(target)), static_cast<char *>(const_cast<void *>(result)),
                          count};
    FetchPlan p;
    cas_kernels(elem)->plan(&a, &p);
    out[0] = p.tile ? MPIR_HIP_CAS_CONTIG_TILE : MPIR_HIP_CAS_CONTIG_ELEMS;
    out[1] = 1;
    out[2] = p.groups;
    out[3] = count;
    out[4] = kTileBytes / g_elem_size[elem];
    out[6] = p.nhead;
    out[7] = p.ntail;
    return MPIR_HIP_OK;
}

int MPIR_Hip_cas_indexed_ordered(const void *origin, const void *compare, void *target, const int64_t *displs,
                                 void *result, const int *order, uint64_t disp_unit, uint64_t count, int elem,
                                 void *hip_stream, int sync) {
    int form = 0;
    int rc = cas_args(displs, order, disp_unit, count, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_CAS_EMPTY) return rc;
    ctx().err[0] = 0;
    const CasEntry &en = *cas_kernels(elem);
    // Everything classified before anything is enqueued, as the fetching ordered
    // call classifies: the four bases, the last byte of the three packed buffers
    // and of a contiguous target, then the two tables -- device memory on the
    // operands' device or, in a synchronous call on the library stream, host
    // memory, which is then read and checked.  A host displacement table also
    // gives the targets' extent, which result must not meet, and beside no order
    // table is held to the promise that equal entries are adjacent.
    const uint64_t esz = g_elem_size[elem];
    const uint64_t bytes = count * esz;
    const char *base[4] = {static_cast<const char *>(origin), static_cast<const char *>(compare),
                           static_cast<char *>(result), static_cast<char *>(target)};
    const void *table[2] = {displs, order};
    const size_t tbytes[2] = {(size_t)count * sizeof(int64_t), (size_t)count * sizeof(int)};
    bool host_table[2] = {false, false};
    int dev = -1;
    DeviceSpan span[4];
    for (int k = 0; k < 4; ++k) {
        int d = -1;
        if (classify_in_span(base[k], &d, span[k]) != LOC_DEVICE || (dev >= 0 && d != dev)) return MPIR_HIP_EBUFFER;
        dev = d;
        if ((k < 3 || !displs) && (classify_in_span(base[k] + (bytes - 1), &d, span[k]) != LOC_DEVICE || d != dev))
            return MPIR_HIP_EBUFFER;
    }
    for (int k = 0; k < 2; ++k) {
        if (!table[k]) continue;
        if (table_on_device(table[k], tbytes[k], &dev, &rc)) {
            if (rc != MPIR_HIP_OK) return rc;
            continue;
        }
        if (hip_stream || !sync) return MPIR_HIP_EBUFFER;       // a host table would be read after the call returned
        host_table[k] = true;
        if (k == 0) {
            const char *first = nullptr, *last = nullptr;
            rc = indexed_host_table(base[3], displs, disp_unit, count, esz, dev, &first, &last);
            if (rc != MPIR_HIP_OK) return rc;
            // the old values must not land on a target: anywhere in the targets' extent is refused
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(result), r1 = r0 + (bytes - 1);
            if (r0 <= reinterpret_cast<uintptr_t>(last) && reinterpret_cast<uintptr_t>(first) <= r1) return MPIR_HIP_EBUFFER;
            if (!order) rc = fetch_ordered_host_adjacent(displs, count);
        } else {
            rc = ordered_host_order(order, host_table[0] ? displs : nullptr, count);
        }
        if (rc != MPIR_HIP_OK) return rc;
    }
    const CasContigArgs ca{base[0], base[1], static_cast<char *>(target), static_cast<char *>(result), count};
    if (form != MPIR_HIP_CAS_INDEXED) {
        FetchPlan p;
        en.plan(&ca, &p);
        if (p.groups > kBatchMaxGroups) {
            snprintf(ctx().err, sizeof(ctx().err), "a compare-and-swap of this size needs more workgroups than one launch holds");
            return MPIR_HIP_ERUNTIME;
        }
    }
    DeviceScope on(dev);
    if (!on.ok()) return on.err();
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) rc = get_stream(dev, S_MAIN, &s);
    if (rc != MPIR_HIP_OK) return rc;
    if (host_table[0] || host_table[1]) {
        // host tables into the thread's table buffer, stream-ordered ahead of the
        // kernels; the order table's ints last, so the displacements stay 8-byte aligned
        size_t total = 0;
        for (int k = 0; k < 2; ++k) total += host_table[k] ? tbytes[k] : 0;
        char *buf = nullptr;
        rc = get_tables(dev, total, &buf);
        if (rc != MPIR_HIP_OK) return rc;               // (nothing of this call is queued yet)
        for (int k = 0; k < 2; ++k) {
            if (!host_table[k]) continue;
            const hipError_t ce = hipMemcpyAsync(buf, table[k], tbytes[k], hipMemcpyHostToDevice, s);
            if (ce != hipSuccess) {
                // (the other table's copy may be queued on the library stream)
                ctx().dev[dev].main_pending = true;
                return set_err(ce, "compare-and-swap table copy");
            }
            table[k] = buf;
            buf += tbytes[k];
        }
    }
    hipError_t e = hipSuccess;
    if (form == MPIR_HIP_CAS_INDEXED) {
        // later ranges of sorted positions; the bases and the tables are the call's in
        // every launch (a head test looks back and a run goes on across a launch boundary)
        const uint64_t rpl = cas_rows_per_launch(count);
        for (uint64_t pos0 = 0; pos0 < count && e == hipSuccess; pos0 += rpl) {
            const uint64_t n = std::min(rpl, count - pos0);
            const CasArgs a{base[0], base[1], static_cast<char *>(target), static_cast<const int64_t *>(table[0]),
                            static_cast<char *>(result), static_cast<const int *>(table[1]), disp_unit, (uint32_t)count,
                            (uint32_t)pos0, (uint32_t)n, 0};
            e = en.launch(&a, (n + kCasPerGroup - 1) / kCasPerGroup, s);
        }
    } else {
        e = en.contig(&ca, s);
    }
    // (launches made before one that failed are still queued on the library stream)
    if (!hip_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
    if (e != hipSuccess) rc = set_err(e, "compare-and-swap launch");
    else if (sync) rc = wait_stream(dev, s);
    return rc;
}

}  // extern "C"
