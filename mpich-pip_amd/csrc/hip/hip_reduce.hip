// hip_reduce.hip -- C-ABI shim: the kernel tables, the knobs, the routes of the
// single call (host combine, device, mixed pinned slot, staged pipeline), the
// combine, MPIR_Hip_reduce and the small queries.  The calls on many blocks at
// once (batch, strided, fetching, indexed, ragged, ordered, compare-and-swap)
// are in table_calls.hip, the per-thread streams and buffers in shim_ctx.hpp,
// pointer classification in classify.hip, the host's thread pools and CPU share
// in host_env.hip.
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
SubarrayEntry g_subarray[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
IndexedEntry g_indexed[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
OrderedEntry g_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
ChunkedEntry g_chunked[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
RaggedEntry g_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchEntry g_fetch[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchRaggedEntry g_fetch_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchRaggedEntry g_fetch_ragged_bytes[2][kFetchRaggedSizes];
FetchOrderedEntry g_fetch_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
FetchOrderedEntry g_fetch_ordered_bytes[2][kFetchRaggedSizes];
CasEntry g_cas[kCasSizes];

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

// (these two, and wait_stream below, also serve table_calls.hip: shim_ctx.hpp)
const size_t g_elem_size[MPIR_HIP_NELEMS] = {
    0, 1, 1, 2, 2, 4, 4, 8, 8, 2, 4, 8, 8, 16, 8, 8, 16, 8, 16, 16, 32, 32,
};
static_assert(sizeof(g_elem_size) / sizeof(g_elem_size[0]) == MPIR_HIP_NELEMS, "one size per element class");

bool pair_in_range(int op, int elem) { return op > 0 && op < MPIR_HIP_NOPS && elem > 0 && elem < MPIR_HIP_NELEMS; }
}  // namespace mpir_hip

namespace {

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

}  // namespace

int mpir_hip::wait_stream(int dev, hipStream_t s) {
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

namespace {

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

}  // extern "C"
