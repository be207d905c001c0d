// table_calls.hip -- the shim's calls on many blocks at once: MPIR_Hip_reduce_batch,
// _strided, _subarray, _fetch, _indexed, _indexed_ordered, _indexed_chunked, _ragged,
// _fetch_ragged, _fetch_indexed_ordered, MPIR_Hip_cas_indexed_ordered,
// MPIR_Hip_order_build and MPIR_Hip_runs_build, with their *_plan_info functions.  Every one settles residency before it
// enqueues (a call that fails has written nothing) and then runs on one call
// frame: the steps below, which each entry point calls in its own order -- that
// order decides which error a caller sees (tests/test_table_call_precedence_gpu.py).
// The single call and its routes are in hip_reduce.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <new>

#include "mpir_hip_reduce.h"
#include "kernel_table.hpp"
#include "host_env.hpp"
#include "shim_ctx.hpp"

using namespace mpir_hip;

namespace mpir_hip {
// Strided rows of at least this many bytes take the wide form (one row's tiles
// per G workgroups), shorter ones the narrow form (rows flattened into units):
// MPIR_CVAR_REDUCE_LOCAL_STRIDED_WIDE_KB, default 16, one tile (DESIGN.md §Strided
// reductions has the sweep behind it); MPIR_Hip_set_strided_wide_bytes() at run
// time.  At most 1 GiB, so that a narrow row's units fit 32 bits.
constexpr uint64_t kStridedWideMax = (uint64_t)1 << 30;
std::atomic<uint64_t> g_strided_wide{(uint64_t)cvar_long("MPIR_CVAR_REDUCE_LOCAL_STRIDED_WIDE_KB", 0, 1L << 20, 16) << 10};
// MPIR_Hip_strided_test_max_groups: the calling thread's per-launch workgroup cap (0: kBatchMaxGroups)
thread_local uint64_t t_strided_cap = 0;
}  // namespace mpir_hip

namespace {

// ------------------------------------------------------------ the shared steps
// The frame of a call that enqueues: `dev` current while it lives, the caller's
// stream or the library's.  open() before the first enqueue; close() after the
// last, with its result: the library stream is marked pending where the call
// leaves work on it unwaited (the stream variant, or launches and copies made
// before one that failed), then the error, or a synchronous call's wait.
struct Frame {
    const int dev;
    void *const user_stream;
    const int sync;
    DeviceScope on;
    hipStream_t s;
    Frame(int dev, void *hip_stream, int sync)
        : dev(dev), user_stream(hip_stream), sync(sync), on(dev), s((hipStream_t)hip_stream) {}
    int open() {
        if (!on.ok()) return on.err();
        return s ? MPIR_HIP_OK : get_stream(dev, S_MAIN, &s);
    }
    int close(hipError_t e, const char *what) {
        if (!user_stream && (!sync || e != hipSuccess)) ctx().dev[dev].main_pending = true;
        if (e != hipSuccess) return set_err(e, what);
        return sync ? wait_stream(dev, s) : MPIR_HIP_OK;
    }
    // emit() of the *_launches loops: `launch` on the frame's stream, until one fails
    template <class Fn>
    auto each(Fn launch, hipError_t &e) {
        return [launch, st = s, &e](const auto &a, uint64_t groups) {
            e = launch(&a, groups, st);
            return e == hipSuccess;
        };
    }
};

// Residency: byte addresses that must all be device memory on one device (`dev`,
// once the first names it).  Operand k's addresses share span[k], the allocation
// that answered last.
struct Residency {
    int dev = -1;
    DeviceSpan span[4];
    bool byte(int k, const void *p) {
        int d = -1;
        if (classify_in_span(p, &d, span[k]) != LOC_DEVICE || (dev >= 0 && d != dev)) return false;
        dev = d;
        return true;
    }
    // operand k's base and, where `packed` bytes of it are contiguous, their last byte
    bool operand(int k, const void *base, uint64_t packed = 0) {
        return byte(k, base) && (!packed || byte(k, static_cast<const char *>(base) + (packed - 1)));
    }
};

// A table of a call: where it is (after stage_tables: its device copy), its
// bytes, and what place_table found.
struct Table {
    const void *p;
    size_t bytes;
    bool host = false;
    int dev = -1;
    template <class T>
    const T *as() const { return static_cast<const T *>(p); }
};

// A table is device memory, both its ends on one device (`dev`, or for dev < 0
// any: t.dev names it), or host memory, which a call could only read after it
// returned unless it is synchronous and on the library stream.  MPIR_HIP_EBUFFER otherwise.
int place_table(Table &t, int dev, const void *hip_stream, int sync) {
    DeviceSpan ts;
    int d2 = -1;
    if (classify_in_span(t.p, &t.dev, ts) != LOC_DEVICE) {
        t.host = true;
        return hip_stream || !sync ? MPIR_HIP_EBUFFER : MPIR_HIP_OK;
    }
    if ((dev >= 0 && t.dev != dev) ||
        classify_in_span(static_cast<const char *>(t.p) + (t.bytes - 1), &d2, ts) != LOC_DEVICE || d2 != t.dev)
        return MPIR_HIP_EBUFFER;
    return MPIR_HIP_OK;
}

// The host tables of t[0..n) into the thread's table buffer in array order,
// stream-ordered ahead of the kernels (the earlier synchronous call that read
// the buffer has returned), and the descriptors repointed.  Callers put a table
// of ints last, so that the displacements stay 8-byte aligned.  `extra` bytes
// behind them (256-aligned) come back in *rest.  A copy that fails closes the
// frame with `what`: another table's copy may be queued on the library stream.
int stage_tables(Frame &f, Table *t, int n, const char *what, size_t extra = 0, char **rest = nullptr) {
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += t[k].host ? t[k].bytes : 0;
    if (!total && !extra) return MPIR_HIP_OK;
    const size_t tables = extra ? (total + 255) & ~(size_t)255 : total;
    char *buf = nullptr;
    const int rc = get_tables(f.dev, tables + extra, &buf);
    if (rc != MPIR_HIP_OK) return rc;                   // (nothing of this call is queued yet)
    if (rest) *rest = buf + tables;
    for (int k = 0; k < n; ++k) {
        if (!t[k].host) continue;
        const hipError_t ce = hipMemcpyAsync(buf, t[k].p, t[k].bytes, hipMemcpyHostToDevice, f.s);
        if (ce != hipSuccess) return f.close(ce, what);
        t[k].p = buf;
        buf += t[k].bytes;
    }
    return MPIR_HIP_OK;
}

// [p, p + bytes) meets the extent first .. last (its last byte) of a host table's blocks
bool meets_extent(const void *p, uint64_t bytes, const char *first, const char *last) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), p1 = p0 + (bytes - 1);
    return p0 <= reinterpret_cast<uintptr_t>(last) && reinterpret_cast<uintptr_t>(first) <= p1;
}

// the size class of an element class of 1 << l bytes, l < n (else -1): the
// kernels of the byte ops and of compare-and-swap are per size
int size_class(int elem, int n) {
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return -1;
    int l = 0;
    while (l < n && ((uint64_t)1 << l) != g_elem_size[elem]) ++l;
    return l < n ? l : -1;
}

// workgroups one launch may hold (MPIR_Hip_strided_test_max_groups lowers it)
uint64_t launch_cap() { return t_strided_cap && t_strided_cap < kBatchMaxGroups ? t_strided_cap : kBatchMaxGroups; }

bool disp_unit_ok(uint64_t disp_unit) { return disp_unit && disp_unit <= (~(uint64_t)0 >> 1); }

// the single call's own plan (MPIR_Hip_plan_info): its workgroups
int single_plan(const void *inbuf, const void *inoutbuf, uint64_t count, int op, int elem, uint64_t *groups) {
    const plan_fn fn = g_table[op][elem].plan ? g_table[op][elem].plan : g_table[op][elem].wide;
    if (!fn) return MPIR_HIP_ENOKERNEL;
    ReducePlan p;
    fn(inbuf, const_cast<void *>(inoutbuf), count, &p);
    *groups = p.groups;
    return MPIR_HIP_OK;
}

// the fetch call's own plan (MPIR_Hip_fetch_plan_info): its launches and workgroups into out[1], out[2]
int fetch_single_plan(const void *inbuf, const void *inoutbuf, const void *fetchbuf, uint64_t count, int op, int elem,
                      uint64_t *out) {
    uint64_t f[4];
    const int rc = MPIR_Hip_fetch_plan_info(inbuf, inoutbuf, fetchbuf, count, op, elem, f);
    if (rc != MPIR_HIP_OK) return rc;
    out[1] = f[0] == MPIR_HIP_FETCH_COPY && op == MPIR_HIP_OP_REPLACE ? 2 : 1;
    out[2] = f[1];
    return MPIR_HIP_OK;
}

// ------------------------------------------------------------------ batch calls
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

// ------------------------------------------------- strided and indexed calls
// The plan of a strided call (MPIR_Hip_reduce_strided launches it,
// MPIR_Hip_strided_plan_info reports it) and, a table where the stride was, of
// the indexed calls: the form, what a workgroup covers and how many rows a
// launch takes, all O(1) in the number of rows.
struct StridedPlan {
    int form;                   // MPIR_HIP_STRIDED_*
    uint64_t threshold;         // the wide / narrow threshold in force
    uint64_t row_bytes;
    uint64_t per;               // WIDE: G, workgroups per row; NARROW: units per workgroup
    uint64_t upr;               // NARROW: units per row
    uint64_t rows_per_launch;
    uint64_t launches, groups;  // over the whole call
};
static_assert(MPIR_HIP_INDEXED_EMPTY == MPIR_HIP_STRIDED_EMPTY && MPIR_HIP_INDEXED_SINGLE == MPIR_HIP_STRIDED_SINGLE &&
                  MPIR_HIP_INDEXED_WIDE == MPIR_HIP_STRIDED_WIDE &&
                  MPIR_HIP_INDEXED_NARROW_VEC == MPIR_HIP_STRIDED_NARROW_VEC &&
                  MPIR_HIP_INDEXED_NARROW_ELEMS == MPIR_HIP_STRIDED_NARROW_ELEMS,
              "the indexed forms are the strided forms");

// workgroups of one launch of n rows
uint64_t strided_launch_groups(const StridedPlan &p, uint64_t n) {
    return p.form == MPIR_HIP_STRIDED_WIDE ? n * p.per : (n * p.upr + p.per - 1) / p.per;
}

// The plan of nblocks rows of blocklen elements.  wide_groups(row_bytes, esz): G
// of the wide form; `align`: every address and step that joins the row's bytes
// in the vector form's 16-byte alignment test.
template <class G>
void row_plan(uint64_t nblocks, uint64_t blocklen, int elem, uint64_t align, G wide_groups, StridedPlan &p) {
    const uint64_t esz = g_elem_size[elem], cap = launch_cap();
    p.row_bytes = blocklen * esz;
    p.threshold = g_strided_wide.load(std::memory_order_relaxed);
    if (p.row_bytes >= p.threshold) {
        p.form = MPIR_HIP_STRIDED_WIDE;
        p.per = wide_groups(p.row_bytes, esz);
        p.upr = 0;
        p.rows_per_launch = cap / p.per;                // a row is never split between launches
    } else {
        const bool vec = esz <= 16 && ((p.row_bytes | align) & 15) == 0;
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

// a wide row that one launch cannot hold: `text` is the call's error, MPIR_HIP_ERUNTIME
int plan_fits(const StridedPlan &p, const char *text) {
    if (p.form != MPIR_HIP_STRIDED_WIDE || p.per <= kBatchMaxGroups) return MPIR_HIP_OK;
    snprintf(ctx().err, sizeof(ctx().err), "%s", text);
    return MPIR_HIP_ERUNTIME;
}

// a plan as the *_plan_info functions report it, rows per launch in out[rows_at]
void plan_out(const StridedPlan &p, uint64_t *out, int rows_at) {
    out[0] = (uint64_t)p.form;
    out[1] = p.launches;
    out[2] = p.groups;
    out[3] = p.per;
    out[rows_at] = p.rows_per_launch;
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
    row_plan(nblocks, blocklen, elem,
             in_stride | io_stride | reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(io),
             [&](uint64_t row_bytes, uint64_t esz) { return strided_row_groups_max(row_bytes, esz, io, io_stride); }, p);
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

// ---- subarray calls: a sub-box of an N-dimensional array on either side.
// The normal form of a call's two boxes: a row of blocklen contiguous elements
// under k outer dimensions, dimension 0 the fastest, each with a count and one
// byte stride per side; where each box begins and ends in its array.  A pure
// function of the integer arguments.
static_assert(MPIR_HIP_SUBARRAY_SINGLE == MPIR_HIP_STRIDED_SINGLE && MPIR_HIP_SUBARRAY_WIDE == MPIR_HIP_STRIDED_WIDE &&
                  MPIR_HIP_SUBARRAY_NARROW_VEC == MPIR_HIP_STRIDED_NARROW_VEC &&
                  MPIR_HIP_SUBARRAY_NARROW_ELEMS == MPIR_HIP_STRIDED_NARROW_ELEMS,
              "the subarray kernel's forms are the strided forms");
struct SubarrayBox {
    int k;
    uint64_t blocklen;
    uint64_t n[MPIR_HIP_SUBARRAY_MAXDIMS];
    uint64_t in_stride[MPIR_HIP_SUBARRAY_MAXDIMS], io_stride[MPIR_HIP_SUBARRAY_MAXDIMS];     // bytes
    uint64_t in_off, io_off;        // bytes from the array's origin to the box's first element
    uint64_t in_span, io_span;      // bytes from the box's first to one past its last
};

// one side's sizes and starts, fastest dimension first (null sizes: packed) -- the
// reference's per-dimension checks (type_create_subarray.c:104-133), the element
// strides and the array's bytes.  False: a check fails, or the bytes pass 63 bits.
bool subarray_side(const int *sizes, const int *starts, const int *subsizes, int ndims, int c_order, uint64_t esz,
                   uint64_t stride[], uint64_t *off) {
    uint64_t elems = 1;
    *off = 0;
    for (int j = 0; j < ndims; ++j) {
        const int d = c_order ? ndims - 1 - j : j;
        const int64_t size = sizes ? sizes[d] : subsizes[d], start = sizes ? starts[d] : 0, sub = subsizes[d];
        if (size < 1 || sub < 1 || start < 0 || sub > size || start > size - sub) return false;
        stride[j] = elems;
        *off += (uint64_t)start * elems * esz;
        if (__builtin_mul_overflow(elems, (uint64_t)size, &elems) || elems > (~(uint64_t)0 >> 1) / esz) return false;
    }
    return true;
}

// MPIR_HIP_EARG where the arguments are not a box the reference would build
int subarray_box(const int *in_sizes, const int *in_starts, const int *io_sizes, const int *io_starts, int ndims,
                 const int *subsizes, int c_order, uint64_t esz, SubarrayBox &b) {
    if (ndims < 1 || ndims > MPIR_HIP_SUBARRAY_MAXDIMS || !subsizes || (in_sizes && !in_starts) ||
        (io_sizes && !io_starts))
        return MPIR_HIP_EARG;
    uint64_t is[MPIR_HIP_SUBARRAY_MAXDIMS], os[MPIR_HIP_SUBARRAY_MAXDIMS];
    if (!subarray_side(in_sizes, in_starts, subsizes, ndims, c_order, esz, is, &b.in_off) ||
        !subarray_side(io_sizes, io_starts, subsizes, ndims, c_order, esz, os, &b.io_off))
        return MPIR_HIP_EARG;
    // a dimension of subsize 1 only moved the base; dimension d + 1 joins d where
    // the box spans all of d on both sides.  An outer dimension's count stays
    // below 2^31 (the kernel's indices are 32-bit): past that it is left unmerged.
    uint64_t n[MPIR_HIP_SUBARRAY_MAXDIMS];
    int m = 0;
    for (int j = 0; j < ndims; ++j) {
        const uint64_t sub = (uint64_t)subsizes[c_order ? ndims - 1 - j : j];
        if (sub == 1) continue;
        if (m && is[j] == n[m - 1] * is[m - 1] && os[j] == n[m - 1] * os[m - 1] &&
            ((is[m - 1] == 1 && os[m - 1] == 1 && m == 1) || n[m - 1] * sub < ((uint64_t)1 << 31))) {
            n[m - 1] *= sub;
            continue;
        }
        n[m] = sub;
        is[m] = is[j];
        os[m] = os[j];
        ++m;
    }
    const int row = m && is[0] == 1 && os[0] == 1;
    b.blocklen = row ? n[0] : 1;
    b.k = m - row;
    b.in_span = b.io_span = b.blocklen * esz;
    for (int d = 0; d < b.k; ++d) {
        b.n[d] = n[d + row];
        b.in_stride[d] = is[d + row] * esz;
        b.io_stride[d] = os[d + row] * esz;
        b.in_span += (b.n[d] - 1) * b.in_stride[d];
        b.io_span += (b.n[d] - 1) * b.io_stride[d];
    }
    return MPIR_HIP_OK;
}

// the dimensions one launch covers, and its rows
int subarray_inner(const SubarrayBox &b) { return std::min(b.k, 3); }
uint64_t subarray_rows(const SubarrayBox &b) {
    uint64_t rows = 1;
    for (int d = 0; d < subarray_inner(b); ++d) rows *= b.n[d];
    return rows;
}

// The plan of a box of two or three outer dimensions, or of each of the
// `*peel` such boxes a call of more is looped over: the strided call's plan of
// their rows, with every outer stride where that call has one -- the peeled
// dimensions' too, so that one plan serves every box of the loop.
void subarray_plan(const SubarrayBox &b, const void *in, const void *io, int elem, StridedPlan &p, uint64_t *peel) {
    uint64_t in_or = 0, io_or = 0;
    *peel = 1;
    for (int d = 0; d < b.k; ++d) {
        in_or |= b.in_stride[d];
        io_or |= b.io_stride[d];
        if (d >= subarray_inner(b)) *peel *= b.n[d];
    }
    row_plan(subarray_rows(b), b.blocklen, elem,
             in_or | io_or | reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(io),
             [&](uint64_t row_bytes, uint64_t esz) { return strided_row_groups_max(row_bytes, esz, io, io_or); }, p);
}

// The launches of a plan (in, io: the boxes' first elements): per box of the
// peeled dimensions, later row ranges named by their first row's outer indices.
// emit(args, groups) per launch, until it returns false.
template <class F>
void subarray_launches(const SubarrayBox &b, const StridedPlan &p, const char *in, char *io, F emit) {
    const int ki = subarray_inner(b);
    const uint64_t rows = subarray_rows(b);
    uint64_t at[MPIR_HIP_SUBARRAY_MAXDIMS] = {0};           // the peeled dimensions' indices
    for (;;) {
        SubarrayArgs a;
        memset(&a, 0, sizeof a);
        a.in = in;
        a.io = io;
        for (int d = ki; d < b.k; ++d) {
            a.in += at[d] * b.in_stride[d];
            a.io += at[d] * b.io_stride[d];
        }
        a.blocklen = b.blocklen;
        for (int d = 0; d < 3; ++d) {
            a.n[d] = d < ki ? (uint32_t)b.n[d] : 1;
            a.in_stride[d] = d < ki ? b.in_stride[d] : 0;
            a.io_stride[d] = d < ki ? b.io_stride[d] : 0;
        }
        a.form = (uint32_t)p.form;
        a.per = (uint32_t)(p.form == MPIR_HIP_STRIDED_WIDE ? p.per : p.upr);
        for (uint64_t row0 = 0; row0 < rows; row0 += p.rows_per_launch) {
            const uint64_t n = std::min(p.rows_per_launch, rows - row0);
            uint64_t r = row0;
            for (int d = 0; d < 3; ++d) {
                a.first[d] = (uint32_t)(r % a.n[d]);
                r /= a.n[d];
            }
            a.nrows = (uint32_t)n;
            if (!emit(a, strided_launch_groups(p, n))) return;
        }
        int d = ki;
        while (d < b.k && ++at[d] == b.n[d]) at[d++] = 0;
        if (d >= b.k) return;
    }
}

// the argument checks MPIR_Hip_reduce_subarray makes before it looks at a
// pointer: the pair's kernels, then the box
int subarray_args(const int *in_sizes, const int *in_starts, const int *io_sizes, const int *io_starts, int ndims,
                  const int *subsizes, int c_order, int op, int elem, SubarrayBox &b) {
    if (!pair_in_range(op, elem) || !g_subarray[op][elem].launch || !g_strided[op][elem].launch ||
        !g_batch[op][elem].groups)
        return MPIR_HIP_ENOKERNEL;
    return subarray_box(in_sizes, in_starts, io_sizes, io_starts, ndims, subsizes, c_order, g_elem_size[elem], b);
}

// the argument checks MPIR_Hip_reduce_indexed makes before it looks at a
// pointer; MPIR_HIP_OK with *form EMPTY or SINGLE where that settles the call
int indexed_args(const void *in_displs, const void *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                 int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_indexed[op][elem].launch || !g_batch[op][elem].groups) return MPIR_HIP_ENOKERNEL;
    // (before the counts, as the MPIX entry checks it: the two layers answer alike)
    if (!disp_unit_ok(disp_unit)) return MPIR_HIP_EARG;
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
    row_plan(nblocks, blocklen, elem,
             reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(io) | reinterpret_cast<uintptr_t>(fetch) |
                 (in_displs || io_displs ? disp_unit : 0),
             indexed_row_groups_max, p);
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
    const char *ends[2] = {base + off_lo, base + off_hi + (row_bytes - 1)};
    Residency r;
    r.dev = dev;
    if (!r.byte(0, ends[0]) || !r.byte(0, ends[1])) return MPIR_HIP_EBUFFER;
    if (first) *first = ends[0];
    if (last) *last = ends[1];
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

// ---- chunked indexed calls: the ordered call's plan, twice.
// the argument checks MPIR_Hip_reduce_indexed_chunked makes before it looks at
// a pointer, for a call with its two tables: the ordered call's in its order
int chunked_args(const void *in_displs, const void *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                 int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_chunked[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    return ordered_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, form);
}

// from one partial's slot to the next: the block's bytes rounded up to 16, and
// 16 for the target's address mod 16 (reduce_kernels.hpp, chunk_slot)
uint64_t chunked_slot_bytes(uint64_t row_bytes) { return ((row_bytes + 15) & ~(uint64_t)15) + 16; }

constexpr uint64_t kChunkedAlign = 256;

// the work of a chunked call: room to align the caller's pointer and two slots
// per window of kChunk sorted positions.  False where it passes 63 bits.
bool chunked_worksize(uint64_t nblocks, uint64_t blocklen, int elem, uint64_t *bytes) {
    const uint64_t esz = g_elem_size[elem], top = ~(uint64_t)0 >> 1;
    if (blocklen > (top - 64) / esz) return false;
    const uint64_t slot = chunked_slot_bytes(blocklen * esz), slots = 2 * ((nblocks + kChunk - 1) / kChunk);
    if (slots && slot > (top - kChunkedAlign) / slots) return false;
    *bytes = kChunkedAlign + slots * slot;
    return true;
}

// A host runstart table, read before anything is enqueued: against its
// definition where the order and output tables are host memory too (else
// null), otherwise 0 <= runstart[p] <= p.  MPIR_HIP_EARG otherwise.
int chunked_host_runs(const int *runstart, const int *order, const int64_t *io_displs, uint64_t nblocks) {
    int head = 0;
    for (uint64_t p = 0; p < nblocks; ++p) {
        if (runstart[p] < 0 || (uint64_t)runstart[p] > p) return MPIR_HIP_EARG;
        if (!order || !io_displs) continue;
        if (!p || io_displs[order[p - 1]] != io_displs[order[p]]) head = (int)p;   // (order: checked before)
        if (runstart[p] != head) return MPIR_HIP_EARG;
    }
    return MPIR_HIP_OK;
}

// The launches of a chunked plan: ordered_launches with k_chunk_partials, then
// again with k_fold_partials -- every launch of the first before any of the second.
template <class F>
void chunked_launches(const StridedPlan &p, const void *in, const int64_t *in_displs, void *io, const int64_t *io_displs,
                      const int *order, const int *runstart, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                      char *work, F emit) {
    bool go = true;
    for (int fold = 0; fold < 2 && go; ++fold)
        ordered_launches(p, in, in_displs, io, io_displs, order, disp_unit, nblocks, blocklen,
                         [&](const OrderedArgs &o, uint64_t groups) {
                             const ChunkedArgs a{o, runstart, work, chunked_slot_bytes(p.row_bytes)};
                             return go = emit(a, fold, groups);
                         });
}

// ---- ragged calls: unequal pieces from a table of packed element offsets.
// the argument checks MPIR_Hip_reduce_ragged makes before it looks at a pointer;
// MPIR_HIP_OK with *form EMPTY or SINGLE where that settles the call
int ragged_args(const void *in_displs, const void *io_displs, const void *starts, uint64_t disp_unit, uint64_t npieces,
                uint64_t count, int op, int elem, int *form) {
    if (!pair_in_range(op, elem) || !g_ragged[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    // (before the counts, as the MPIX entry checks it: the two layers answer alike)
    if (!disp_unit_ok(disp_unit)) return MPIR_HIP_EARG;
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

// The plan of a RAGGED call as the *_plan_info functions report it: one launch
// of ragged_groups workgroups, each a span of 16 KiB of packed elements; the
// rounds of the wave-wide search and the boundaries a workgroup holds in LDS come
// from the kernel's own constants.  Host arithmetic on the counts alone: no
// table is read.
void ragged_plan_out(uint64_t npieces, uint64_t count, int elem, uint64_t *out) {
    const uint64_t esz = g_elem_size[elem];
    out[1] = 1;
    out[2] = ragged_groups(count, esz);
    out[3] = kTileBytes / esz;
    out[4] = ragged_search_rounds(npieces);
    out[5] = kRaggedLdsEntries;
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
    Residency r;                                // (count > 0: some piece is not empty)
    r.dev = dev;
    if (!r.byte(0, base + lo) || !r.byte(0, base + hi)) return MPIR_HIP_EBUFFER;
    if (first) *first = base + lo;
    if (last) *last = base + hi;
    return MPIR_HIP_OK;
}

// The tables of a ragged call, read from the last (starts) to the first: each is
// device memory on any device, or a host table, which is then read for what is
// wrong with it whatever the operands are -- starts for its three conditions, a
// displacement table for its products (MPIR_HIP_EARG).
int ragged_place_tables(Table *t, int n, uint64_t disp_unit, uint64_t npieces, uint64_t count, const void *hip_stream,
                        int sync) {
    for (int k = n - 1; k >= 0; --k) {
        if (!t[k].p) continue;
        int rc = place_table(t[k], -1, hip_stream, sync);
        if (rc == MPIR_HIP_OK && t[k].host)
            rc = k == n - 1 ? ragged_host_starts(t[k].as<int64_t>(), npieces, count)
                            : ragged_host_products(t[k].as<int64_t>(), disp_unit, npieces);
        if (rc != MPIR_HIP_OK) return rc;
    }
    return MPIR_HIP_OK;
}

// ---- fetching ragged calls.  The kernel of (op, elem): the pair's own, or for
// the two byte ops the one of the element's size (null: none)
fetch_ragged_fn fetch_ragged_kernel(int op, int elem) {
    if (op == MPIR_HIP_OP_NO_OP || op == MPIR_HIP_OP_REPLACE) {
        const int l = size_class(elem, kFetchRaggedSizes);
        return l < 0 ? nullptr : g_fetch_ragged_bytes[op == MPIR_HIP_OP_REPLACE][l].launch;
    }
    return pair_in_range(op, elem) ? g_fetch_ragged[op][elem].launch : nullptr;
}

// the argument checks MPIR_Hip_reduce_fetch_ragged makes before it looks at a
// pointer: ragged_args' in ragged_args' order, with one table.  MPIR_HIP_OK with
// *form EMPTY or SINGLE where that settles the call.
int fetch_ragged_args(const void *io_displs, const void *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count,
                      int op, int elem, int *form) {
    if (!fetch_ragged_kernel(op, elem)) return MPIR_HIP_ENOKERNEL;
    if (!disp_unit_ok(disp_unit)) return MPIR_HIP_EARG;
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
    if (op == MPIR_HIP_OP_NO_OP || op == MPIR_HIP_OP_REPLACE) {
        const int l = size_class(elem, kFetchRaggedSizes);
        return l < 0 ? nullptr : g_fetch_ordered_bytes[op == MPIR_HIP_OP_REPLACE][l].launch;
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
    if (!disp_unit_ok(disp_unit)) return MPIR_HIP_EARG;
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

// The host target table of a call that also writes the old values out (to `out`,
// `bytes` of it): indexed_host_table; the old values must not land on a target
// block -- anywhere in the blocks' extent is refused, MPIR_HIP_EBUFFER; and beside
// no order table it is held to the promise that equal entries are adjacent.
int fetching_host_table(const char *base, const int64_t *displs, const int *order, uint64_t disp_unit, uint64_t nblocks,
                        uint64_t row_bytes, int dev, const void *out, uint64_t bytes) {
    const char *first = nullptr, *last = nullptr;
    const int rc = indexed_host_table(base, displs, disp_unit, nblocks, row_bytes, dev, &first, &last);
    if (rc != MPIR_HIP_OK) return rc;
    if (meets_extent(out, bytes, first, last)) return MPIR_HIP_EBUFFER;
    return order ? MPIR_HIP_OK : fetch_ordered_host_adjacent(displs, nblocks);
}

// ---- ordered compare-and-swap.  The kernels of an element class: those of its
// size, 1 to 8 bytes (null: none)
const CasEntry *cas_kernels(int elem) {
    const int l = size_class(elem, kCasSizes);
    return l >= 0 && g_cas[l].launch && g_cas[l].contig && g_cas[l].plan ? &g_cas[l] : nullptr;
}

// the argument checks MPIR_Hip_cas_indexed_ordered makes before it looks at a
// pointer, in the fetching ordered call's order.  MPIR_HIP_OK with *form EMPTY,
// INDEXED, or CONTIG_ELEMS for a call with no table (the plan then says which of
// the contiguous kernel's two paths).
int cas_args(const void *displs, const void *order, uint64_t disp_unit, uint64_t count, int elem, int *form) {
    if (!cas_kernels(elem)) return MPIR_HIP_ENOKERNEL;
    if (!disp_unit_ok(disp_unit)) return MPIR_HIP_EARG;
    *form = MPIR_HIP_CAS_EMPTY;
    if (!count) return MPIR_HIP_OK;
    if (count > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    if (!displs && order) return MPIR_HIP_EARG;             // a contiguous target has no repeats to order
    *form = displs ? MPIR_HIP_CAS_INDEXED : MPIR_HIP_CAS_CONTIG_ELEMS;
    return MPIR_HIP_OK;
}

// sorted positions of one launch of the indexed form: whole workgroups up to the per-launch cap
uint64_t cas_rows_per_launch(uint64_t count) { return std::min(launch_cap() * kCasPerGroup, count); }

}  // namespace

extern "C" {

int MPIR_Hip_batch_plan_info(const MPIR_Hip_seg *segs, int nsegs, int op, int elem, uint64_t out[6],
                             uint32_t *seg_kind, uint32_t *seg_groups) {
    if (!batch_args_ok(segs, nsegs, op, elem)) return MPIR_HIP_ENOKERNEL;
    const BatchEntry &en = g_batch[op][elem];
    uint64_t totals[5];
    const int one = batch_single(segs, nsegs);
    if (one >= 0) {
        uint64_t groups = 0;
        const int rc = single_plan(segs[one].in, segs[one].io, segs[one].count, op, elem, &groups);
        if (rc != MPIR_HIP_OK) return rc;
        for (int i = 0; i < nsegs; ++i) {
            if (seg_kind) seg_kind[i] = i == one ? MPIR_HIP_BATCH_SEG_SINGLE : MPIR_HIP_BATCH_SEG_EMPTY;
            if (seg_groups) seg_groups[i] = i == one ? (uint32_t)groups : 0;
        }
        totals[0] = 1;
        totals[1] = groups;
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
    int nonempty = 0;
    Residency r;
    for (int i = 0; i < nsegs; ++i) {
        if (!segs[i].count) continue;
        int tile = 0;
        if (!r.byte(0, segs[i].in) || !r.byte(1, segs[i].io)) return MPIR_HIP_EBUFFER;
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
    Frame f(r.dev, hip_stream, sync);
    const int rc = f.open();
    if (rc != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    uint64_t totals[5];
    batch_launches(en, segs, nsegs, nullptr, nullptr, totals, f.each(en.launch, e));
    return f.close(e, "batch launch");
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
        out[1] = 1;
        out[7] = nblocks;
        return single_plan(inbuf, inoutbuf, nblocks * blocklen, op, elem, &out[2]);
    }
    StridedPlan p;
    strided_plan(inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen, elem, p);
    plan_out(p, out, 7);
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
    Residency r;
    if (!r.operand(0, inbuf, (nblocks - 1) * in_stride + row_bytes) ||
        !r.operand(1, inoutbuf, (nblocks - 1) * io_stride + row_bytes))
        return MPIR_HIP_EBUFFER;
    // one row, or contiguous rows: the single call -- the direct AQL dispatch
    // when synchronous, every existing plan
    if (form == MPIR_HIP_STRIDED_SINGLE)
        return MPIR_Hip_reduce(inbuf, inoutbuf, nblocks * blocklen, op, elem, hip_stream, sync);
    StridedPlan p;
    strided_plan(inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen, elem, p);
    if ((rc = plan_fits(p, "a strided row needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    strided_launches(p, inbuf, in_stride, inoutbuf, io_stride, nblocks, blocklen, f.each(g_strided[op][elem].launch, e));
    return f.close(e, "strided launch");
}

int MPIR_Hip_subarray_plan_info(const void *inbuf, const int *in_sizes, const int *in_starts, const void *inoutbuf,
                                const int *io_sizes, const int *io_starts, int ndims, const int *subsizes, int c_order,
                                int op, int elem, uint64_t out[MPIR_HIP_SUBARRAY_PLAN_WORDS]) {
    SubarrayBox b;
    int rc = subarray_args(in_sizes, in_starts, io_sizes, io_starts, ndims, subsizes, c_order, op, elem, b);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < MPIR_HIP_SUBARRAY_PLAN_WORDS; ++k) out[k] = 0;
    const char *in = static_cast<const char *>(inbuf) + b.in_off, *io = static_cast<const char *>(inoutbuf) + b.io_off;
    out[5] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    out[7] = (uint64_t)b.k;
    out[8] = b.blocklen;
    out[9] = b.in_off;
    out[10] = b.io_off;
    for (int d = 0; d < b.k; ++d) {
        out[16 + d] = b.n[d];
        out[24 + d] = b.in_stride[d];
        out[32 + d] = b.io_stride[d];
    }
    if (b.k == 0) {
        out[0] = MPIR_HIP_SUBARRAY_SINGLE;
        out[1] = 1;
        out[6] = 1;
        return single_plan(in, io, b.blocklen, op, elem, &out[2]);
    }
    if (b.k == 1) {
        // the strided call's own report of the five numbers it is handed
        uint64_t s[8];
        rc = MPIR_Hip_strided_plan_info(in, b.in_stride[0], io, b.io_stride[0], b.n[0], b.blocklen, op, elem, s);
        if (rc != MPIR_HIP_OK) return rc;
        out[0] = MPIR_HIP_SUBARRAY_STRIDED;
        out[1] = s[1];
        out[2] = s[2];
        out[3] = s[3];
        out[5] = s[6];
        out[6] = s[7];
        out[11] = s[0];
        out[12] = s[4];
        out[13] = s[5];
        return MPIR_HIP_OK;
    }
    StridedPlan p;
    uint64_t peel = 1;
    subarray_plan(b, in, io, elem, p, &peel);
    out[0] = (uint64_t)p.form;
    out[1] = peel * p.launches;
    out[2] = peel * p.groups;
    out[3] = p.per;
    out[4] = p.upr;
    out[6] = p.rows_per_launch;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_subarray(const void *inbuf, const int *in_sizes, const int *in_starts, void *inoutbuf,
                             const int *io_sizes, const int *io_starts, int ndims, const int *subsizes, int c_order,
                             int op, int elem, void *hip_stream, int sync) {
    SubarrayBox b;
    int rc = subarray_args(in_sizes, in_starts, io_sizes, io_starts, ndims, subsizes, c_order, op, elem, b);
    if (rc != MPIR_HIP_OK) return rc;
    ctx().err[0] = 0;
    // the first and the last byte of each operand's box, before anything is
    // launched: a call that fails has written nothing
    const char *in = static_cast<const char *>(inbuf) + b.in_off;
    char *io = static_cast<char *>(inoutbuf) + b.io_off;
    Residency r;
    if (!r.operand(0, in, b.in_span) || !r.operand(1, io, b.io_span)) return MPIR_HIP_EBUFFER;
    // a box that is one run is the single call, one that is rows at one stride
    // the strided call: their planners, kernels and plans, not restated here
    if (b.k == 0) return MPIR_Hip_reduce(in, io, b.blocklen, op, elem, hip_stream, sync);
    if (b.k == 1)
        return MPIR_Hip_reduce_strided(in, b.in_stride[0], io, b.io_stride[0], b.n[0], b.blocklen, op, elem, hip_stream,
                                       sync);
    StridedPlan p;
    uint64_t peel = 1;
    subarray_plan(b, in, io, elem, p, &peel);
    if ((rc = plan_fits(p, "a subarray row needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    subarray_launches(b, p, in, io, f.each(g_subarray[op][elem].launch, e));
    return f.close(e, "subarray launch");
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
        out[1] = 1;
        out[5] = nblocks;
        return single_plan(inbuf, inoutbuf, nblocks * blocklen, op, elem, &out[2]);
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    plan_out(p, out, 5);
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
    const uint64_t row_bytes = blocklen * g_elem_size[elem], bytes = nblocks * row_bytes;
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    Table t[2] = {{in_displs, (size_t)nblocks * sizeof(int64_t)}, {io_displs, (size_t)nblocks * sizeof(int64_t)}};
    Residency r;
    if (!r.operand(0, base[0], in_displs ? 0 : bytes) || !r.operand(1, base[1], io_displs ? 0 : bytes))
        return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 2; ++k) {
        if (!t[k].p) continue;
        rc = place_table(t[k], r.dev, hip_stream, sync);
        if (rc == MPIR_HIP_OK && t[k].host)
            rc = indexed_host_table(base[k], t[k].as<int64_t>(), disp_unit, nblocks, row_bytes, r.dev);
        if (rc != MPIR_HIP_OK) return rc;
    }
    // both tables NULL: the single call -- the direct AQL dispatch when
    // synchronous, every existing plan
    if (form == MPIR_HIP_INDEXED_SINGLE)
        return MPIR_Hip_reduce(inbuf, inoutbuf, nblocks * blocklen, op, elem, hip_stream, sync);
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    if ((rc = plan_fits(p, "an indexed block needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 2, "indexed table copy")) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    indexed_launches(p, inbuf, t[0].as<int64_t>(), inoutbuf, t[1].as<int64_t>(), disp_unit, nblocks, blocklen,
                     f.each(g_indexed[op][elem].launch, e));
    return f.close(e, "indexed launch");
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
    plan_out(p, out, 5);
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
    const uint64_t row_bytes = blocklen * g_elem_size[elem], bytes = nblocks * row_bytes;
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    Table t[3] = {{in_displs, (size_t)nblocks * sizeof(int64_t)}, {io_displs, (size_t)nblocks * sizeof(int64_t)},
                  {order, (size_t)nblocks * sizeof(int)}};
    Residency r;
    if (!r.operand(0, base[0], in_displs ? 0 : bytes) || !r.operand(1, base[1])) return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 3; ++k) {
        if (!t[k].p) continue;
        if ((rc = place_table(t[k], r.dev, hip_stream, sync)) != MPIR_HIP_OK) return rc;
        if (!t[k].host) continue;
        if (k < 2) rc = indexed_host_table(base[k], t[k].as<int64_t>(), disp_unit, nblocks, row_bytes, r.dev);
        else rc = ordered_host_order(order, t[1].host ? io_displs : nullptr, nblocks);
        if (rc != MPIR_HIP_OK) return rc;
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    if ((rc = plan_fits(p, "an indexed block needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 3, "ordered indexed table copy")) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    ordered_launches(p, inbuf, t[0].as<int64_t>(), inoutbuf, t[1].as<int64_t>(), t[2].as<int>(), disp_unit, nblocks,
                     blocklen, f.each(g_ordered[op][elem].launch, e));
    return f.close(e, "ordered indexed launch");
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
    // the two tables and the work, each device memory on the one device or (a
    // table, synchronously on the library stream) host memory; every refusal
    // here is MPIR_HIP_EBUFFER
    Table td{displs, (size_t)nblocks * sizeof(int64_t)}, to{order, (size_t)nblocks * sizeof(int)}, tw{work, need};
    int rc = place_table(td, -1, hip_stream, sync);
    if (rc == MPIR_HIP_OK) rc = place_table(to, td.host ? -1 : td.dev, hip_stream, sync);
    if (rc != MPIR_HIP_OK || (!work && hip_stream)) return MPIR_HIP_EBUFFER;
    if (td.host && to.host) {
        // both tables on the host: a host sort, no GPU runtime needed
        for (uint64_t k = 0; k < nblocks; ++k) order[k] = (int)k;
        std::stable_sort(order, order + nblocks, [displs](int a, int b) { return displs[a] < displs[b]; });
        return MPIR_HIP_OK;
    }
    const int dev = td.host ? to.dev : td.dev;
    if (work && place_table(tw, dev, nullptr, 0) != MPIR_HIP_OK) return MPIR_HIP_EBUFFER;    // (never host memory)
    Frame f(dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    // what the caller did not give in device memory comes from the thread's table
    // buffer (a synchronous call: done with it on return): a host displs' device
    // copy, and behind it a host order's device side and the scratch
    const size_t oside = to.host ? (to.bytes + 255) & ~(size_t)255 : 0;
    char *rest = nullptr;
    if ((rc = stage_tables(f, &td, 1, "order build table copy", oside + (work ? 0 : need), &rest)) != MPIR_HIP_OK) return rc;
    int *d_order = to.host ? reinterpret_cast<int *>(rest) : order;
    if (!work) work = rest + oside;
    size_t wants = 0;
    // (never past the reported size, whatever the caller's buffer holds beyond it)
    hipError_t e = order_sort(td.as<int64_t>(), nblocks, d_order, work, need, f.s, &wants);
    if (e == hipSuccess && to.host) e = hipMemcpyAsync(order, d_order, to.bytes, hipMemcpyDeviceToHost, f.s);
    rc = f.close(e, "order build");
    if (e != hipSuccess && wants > need)
        snprintf(ctx().err, sizeof(ctx().err), "the order sort needs %zu bytes of work, MPIR_Hip_order_worksize gave %zu",
                 wants, need);
    return rc;
}

int MPIR_Hip_chunked_worksize(uint64_t nblocks, uint64_t blocklen, int elem, uint64_t *work_bytes) {
    if (elem <= 0 || elem >= MPIR_HIP_NELEMS) return MPIR_HIP_ENOKERNEL;
    if (nblocks > (uint64_t)INT32_MAX || !chunked_worksize(nblocks, blocklen, elem, work_bytes)) return MPIR_HIP_EARG;
    return MPIR_HIP_OK;
}

int MPIR_Hip_indexed_chunked_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                       const int64_t *io_displs, const int *order, const int *runstart,
                                       uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                       uint64_t out[8]) {
    if (!pair_in_range(op, elem) || !g_chunked[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    if (!order && !runstart) {
        const int rc = MPIR_Hip_indexed_plan_info(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, op,
                                                  elem, out);
        if (rc == MPIR_HIP_OK) {
            out[6] = out[1];
            out[7] = 0;
        }
        return rc;
    }
    int form = 0;
    const int rc = chunked_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK) return rc;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[0] = (uint64_t)form;
    out[4] = mpir_hip::g_strided_wide.load(std::memory_order_relaxed);
    if (form == MPIR_HIP_INDEXED_EMPTY) return MPIR_HIP_OK;
    if (!order || !runstart) return MPIR_HIP_EARG;
    if (!chunked_worksize(nblocks, blocklen, elem, &out[7])) return MPIR_HIP_EARG;
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    plan_out(p, out, 5);
    out[6] = 2 * p.launches;
    return MPIR_HIP_OK;
}

int MPIR_Hip_reduce_indexed_chunked(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                    const int64_t *io_displs, const int *order, const int *runstart,
                                    uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                    void *work, uint64_t work_bytes, void *hip_stream, int sync) {
    if (!pair_in_range(op, elem) || !g_chunked[op][elem].launch) return MPIR_HIP_ENOKERNEL;
    // neither table: a promise of no repeats, the indexed call unchanged
    if (!order && !runstart)
        return MPIR_Hip_reduce_indexed(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, op, elem,
                                       hip_stream, sync);
    int form = 0;
    int rc = chunked_args(in_displs, io_displs, disp_unit, nblocks, blocklen, op, elem, &form);
    if (rc != MPIR_HIP_OK || form == MPIR_HIP_INDEXED_EMPTY) return rc;
    uint64_t need = 0;
    if (!order || !runstart || !chunked_worksize(nblocks, blocklen, elem, &need) || (work && work_bytes < need))
        return MPIR_HIP_EARG;
    ctx().err[0] = 0;
    // Everything is settled before anything is enqueued (a call that fails has
    // written nothing), tables first as the ragged call settles them: each is
    // device memory on any device or, in a synchronous call on the library
    // stream, host memory, and a host order or runstart is then read for what is
    // wrong with it whatever the operands are (MPIR_HIP_EARG).  Then residency
    // as the ordered call's: both bases, the last byte of a packed input, the
    // device tables on the operands' device, a host displacement table's
    // extremes, and the work.
    const uint64_t row_bytes = blocklen * g_elem_size[elem], bytes = nblocks * row_bytes;
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    Table t[4] = {{in_displs, (size_t)nblocks * sizeof(int64_t)}, {io_displs, (size_t)nblocks * sizeof(int64_t)},
                  {order, (size_t)nblocks * sizeof(int)}, {runstart, (size_t)nblocks * sizeof(int)}};
    for (int k = 0; k < 4; ++k)
        if (t[k].p && (rc = place_table(t[k], -1, hip_stream, sync)) != MPIR_HIP_OK) return rc;
    if (t[2].host && (rc = ordered_host_order(order, t[1].host ? io_displs : nullptr, nblocks)) != MPIR_HIP_OK) return rc;
    if (t[3].host &&
        (rc = chunked_host_runs(runstart, t[1].host && t[2].host ? order : nullptr, io_displs, nblocks)) != MPIR_HIP_OK)
        return rc;
    Residency r;
    if (!r.operand(0, base[0], in_displs ? 0 : bytes) || !r.operand(1, base[1])) return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 4; ++k) {
        if (!t[k].p) continue;
        if (!t[k].host && t[k].dev != r.dev) return MPIR_HIP_EBUFFER;
        if (t[k].host && k < 2 &&
            (rc = indexed_host_table(base[k], t[k].as<int64_t>(), disp_unit, nblocks, row_bytes, r.dev)) != MPIR_HIP_OK)
            return rc;
    }
    Table tw{work, (size_t)need};
    if (work ? place_table(tw, r.dev, nullptr, 0) != MPIR_HIP_OK : hip_stream != nullptr) return MPIR_HIP_EBUFFER;
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p);
    if ((rc = plan_fits(p, "an indexed block needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    // (no work given: the thread's table buffer, behind the host tables' copies)
    char *rest = nullptr;
    if ((rc = stage_tables(f, t, 4, "chunked indexed table copy", work ? 0 : need, &rest)) != MPIR_HIP_OK) return rc;
    // (never past the reported size, whatever the caller's buffer holds beyond it)
    char *w = work ? reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(work) + kChunkedAlign - 1) & ~(uintptr_t)(kChunkedAlign - 1))
                   : rest;
    hipError_t e = hipSuccess;
    const chunked_fn launch = g_chunked[op][elem].launch;
    chunked_launches(p, inbuf, t[0].as<int64_t>(), inoutbuf, t[1].as<int64_t>(), t[2].as<int>(), t[3].as<int>(), disp_unit,
                     nblocks, blocklen, w, [&](const ChunkedArgs &a, int fold, uint64_t groups) {
                         e = launch(&a, fold, groups, f.s);
                         return e == hipSuccess;
                     });
    return f.close(e, "chunked indexed launch");
}

int MPIR_Hip_runs_build(const int64_t *displs, const int *order, uint64_t nblocks, int *runstart, void *hip_stream,
                        int sync) {
    if (nblocks > (uint64_t)INT32_MAX) return MPIR_HIP_EARG;
    if (!nblocks) return MPIR_HIP_OK;
    ctx().err[0] = 0;
    // the three tables, each device memory on the one device or (synchronously on
    // the library stream) host memory; every refusal here is MPIR_HIP_EBUFFER
    Table t[3] = {{displs, (size_t)nblocks * sizeof(int64_t)}, {order, (size_t)nblocks * sizeof(int)},
                  {runstart, (size_t)nblocks * sizeof(int)}};
    int dev = -1;
    for (int k = 0; k < 3; ++k) {
        if (place_table(t[k], dev, hip_stream, sync) != MPIR_HIP_OK) return MPIR_HIP_EBUFFER;
        if (!t[k].host) dev = t[k].dev;
    }
    if (t[0].host && t[1].host && t[2].host) {
        // all on the host: a host loop, no GPU runtime needed (an order entry out
        // of range: MPIR_HIP_EARG, nothing written)
        for (uint64_t p = 0; p < nblocks; ++p)
            if (order[p] < 0 || (uint64_t)order[p] >= nblocks) return MPIR_HIP_EARG;
        for (uint64_t p = 0; p < nblocks; ++p)
            runstart[p] = p && displs[order[p - 1]] == displs[order[p]] ? runstart[p - 1] : (int)p;
        return MPIR_HIP_OK;
    }
    Frame f(dev, hip_stream, sync);
    int rc = f.open();
    if (rc != MPIR_HIP_OK) return rc;
    // a host runstart's device side comes from the thread's table buffer, behind
    // the host inputs' copies (a synchronous call: done with it on return)
    const bool rhost = t[2].host;
    char *rest = nullptr;
    if ((rc = stage_tables(f, t, 2, "runs build table copy", rhost ? t[2].bytes : 0, &rest)) != MPIR_HIP_OK) return rc;
    int *d_runs = rhost ? reinterpret_cast<int *>(rest) : runstart;
    hipError_t e = runs_build(t[0].as<int64_t>(), t[1].as<int>(), nblocks, d_runs, f.s);
    if (e == hipSuccess && rhost) e = hipMemcpyAsync(runstart, d_runs, t[2].bytes, hipMemcpyDeviceToHost, f.s);
    return f.close(e, "runs build");
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
        out[1] = 1;
        return single_plan(inbuf, inoutbuf, count, op, elem, &out[2]);
    }
    ragged_plan_out(npieces, count, elem, out);
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
    // written nothing).  First the tables (ragged_place_tables).  Then residency:
    // both bases on one device; the last byte of a packed side; the device tables
    // on that device; and, where starts is a host table beside a host
    // displacement table, the pieces' extremes.
    const uint64_t esz = g_elem_size[elem];
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    // both tables NULL: the single call, and starts is not looked at
    const bool single = form == MPIR_HIP_RAGGED_SINGLE;
    Table t[3] = {{in_displs, (size_t)npieces * sizeof(int64_t)}, {io_displs, (size_t)npieces * sizeof(int64_t)},
                  {single ? nullptr : starts, (size_t)(npieces + 1) * sizeof(int64_t)}};
    if ((rc = ragged_place_tables(t, 3, disp_unit, npieces, count, hip_stream, sync)) != MPIR_HIP_OK) return rc;
    Residency r;
    if (!r.operand(0, base[0], in_displs ? 0 : count * esz) || !r.operand(1, base[1], io_displs ? 0 : count * esz))
        return MPIR_HIP_EBUFFER;
    if (single) return MPIR_Hip_reduce(inbuf, inoutbuf, count, op, elem, hip_stream, sync);
    for (int k = 0; k < 3; ++k) {
        if (!t[k].p) continue;
        if (!t[k].host && t[k].dev != r.dev) return MPIR_HIP_EBUFFER;
        if (t[k].host && k < 2 && t[2].host) {
            rc = ragged_host_extremes(base[k], t[k].as<int64_t>(), starts, disp_unit, npieces, esz, r.dev);
            if (rc != MPIR_HIP_OK) return rc;
        }
    }
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 3, "ragged table copy")) != MPIR_HIP_OK) return rc;
    const RaggedArgs a{base[0], static_cast<char *>(inoutbuf), t[0].as<int64_t>(), t[1].as<int64_t>(), t[2].as<int64_t>(),
                       disp_unit, (uint32_t)npieces, (uint32_t)count};
    return f.close(g_ragged[op][elem].launch(&a, f.s), "ragged launch");
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
    Residency r;
    if (!r.operand(0, io, bytes) || !r.operand(1, fe, bytes) || (op != MPIR_HIP_OP_NO_OP && !r.operand(2, in, bytes)))
        return MPIR_HIP_EBUFFER;
    const FetchArgs a{in, io, fe, count};
    if (path == MPIR_HIP_FETCH_TILE) {
        FetchPlan p;
        g_fetch[op][elem].plan(&a, &p);
        if (p.groups > kBatchMaxGroups) {
            snprintf(ctx().err, sizeof(ctx().err), "a fetching reduction of this size needs more workgroups than one launch holds");
            return MPIR_HIP_ERUNTIME;
        }
    }
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    hipError_t e;
    if (path == MPIR_HIP_FETCH_COPY) {
        // stream-ordered device copies: the old bytes out, then (REPLACE) the new ones in
        e = hipMemcpyAsync(fe, io, bytes, hipMemcpyDeviceToDevice, f.s);
        if (e == hipSuccess && op == MPIR_HIP_OP_REPLACE && in != io)
            e = hipMemcpyAsync(io, in, bytes, hipMemcpyDeviceToDevice, f.s);
    } else {
        e = g_fetch[op][elem].launch(&a, f.s);
    }
    return f.close(e, "fetch launch");
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
    if (form == MPIR_HIP_RAGGED_SINGLE) return fetch_single_plan(inbuf, inoutbuf, fetchbuf, count, op, elem, out);
    ragged_plan_out(npieces, count, elem, out);
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
    // written nothing), in MPIR_Hip_reduce_ragged's order.  First the tables
    // (ragged_place_tables).  Then residency: the three bases on one device (NO_OP
    // never looks at inbuf), the last byte of the two packed sides, the device
    // tables on that device; and, where both tables are host tables, the pieces'
    // extremes and fetchbuf's range against the extent between them.
    const uint64_t esz = g_elem_size[elem], bytes = count * esz;
    Table t[2] = {{io_displs, (size_t)npieces * sizeof(int64_t)}, {starts, (size_t)(npieces + 1) * sizeof(int64_t)}};
    if ((rc = ragged_place_tables(t, 2, disp_unit, npieces, count, hip_stream, sync)) != MPIR_HIP_OK) return rc;
    const char *in = static_cast<const char *>(inbuf);
    char *io = static_cast<char *>(inoutbuf), *fe = static_cast<char *>(fetchbuf);
    Residency r;
    if (!r.operand(0, io) || !r.operand(1, fe, bytes) || (op != MPIR_HIP_OP_NO_OP && !r.operand(2, in, bytes)))
        return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 2; ++k)
        if (!t[k].host && t[k].dev != r.dev) return MPIR_HIP_EBUFFER;
    if (t[0].host && t[1].host) {
        const char *first = nullptr, *last = nullptr;
        rc = ragged_host_extremes(io, io_displs, starts, disp_unit, npieces, esz, r.dev, &first, &last);
        if (rc != MPIR_HIP_OK) return rc;
        // the old bytes must not land on a piece: anywhere in the pieces' extent is refused
        if (meets_extent(fe, bytes, first, last)) return MPIR_HIP_EBUFFER;
    }
    const fetch_ragged_fn launch = fetch_ragged_kernel(op, elem);
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 2, "fetch ragged table copy")) != MPIR_HIP_OK) return rc;
    const FetchRaggedArgs a{in, io, fe, t[0].as<int64_t>(), t[1].as<int64_t>(), disp_unit, (uint32_t)npieces,
                            (uint32_t)count, (uint32_t)fetch_ragged_packed_aligned(in, fe, op), 0};
    return f.close(launch(&a, f.s), "fetch ragged launch");
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
    if (form == MPIR_HIP_INDEXED_SINGLE)
        return fetch_single_plan(inbuf, inoutbuf, fetchbuf, nblocks * blocklen, op, elem, out);
    const bool no_op = op == MPIR_HIP_OP_NO_OP;
    StridedPlan p;
    indexed_plan(no_op ? nullptr : inbuf, no_op ? nullptr : in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen,
                 elem, p, fetchbuf);
    plan_out(p, out, 5);
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
    // memory, which is then read and checked (a host output table: fetching_host_table).
    const bool no_op = op == MPIR_HIP_OP_NO_OP;
    if (no_op) {
        inbuf = nullptr;
        in_displs = nullptr;
    }
    const uint64_t row_bytes = blocklen * g_elem_size[elem], bytes = nblocks * row_bytes;
    const char *base[2] = {static_cast<const char *>(inbuf), static_cast<char *>(inoutbuf)};
    Table t[3] = {{in_displs, (size_t)nblocks * sizeof(int64_t)}, {io_displs, (size_t)nblocks * sizeof(int64_t)},
                  {order, (size_t)nblocks * sizeof(int)}};
    Residency r;
    if ((!no_op && !r.operand(0, base[0], in_displs ? 0 : bytes)) || !r.operand(1, base[1]) ||
        !r.operand(2, fetchbuf, bytes))
        return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 3; ++k) {
        if (!t[k].p) continue;
        if ((rc = place_table(t[k], r.dev, hip_stream, sync)) != MPIR_HIP_OK) return rc;
        if (!t[k].host) continue;
        if (k == 0) rc = indexed_host_table(base[0], in_displs, disp_unit, nblocks, row_bytes, r.dev);
        else if (k == 1) rc = fetching_host_table(base[1], io_displs, order, disp_unit, nblocks, row_bytes, r.dev, fetchbuf, bytes);
        else rc = ordered_host_order(order, t[1].host ? io_displs : nullptr, nblocks);
        if (rc != MPIR_HIP_OK) return rc;
    }
    StridedPlan p;
    indexed_plan(inbuf, in_displs, inoutbuf, io_displs, disp_unit, nblocks, blocklen, elem, p, fetchbuf);
    if ((rc = plan_fits(p, "an indexed block needs more workgroups than one launch holds")) != MPIR_HIP_OK) return rc;
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 3, "fetching ordered indexed table copy")) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    const fetch_ordered_fn launch = fetch_ordered_kernel(op, elem);
    // ordered_launches with fetch beside
    ordered_launches(p, inbuf, t[0].as<int64_t>(), inoutbuf, t[1].as<int64_t>(), t[2].as<int>(), disp_unit, nblocks,
                     blocklen, [&](const OrderedArgs &o, uint64_t groups) {
                         const FetchOrderedArgs a{o, static_cast<char *>(fetchbuf)};
                         e = launch(&a, groups, f.s);
                         return e == hipSuccess;
                     });
    return f.close(e, "fetching ordered indexed launch");
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
    // memory, which is then read and checked (a host displacement table:
    // fetching_host_table, `result` where that call has fetchbuf).
    const uint64_t esz = g_elem_size[elem], bytes = count * esz;
    const char *org = static_cast<const char *>(origin), *cmp = static_cast<const char *>(compare);
    char *tgt = static_cast<char *>(target), *res = static_cast<char *>(result);
    Table t[2] = {{displs, (size_t)count * sizeof(int64_t)}, {order, (size_t)count * sizeof(int)}};
    Residency r;
    if (!r.operand(0, org, bytes) || !r.operand(1, cmp, bytes) || !r.operand(2, res, bytes) ||
        !r.operand(3, tgt, displs ? 0 : bytes))
        return MPIR_HIP_EBUFFER;
    for (int k = 0; k < 2; ++k) {
        if (!t[k].p) continue;
        rc = place_table(t[k], r.dev, hip_stream, sync);
        if (rc == MPIR_HIP_OK && t[k].host)
            rc = k == 0 ? fetching_host_table(tgt, displs, order, disp_unit, count, esz, r.dev, result, bytes)
                        : ordered_host_order(order, t[0].host ? displs : nullptr, count);
        if (rc != MPIR_HIP_OK) return rc;
    }
    const CasContigArgs ca{org, cmp, tgt, res, count};
    if (form != MPIR_HIP_CAS_INDEXED) {
        FetchPlan p;
        en.plan(&ca, &p);
        if (p.groups > kBatchMaxGroups) {
            snprintf(ctx().err, sizeof(ctx().err), "a compare-and-swap of this size needs more workgroups than one launch holds");
            return MPIR_HIP_ERUNTIME;
        }
    }
    Frame f(r.dev, hip_stream, sync);
    if ((rc = f.open()) != MPIR_HIP_OK) return rc;
    if ((rc = stage_tables(f, t, 2, "compare-and-swap table copy")) != MPIR_HIP_OK) return rc;
    hipError_t e = hipSuccess;
    if (form == MPIR_HIP_CAS_INDEXED) {
        // later ranges of sorted positions; the bases and the tables are the call's in
        // every launch (a head test looks back and a run goes on across a launch boundary)
        const uint64_t rpl = cas_rows_per_launch(count);
        for (uint64_t pos0 = 0; pos0 < count && e == hipSuccess; pos0 += rpl) {
            const uint64_t n = std::min(rpl, count - pos0);
            const CasArgs a{org, cmp, tgt, t[0].as<int64_t>(), res, t[1].as<int>(), disp_unit, (uint32_t)count,
                            (uint32_t)pos0, (uint32_t)n, 0};
            e = en.launch(&a, (n + kCasPerGroup - 1) / kCasPerGroup, f.s);
        }
    } else {
        e = en.contig(&ca, f.s);
    }
    return f.close(e, "compare-and-swap launch");
}

}  // extern "C"
