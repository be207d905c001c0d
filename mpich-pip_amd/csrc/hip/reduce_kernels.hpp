// reduce_kernels.hpp -- gfx950 streaming kernels for MPIR_Reduce_local.
//
// The combine is element-wise: 2 reads + 1 write per element, arithmetic
// intensity <= 1/12 op/B for fp32, so the roofline is HBM bandwidth and MFMA
// is irrelevant.  The shape below is the winner of tools/bw_sweep*.hip on
// MI355X (256 MiB/operand fp32 SUM, profiles/ and DESIGN.md §Kernels):
//
//   * one 16 KiB tile per operand per 256-thread workgroup (4 x 16 B per lane,
//     lane-contiguous 1 KiB wave-instructions, each wave a contiguous 4 KiB
//     of the tile), no grid-stride loop: the grid
//     is vbytes / 16 KiB workgroups (16384 at 256 MiB), which keeps every CU's
//     queue deep and the DRAM pages of a tile together;
//   * all 8 loads of a lane issued before the first combine (latency hiding
//     by ILP + 8 waves/CU of TLP), with a one-instruction issue gap after
//     each (inout, in) pair (issue_gap below: 0.810 -> 0.830-0.841 of peak);
//   * buffer_load/store_dwordx4 with the `nt` cache policy (aux = 2) on both
//     operands and on the store (a result of at most 64 MiB is stored sc1
//     instead, so it stays in the Infinity Cache for its next reader:
//     kKeepBytes below): streamed-once data should not displace L2 / Infinity
//     Cache lines; measured 0.81 of the 8 TB/s HBM peak vs 0.70 for
//     default-policy loads and 0.63 for a grid-stride loop (before the gap);
//   * the buffer descriptor covers exactly this tile's bytes, so the ragged
//     last tile needs no branch: out-of-range loads return 0 and out-of-range
//     stores are dropped by the hardware range check.
// The < 16 B head (to 16 B-align inout) and tail are handled element-wise by
// workgroup 0 (k_reduce_tile), so a call is always exactly one launch; without
// them the launch takes k_reduce_tile_lean.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mpir_hip_reduce.h"
#include "reduce_ops.hpp"

namespace mpir_hip {

constexpr int kThreads = 256;
constexpr int kVecPerLane = 4;
constexpr uint32_t kTileBytes = kThreads * kVecPerLane * 16;  // 16 KiB per operand
constexpr int kCachePolicyNT = 2;                             // aux bit: nt
constexpr int kCachePolicySC1 = 16;                           // aux bit: sc1 (device scope)
// Store policy (keep_for(), hip_reduce.hip): a result of at most `keep` bytes
// (MPIR_CVAR_REDUCE_LOCAL_KEEP_MB, default kKeepBytes = 64 MiB) is stored with
// sc1 instead of nt, a larger one nt.  An sc1 store allocates in the 256 MB
// Infinity Cache (MALL), an nt store bypasses it; so a result of at most 64 MiB
// stays there for its next reader (the next schedule step, the RCCL send of a
// block, the D2H copy of a staged chunk): 64 MiB re-read within ~256 MiB of
// traffic 27.0 vs 33.2 us (tools/archive/sync_store_ab.hip,
// profiles/archive/r01s4_sync_store_ab.log).  With nothing re-read the two policies
// are within noise at <= 64 MiB, and at 256 MiB sc1 on any part of the result
// costs ~1 us (profiles/archive/r02/pairs_ab.log: a "last 64 MiB sc1" variant only won
// where the bench's own rotation let the next call but three re-read that tail
// from the MALL; withdrawn).  The kernels take the per-call `keep` and store
// sc1 the tiles in the last `keep` bytes: keep = vbytes (all) or 0 (none).
// Nothing else changes: the bytes reach HBM either way (MALL is memory-side).
constexpr uint64_t kKeepBytes = 64ull << 20;
uint64_t keep_bytes();               // MPIR_CVAR_REDUCE_LOCAL_KEEP_MB (hip_reduce.hip)
uint64_t keep_for(uint64_t vbytes);  // the per-call `keep` argument of the kernels

// true for a tile that starts inside the last `keep` bytes of a `vbytes` region
__device__ __forceinline__ bool keep_tile(uint64_t base, uint64_t vbytes, uint64_t keep) {
    return vbytes - base <= keep;
}


typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// one 16-byte store; `keep` (uniform per workgroup: keep_tile) picks sc1
__device__ __forceinline__ void store16(u32x4 v, __amdgpu_buffer_rsrc_t r, int off, bool keep) {
    if (keep) __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kCachePolicySC1);
    else __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kCachePolicyNT);
}

template <class T>
struct Pack16 {
    static_assert(16 % sizeof(T) == 0, "element must divide 16 bytes");
    T e[16 / sizeof(T)];
};

template <class T>
struct TileArgs {
    const char *in;     // 16 B-aligned vector region of inbuf
    char *io;           // 16 B-aligned vector region of inoutbuf
    uint64_t vbytes;    // bytes in the vector region (multiple of 16)
    const T *head_in;   // elements before the vector region
    T *head_io;
    uint32_t nhead;
    const T *tail_in;   // elements after the vector region
    T *tail_io;
    uint32_t ntail;
    uint64_t keep;      // keep_for(vbytes): the last `keep` bytes are stored sc1
};

template <class Op, class T>
__device__ __forceinline__ u32x4 combine16(u32x4 a, u32x4 b) {
    Pack16<T> pa = __builtin_bit_cast(Pack16<T>, a);
    Pack16<T> pb = __builtin_bit_cast(Pack16<T>, b);
    Op op;
    if constexpr (nan_fast<Op, T>::value) {
        // plain IEEE arithmetic (packed where the ISA has it); the x86 NaN
        // rule runs only for lanes whose vector produced a NaN
        Pack16<T> pr;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < (int)(16 / sizeof(T)); ++k) {
            pr.e[k] = Op::raw(pa.e[k], pb.e[k]);
            bad |= isnan_(pr.e[k]);
        }
        if (__builtin_expect(bad, 0)) {
#pragma unroll
            for (int k = 0; k < (int)(16 / sizeof(T)); ++k) pr.e[k] = op(pa.e[k], pb.e[k]);
        }
        return __builtin_bit_cast(u32x4, pr);
    } else {
#pragma unroll
        for (int k = 0; k < (int)(16 / sizeof(T)); ++k) pa.e[k] = op(pa.e[k], pb.e[k]);
        return __builtin_bit_cast(u32x4, pa);
    }
}

// A short issue gap (s_nop 0, pinned in place by scheduling barriers) after
// every (inout, in) pair of 16 B loads.  rocprofv3 kernel trace, 256 MiB fp32
// SUM, same tile otherwise: 119.7 us (0.841 of the HBM peak) vs 124.2 us
// (0.810) with the eight loads back to back (tools/shape_ab.hip,
// profiles/archive/r01s3_shape_ab.log); a gap after every load, or s_nop 3, measured
// the same, s_nop 7 less.
__device__ __forceinline__ void issue_gap() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 0");
    __builtin_amdgcn_sched_barrier(0);
}

// The tile grid sits on kTileBytes boundaries of inoutbuf's ADDRESS, not of
// its start: tile t covers [t * kTileBytes - s, (t + 1) * kTileBytes - s) of the
// vector region, s = io mod kTileBytes, clipped to [0, vbytes).  Operands that
// start off a 16 KiB boundary otherwise put every tile across two 16 KiB
// blocks, every wave's 4 KiB across two 4 KiB blocks (and at 64 B off, every
// 1 KiB access across nine 128 B lines instead of eight): measured at 256 MiB
// (tools/archive/align_sweep.py, profiles/archive/r03/align_sweep.log), both operands 64 B /
// 4 KiB / 8 KiB off a 2 MiB boundary took 125.0 / 124.0 / 128.5 us against
// 120.8 us aligned.  Tile 0 is then the partial block up to the first
// boundary: its lanes below the cut get offsets that wrap past the buffer
// descriptor's range (loads return 0, stores are dropped), like the lanes past
// the end of the last tile.  `in` shares io's offset mod 16 (tile_split), not
// necessarily mod 16 KiB.
__device__ __forceinline__ uint32_t tile_shift(const void *io) {
    return (uint32_t)(reinterpret_cast<uintptr_t>(io) & (kTileBytes - 1));
}

// workgroups of the tile grid over a vector region of vbytes at io
__host__ __device__ inline uint64_t tile_groups(const void *io, uint64_t vbytes) {
    const uint64_t s = reinterpret_cast<uintptr_t>(io) & (kTileBytes - 1);
    const uint64_t g = (vbytes + s + kTileBytes - 1) / kTileBytes;
    return g ? g : 1;
}

// Tile `tile` of the grid: each wave owns a contiguous 4 KiB of it (one 1 KiB
// lane-contiguous access per instruction).
template <class Op, class T>
__device__ __forceinline__ void reduce_tile(const char *in, char *io, uint64_t tile, uint64_t vbytes, uint64_t keepb) {
    const int64_t start = (int64_t)(tile * kTileBytes) - (int64_t)tile_shift(io);
    const uint64_t lo = start > 0 ? (uint64_t)start : 0;
    if (lo >= vbytes) return;
    const uint64_t end = (uint64_t)(start + kTileBytes);
    const int nrec = (int)((end < vbytes ? end : vbytes) - lo);
    const int cut = (int)(lo - start);       // 0, or s for tile 0: lanes below it wrap out of range
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *)(in + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(io + lo), 0, nrec, 0x00020000);
    const int t = (int)threadIdx.x;
    const int wb = (t >> 6) * (kVecPerLane * 1024) + (t & 63) * 16 - cut;
    u32x4 a[kVecPerLane], b[kVecPerLane];
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) {
        a[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, wb + u * 1024, 0, kCachePolicyNT);
        b[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, wb + u * 1024, 0, kCachePolicyNT);
        if (u + 1 < kVecPerLane) issue_gap();
    }
    const bool keep = keep_tile(lo, vbytes, keepb);
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) store16(combine16<Op, T>(a[u], b[u]), rio, wb + u * 1024, keep);
}

// With head / tail elements (nhead or ntail != 0), workgroup 0 combines them
// after its tile.
template <class Op, class T>
__device__ __forceinline__ void reduce_tile_body(const TileArgs<T> &args) {
    reduce_tile<Op, T>(args.in, args.io, blockIdx.x, args.vbytes, args.keep);
    if (blockIdx.x == 0) {
        Op op;
        const unsigned t = threadIdx.x;
        if (t < args.nhead) args.head_io[t] = op(args.head_io[t], args.head_in[t]);
        else if (t >= 64 && t - 64 < args.ntail) args.tail_io[t - 64] = op(args.tail_io[t - 64], args.tail_in[t - 64]);
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_tile(TileArgs<T> args) {
    reduce_tile_body<Op, T>(args);
}

// No head / tail (the common case: 16 B-aligned buffers, bytes a multiple of
// 16): four scalar arguments and nothing after the tile.
template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_tile_lean(const char *in, char *io, uint64_t vbytes, uint64_t keep) {
    reduce_tile<Op, T>(in, io, blockIdx.x, vbytes, keep);
}

// inbuf misaligned relative to inoutbuf: (in - io) mod 16 = delta != 0, the
// case of a schedule step whose tmp_buf and recvbuf sub-ranges start at
// different offsets mod 16.  inoutbuf is peeled to 16 B alignment as in
// k_reduce_tile and streamed the same way; inbuf is read as ALIGNED 16-byte
// vectors (lane k loads vector k of the tile, starting delta bytes before the
// operand) and each lane rebuilds its 16 operand bytes from its own vector and
// its neighbour's: a wavefront shuffle (ds_bpermute) hands lane k the vector
// of lane k+1, lane 63 of each wave loads that one itself, and
// v_alignbyte funnels the two at byte offset delta.  The in-buffer descriptor
// ends at the last 16 B vector holding operand bytes; loads past it read 0.
template <int D>
__device__ __forceinline__ u32x4 funnel_d(const uint32_t (&w)[8], uint32_t sh) {
    u32x4 r;
    r.x = __builtin_amdgcn_alignbyte(w[D + 1], w[D + 0], sh);
    r.y = __builtin_amdgcn_alignbyte(w[D + 2], w[D + 1], sh);
    r.z = __builtin_amdgcn_alignbyte(w[D + 3], w[D + 2], sh);
    r.w = __builtin_amdgcn_alignbyte(w[D + 4], w[D + 3], sh);
    return r;
}

// bytes [delta, delta + 16) of the 32-byte concatenation lo:hi (delta uniform)
__device__ __forceinline__ u32x4 funnel16(u32x4 lo, u32x4 hi, uint32_t delta) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t sh = delta & 3;
    switch (delta >> 2) {
    case 0: return funnel_d<0>(w, sh);
    case 1: return funnel_d<1>(w, sh);
    case 2: return funnel_d<2>(w, sh);
    default: return funnel_d<3>(w, sh);
    }
}

template <class T>
struct ShiftArgs {
    TileArgs<T> t;      // t.in is unused: the in region is in_al + delta
    const char *in_al;  // in region start rounded down to 16 B
    uint32_t delta;     // 1..15
};

template <class Op, class T>
__device__ __forceinline__ void reduce_shift_body(const ShiftArgs<T> &args) {
    const TileArgs<T> &ta = args.t;
    const uint64_t base = (uint64_t)blockIdx.x * kTileBytes;
    if (base < ta.vbytes) {
        const uint64_t left = ta.vbytes - base;
        const int nrec = (int)(left < kTileBytes ? left : kTileBytes);
        // operand bytes from in_al + base on, rounded up to whole 16 B vectors: the
        // range check of a dwordx4 load is per access, so the vector holding the
        // operand's last bytes must be fully in range (an aligned 16 B block never
        // crosses a page, so its bytes past the operand are mapped; they are unused)
        const uint64_t in_left = (args.delta + left + 15) & ~(uint64_t)15;
        const int nrec_in = (int)(in_left < kTileBytes + 16 ? in_left : kTileBytes + 16);
        __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *)(args.in_al + base), 0, nrec_in, 0x00020000);
        __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(ta.io + base), 0, nrec, 0x00020000);
        const bool last_lane = (threadIdx.x & 63) == 63;
        // wave-contiguous 4 KiB per wave, as in the aligned tile kernel
        const int wb = ((int)threadIdx.x >> 6) * (kVecPerLane * 1024) + ((int)threadIdx.x & 63) * 16;
        u32x4 a[kVecPerLane], b[kVecPerLane], n63[kVecPerLane];
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int off = wb + u * 1024;
            a[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, off, 0, kCachePolicyNT);
            b[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, off, 0, kCachePolicyNT);
            // lane 63's neighbour vector: every lane issues the load, the others
            // at an offset past the descriptor's range (returns 0, no memory
            // request) -- a branch here would make the compiler drain vmcnt
            n63[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, last_lane ? off + 16 : 0x40000000, 0, kCachePolicyNT);
            if (u + 1 < kVecPerLane) issue_gap();
        }
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int off = wb + u * 1024;
            // neighbour from the shuffle, OR the lane-63 load (0 on every other
            // lane): branch-free, so the load cannot be sunk into a branch
            const uint32_t keep = last_lane ? 0u : ~0u;
            u32x4 nb;
            nb.x = (__shfl_down(b[u].x, 1, 64) & keep) | n63[u].x;
            nb.y = (__shfl_down(b[u].y, 1, 64) & keep) | n63[u].y;
            nb.z = (__shfl_down(b[u].z, 1, 64) & keep) | n63[u].z;
            nb.w = (__shfl_down(b[u].w, 1, 64) & keep) | n63[u].w;
            store16(combine16<Op, T>(a[u], funnel16(b[u], nb, args.delta)), rio, off, keep_tile(base, ta.vbytes, ta.keep));
        }
    }
    if (blockIdx.x == 0) {
        Op op;
        const unsigned t = threadIdx.x;
        if (t < ta.nhead) {
            T x = ta.head_io[t], y;
            __builtin_memcpy(&y, reinterpret_cast<const char *>(ta.head_in) + t * sizeof(T), sizeof(T));
            ta.head_io[t] = op(x, y);
        } else if (t >= 64 && t - 64 < ta.ntail) {
            T x = ta.tail_io[t - 64], y;
            __builtin_memcpy(&y, reinterpret_cast<const char *>(ta.tail_in) + (t - 64) * sizeof(T), sizeof(T));
            ta.tail_io[t - 64] = op(x, y);
        }
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_shift(ShiftArgs<T> args) {
    reduce_shift_body<Op, T>(args);
}

// General path: inbuf and inoutbuf differ in alignment mod 16 (sub-range
// displacements of arbitrary element counts), or elements are not even
// naturally aligned.  Element-granular, coalesced, grid-stride; the stride
// (grid x kThreads) is an argument, not gridDim, so the direct AQL dispatch
// can launch it without hidden arguments.
template <class Op, class T, bool NATURAL>
__device__ __forceinline__ void reduce_elems(const char *in, char *io, uint64_t n, uint64_t stride) {
    Op op;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        if constexpr (NATURAL) {
            const T *pi = reinterpret_cast<const T *>(in) + i;
            T *po = reinterpret_cast<T *>(io) + i;
            *po = op(*po, *pi);
        } else {
            T x, y;
            __builtin_memcpy(&x, io + i * sizeof(T), sizeof(T));
            __builtin_memcpy(&y, in + i * sizeof(T), sizeof(T));
            x = op(x, y);
            __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
        }
    }
}

template <class Op, class T, bool NATURAL>
__global__ __launch_bounds__(kThreads) void k_reduce_elems(const char *in, char *io, uint64_t n, uint64_t stride) {
    reduce_elems<Op, T, NATURAL>(in, io, n, stride);
}

// The tile kernels' split of [in, io) x count into head elements (to 16 B-align
// inoutbuf) / a 16 B vector body / tail elements.  False when the two pointers
// do not share their alignment mod 16 (or are not naturally aligned).
template <class T>
bool tile_split(const void *in_, void *io_, uint64_t count, TileArgs<T> &a) {
    const char *in = static_cast<const char *>(in_);
    char *io = static_cast<char *>(io_);
    const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(io);
    const uint64_t nbytes = count * sizeof(T);
    const bool natural = (ai % alignof(T) == 0) && (ao % alignof(T) == 0);
    const uint64_t head0 = (16 - (ao & 15)) & 15;
    if (!(natural && ((ai ^ ao) & 15) == 0 && head0 % sizeof(T) == 0)) return false;
    const uint64_t head_bytes = head0 < nbytes ? head0 : nbytes;
    const uint64_t rest = nbytes - head_bytes;
    const uint64_t vbytes = rest & ~(uint64_t)15;
    a.in = in + head_bytes;
    a.io = io + head_bytes;
    a.vbytes = vbytes;
    a.head_in = reinterpret_cast<const T *>(in);
    a.head_io = reinterpret_cast<T *>(io);
    a.nhead = (uint32_t)(head_bytes / sizeof(T));
    a.tail_in = reinterpret_cast<const T *>(in + head_bytes + vbytes);
    a.tail_io = reinterpret_cast<T *>(io + head_bytes + vbytes);
    a.ntail = (uint32_t)((rest - vbytes) / sizeof(T));
    a.keep = keep_for(vbytes);
    return true;
}

// The launch plan of one single-operand reduction: which kernel, its grid and
// its argument bytes.  launch_reduce launches it through HIP; the direct AQL
// dispatch (direct_dispatch.hip) launches the same kernel body from its code
// object -- so both paths treat every call identically.
enum : int {
    kPlanLean = 0,      // k_reduce_tile_lean: 16 B-aligned, 16 B multiple (LeanArgs)
    kPlanFull = 1,      // k_reduce_tile: equal alignment mod 16, head / tail elements (TileArgs)
    kPlanShift = 2,     // k_reduce_shift: unequal alignment, >= 2 tiles (ShiftArgs)
    kPlanElems = 3,     // k_reduce_elems<NATURAL = true> (ElemsArgs)
    kPlanElemsU = 4,    // k_reduce_elems<NATURAL = false> (ElemsArgs)
    kPlanKinds = 5,
    // the 32-byte classes' launcher (launch_reduce_wide; HIP launch only, no direct dispatch)
    kPlanWideTile = kPlanKinds,         // k_reduce_tile_wide: both pointers 16 B-aligned (LeanArgs, vbytes = all bytes)
    kPlanWideElems = kPlanKinds + 1     // k_reduce_elems<NATURAL = false> (ElemsArgs)
};
struct LeanArgs { const char *in; char *io; uint64_t vbytes; uint64_t keep; };
struct ElemsArgs { const char *in; char *io; uint64_t n; uint64_t stride; };
struct ReducePlan {
    int kind;
    uint32_t arg_bytes;
    uint64_t groups;    // workgroups of kThreads
    alignas(16) unsigned char args[sizeof(ShiftArgs<char>)];
};

// The direct AQL dispatch's kernarg slot (direct_dispatch.hip writes it,
// direct_tiles.hip's kernels read it): one 128-byte L2 line, two 64-byte halves.
//   words 0-5, 8-13   the plan's argument bytes (at most kSlotArgBytes)
//   word 6            address of the device's error word (host memory)
//   words 7, 15       the nonce, one copy per half: the queue index + 1 of the
//                     last packet that stamped the slot (its dispatch id + 1)
struct KargSlot { uint64_t w[16]; };
constexpr uint32_t kSlotArgBytes = 96;
static_assert(sizeof(ShiftArgs<char>) <= kSlotArgBytes, "ShiftArgs must fit the kernarg slot");

// Fills `p` (padding bytes zero: the direct path's kernarg cache compares bytes).
template <class T>
void plan_reduce(const void *in_, void *io_, uint64_t count, ReducePlan &p) {
    __builtin_memset(&p, 0, sizeof p);
    const char *in = static_cast<const char *>(in_);
    char *io = static_cast<char *>(io_);
    const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(io);
    const uint64_t nbytes = count * sizeof(T);
    const bool natural = (ai % alignof(T) == 0) && (ao % alignof(T) == 0);
    const uint64_t head0 = (16 - (ao & 15)) & 15;
    TileArgs<T> ta;
    __builtin_memset(&ta, 0, sizeof ta);
    if (tile_split<T>(in_, io_, count, ta)) {
        p.groups = tile_groups(ta.io, ta.vbytes);
        if (ta.nhead || ta.ntail) {
            p.kind = kPlanFull;
            __builtin_memcpy(p.args, &ta, sizeof ta);
            p.arg_bytes = sizeof ta;
        } else {
            const LeanArgs la{ta.in, ta.io, ta.vbytes, ta.keep};
            p.kind = kPlanLean;
            __builtin_memcpy(p.args, &la, sizeof la);
            p.arg_bytes = sizeof la;
        }
    } else if ((ao % alignof(T) == 0) && head0 % sizeof(T) == 0 && nbytes >= 2 * kTileBytes) {
        // inoutbuf element-aligned, inbuf at any other offset mod 16: the
        // aligned-load + shuffle + funnel tile kernel (small counts stay
        // on the element kernel, where a launch's setup dominates anyway)
        const uint64_t head_bytes = head0;
        const uint64_t rest = nbytes - head_bytes;
        const uint64_t vbytes = rest & ~(uint64_t)15;
        ShiftArgs<T> a;
        __builtin_memset(&a, 0, sizeof a);
        a.t.in = nullptr;
        a.t.io = io + head_bytes;
        a.t.vbytes = vbytes;
        a.t.head_in = reinterpret_cast<const T *>(in);
        a.t.head_io = reinterpret_cast<T *>(io);
        a.t.nhead = (uint32_t)(head_bytes / sizeof(T));
        a.t.tail_in = reinterpret_cast<const T *>(in + head_bytes + vbytes);
        a.t.tail_io = reinterpret_cast<T *>(io + head_bytes + vbytes);
        a.t.ntail = (uint32_t)((rest - vbytes) / sizeof(T));
        a.t.keep = keep_for(vbytes);
        const uintptr_t vin = ai + head_bytes;
        a.delta = (uint32_t)(vin & 15);
        a.in_al = reinterpret_cast<const char *>(vin - a.delta);
        p.kind = kPlanShift;
        p.groups = (vbytes + kTileBytes - 1) / kTileBytes;
        __builtin_memcpy(p.args, &a, sizeof a);
        p.arg_bytes = sizeof a;
    } else {
        uint64_t grid = (count + kThreads - 1) / kThreads;
        if (grid > 4096) grid = 4096;
        if (grid == 0) grid = 1;
        const ElemsArgs ea{in, io, count, grid * kThreads};
        p.kind = natural ? kPlanElems : kPlanElemsU;
        p.groups = grid;
        __builtin_memcpy(p.args, &ea, sizeof ea);
        p.arg_bytes = sizeof ea;
    }
}

// the same, type-erased (Entry::plan, kernel_table.hpp)
template <class T>
void plan_reduce_any(const void *in, void *io, uint64_t count, ReducePlan *p) {
    plan_reduce<T>(in, io, count, *p);
}

// Host-side launcher: the plan's kernel through HIP.  Returns the launch error.
template <class Op, class T>
hipError_t launch_reduce(const void *in, void *io, uint64_t count, hipStream_t s) {
    ReducePlan p;
    plan_reduce<T>(in, io, count, p);
    const dim3 grid((unsigned)p.groups), block(kThreads);
    switch (p.kind) {
    case kPlanLean: {
        LeanArgs a;
        __builtin_memcpy(&a, p.args, sizeof a);
        hipLaunchKernelGGL((k_reduce_tile_lean<Op, T>), grid, block, 0, s, a.in, a.io, a.vbytes, a.keep);
        break;
    }
    case kPlanFull: {
        TileArgs<T> a;
        __builtin_memcpy(&a, p.args, sizeof a);
        hipLaunchKernelGGL((k_reduce_tile<Op, T>), grid, block, 0, s, a);
        break;
    }
    case kPlanShift: {
        ShiftArgs<T> a;
        __builtin_memcpy(&a, p.args, sizeof a);
        hipLaunchKernelGGL((k_reduce_shift<Op, T>), grid, block, 0, s, a);
        break;
    }
    default: {
        ElemsArgs a;
        __builtin_memcpy(&a, p.args, sizeof a);
        if (p.kind == kPlanElems)
            hipLaunchKernelGGL((k_reduce_elems<Op, T, true>), grid, block, 0, s, a.in, a.io, a.n, a.stride);
        else
            hipLaunchKernelGGL((k_reduce_elems<Op, T, false>), grid, block, 0, s, a.in, a.io, a.n, a.stride);
        break;
    }
    }
    return hipGetLastError();
}

// Elements wider than 16 bytes (long double _Complex, MPI_LONG_DOUBLE_INT:
// 32 B): the LDS transpose.  The tile is loaded and stored lane-contiguous
// (fully coalesced buffer_load/store_dwordx4 nt, like k_reduce_tile), staged
// through LDS, and each lane combines whole elements out of LDS -- the soft
// x87 combine needs an element's two 16-byte halves in one lane.  Measured at
// 256 MiB (profiles/archive/r01_kernel_ab_wide_lds.log): SUM 0.78, MAXLOC 0.81 of the
// HBM peak vs 0.65 when each lane loads its own halves (lanes 32 B apart, every
// 128-byte line fetched twice under `nt`).  The buffer range check handles
// the ragged last tile (zeros in, stores dropped).
template <class Op, class T, int EPL>
__global__ __launch_bounds__(kThreads) void k_reduce_tile_wide(const char *in, char *io, uint64_t nbytes, uint64_t keep) {
    static_assert(sizeof(T) == 32, "two 16-byte halves per element");
    constexpr int NV = 2 * EPL;                       // 16-byte vectors per lane per operand
    constexpr uint32_t tile = kThreads * NV * 16;
    __shared__ u32x4 sa[kThreads * NV], sb[kThreads * NV];
    const uint64_t base = (uint64_t)blockIdx.x * tile;
    if (base >= nbytes) return;
    const uint64_t left = nbytes - base;
    const int nrec = (int)(left < tile ? left : tile);
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *)(in + base), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(io + base), 0, nrec, 0x00020000);
    const int t = (int)threadIdx.x;
    // each wave owns a contiguous NV KiB of the tile; LDS slot = byte offset / 16,
    // so element e still sits in slots 2e, 2e+1 whichever lane loaded it
    const int wv = (t >> 6) * NV * 64 + (t & 63);    // 16-byte vector index of v = 0
    u32x4 a[NV], b[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        a[v] = __builtin_amdgcn_raw_buffer_load_b128(rio, (wv + v * 64) * 16, 0, kCachePolicyNT);
        b[v] = __builtin_amdgcn_raw_buffer_load_b128(rin, (wv + v * 64) * 16, 0, kCachePolicyNT);
        if (v + 1 < NV) issue_gap();
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        sa[wv + v * 64] = a[v];
        sb[wv + v * 64] = b[v];
    }
    __syncthreads();
    Op op;
    struct V { u32x4 h[2]; };
#pragma unroll
    for (int u = 0; u < EPL; ++u) {
        const int e = u * kThreads + t;
        const T x = __builtin_bit_cast(T, V{{sa[2 * e], sa[2 * e + 1]}});
        const T y = __builtin_bit_cast(T, V{{sb[2 * e], sb[2 * e + 1]}});
        const V r = __builtin_bit_cast(V, op(x, y));
        sa[2 * e] = r.h[0];
        sa[2 * e + 1] = r.h[1];
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v)
        store16(sa[wv + v * 64], rio, (wv + v * 64) * 16, keep_tile(base, nbytes, keep));
}

// EPL: elements per lane (2 for the memory-bound ops; the compute-bound soft
// x87 complex PROD does better with 1, more waves per element).
// Pointers not 16 B-aligned take the element-granular kernel.
// The 32-byte classes' plan: the LDS-transpose tile kernel when both pointers
// are 16 B-aligned, else the element kernel.  launch_reduce_wide launches it;
// MPIR_Hip_plan_info reports it (Entry::wide, kernel_table.hpp).
template <class T, int EPL>
void plan_reduce_wide(const void *in_, void *io_, uint64_t count, ReducePlan *p) {
    static_assert(sizeof(T) > 16, "16-byte and smaller elements use plan_reduce");
    __builtin_memset(p, 0, sizeof *p);
    const char *in = static_cast<const char *>(in_);
    char *io = static_cast<char *>(io_);
    const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(io);
    if (ai % 16 == 0 && ao % 16 == 0) {
        constexpr uint32_t tile = kThreads * EPL * 32;
        const uint64_t nbytes = count * sizeof(T);
        uint64_t grid = (nbytes + tile - 1) / tile;
        if (grid == 0) grid = 1;
        const LeanArgs la{in, io, nbytes, keep_for(nbytes)};
        p->kind = kPlanWideTile;
        p->groups = grid;
        __builtin_memcpy(p->args, &la, sizeof la);
        p->arg_bytes = sizeof la;
        return;
    }
    uint64_t grid = (count + kThreads - 1) / kThreads;
    if (grid > 4096) grid = 4096;
    if (grid == 0) grid = 1;
    const ElemsArgs ea{in, io, count, grid * kThreads};
    p->kind = kPlanWideElems;
    p->groups = grid;
    __builtin_memcpy(p->args, &ea, sizeof ea);
    p->arg_bytes = sizeof ea;
}

template <class Op, class T, int EPL = 2>
hipError_t launch_reduce_wide(const void *in_, void *io_, uint64_t count, hipStream_t s) {
    ReducePlan p;
    plan_reduce_wide<T, EPL>(in_, io_, count, &p);
    if (p.kind == kPlanWideTile) {
        LeanArgs a;
        __builtin_memcpy(&a, p.args, sizeof a);
        hipLaunchKernelGGL((k_reduce_tile_wide<Op, T, EPL>), dim3((unsigned)p.groups), dim3(kThreads), 0, s, a.in, a.io,
                           a.vbytes, a.keep);
        return hipGetLastError();
    }
    ElemsArgs a;
    __builtin_memcpy(&a, p.args, sizeof a);
    hipLaunchKernelGGL((k_reduce_elems<Op, T, false>), dim3((unsigned)p.groups), dim3(kThreads), 0, s, a.in, a.io, a.n,
                       a.stride);
    return hipGetLastError();
}

// ============================================================================
// Batched reductions (MPIR_Hip_reduce_batch): many independent (in, io, count)
// segments under one (op, type) in ONE launch, each segment's result what the
// single call gives.  A synchronous small call costs what the command
// processor takes to start and retire a dispatch, whatever its size; a caller
// with many small combines to make pays that once here.
//
//   * The segment table travels by value in the kernel arguments (as AnyArgs'
//     64 pointers do): no device table, copy or scratch, so an enqueued batch
//     is self-contained.  kBatchMaxSegs descriptors fit HIP's 4 KiB of kernel
//     arguments; a larger batch is several back-to-back launches.
//   * The grid is the sum of the segments' workgroup counts.  A workgroup finds
//     its segment by a binary search of the descriptors' first workgroups --
//     uniform across the workgroup, so scalar loads from the kernarg segment --
//     and takes tile blockIdx.x - first of it.
//   * A segment whose pointers are naturally aligned and share their offset
//     mod 16 (seg_split) runs reduce_tile on the 16 KiB grid of inoutbuf's
//     address, exactly as k_reduce_tile does, its tile 0 also the head and tail
//     elements; stores are nt (keep = 0: batched segments are small, and the
//     single call stores results of at most 16 MiB nt too).  Every other
//     segment, and every segment of the 32-byte classes, runs the element form:
//     workgroup g of it owns elements [g, g + 1) x kTileBytes / sizeof(T).
//   * seg_split / batch_seg_groups are the one source of a segment's split and
//     workgroup count: the host's planner sums the count into the descriptors'
//     first workgroups and the kernel bounds its tile index by it.
// ============================================================================
// The split of one segment, on the pointer values alone: tile_split's
// condition and arithmetic (head elements to 16 B-align inoutbuf / a 16 B
// vector body / tail elements), restated as a __host__ __device__ function so
// that the batch's planner and its kernel, which splits each of its segments on
// the device, take it from one place.  tests/test_batch_cpu.py holds it to
// tile_split: a tile-path segment's workgroups are MPIR_Hip_plan_info's.
struct SegSplit {
    bool tile;              // the tile kernels apply (false: the counts below are 0)
    uint64_t head_bytes;    // bytes before the vector region (at most the payload)
    uint64_t vbytes;        // multiple of 16
    uint32_t nhead, ntail;  // elements
};
template <class T>
__host__ __device__ inline SegSplit seg_split(const void *in, const void *io, uint64_t count) {
    SegSplit s = {false, 0, 0, 0, 0};
    if constexpr (sizeof(T) <= 16) {
        const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(io);
        const uint64_t nbytes = count * sizeof(T);
        const bool natural = (ai % alignof(T) == 0) && (ao % alignof(T) == 0);
        const uint64_t head0 = (16 - (ao & 15)) & 15;
        if (!(natural && ((ai ^ ao) & 15) == 0 && head0 % sizeof(T) == 0)) return s;
        const uint64_t head_bytes = head0 < nbytes ? head0 : nbytes;
        const uint64_t rest = nbytes - head_bytes;
        s.tile = true;
        s.head_bytes = head_bytes;
        s.vbytes = rest & ~(uint64_t)15;
        s.nhead = (uint32_t)(head_bytes / sizeof(T));
        s.ntail = (uint32_t)((rest - s.vbytes) / sizeof(T));
    }
    return s;
}

// element i of a segment: io[i] = op(io[i], in[i]), the element form of
// reduce_elems<..., false> (any alignment)
template <class Op, class T>
__device__ __forceinline__ void batch_elem_at(const char *in, char *io, uint64_t i) {
    Op op;
    T x, y;
    __builtin_memcpy(&x, io + i * sizeof(T), sizeof(T));
    __builtin_memcpy(&y, in + i * sizeof(T), sizeof(T));
    x = op(x, y);
    __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
}

constexpr int kBatchMaxSegs = 127;
// a launch closes before its workgroups pass this: 2^23 x 256 threads keeps the
// grid's work-item count inside the 32 bits an AQL packet holds
constexpr uint64_t kBatchMaxGroups = MPIR_HIP_BATCH_MAX_GROUPS;

struct BatchSeg {
    const char *in;
    char *io;
    uint64_t count;     // elements, > 0
    uint64_t first;     // the segment's first workgroup in this launch's grid
};
struct BatchArgs {
    uint32_t nsegs;     // descriptors in use, >= 1; seg[0].first == 0, first strictly increasing
    uint32_t pad_;
    BatchSeg seg[kBatchMaxSegs];
};
static_assert(sizeof(BatchArgs) <= 4096, "the segment table must fit HIP's 4 KiB of kernel arguments");
static_assert(kBatchMaxGroups * kThreads < (1ull << 32), "the grid's work-items must fit an AQL packet's 32 bits");

// workgroups of one segment (count > 0), given its split
template <class T>
__host__ __device__ inline uint64_t batch_seg_groups(const SegSplit &s, const void *io, uint64_t count) {
    if (s.tile) return tile_groups(static_cast<const char *>(io) + s.head_bytes, s.vbytes);
    constexpr uint64_t per = kTileBytes / sizeof(T);
    return (count + per - 1) / per;
}

// the same, type-erased (BatchEntry::groups, kernel_table.hpp); *tile: the path
template <class T>
uint64_t batch_groups_any(const void *in, const void *io, uint64_t count, int *tile) {
    const SegSplit s = seg_split<T>(in, io, count);
    *tile = s.tile;
    return batch_seg_groups<T>(s, io, count);
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_batch(BatchArgs a) {
    const uint32_t wg = blockIdx.x;
    uint32_t lo = 0, hi = a.nsegs;          // seg[lo].first <= wg < seg[hi].first (hi == nsegs: the grid's end)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.seg[mid].first <= wg) lo = mid;
        else hi = mid;
    }
    const char *in = a.seg[lo].in;
    char *io = a.seg[lo].io;
    const uint64_t count = a.seg[lo].count;
    const uint64_t tile = wg - a.seg[lo].first;
    const SegSplit s = seg_split<T>(in, io, count);
    if (tile >= batch_seg_groups<T>(s, io, count)) return;
    if constexpr (sizeof(T) <= 16) {
        if (s.tile) {
            reduce_tile<Op, T>(in + s.head_bytes, io + s.head_bytes, tile, s.vbytes, 0);
            if (tile == 0) {
                Op op;
                const unsigned t = threadIdx.x;
                if (t < s.nhead) {
                    T *p = reinterpret_cast<T *>(io) + t;
                    *p = op(*p, reinterpret_cast<const T *>(in)[t]);
                } else if (t >= 64 && t - 64 < s.ntail) {
                    T *p = reinterpret_cast<T *>(io + s.head_bytes + s.vbytes) + (t - 64);
                    *p = op(*p, reinterpret_cast<const T *>(in + s.head_bytes + s.vbytes)[t - 64]);
                }
            }
            return;
        }
    }
    constexpr uint64_t per = kTileBytes / sizeof(T);
    const uint64_t base = tile * per;
    const uint64_t end = base + per < count ? base + per : count;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads) batch_elem_at<Op, T>(in, io, i);
}

template <class Op, class T>
hipError_t launch_batch(const BatchArgs *a, uint64_t groups, hipStream_t s) {
    if (a->nsegs < 1 || a->nsegs > (uint32_t)kBatchMaxSegs || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_batch<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Strided reductions (MPIR_Hip_reduce_strided): nrows equal rows of blocklen
// elements, row r at in + r * in_stride and io + r * io_stride (bytes), each
// row's result what the single call gives on it.  An MPI_Type_vector operand
// -- a sub-matrix, a halo face, a column -- needs no segment table: five numbers
// describe it and the workgroup-to-row mapping is arithmetic, so any number of
// rows is one launch (up to kBatchMaxGroups workgroups), with 56 bytes of kernel
// arguments.  Two forms, chosen on the host by the row's bytes:
//
//   * WIDE (row bytes >= the threshold): the grid is nrows x G, G = the most
//     workgroups any row can need (strided_row_groups_max).  Workgroup wg takes
//     row wg / G, tile wg % G, computes that row's pointers and runs the batch's
//     segment code on them (reduce_seg: seg_split on the device, the 16 KiB tile
//     grid of the row's own inoutbuf address or the element form).  Rows may
//     differ in path when the strides differ mod 16; a row that needs fewer than
//     G workgroups leaves the rest idle, at most one, and none when inoutbuf's
//     base and stride are multiples of 16 KiB.  The row's pointers come from
//     blockIdx and the kernel arguments alone, so the tile's buffer descriptors
//     stay in scalar registers.
//   * NARROW: the rows flattened into units, workgroup g owning units
//     [g, g + 1) x 16 KiB / unit bytes wherever they fall -- its span may begin
//     and end in the middle of a row.  A unit is one 16-byte vector (nt loads
//     and store, combine16) when the row bytes, both strides and both bases are
//     multiples of 16 and the element is at most 16 bytes, else one element in
//     batch_elem_at's form (any alignment).  The workgroup divides its first
//     unit by the units per row once, in 64 bits; a lane's unit is at most
//     16383 further on, so its row and column are one 32-bit division.  (Each
//     lane addresses another row: per-lane global addresses, no descriptor.)
//
// No LDS, no scratch, no gridDim: everything comes from the arguments.
// ============================================================================
struct StridedArgs {
    const char *in;         // row 0 of this launch
    char *io;
    uint64_t in_stride;     // bytes between rows (0: one input row for every output row)
    uint64_t io_stride;     // bytes, >= the row's bytes
    uint64_t blocklen;      // elements per row, > 0
    uint32_t nrows;         // rows of this launch, > 0
    uint32_t form;          // MPIR_HIP_STRIDED_WIDE / _NARROW_VEC / _NARROW_ELEMS
    uint32_t per;           // WIDE: G, workgroups per row; NARROW: units per row
    uint32_t pad_;
};

// G of the wide form: the most workgroups batch_seg_groups can give a row of
// row_bytes, whatever its pointers.  The tile path's count is largest with no
// head (vbytes = row_bytes rounded down to 16) and the vector region 16 B short
// of a grid boundary; the element path's is row_bytes / 16 KiB rounded up, never
// more.  With inoutbuf's base and stride both on the 16 KiB grid every row starts
// a tile, and the element path's count bounds both.
inline uint64_t strided_row_groups_max(uint64_t row_bytes, size_t esz, const void *io, uint64_t io_stride) {
    const uint64_t elems = (row_bytes + kTileBytes - 1) / kTileBytes;
    const bool on_grid = ((reinterpret_cast<uintptr_t>(io) | io_stride) & (kTileBytes - 1)) == 0;
    if (esz > 16 || on_grid) return elems ? elems : 1;
    const uint64_t tiles = ((row_bytes & ~(uint64_t)15) + 2 * (uint64_t)kTileBytes - 17) / kTileBytes;
    return tiles > elems ? tiles : elems;
}

// Workgroup `tile` of the segment (in, io, count), all three uniform across the
// workgroup: its 16 KiB tile of the grid over inoutbuf's address (tile 0 also the
// head and tail elements), or its run of the element form.  A tile at or past
// the segment's own workgroup count does nothing.  What k_reduce_batch does for
// a segment once it has found it, for the strided kernel's wide rows: the split
// and the workgroup count come from the same seg_split / batch_seg_groups.
template <class Op, class T>
__device__ __forceinline__ void reduce_seg(const char *in, char *io, uint64_t count, uint64_t tile) {
    const SegSplit s = seg_split<T>(in, io, count);
    if (tile >= batch_seg_groups<T>(s, io, count)) return;
    if constexpr (sizeof(T) <= 16) {
        if (s.tile) {
            reduce_tile<Op, T>(in + s.head_bytes, io + s.head_bytes, tile, s.vbytes, 0);
            if (tile == 0) {
                Op op;
                const unsigned t = threadIdx.x;
                if (t < s.nhead) {
                    T *p = reinterpret_cast<T *>(io) + t;
                    *p = op(*p, reinterpret_cast<const T *>(in)[t]);
                } else if (t >= 64 && t - 64 < s.ntail) {
                    T *p = reinterpret_cast<T *>(io + s.head_bytes + s.vbytes) + (t - 64);
                    *p = op(*p, reinterpret_cast<const T *>(in + s.head_bytes + s.vbytes)[t - 64]);
                }
            }
            return;
        }
    }
    constexpr uint64_t per = kTileBytes / sizeof(T);
    const uint64_t base = tile * per;
    const uint64_t end = base + per < count ? base + per : count;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads) batch_elem_at<Op, T>(in, io, i);
}

// units of the narrow forms: bytes of one, and how many a workgroup owns
template <class T>
constexpr uint32_t strided_units_per_group(bool vec) { return kTileBytes / (vec ? 16 : (uint32_t)sizeof(T)); }

template <class Op, class T>
__device__ __forceinline__ void reduce_strided_narrow(const StridedArgs &a) {
    const uint32_t upr = a.per;                             // units per row
    const unsigned t = threadIdx.x;
    if constexpr (sizeof(T) <= 16) {
        if (a.form == MPIR_HIP_STRIDED_NARROW_VEC) {
            constexpr uint32_t upw = strided_units_per_group<T>(true);
            constexpr int per_lane = (int)(upw / kThreads);
            const uint64_t u0 = (uint64_t)blockIdx.x * upw;
            const uint64_t row0 = u0 / upr;
            const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
            u32x4 x[per_lane], y[per_lane];
            u32x4 *po[per_lane];
            bool ok[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                const uint32_t c = col0 + t + (uint32_t)j * kThreads;
                const uint32_t q = c / upr;
                const uint64_t row = row0 + q, off = (uint64_t)(c - q * upr) * 16;
                ok[j] = row < a.nrows;
                po[j] = reinterpret_cast<u32x4 *>(a.io + row * a.io_stride + off);
                if (ok[j]) {
                    x[j] = __builtin_nontemporal_load(po[j]);
                    y[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.in + row * a.in_stride + off));
                }
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j)
                if (ok[j]) __builtin_nontemporal_store(combine16<Op, T>(x[j], y[j]), po[j]);
            return;
        }
    }
    constexpr uint32_t upw = strided_units_per_group<T>(false);
    const uint64_t u0 = (uint64_t)blockIdx.x * upw;
    const uint64_t row0 = u0 / upr;
    const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
    for (uint32_t k = t; k < upw; k += kThreads) {
        const uint32_t c = col0 + k;
        const uint32_t q = c / upr;
        const uint64_t row = row0 + q;
        if (row >= a.nrows) break;                          // rows only grow with k
        batch_elem_at<Op, T>(a.in + row * a.in_stride, a.io + row * a.io_stride, c - q * upr);
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_strided(StridedArgs a) {
    if (a.form == MPIR_HIP_STRIDED_WIDE) {
        const uint32_t row = blockIdx.x / a.per;
        if (row >= a.nrows) return;
        reduce_seg<Op, T>(a.in + row * a.in_stride, a.io + row * a.io_stride, a.blocklen, blockIdx.x - row * a.per);
        return;
    }
    reduce_strided_narrow<Op, T>(a);
}

// one launch: `groups` workgroups over a.nrows rows (the planner's count:
// nrows x G, or the rows' units over the units a workgroup owns, rounded up)
template <class Op, class T>
hipError_t launch_strided(const StridedArgs *a, uint64_t groups, hipStream_t s) {
    if (!a->nrows || !a->per || !a->blocklen || groups < 1 || groups > kBatchMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_strided<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Subarray reductions (MPIR_Hip_reduce_subarray): the rows of a sub-box of an
// N-dimensional array, each row's result what the single call gives on it.  The
// host brings the box to a row of blocklen contiguous elements under up to three
// outer dimensions (more are looped on the host), each with a count and one byte
// stride per side.  It is the strided kernel with the row's address a sum over
// the outer indices where that kernel has one product: rows are numbered with
// outer dimension 1 fastest, row r = i1 + n1 * (i2 + n2 * i3) at
// i1 * stride[0] + i2 * stride[1] + i3 * stride[2] of either side.  112 bytes of
// kernel arguments, no table.  The forms are the strided kernel's:
//
//   * WIDE: the grid is nrows x G; workgroup wg takes row wg / G of the launch,
//     finds its outer indices on uniform values (subarray_step: two 32-bit
//     divisions), forms both row pointers from blockIdx and the arguments alone
//     (the tile's buffer descriptors stay in scalar registers) and runs
//     reduce_seg with tile wg % G.
//   * NARROW: the rows flattened into units as the strided kernel flattens them.
//     The workgroup divides its first unit by the units per row once and finds
//     that row's outer indices, all uniform; a lane's row is at most 16383
//     further on: the strided kernel's one 32-bit division gives its distance,
//     subarray_step from the workgroup's indices its own.
//
// A launch names its first row by that row's outer indices (first[]): later
// launches of a call continue at a later row with the same two pointers, since
// the rows of one launch do not share one stride.  No LDS, no scratch, no gridDim.
// ============================================================================
struct SubarrayArgs {
    const char *in;         // the input box's first element
    char *io;
    uint64_t blocklen;      // elements per row, > 0
    uint64_t in_stride[3];  // bytes per step of outer dimension 1, 2, 3 (a dimension not in use: 0)
    uint64_t io_stride[3];
    uint32_t n[3];          // the outer dimensions' counts, 1 to 2^31 - 1 (not in use: 1)
    uint32_t first[3];      // outer indices of this launch's row 0, first[d] < n[d]
    uint32_t nrows;         // rows of this launch, > 0
    uint32_t form;          // MPIR_HIP_STRIDED_WIDE / _NARROW_VEC / _NARROW_ELEMS
    uint32_t per;           // WIDE: G, workgroups per row; NARROW: units per row
    uint32_t pad_;
};
static_assert(sizeof(SubarrayArgs) == 112, "the subarray kernel's arguments");

// The outer indices i[] of the row q rows after the row at f[] (f[d] < n[d]), in
// 32 bits: a remainder and a start are both below 2^31, and so is each carry's sum.
// The row is one of the box (the caller bounds q by the launch's rows), so i[2]
// needs no reduction.
__device__ __forceinline__ void subarray_step(const SubarrayArgs &a, const uint32_t f[3], uint32_t q, uint32_t i[3]) {
    const uint32_t q1 = q / a.n[0];
    uint32_t i1 = f[0] + (q - q1 * a.n[0]);
    uint32_t carry = i1 >= a.n[0];
    i1 -= carry ? a.n[0] : 0;
    const uint32_t q2 = q1 / a.n[1];
    uint32_t i2 = f[1] + (q1 - q2 * a.n[1]) + carry;
    carry = i2 >= a.n[1];
    i2 -= carry ? a.n[1] : 0;
    i[0] = i1;
    i[1] = i2;
    i[2] = f[2] + q2 + carry;
}

__device__ __forceinline__ uint64_t subarray_off(const uint64_t stride[3], const uint32_t i[3]) {
    return i[0] * stride[0] + i[1] * stride[1] + i[2] * stride[2];
}

template <class Op, class T>
__device__ __forceinline__ void reduce_subarray_narrow(const SubarrayArgs &a) {
    const uint32_t upr = a.per;                             // units per row
    const unsigned t = threadIdx.x;
    uint32_t b[3], i[3];                                    // the workgroup's first row, a lane's row
    if constexpr (sizeof(T) <= 16) {
        if (a.form == MPIR_HIP_STRIDED_NARROW_VEC) {
            constexpr uint32_t upw = strided_units_per_group<T>(true);
            constexpr int per_lane = (int)(upw / kThreads);
            const uint64_t u0 = (uint64_t)blockIdx.x * upw;
            const uint64_t row0 = u0 / upr;
            const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
            subarray_step(a, a.first, (uint32_t)row0, b);
            u32x4 x[per_lane], y[per_lane];
            u32x4 *po[per_lane];
            bool ok[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                const uint32_t c = col0 + t + (uint32_t)j * kThreads;
                const uint32_t q = c / upr;
                const uint64_t off = (uint64_t)(c - q * upr) * 16;
                ok[j] = row0 + q < a.nrows;
                if (ok[j]) {
                    subarray_step(a, b, q, i);
                    po[j] = reinterpret_cast<u32x4 *>(a.io + subarray_off(a.io_stride, i) + off);
                    x[j] = __builtin_nontemporal_load(po[j]);
                    y[j] = __builtin_nontemporal_load(
                        reinterpret_cast<const u32x4 *>(a.in + subarray_off(a.in_stride, i) + off));
                }
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j)
                if (ok[j]) __builtin_nontemporal_store(combine16<Op, T>(x[j], y[j]), po[j]);
            return;
        }
    }
    constexpr uint32_t upw = strided_units_per_group<T>(false);
    const uint64_t u0 = (uint64_t)blockIdx.x * upw;
    const uint64_t row0 = u0 / upr;
    const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
    subarray_step(a, a.first, (uint32_t)row0, b);
    for (uint32_t k = t; k < upw; k += kThreads) {
        const uint32_t c = col0 + k;
        const uint32_t q = c / upr;
        if (row0 + q >= a.nrows) break;                     // rows only grow with k
        subarray_step(a, b, q, i);
        batch_elem_at<Op, T>(a.in + subarray_off(a.in_stride, i), a.io + subarray_off(a.io_stride, i), c - q * upr);
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_subarray(SubarrayArgs a) {
    if (a.form == MPIR_HIP_STRIDED_WIDE) {
        const uint32_t row = blockIdx.x / a.per;
        if (row >= a.nrows) return;
        uint32_t i[3];
        subarray_step(a, a.first, row, i);
        reduce_seg<Op, T>(a.in + subarray_off(a.in_stride, i), a.io + subarray_off(a.io_stride, i), a.blocklen,
                          blockIdx.x - row * a.per);
        return;
    }
    reduce_subarray_narrow<Op, T>(a);
}

// one launch: `groups` workgroups over a.nrows rows from the row at a.first (the
// planner's count, as for launch_strided)
template <class Op, class T>
hipError_t launch_subarray(const SubarrayArgs *a, uint64_t groups, hipStream_t s) {
    if (!a->nrows || !a->per || !a->blocklen || !a->n[0] || !a->n[1] || !a->n[2] || a->first[0] >= a->n[0] ||
        a->first[1] >= a->n[1] || a->first[2] >= a->n[2] || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    // the launch's last row is a row of the box: no index leaves its dimension
    const unsigned __int128 n01 = (unsigned __int128)a->n[0] * a->n[1];
    if (a->first[0] + (unsigned __int128)a->n[0] * a->first[1] + n01 * a->first[2] + a->nrows > n01 * a->n[2])
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_subarray<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Indexed reductions (MPIR_Hip_reduce_indexed): nrows equal blocks of blocklen
// elements, block k at in + in_displs[k] * disp_unit and io + io_displs[k] *
// disp_unit (signed displacements, device tables), a side with no table packed
// (block k at k * the block's bytes).  The target of an accumulate on an
// MPI_Type_create_indexed_block / hindexed_block type -- a scatter-add, or the
// gather the other way round.  It is the strided kernel with a block's byte
// offset read from a table instead of computed as row * stride, so any number
// of blocks is one launch (up to kBatchMaxGroups workgroups) with 64 bytes of
// kernel arguments; the forms are the strided kernel's:
//
//   * WIDE: the grid is nrows x G.  The host cannot read a device table, so G
//     is the most workgroups a block can need at any address
//     (indexed_row_groups_max), never the on-grid count.  Workgroup wg takes
//     block wg / G: it loads that block's displacements from an address formed
//     from the kernel arguments and blockIdx alone, passes their halves through
//     readfirstlane so that the block's pointers are wave-uniform to the
//     compiler too (reduce_tile's buffer descriptors stay in scalar registers,
//     no waterfall loop), and runs reduce_seg with tile wg % G.
//   * NARROW: the blocks flattened into units as the strided kernel flattens
//     rows, one 64-bit division per workgroup and a 32-bit one per lane; a lane
//     then loads its blocks' displacements.  A unit is a 16-byte vector only
//     when the host can prove every address a multiple of 16 without reading
//     the table: block bytes and both bases multiples of 16, and disp_unit a
//     multiple of 16 for each side that has a table; else one element through
//     batch_elem_at.  In the vector form a side's four table loads are one
//     straight run (the null tests are outside the unrolled loops, a unit past
//     the last block is clamped into it instead of branched around), so a lane
//     waits one memory round trip per side with a table before its data loads,
//     which again issue together.  The element form loads a displacement per
//     element and waits for it: one more round trip in each iteration.
//
// No LDS, no scratch, no gridDim.  Tile and vector stores are nt; element
// stores are batch_elem_at's plain stores, as in the batch and the strided call.
// ============================================================================
struct IndexedArgs {
    const char *in;             // the bases; of a packed side, block 0 of this launch
    char *io;
    const int64_t *in_displs;   // entry 0 is this launch's first block; null: packed
    const int64_t *io_displs;
    uint64_t disp_unit;         // bytes per displacement unit, > 0
    uint64_t blocklen;          // elements per block, > 0
    uint32_t nrows;             // blocks of this launch, > 0
    uint32_t form;              // MPIR_HIP_INDEXED_WIDE / _NARROW_VEC / _NARROW_ELEMS
    uint32_t per;               // WIDE: G, workgroups per block; NARROW: units per block
    uint32_t pad_;
};

// G of the wide form: strided_row_groups_max with no promise about where a
// block's inoutbuf address falls on the 16 KiB grid
inline uint64_t indexed_row_groups_max(uint64_t row_bytes, size_t esz) {
    return strided_row_groups_max(row_bytes, esz, reinterpret_cast<const void *>((uintptr_t)16), 0);
}

// byte offset of block `row`: the table's entry times disp_unit (the product
// wraps as pointer arithmetic does: displacements are signed), or the packed place
__device__ __forceinline__ uint64_t indexed_off(const int64_t *displs, uint64_t row, uint64_t disp_unit,
                                                uint64_t row_bytes) {
    return displs ? (uint64_t)displs[row] * disp_unit : row * row_bytes;
}

// a 16-byte vector in the global address space: the narrow vector form's
// per-lane accesses are global_load / global_store, not flat
typedef u32x4 __attribute__((address_space(1))) global_u32x4;

template <class Op, class T>
__device__ __forceinline__ void reduce_indexed_narrow(const IndexedArgs &a) {
    const uint32_t upr = a.per;                             // units per block
    const uint64_t row_bytes = a.blocklen * sizeof(T);
    const unsigned t = threadIdx.x;
    if constexpr (sizeof(T) <= 16) {
        if (a.form == MPIR_HIP_INDEXED_NARROW_VEC) {
            constexpr uint32_t upw = strided_units_per_group<T>(true);
            constexpr int per_lane = (int)(upw / kThreads);
            const uint64_t u0 = (uint64_t)blockIdx.x * upw;
            const uint64_t row0 = u0 / upr;
            const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
            // A unit past the launch's last block is clamped into that block: its
            // table and data loads stay inside the operands and need no branch, so
            // each batch of loads issues back to back; only the store is guarded.
            // (The workgroup's first unit is always a real one: nrows > row0.)
            const uint64_t last = a.nrows - 1;
            u32x4 x[per_lane], y[per_lane];
            uint64_t row[per_lane], off[per_lane], oi[per_lane], oo[per_lane];
            bool ok[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                const uint32_t c = col0 + t + (uint32_t)j * kThreads;
                const uint32_t q = c / upr;
                const uint64_t r = row0 + q;
                ok[j] = r <= last;
                row[j] = ok[j] ? r : last;
                off[j] = (uint64_t)(c - q * upr) * 16;
                oi[j] = oo[j] = row[j] * row_bytes;         // the packed place
            }
            // the null tests are uniform and outside the unrolled loops: a side's
            // per_lane table loads are one straight run
            if (a.io_displs) {
                int64_t d[per_lane];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) d[j] = a.io_displs[row[j]];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) oo[j] = (uint64_t)d[j] * a.disp_unit;
            }
            if (a.in_displs) {
                int64_t d[per_lane];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) d[j] = a.in_displs[row[j]];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) oi[j] = (uint64_t)d[j] * a.disp_unit;
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                x[j] = __builtin_nontemporal_load((const global_u32x4 *)(a.io + oo[j] + off[j]));
                y[j] = __builtin_nontemporal_load((const global_u32x4 *)(a.in + oi[j] + off[j]));
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j)
                if (ok[j])
                    __builtin_nontemporal_store(combine16<Op, T>(x[j], y[j]),
                                                (global_u32x4 *)(a.io + oo[j] + off[j]));
            return;
        }
    }
    constexpr uint32_t upw = strided_units_per_group<T>(false);
    const uint64_t u0 = (uint64_t)blockIdx.x * upw;
    const uint64_t row0 = u0 / upr;
    const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
    for (uint32_t k = t; k < upw; k += kThreads) {
        const uint32_t c = col0 + k;
        const uint32_t q = c / upr;
        const uint64_t row = row0 + q;
        if (row >= a.nrows) break;                          // blocks only grow with k
        batch_elem_at<Op, T>(a.in + indexed_off(a.in_displs, row, a.disp_unit, row_bytes),
                             a.io + indexed_off(a.io_displs, row, a.disp_unit, row_bytes), c - q * upr);
    }
}

// a 64-bit value every lane of the wave holds, made provably so
__device__ __forceinline__ uint64_t wave_uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_indexed(IndexedArgs a) {
    if (a.form == MPIR_HIP_INDEXED_WIDE) {
        const uint32_t row = blockIdx.x / a.per;
        if (row >= a.nrows) return;
        const uint64_t row_bytes = a.blocklen * sizeof(T);
        const uint64_t oi = wave_uniform64(indexed_off(a.in_displs, row, a.disp_unit, row_bytes));
        const uint64_t oo = wave_uniform64(indexed_off(a.io_displs, row, a.disp_unit, row_bytes));
        reduce_seg<Op, T>(a.in + oi, a.io + oo, a.blocklen, blockIdx.x - row * a.per);
        return;
    }
    reduce_indexed_narrow<Op, T>(a);
}

// one launch: `groups` workgroups over a.nrows blocks (the planner's count, as
// for launch_strided)
template <class Op, class T>
hipError_t launch_indexed(const IndexedArgs *a, uint64_t groups, hipStream_t s) {
    if (!a->nrows || !a->per || !a->blocklen || !a->disp_unit || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_indexed<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Ordered indexed reductions (MPIR_Hip_reduce_indexed_ordered): the indexed
// call with an output table that may name one target block any number of times,
// the blocks of one target combined one after another in table order -- what a
// sequence of MPI_Reduce_local calls leaves, bit for bit, and what a target that
// has queued several accumulates to one location must do.  A third table,
// `order` (nblocks ints, a stable argsort of io_displs), puts the blocks of one
// target side by side: a RUN of sorted positions.  Rows of the indexed kernel
// become sorted positions p; the plan and the forms are the indexed call's.
//
//   * Head test: position p heads a run iff p == 0 or io_displs[order[p - 1]]
//     != io_displs[order[p]].  Only a head works: a workgroup (WIDE) or a lane's
//     unit (NARROW) at any other position ends at once, having loaded two
//     entries of each table and no data.
//   * Run loop: the head loads its tile, vector or element of the target ONCE,
//     then for q = p, p + 1, ... while q < nblocks and io_displs[order[q]] is
//     the head's, loads the same piece of input block order[q] and combines it
//     into registers, each step rounded as the type rounds it; then it stores
//     once.  A run is folded serially by one slice of one workgroup: the order
//     is the contract, a tree would change floating-point results.  A target
//     with very many contributions (a hot row) therefore costs one dependent
//     chain of table and data loads per contribution.
//   * Launches: the kernel takes the call's tables and bases unadvanced, the
//     launch's first sorted position (pos0) and the whole nblocks, so a later
//     launch's head test looks back across the launch boundary and a run goes on
//     past its launch's last position.  A run belongs entirely to its head, so no
//     two workgroups, of one launch or of two, ever write one target.
//   * WIDE: the split of a target block into workgroups comes from the target's
//     address alone (seg_split with inoutbuf on both sides: the 16 KiB tile grid
//     of its address where it is naturally aligned, else the element form), so
//     that a workgroup owns one piece of the target over the whole run whatever
//     the input blocks' alignments.  An input block that shares the target's
//     offset mod 16 is read through a buffer descriptor as reduce_tile reads it;
//     any other is read element by element into the same registers.  The block
//     numbers and displacements pass through readfirstlane (wave_uniform64), so
//     descriptors stay in scalar registers.  G is the indexed call's.
//   * NARROW_VEC: a lane's four units' order and displacement loads issue in
//     straight runs, as in the indexed kernel; only heads load data.  A head
//     then walks its run kOrderedAhead positions at a time: the table entries
//     of the next four positions load together, then the data of those still
//     in the run, and the combines follow in order -- three dependent round
//     trips per four contributions instead of per one.
//   * Every index read from `order` is clamped into [0, nblocks): a device order
//     table that breaks its conditions gives an undefined result, but the
//     kernel's reads of all three tables stay inside them.
//
// No LDS, no scratch, no gridDim.  Tile and vector stores are nt.
// ============================================================================
struct OrderedArgs {
    const char *in;             // the call's bases and tables, the same in every launch
    char *io;
    const int64_t *in_displs;   // null: packed input, block k at k * the block's bytes
    const int64_t *io_displs;   // never null
    const int *order;           // sorted position -> block number
    uint64_t disp_unit;         // bytes per displacement unit, > 0
    uint64_t blocklen;          // elements per block, > 0
    uint32_t nblocks;           // blocks of the whole call
    uint32_t pos0;              // this launch's first sorted position
    uint32_t nrows;             // sorted positions of this launch, > 0
    uint32_t form;              // MPIR_HIP_INDEXED_WIDE / _NARROW_VEC / _NARROW_ELEMS
    uint32_t per;               // WIDE: G, workgroups per block; NARROW: units per block
    uint32_t pad_;
};

// The helpers below serve two kernels.  Fetch = false is k_reduce_indexed_ordered
// as described above.  Fetch = true is k_reduce_fetch_indexed_ordered (its own
// section, below): before every combine the running value goes to block
// k's place in a packed `fetch` buffer, a null `order` is the identity, and Op may
// be one of the two byte functors (OpFetchNoOp: no input is read and the target
// is never stored; OpFetchSwap: the input's bytes become the running value) over
// T = RawBytes<size>.  Everything the fetching form adds sits under `if constexpr
// (Fetch)`, so the Fetch = false instantiations are the code they were.
struct OpFetchNoOp;
struct OpFetchSwap;
template <int N>
struct RawBytes;

// the block at sorted position p (p < nblocks), clamped into the tables
template <bool Fetch = false>
__device__ __forceinline__ uint32_t ordered_block(const OrderedArgs &a, uint32_t p) {
    if constexpr (Fetch)
        if (!a.order) return p;                             // (uniform: a kernel argument)
    const uint32_t k = (uint32_t)a.order[p];
    return k < a.nblocks ? k : a.nblocks - 1;
}

// combine16 for the ops of either kernel
template <class Op, class T>
__device__ __forceinline__ u32x4 ordered_combine16(u32x4 x, u32x4 y) {
    if constexpr (__is_same(Op, OpFetchNoOp)) return x;
    else if constexpr (__is_same(Op, OpFetchSwap)) return y;
    else return combine16<Op, T>(x, y);
}

// N bytes of no type to dst (any alignment), nt like every store to fetchbuf
template <class Raw>
__device__ __forceinline__ void ordered_fetch_store(char *dst, const Raw &x) {
    typedef decltype(Raw::v) __attribute__((aligned(1))) unaligned_t;
    __builtin_nontemporal_store(x.v, reinterpret_cast<unaligned_t *>(dst));
}

// Element i of the run headed by position p (block k0, displacement d0, target
// block at io): loaded once, every block of the run combined in, stored once.
// Fetch: the element's bytes as they stand before block k's combine go to block
// k of `fetch` -- for the head the target's own bytes, never a value of type T.
template <class Op, class T, bool Fetch = false>
__device__ __forceinline__ void ordered_elem_run(const OrderedArgs &a, uint32_t p, uint32_t k0, int64_t d0, char *io,
                                                 uint64_t row_bytes, uint64_t i, char *fetch = nullptr) {
    if constexpr (Fetch) {
        typedef RawBytes<(int)sizeof(T)> Raw;
        constexpr bool no_op = __is_same(Op, OpFetchNoOp), swap = __is_same(Op, OpFetchSwap);
        Raw x;
        __builtin_memcpy(&x, io + i * sizeof(T), sizeof(T));
        uint32_t k = k0;
        for (uint32_t q = p;;) {
            ordered_fetch_store(fetch + (uint64_t)k * row_bytes + i * sizeof(T), x);
            if constexpr (!no_op) {
                const char *in = a.in + indexed_off(a.in_displs, k, a.disp_unit, row_bytes);
                if constexpr (swap) {
                    __builtin_memcpy(&x, in + i * sizeof(T), sizeof(T));
                } else {
                    Op op;
                    T y;
                    __builtin_memcpy(&y, in + i * sizeof(T), sizeof(T));
                    x = __builtin_bit_cast(Raw, op(__builtin_bit_cast(T, x), y));
                }
            }
            if (++q >= a.nblocks) break;
            k = ordered_block<true>(a, q);
            if (a.io_displs[k] != d0) break;
        }
        if constexpr (!no_op) __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
    } else {
        Op op;
        T x, y;
        __builtin_memcpy(&x, io + i * sizeof(T), sizeof(T));
        uint32_t k = k0;
        for (uint32_t q = p;;) {
            const char *in = a.in + indexed_off(a.in_displs, k, a.disp_unit, row_bytes);
            __builtin_memcpy(&y, in + i * sizeof(T), sizeof(T));
            x = op(x, y);
            if (++q >= a.nblocks) break;
            k = ordered_block(a, q);
            if (a.io_displs[k] != d0) break;
        }
        __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
    }
}

// A workgroup's tile of the running value (x: the lane's kVecPerLane vectors at
// byte offsets wb + u * 1024 of the nrec-byte tile at io_tile) out to `fe`, the
// same tile of a block of fetch: through a descriptor bounded like the target's
// (lanes outside the tile are dropped) where fe shares the target's 16-byte
// phase, else element by element
// under the guard the off-phase input path has.  nt stores both.
template <class T>
__device__ __forceinline__ void ordered_wide_fetch(const u32x4 (&x)[kVecPerLane], char *fe, const char *io_tile, int nrec,
                                                   int wb) {
    if (((reinterpret_cast<uintptr_t>(fe) ^ reinterpret_cast<uintptr_t>(io_tile)) & 15) == 0) {
        __amdgpu_buffer_rsrc_t rfe = __builtin_amdgcn_make_buffer_rsrc((void *)fe, 0, nrec, 0x00020000);
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) store16(x[u], rfe, wb + u * 1024, false);
    } else {
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int off = wb + u * 1024;
            if ((unsigned)off < (unsigned)nrec) {
                const Pack16<T> v = __builtin_bit_cast(Pack16<T>, x[u]);
#pragma unroll
                for (int e = 0; e < (int)(16 / sizeof(T)); ++e)
                    ordered_fetch_store(fe + off + e * (int)sizeof(T),
                                        __builtin_bit_cast(RawBytes<(int)sizeof(T)>, v.e[e]));
            }
        }
    }
}

template <class Op, class T, bool Fetch = false>
__device__ __forceinline__ void reduce_ordered_wide(const OrderedArgs &a, char *fetch = nullptr) {
    constexpr bool no_op = __is_same(Op, OpFetchNoOp);
    const uint32_t r = blockIdx.x / a.per;
    if (r >= a.nrows) return;
    const uint32_t p = a.pos0 + r;
    const uint64_t tile = blockIdx.x - r * a.per;
    const uint64_t row_bytes = a.blocklen * sizeof(T);
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ordered_block<Fetch>(a, p));
    const int64_t d0 = (int64_t)wave_uniform64((uint64_t)a.io_displs[k0]);
    if (p && a.io_displs[ordered_block<Fetch>(a, p - 1)] == d0) return;    // not a head
    char *io = a.io + (uint64_t)d0 * a.disp_unit;
    // the target's own split: an input block's alignment decides only how it is read
    const SegSplit s = seg_split<T>(io, io, a.blocklen);
    if (tile >= batch_seg_groups<T>(s, io, a.blocklen)) return;
    if constexpr (sizeof(T) <= 16) {
        if (s.tile) {
            char *iov = io + s.head_bytes;
            const int64_t start = (int64_t)(tile * kTileBytes) - (int64_t)tile_shift(iov);
            const uint64_t lo = start > 0 ? (uint64_t)start : 0;
            if (lo < s.vbytes) {
                const uint64_t end = (uint64_t)(start + kTileBytes);
                const int nrec = (int)((end < s.vbytes ? end : s.vbytes) - lo);
                const int cut = (int)(lo - start);
                __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(iov + lo), 0, nrec, 0x00020000);
                const int t = (int)threadIdx.x;
                const int wb = (t >> 6) * (kVecPerLane * 1024) + (t & 63) * 16 - cut;
                u32x4 x[kVecPerLane];
#pragma unroll
                for (int u = 0; u < kVecPerLane; ++u)
                    x[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, wb + u * 1024, 0, kCachePolicyNT);
                uint32_t k = k0;
                for (uint32_t q = p;;) {
                    if constexpr (Fetch)
                        ordered_wide_fetch<T>(x, fetch + (uint64_t)k * row_bytes + s.head_bytes + lo, iov + lo, nrec, wb);
                    if constexpr (!no_op) {
                        const uint64_t oi = wave_uniform64(indexed_off(a.in_displs, k, a.disp_unit, row_bytes));
                        const char *in = a.in + oi + s.head_bytes + lo;
                        if (((reinterpret_cast<uintptr_t>(in) ^ reinterpret_cast<uintptr_t>(iov + lo)) & 15) == 0) {
                            __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *)in, 0, nrec, 0x00020000);
                            u32x4 y[kVecPerLane];
#pragma unroll
                            for (int u = 0; u < kVecPerLane; ++u)
                                y[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, wb + u * 1024, 0, kCachePolicyNT);
#pragma unroll
                            for (int u = 0; u < kVecPerLane; ++u) x[u] = ordered_combine16<Op, T>(x[u], y[u]);
                        } else {
                            // an input block off the target's 16-byte phase: its elements one
                            // by one, only where the lane's vector lies inside the tile
#pragma unroll
                            for (int u = 0; u < kVecPerLane; ++u) {
                                const int off = wb + u * 1024;
                                if ((unsigned)off < (unsigned)nrec) {
                                    Pack16<T> y;
#pragma unroll
                                    for (int e = 0; e < (int)(16 / sizeof(T)); ++e)
                                        __builtin_memcpy(&y.e[e], in + off + e * (int)sizeof(T), sizeof(T));
                                    x[u] = ordered_combine16<Op, T>(x[u], __builtin_bit_cast(u32x4, y));
                                }
                            }
                        }
                    }
                    if (++q >= a.nblocks) break;
                    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)ordered_block<Fetch>(a, q));
                    if (a.io_displs[k] != d0) break;
                }
                if constexpr (!no_op) {
#pragma unroll
                    for (int u = 0; u < kVecPerLane; ++u) store16(x[u], rio, wb + u * 1024, false);
                }
            }
            if (tile == 0) {
                // the head and tail elements, a lane each as in reduce_seg
                const unsigned t = threadIdx.x;
                if (t < s.nhead) ordered_elem_run<Op, T, Fetch>(a, p, k0, d0, io, row_bytes, t, fetch);
                else if (t >= 64 && t - 64 < s.ntail)
                    ordered_elem_run<Op, T, Fetch>(a, p, k0, d0, io, row_bytes,
                                                   (s.head_bytes + s.vbytes) / sizeof(T) + (t - 64), fetch);
            }
            return;
        }
    }
    constexpr uint64_t per = kTileBytes / sizeof(T);
    const uint64_t base = tile * per;
    const uint64_t end = base + per < a.blocklen ? base + per : a.blocklen;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads)
        ordered_elem_run<Op, T, Fetch>(a, p, k0, d0, io, row_bytes, i, fetch);
}

// sorted positions the narrow vector form looks ahead of a run's current end
constexpr int kOrderedAhead = 4;

template <class Op, class T, bool Fetch = false>
__device__ __forceinline__ void reduce_ordered_narrow(const OrderedArgs &a, char *fetch = nullptr) {
    constexpr bool no_op = __is_same(Op, OpFetchNoOp);
    const uint32_t upr = a.per;                             // units per block
    const uint64_t row_bytes = a.blocklen * sizeof(T);
    const unsigned t = threadIdx.x;
    if constexpr (sizeof(T) <= 16) {
        if (a.form == MPIR_HIP_INDEXED_NARROW_VEC) {
            constexpr uint32_t upw = strided_units_per_group<T>(true);
            constexpr int per_lane = (int)(upw / kThreads);
            const uint64_t u0 = (uint64_t)blockIdx.x * upw;
            const uint64_t row0 = u0 / upr;
            const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
            // a unit past the launch's last position is clamped into it, as the
            // indexed kernel clamps: its table loads need no branch
            const uint64_t last = a.nrows - 1;
            uint32_t pos[per_lane], k[per_lane], kp[per_lane], kn[per_lane];
            uint64_t off[per_lane], oi[per_lane];
            int64_t d[per_lane], dp[per_lane], dn[per_lane];
            bool head[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                const uint32_t c = col0 + t + (uint32_t)j * kThreads;
                const uint32_t q = c / upr;
                const uint64_t r = row0 + q;
                head[j] = r <= last;
                pos[j] = a.pos0 + (uint32_t)(head[j] ? r : last);
                off[j] = (uint64_t)(c - q * upr) * 16;
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j) k[j] = ordered_block<Fetch>(a, pos[j]);
#pragma unroll
            for (int j = 0; j < per_lane; ++j) kp[j] = ordered_block<Fetch>(a, pos[j] ? pos[j] - 1 : 0);
            // (the position after, with the same loads: whether a run goes on at all is
            // then known without another round trip, and a run of one ends here)
#pragma unroll
            for (int j = 0; j < per_lane; ++j)
                kn[j] = ordered_block<Fetch>(a, pos[j] + 1 < a.nblocks ? pos[j] + 1 : pos[j]);
#pragma unroll
            for (int j = 0; j < per_lane; ++j) d[j] = a.io_displs[k[j]];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) dp[j] = a.io_displs[kp[j]];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) dn[j] = a.io_displs[kn[j]];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                head[j] = head[j] && (pos[j] == 0 || d[j] != dp[j]);
                oi[j] = (uint64_t)k[j] * row_bytes;         // the packed place
            }
            if (!no_op && a.in_displs) {
                int64_t di[per_lane];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) di[j] = a.in_displs[k[j]];
#pragma unroll
                for (int j = 0; j < per_lane; ++j) oi[j] = (uint64_t)di[j] * a.disp_unit;
            }
            // only heads touch data: the target's vector once, its own block's first
            u32x4 x[per_lane], y[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                x[j] = y[j] = u32x4{0, 0, 0, 0};
                if (head[j]) {
                    x[j] = __builtin_nontemporal_load((const global_u32x4 *)(a.io + (uint64_t)d[j] * a.disp_unit + off[j]));
                    if constexpr (!no_op)
                        y[j] = __builtin_nontemporal_load((const global_u32x4 *)(a.in + oi[j] + off[j]));
                }
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                if (!head[j]) continue;
                // (Fetch: the target's own bytes to the head block's place, then every
                // later block of the run gets v as it stands before its combine)
                if constexpr (Fetch)
                    __builtin_nontemporal_store(x[j], (global_u32x4 *)(fetch + (uint64_t)k[j] * row_bytes + off[j]));
                u32x4 v = ordered_combine16<Op, T>(x[j], y[j]);
                // the rest of the run, kOrderedAhead positions at a time: their order
                // entries, then their displacements, then the data of those that still
                // belong to the run issue together (a position past the table is
                // clamped into it and not counted), so a step costs a fraction of the
                // three dependent round trips; the combines stay in order
                bool more = dn[j] == d[j];
                for (uint32_t q = pos[j] + 1; more && q < a.nblocks; q += kOrderedAhead) {
                    uint32_t kq[kOrderedAhead];
                    int64_t dq[kOrderedAhead];
                    uint64_t oq[kOrderedAhead];
                    u32x4 w[kOrderedAhead];
                    bool in_run[kOrderedAhead];
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i)
                        kq[i] = ordered_block<Fetch>(a, q + i < a.nblocks ? q + i : a.nblocks - 1);
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i) dq[i] = a.io_displs[kq[i]];
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i)
                        oq[i] = no_op ? 0 : indexed_off(a.in_displs, kq[i], a.disp_unit, row_bytes);
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i) {
                        more = more && q + i < a.nblocks && dq[i] == d[j];
                        w[i] = u32x4{0, 0, 0, 0};
                        if constexpr (!no_op)
                            if (more) w[i] = __builtin_nontemporal_load((const global_u32x4 *)(a.in + oq[i] + off[j]));
                        in_run[i] = more;
                    }
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i)
                        if (in_run[i]) {
                            if constexpr (Fetch)
                                __builtin_nontemporal_store(v, (global_u32x4 *)(fetch + (uint64_t)kq[i] * row_bytes + off[j]));
                            v = ordered_combine16<Op, T>(v, w[i]);
                        }
                }
                if constexpr (!no_op)
                    __builtin_nontemporal_store(v, (global_u32x4 *)(a.io + (uint64_t)d[j] * a.disp_unit + off[j]));
            }
            return;
        }
    }
    constexpr uint32_t upw = strided_units_per_group<T>(false);
    const uint64_t u0 = (uint64_t)blockIdx.x * upw;
    const uint64_t row0 = u0 / upr;
    const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
    for (uint32_t u = t; u < upw; u += kThreads) {
        const uint32_t c = col0 + u;
        const uint32_t q = c / upr;
        const uint64_t r = row0 + q;
        if (r >= a.nrows) break;                            // positions only grow with u
        const uint32_t p = a.pos0 + (uint32_t)r;
        const uint32_t k0 = ordered_block<Fetch>(a, p);
        const int64_t d0 = a.io_displs[k0];
        if (p && a.io_displs[ordered_block<Fetch>(a, p - 1)] == d0) continue;   // not a head
        ordered_elem_run<Op, T, Fetch>(a, p, k0, d0, a.io + (uint64_t)d0 * a.disp_unit, row_bytes, c - q * upr, fetch);
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_indexed_ordered(OrderedArgs a) {
    if (a.form == MPIR_HIP_INDEXED_WIDE) reduce_ordered_wide<Op, T>(a);
    else reduce_ordered_narrow<Op, T>(a);
}

// one launch: `groups` workgroups over sorted positions [pos0, pos0 + nrows)
template <class Op, class T>
hipError_t launch_indexed_ordered(const OrderedArgs *a, uint64_t groups, hipStream_t s) {
    if (!a->nrows || !a->per || !a->blocklen || !a->disp_unit || !a->io_displs || !a->order ||
        (uint64_t)a->pos0 + a->nrows > a->nblocks || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_indexed_ordered<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Chunked indexed reductions (MPIR_Hip_reduce_indexed_chunked): the ordered
// call's tables and run walk, but a run's contributions are cut into chunks of
// kChunk = 64 counted from the run's first position, each chunk folded into a
// partial that starts as a byte copy of the chunk's first input block, and the
// partials then folded into the target in order.  The association is fixed by
// the run's own length alone, so the bits are deterministic; a hot row's serial
// depth falls from L to 64 + L / 64.  A fourth table, `runstart` (nblocks ints:
// the first sorted position of the run position p lies in), tells a position
// where its chunk starts without a walk back.  Two launches per call, always:
//
//   * k_chunk_partials: the ordered plan's units over sorted positions.  A
//     unit at p works iff (p - runstart[p]) % 64 == 0.  It loads its piece of
//     input block order[p], walks at most 63 further positions while the
//     displacement is its own (NARROW_VEC: kOrderedAhead at a time), and then
//     either -- the run's first chunk, and position p + 64 is not the run's --
//     loads the target, combines the partial into it and stores, or stores the
//     partial to its slot of `work`.
//   * k_fold_partials: a unit at a head (p == runstart[p]) whose run goes on at
//     p + 64 loads the target, combines the partials of chunks p, p + 64, ...
//     while the displacement at that position is the head's, and stores once.
//   * Slots: slot 2 * (q / 64) + (q heads its run) for the chunk at q: a window
//     of 64 positions starts at most one first chunk and one short last chunk
//     of runs longer than a chunk.  A slot is slot_bytes apart (the block's
//     bytes rounded up to 16, and 16 more); the partial sits at the target
//     block's address mod 16 inside it, so a WIDE workgroup reaches its piece of
//     every partial through a buffer descriptor as it reaches the target.
//   * The launch split, the forms, pos0 / nrows and the clamping of `order` are
//     the ordered kernel's; runstart[p] is clamped to at most p, so a slot index
//     stays below 2 * ceil(nblocks / 64) whatever a device table holds.
//
// No workgroup waits for another: the two kernels are ordered by the stream.
// No LDS, no scratch, no gridDim.  Tile and vector stores are nt.
// ============================================================================
constexpr uint32_t kChunk = MPIR_HIP_REDUCE_CHUNK;

struct ChunkedArgs {
    OrderedArgs o;              // as for k_reduce_indexed_ordered
    const int *runstart;        // sorted position -> first sorted position of its run
    char *work;                 // the partials' slots, 16-byte aligned
    uint64_t slot_bytes;        // from one slot to the next, a multiple of 16
};

// what the unit at sorted position p is: its block and displacement, whether p
// heads its run (first) and whether position p + kChunk is the run's too (cont).
// True where the unit works in this kernel.
template <bool Fold>
__device__ __forceinline__ bool chunk_unit(const ChunkedArgs &a, uint32_t p, uint32_t &k0, int64_t &d0, bool &first,
                                           bool &cont) {
    const OrderedArgs &o = a.o;
    uint32_t rs = (uint32_t)a.runstart[p];
    if (rs > p) rs = p;
    const uint32_t p64 = p + kChunk;
    k0 = ordered_block(o, p);
    const uint32_t k64 = ordered_block(o, p64 < o.nblocks ? p64 : o.nblocks - 1);
    d0 = o.io_displs[k0];
    cont = p64 < o.nblocks && o.io_displs[k64] == d0;
    first = rs == p;
    return Fold ? first && cont : (p - rs) % kChunk == 0;
}

// the partial of the chunk at sorted position q (first: q heads its run) of the target block at io
__device__ __forceinline__ char *chunk_slot(const ChunkedArgs &a, uint32_t q, bool first, const char *io) {
    return a.work + (2 * (uint64_t)(q / kChunk) + (first ? 1 : 0)) * a.slot_bytes + (reinterpret_cast<uintptr_t>(io) & 15);
}

// Element i of the unit at position p, either kernel's work on it
template <class Op, class T, bool Fold>
__device__ __forceinline__ void chunk_elem_run(const ChunkedArgs &a, uint32_t p, uint32_t k0, int64_t d0, bool first,
                                               bool cont, char *io, uint64_t row_bytes, uint64_t i) {
    const OrderedArgs &o = a.o;
    Op op;
    T x, y;
    if constexpr (Fold) {
        __builtin_memcpy(&x, io + i * sizeof(T), sizeof(T));
        for (uint32_t q = p;;) {
            __builtin_memcpy(&y, chunk_slot(a, q, q == p, io) + i * sizeof(T), sizeof(T));
            x = op(x, y);
            q += kChunk;
            if (q >= o.nblocks || o.io_displs[ordered_block(o, q)] != d0) break;
        }
        __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
    } else {
        __builtin_memcpy(&x, o.in + indexed_off(o.in_displs, k0, o.disp_unit, row_bytes) + i * sizeof(T), sizeof(T));
        const uint32_t qend = p + kChunk < o.nblocks ? p + kChunk : o.nblocks;
        for (uint32_t q = p + 1; q < qend; ++q) {
            const uint32_t k = ordered_block(o, q);
            if (o.io_displs[k] != d0) break;
            __builtin_memcpy(&y, o.in + indexed_off(o.in_displs, k, o.disp_unit, row_bytes) + i * sizeof(T), sizeof(T));
            x = op(x, y);
        }
        if (first && !cont) {
            __builtin_memcpy(&y, io + i * sizeof(T), sizeof(T));
            y = op(y, x);
            __builtin_memcpy(io + i * sizeof(T), &y, sizeof(T));
        } else {
            __builtin_memcpy(chunk_slot(a, p, first, io) + i * sizeof(T), &x, sizeof(T));
        }
    }
}

// A workgroup's tile (the lane's kVecPerLane vectors at byte offsets wb + u *
// 1024 of the nrec-byte tile at io_tile) of a block at src: through a descriptor
// where src shares the target's 16-byte phase, else element by element inside
// the tile; vectors outside it come back zero.
template <class T>
__device__ __forceinline__ void chunk_wide_load(u32x4 (&y)[kVecPerLane], const char *src, const char *io_tile, int nrec,
                                                int wb) {
    if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(io_tile)) & 15) == 0) {
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)src, 0, nrec, 0x00020000);
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) y[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, wb + u * 1024, 0, kCachePolicyNT);
    } else {
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int off = wb + u * 1024;
            y[u] = u32x4{0, 0, 0, 0};
            if ((unsigned)off < (unsigned)nrec) {
                Pack16<T> e;
#pragma unroll
                for (int j = 0; j < (int)(16 / sizeof(T)); ++j)
                    __builtin_memcpy(&e.e[j], src + off + j * (int)sizeof(T), sizeof(T));
                y[u] = __builtin_bit_cast(u32x4, e);
            }
        }
    }
}

template <class Op, class T, bool Fold>
__device__ __forceinline__ void chunked_wide(const ChunkedArgs &a) {
    const OrderedArgs &o = a.o;
    const uint32_t r = blockIdx.x / o.per;
    if (r >= o.nrows) return;
    const uint32_t p = o.pos0 + r;
    const uint64_t tile = blockIdx.x - r * o.per;
    const uint64_t row_bytes = o.blocklen * sizeof(T);
    uint32_t k0;
    int64_t d0;
    bool first, cont;
    if (!chunk_unit<Fold>(a, p, k0, d0, first, cont)) return;
    k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k0);
    d0 = (int64_t)wave_uniform64((uint64_t)d0);
    char *io = o.io + (uint64_t)d0 * o.disp_unit;
    // the target's own split, as in the ordered kernel: a workgroup owns the same
    // piece of the target, of every input block and of every partial
    const SegSplit s = seg_split<T>(io, io, o.blocklen);
    if (tile >= batch_seg_groups<T>(s, io, o.blocklen)) return;
    const uint32_t qend = p + kChunk < o.nblocks ? p + kChunk : o.nblocks;
    if constexpr (sizeof(T) <= 16) {
        if (s.tile) {
            char *iov = io + s.head_bytes;
            const int64_t start = (int64_t)(tile * kTileBytes) - (int64_t)tile_shift(iov);
            const uint64_t lo = start > 0 ? (uint64_t)start : 0;
            if (lo < s.vbytes) {
                const uint64_t end = (uint64_t)(start + kTileBytes);
                const int nrec = (int)((end < s.vbytes ? end : s.vbytes) - lo);
                const int cut = (int)(lo - start);
                const uint64_t at = s.head_bytes + lo;          // the tile's place in a block
                __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(iov + lo), 0, nrec, 0x00020000);
                const int t = (int)threadIdx.x;
                const int wb = (t >> 6) * (kVecPerLane * 1024) + (t & 63) * 16 - cut;
                u32x4 x[kVecPerLane], y[kVecPerLane];
                if constexpr (Fold) {
#pragma unroll
                    for (int u = 0; u < kVecPerLane; ++u)
                        x[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, wb + u * 1024, 0, kCachePolicyNT);
                    for (uint32_t q = p;;) {
                        chunk_wide_load<T>(y, chunk_slot(a, q, q == p, io) + at, iov + lo, nrec, wb);
#pragma unroll
                        for (int u = 0; u < kVecPerLane; ++u) x[u] = combine16<Op, T>(x[u], y[u]);
                        q += kChunk;
                        if (q >= o.nblocks) break;
                        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)ordered_block(o, q));
                        if (o.io_displs[k] != d0) break;
                    }
#pragma unroll
                    for (int u = 0; u < kVecPerLane; ++u) store16(x[u], rio, wb + u * 1024, false);
                } else {
                    chunk_wide_load<T>(x, o.in + wave_uniform64(indexed_off(o.in_displs, k0, o.disp_unit, row_bytes)) + at,
                                       iov + lo, nrec, wb);
                    for (uint32_t q = p + 1; q < qend; ++q) {
                        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)ordered_block(o, q));
                        if (o.io_displs[k] != d0) break;
                        chunk_wide_load<T>(y, o.in + wave_uniform64(indexed_off(o.in_displs, k, o.disp_unit, row_bytes)) + at,
                                           iov + lo, nrec, wb);
#pragma unroll
                        for (int u = 0; u < kVecPerLane; ++u) x[u] = combine16<Op, T>(x[u], y[u]);
                    }
                    if (first && !cont) {
#pragma unroll
                        for (int u = 0; u < kVecPerLane; ++u)
                            y[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, wb + u * 1024, 0, kCachePolicyNT);
#pragma unroll
                        for (int u = 0; u < kVecPerLane; ++u) store16(combine16<Op, T>(y[u], x[u]), rio, wb + u * 1024, false);
                    } else {
                        __amdgpu_buffer_rsrc_t rw =
                            __builtin_amdgcn_make_buffer_rsrc((void *)(chunk_slot(a, p, first, io) + at), 0, nrec, 0x00020000);
#pragma unroll
                        for (int u = 0; u < kVecPerLane; ++u) store16(x[u], rw, wb + u * 1024, false);
                    }
                }
            }
            if (tile == 0) {
                // the head and tail elements, a lane each as in reduce_seg
                const unsigned t = threadIdx.x;
                if (t < s.nhead) chunk_elem_run<Op, T, Fold>(a, p, k0, d0, first, cont, io, row_bytes, t);
                else if (t >= 64 && t - 64 < s.ntail)
                    chunk_elem_run<Op, T, Fold>(a, p, k0, d0, first, cont, io, row_bytes,
                                                (s.head_bytes + s.vbytes) / sizeof(T) + (t - 64));
            }
            return;
        }
    }
    constexpr uint64_t per = kTileBytes / sizeof(T);
    const uint64_t base = tile * per;
    const uint64_t end = base + per < o.blocklen ? base + per : o.blocklen;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads)
        chunk_elem_run<Op, T, Fold>(a, p, k0, d0, first, cont, io, row_bytes, i);
}

template <class Op, class T, bool Fold>
__device__ __forceinline__ void chunked_narrow(const ChunkedArgs &a) {
    const OrderedArgs &o = a.o;
    const uint32_t upr = o.per;                             // units per block
    const uint64_t row_bytes = o.blocklen * sizeof(T);
    const unsigned t = threadIdx.x;
    if constexpr (sizeof(T) <= 16) {
        if (o.form == MPIR_HIP_INDEXED_NARROW_VEC) {
            constexpr uint32_t upw = strided_units_per_group<T>(true);
            constexpr int per_lane = (int)(upw / kThreads);
            const uint64_t u0 = (uint64_t)blockIdx.x * upw;
            const uint64_t row0 = u0 / upr;
            const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
            // a unit past the launch's last position is clamped into it, as in the ordered kernel
            const uint64_t last = o.nrows - 1;
            uint32_t pos[per_lane], rs[per_lane], k[per_lane], k64[per_lane];
            uint64_t off[per_lane];
            int64_t d[per_lane], d64[per_lane];
            bool act[per_lane], first[per_lane], cont[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                const uint32_t c = col0 + t + (uint32_t)j * kThreads;
                const uint32_t q = c / upr;
                const uint64_t r = row0 + q;
                act[j] = r <= last;
                pos[j] = o.pos0 + (uint32_t)(act[j] ? r : last);
                off[j] = (uint64_t)(c - q * upr) * 16;
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j) rs[j] = (uint32_t)a.runstart[pos[j]];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) k[j] = ordered_block(o, pos[j]);
#pragma unroll
            for (int j = 0; j < per_lane; ++j)
                k64[j] = ordered_block(o, pos[j] + kChunk < o.nblocks ? pos[j] + kChunk : o.nblocks - 1);
#pragma unroll
            for (int j = 0; j < per_lane; ++j) d[j] = o.io_displs[k[j]];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) d64[j] = o.io_displs[k64[j]];
            u32x4 x[per_lane];
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                if (rs[j] > pos[j]) rs[j] = pos[j];
                first[j] = rs[j] == pos[j];
                cont[j] = pos[j] + kChunk < o.nblocks && d64[j] == d[j];
                act[j] = act[j] && (Fold ? first[j] && cont[j] : (pos[j] - rs[j]) % kChunk == 0);
                x[j] = u32x4{0, 0, 0, 0};
                // only working units touch data: the target's vector (the fold), or
                // the chunk's first input block's
                if (act[j]) {
                    const char *src = Fold ? o.io + (uint64_t)d[j] * o.disp_unit
                                           : o.in + indexed_off(o.in_displs, k[j], o.disp_unit, row_bytes);
                    x[j] = __builtin_nontemporal_load((const global_u32x4 *)(src + off[j]));
                }
            }
#pragma unroll
            for (int j = 0; j < per_lane; ++j) {
                if (!act[j]) continue;
                char *io = o.io + (uint64_t)d[j] * o.disp_unit;
                u32x4 v = x[j];
                // the sources that follow, kOrderedAhead at a time as the ordered kernel
                // looks ahead: positions p + 1 .. p + 63 and their input blocks, or (the
                // fold) positions p, p + 64, ... and their partials
                const uint32_t step = Fold ? kChunk : 1;
                const uint32_t qend = Fold || pos[j] + kChunk >= o.nblocks ? o.nblocks : pos[j] + kChunk;
                bool more = true;
                for (uint32_t q = Fold ? pos[j] : pos[j] + 1; more && q < qend; q += kOrderedAhead * step) {
                    uint32_t kq[kOrderedAhead];
                    int64_t dq[kOrderedAhead];
                    u32x4 w[kOrderedAhead];
                    bool in_run[kOrderedAhead];
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i)
                        kq[i] = ordered_block(o, q + i * step < o.nblocks ? q + i * step : o.nblocks - 1);
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i) dq[i] = o.io_displs[kq[i]];
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i) {
                        const uint32_t qi = q + i * step;
                        more = more && qi < qend && dq[i] == d[j];
                        w[i] = u32x4{0, 0, 0, 0};
                        if (more) {
                            const char *src = Fold ? chunk_slot(a, qi, qi == pos[j], io)
                                                   : o.in + indexed_off(o.in_displs, kq[i], o.disp_unit, row_bytes);
                            w[i] = __builtin_nontemporal_load((const global_u32x4 *)(src + off[j]));
                        }
                        in_run[i] = more;
                    }
#pragma unroll
                    for (int i = 0; i < kOrderedAhead; ++i)
                        if (in_run[i]) v = combine16<Op, T>(v, w[i]);
                }
                if (Fold) {
                    __builtin_nontemporal_store(v, (global_u32x4 *)(io + off[j]));
                } else if (first[j] && !cont[j]) {
                    const u32x4 tg = __builtin_nontemporal_load((const global_u32x4 *)(io + off[j]));
                    __builtin_nontemporal_store(combine16<Op, T>(tg, v), (global_u32x4 *)(io + off[j]));
                } else {
                    __builtin_nontemporal_store(v, (global_u32x4 *)(chunk_slot(a, pos[j], first[j], io) + off[j]));
                }
            }
            return;
        }
    }
    constexpr uint32_t upw = strided_units_per_group<T>(false);
    const uint64_t u0 = (uint64_t)blockIdx.x * upw;
    const uint64_t row0 = u0 / upr;
    const uint32_t col0 = (uint32_t)(u0 - row0 * upr);
    for (uint32_t u = t; u < upw; u += kThreads) {
        const uint32_t c = col0 + u;
        const uint32_t q = c / upr;
        const uint64_t r = row0 + q;
        if (r >= o.nrows) break;                            // positions only grow with u
        const uint32_t p = o.pos0 + (uint32_t)r;
        uint32_t k0;
        int64_t d0;
        bool first, cont;
        if (!chunk_unit<Fold>(a, p, k0, d0, first, cont)) continue;
        chunk_elem_run<Op, T, Fold>(a, p, k0, d0, first, cont, o.io + (uint64_t)d0 * o.disp_unit, row_bytes, c - q * upr);
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_chunk_partials(ChunkedArgs a) {
    if (a.o.form == MPIR_HIP_INDEXED_WIDE) chunked_wide<Op, T, false>(a);
    else chunked_narrow<Op, T, false>(a);
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_fold_partials(ChunkedArgs a) {
    if (a.o.form == MPIR_HIP_INDEXED_WIDE) chunked_wide<Op, T, true>(a);
    else chunked_narrow<Op, T, true>(a);
}

// one launch of either kernel (fold: k_fold_partials): `groups` workgroups over
// sorted positions [pos0, pos0 + nrows)
template <class Op, class T>
hipError_t launch_indexed_chunked(const ChunkedArgs *a, int fold, uint64_t groups, hipStream_t s) {
    const OrderedArgs &o = a->o;
    if (!o.nrows || !o.per || !o.blocklen || !o.disp_unit || !o.io_displs || !o.order || !a->runstart || !a->work ||
        (reinterpret_cast<uintptr_t>(a->work) & 15) || (a->slot_bytes & 15) || a->slot_bytes < o.blocklen * sizeof(T) + 16 ||
        (uint64_t)o.pos0 + o.nrows > o.nblocks || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    if (fold) hipLaunchKernelGGL((k_fold_partials<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    else hipLaunchKernelGGL((k_chunk_partials<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Fetching ordered indexed reductions (MPIR_Hip_reduce_fetch_indexed_ordered):
// the ordered kernel with every intermediate value of a run handed out.  The
// call is MPIX_Reduce_local_fetch block by block in table order: block k of the
// packed `fetch` buffer receives the bytes target block io_displs[k] held after
// contributions 0 .. k - 1 and before contribution k -- what each of the
// MPI_Fetch_and_op / MPI_Get_accumulate operations a target has queued for one
// location must answer, a deterministic fetch-and-add, an exclusive scan by key.
//
// The ordered kernel already holds that value in registers at every step, so
// this kernel is the same functions with Fetch = true: the same head test, run
// loop, launches (pos0 / nrows / nblocks), split of a wide target and clamped
// table reads.  What it adds:
//
//   * One value: the registers stored to fetch and the registers combined are
//     the same ones.  The target is loaded once per run and stored once per run,
//     for MPI_NO_OP never.
//   * The head's store is the target's own bytes (a vector, or an element's
//     RawBytes), so NaN payloads and padding arrive as they were; a later block's
//     store is the bytes the ordered kernel would have stored to the target had
//     the run ended there.
//   * NARROW_VEC: the head stores x to fetch + k * row_bytes + off before its
//     first combine; in the look-ahead loop the four table and data loads still
//     issue together, and between the ordered combines v goes to block kq[i]'s
//     place.  fetch must be a multiple of 16 for this form (the host's plan).
//   * WIDE: ordered_wide_fetch before each ordered_wide_combine.  Packed fetch
//     blocks sit at k * row_bytes, so one run may take the descriptor stores for
//     some blocks and the element stores for others.
//   * A null `order` is the identity (sorted position p is block p): the caller's
//     promise that equal entries of io_displs are adjacent.  The test is on a
//     kernel argument, uniform.
//   * MPI_NO_OP and MPI_REPLACE are OpFetchNoOp / OpFetchSwap over
//     RawBytes<size>, as in k_reduce_fetch_ragged: NO_OP reads neither `in` nor
//     in_displs and stores no target (every block of a run receives the same old
//     bytes); REPLACE hands block k the previous block's input bytes.
//
// Block k's place in fetch belongs to the one lane that owns that piece of k's
// run, so no two lanes write one byte of fetch.  Every k is clamped below
// nblocks: whatever a device order table holds, stores stay inside fetch's
// nblocks x row_bytes and inside target blocks the displacement table names.
//
// No LDS, no scratch, no gridDim.  88 bytes of kernel arguments.  Every store to
// fetch and every tile and vector store is nt.
// ============================================================================
struct FetchOrderedArgs {
    OrderedArgs o;              // as for k_reduce_indexed_ordered, but `order` may be null (identity)
    char *fetch;                // packed by block number: block k at k * the block's bytes
};

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_fetch_indexed_ordered(FetchOrderedArgs a) {
    if (a.o.form == MPIR_HIP_INDEXED_WIDE) reduce_ordered_wide<Op, T, true>(a.o, a.fetch);
    else reduce_ordered_narrow<Op, T, true>(a.o, a.fetch);
}

// one launch: `groups` workgroups over sorted positions [pos0, pos0 + nrows)
template <class Op, class T>
hipError_t launch_fetch_indexed_ordered(const FetchOrderedArgs *a, uint64_t groups, hipStream_t s) {
    const OrderedArgs &o = a->o;
    if (!o.nrows || !o.per || !o.blocklen || !o.disp_unit || !o.io_displs || !a->fetch ||
        (uint64_t)o.pos0 + o.nrows > o.nblocks || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_fetch_indexed_ordered<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Ragged reductions (MPIR_Hip_reduce_ragged): npieces unequal pieces, piece k of
// starts[k + 1] - starts[k] elements (starts: npieces + 1 packed element offsets,
// CSR row pointers, a device table) at in + in_displs[k] * disp_unit and io +
// io_displs[k] * disp_unit; a side with no table is packed (piece k at
// starts[k] elements).  The target of an accumulate on an MPI_Type_indexed /
// hindexed type, or any IOV the segment code makes (do_accumulate_op,
// mpidrma.h:930-1021: starts is its running accumulated_count).
//
// Work goes by packed element, never by piece (a 3-element and a 3-million-
// element piece may share a call): workgroup g owns packed elements [g, g + 1) x
// kTileBytes / sizeof(T), the element paths' span everywhere else here, so the
// grid is ceil(count x sizeof(T) / 16 KiB), known on the host without a table,
// and the call is one launch always.
//
//   * The span's first piece, the largest p with starts[p] <= the span's first
//     element (so empty pieces before it are skipped), comes from a wave-wide
//     64-ary search: each lane probes one of 64 evenly spaced entries of the
//     range, a ballot and a population count pick the sub-range;
//     ceil(log64(npieces + 1)) dependent rounds (ragged_search_rounds) where a
//     binary search had ceil(log2).  Each wave searches for itself (no LDS, no
//     barrier); the result passes through readfirstlane.  The range is narrowed
//     by index arithmetic alone, so whatever the table holds no index leaves
//     [0, npieces].
//   * The piece boundaries inside the span go to LDS, 32-bit and relative to
//     the span's first element, 256 entries a pass until one reaches the span's
//     end (entries past starts[npieces] count as the end), at most
//     kRaggedLdsEntries.  With the first pass go the loads of the two
//     displacement tables' entries for the span's first 256 pieces, whose
//     products with disp_unit are kept in LDS as well.  A lane finds the piece
//     of each of its units by a binary search there.  A unit beyond the last boundary held (a span with
//     more boundaries than the table: one-byte elements in one-element pieces)
//     searches the global table from there on, again bounded by index.
//   * A lane's unit is a 16-byte chunk of PACKED space (V = 16 / sizeof(T)
//     elements; one element for the 32-byte classes).  The host cannot read a
//     device table, so the form is chosen per chunk on the device: a chunk that
//     lies inside one piece, does not pass count, and whose two byte addresses
//     are multiples of 16 moves as one nt global_load_dwordx4 per operand,
//     combine16, one nt global_store_dwordx4; any other chunk goes element by
//     element through batch_elem_at, each element stepping forward to its own
//     piece.  A lane looks up its units' pieces, then reads all their
//     byte offsets in one run (from LDS, or from the tables for a piece past
//     the span's 256th), then issues its vector loads together.
//
// 256 threads, 56 bytes of kernel arguments, 15 KiB of static LDS (eight
// workgroups' worth fits a CU), no scratch, no gridDim.
// ============================================================================
struct RaggedArgs {
    const char *in;             // the bases
    char *io;
    const int64_t *in_displs;   // npieces entries; null: packed
    const int64_t *io_displs;
    const int64_t *starts;      // npieces + 1 entries
    uint64_t disp_unit;         // bytes per displacement unit, > 0
    uint32_t npieces;           // > 0
    uint32_t count;             // packed elements, > 0
};

// count is an int at the public entry point: (2^31 - 1) elements of at most 32
// bytes are fewer than 2^22 spans of 16 KiB -- one launch always
static_assert(((uint64_t)INT32_MAX * 32 + kTileBytes - 1) / kTileBytes < kBatchMaxGroups,
              "a ragged reduction of INT_MAX elements must fit one launch");

// boundaries a workgroup keeps in LDS: 11 passes of 256, 11 KiB; and the byte
// offsets of the span's first 256 pieces on both sides, 4 KiB
constexpr uint32_t kRaggedLdsEntries = 11 * kThreads;
constexpr uint32_t kRaggedLdsOffsets = kThreads;
static_assert(kRaggedLdsEntries * sizeof(uint32_t) + 2 * kRaggedLdsOffsets * sizeof(uint64_t) <= (16u << 10),
              "static LDS of at most 16 KiB");

// the workgroups of a call, and the search's rounds: the least r with 64^r >= npieces + 1
inline uint64_t ragged_groups(uint64_t count, size_t esz) { return (count * esz + kTileBytes - 1) / kTileBytes; }
inline uint32_t ragged_search_rounds(uint64_t npieces) {
    uint32_t r = 0;
    for (uint64_t m = npieces + 1; m > 1; m = (m + 63) >> 6) ++r;
    return r;
}

// The largest p in [0, npieces] with starts[p] <= e0 (starts[0] == 0 makes one
// exist).  [lo, hi) holds it; a round probes lo + lane * step, step = ceil((hi -
// lo) / 64): the lanes whose entry is <= e0 are a prefix, c of them, and the
// answer lies in [lo + (c - 1) * step, lo + c * step).  Only lanes with a probe
// below hi count, so the new range is inside the old one whatever was loaded.
__device__ __forceinline__ uint32_t ragged_first_piece(const int64_t *starts, uint32_t npieces, uint64_t e0) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = 0, hi = npieces + 1;
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + 63) >> 6;
        const uint64_t q = (uint64_t)lo + (uint64_t)lane * step;
        const bool le = q < hi && starts[q] <= (int64_t)e0;
        uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(le));
        c = c ? c : 1;
        lo += (c - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
}

// what a workgroup knows of its span
struct RaggedSpan {
    const int64_t *starts;
    const uint32_t *bnd;    // LDS: min(starts[p0 + 1 + i] - e0, len), i < nvalid
    const uint64_t *off_in, *off_io;    // LDS: displs[p0 + i] * disp_unit, i < kRaggedLdsOffsets (sides with a table)
    uint32_t e0;            // the span's first packed element
    int32_t s0;             // starts[p0] - e0, <= 0
    uint32_t len;           // elements in the span (count clips the last)
    uint32_t p0;            // the span's first piece
    uint32_t nvalid;        // boundaries in LDS
    uint32_t npieces;
};
// a piece as a lane holds it: its index and its elements [s, e) relative to the
// span's first (e clipped to the span's length)
struct RaggedPiece {
    uint32_t k;
    int32_t s, e;
};

// starts[m] relative to the span, clipped to [0, len]; past the table: len
__device__ __forceinline__ int32_t ragged_bound(const RaggedSpan &w, uint64_t m) {
    const uint64_t i = m - w.p0 - 1;
    if (i < w.nvalid) return (int32_t)w.bnd[i];
    if (m > w.npieces) return (int32_t)w.len;
    const int64_t v = w.starts[m] - (int64_t)w.e0;
    return (int32_t)(v < 0 ? 0 : v < (int64_t)w.len ? v : (int64_t)w.len);
}

// The piece that holds element r of the span (r < len), from the boundaries in
// LDS; false where r lies beyond the last of them (p is then piece p0, a valid
// index to load by, and not r's piece).
__device__ __forceinline__ bool ragged_piece_lds(const RaggedSpan &w, uint32_t r, RaggedPiece &p) {
    uint32_t lo = 0, hi = w.nvalid;         // the boundaries <= r are bnd[0, lo)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (w.bnd[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < w.nvalid;
    const uint32_t j = found ? lo : 0;
    p.k = w.p0 + j;
    p.s = j ? (int32_t)w.bnd[j - 1] : w.s0;
    p.e = (int32_t)w.bnd[j];
    return found;
}

// ... and from the global table where LDS does not reach: the largest k in
// [p0 + nvalid, npieces] with starts[k] <= e0 + r, the range halved by index
__device__ __forceinline__ void ragged_piece_far(const RaggedSpan &w, uint32_t r, RaggedPiece &p) {
    uint64_t a = (uint64_t)w.p0 + w.nvalid, b = (uint64_t)w.npieces + 1;
    if (a > w.npieces) a = w.npieces;
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (w.starts[mid] <= (int64_t)((uint64_t)w.e0 + r)) a = mid;
        else b = mid;
    }
    p.k = (uint32_t)a;
    p.s = (int32_t)(w.starts[a] - (int64_t)w.e0);
    p.e = ragged_bound(w, a + 1);
}

// piece k's byte offset on one side: its table entry times disp_unit (wrapping
// as pointer arithmetic does), from LDS for the span's first pieces, or its
// packed place.  k is kept below npieces, the tables' length, whatever starts
// held.
__device__ __forceinline__ uint64_t ragged_off(const RaggedSpan &w, const int64_t *displs, const uint64_t *held,
                                               uint64_t disp_unit, const RaggedPiece &p, size_t esz) {
    if (!displs) return (uint64_t)((int64_t)w.e0 + p.s) * esz;
    const uint32_t k = p.k < w.npieces ? p.k : w.npieces - 1;
    const uint32_t j = k - w.p0;
    return j < kRaggedLdsOffsets ? held[j] : (uint64_t)displs[k] * disp_unit;
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_ragged(RaggedArgs a) {
    constexpr uint32_t per = kTileBytes / sizeof(T);                    // the span's elements
    constexpr uint32_t V = sizeof(T) <= 16 ? 16 / sizeof(T) : 1;        // a unit's elements
    constexpr int per_lane = (int)(per / V / kThreads);
    __shared__ uint32_t bnd[kRaggedLdsEntries];
    __shared__ uint64_t off_in[kRaggedLdsOffsets], off_io[kRaggedLdsOffsets];
    const unsigned t = threadIdx.x;
    const uint64_t e0 = (uint64_t)blockIdx.x * per;
    if (e0 >= a.count) return;
    RaggedSpan w;
    w.starts = a.starts;
    w.bnd = bnd;
    w.off_in = off_in;
    w.off_io = off_io;
    w.npieces = a.npieces;
    w.e0 = (uint32_t)e0;
    w.len = a.count - w.e0 < per ? a.count - w.e0 : per;
    w.p0 = ragged_first_piece(a.starts, a.npieces, e0);
    w.s0 = (int32_t)(a.starts[w.p0] - (int64_t)e0);
    // The first 256 boundaries after starts[p0], and with them the byte offsets
    // of pieces p0 ... p0 + 255 on the sides with a table: three loads at
    // indices kept inside the tables (a side with no table reads starts, and the
    // value is never used), none behind a branch, so that they leave together
    // and a lane that has found its unit's piece in LDS finds the piece's place
    // there too, not one more trip to memory away.
    {
        const uint64_t k = (uint64_t)w.p0 + t < a.npieces ? (uint64_t)w.p0 + t : a.npieces - 1;
        const uint64_t m = (uint64_t)w.p0 + 1 + t;
        const int64_t di = (a.in_displs ? a.in_displs : a.starts)[k];
        const int64_t dj = (a.io_displs ? a.io_displs : a.starts)[k];
        int64_t v = a.starts[m <= a.npieces ? m : a.npieces] - (int64_t)e0;
        v = m > a.npieces || v > (int64_t)w.len ? (int64_t)w.len : v < 0 ? 0 : v;
        off_in[t] = (uint64_t)di * a.disp_unit;
        off_io[t] = (uint64_t)dj * a.disp_unit;
        bnd[t] = (uint32_t)v;
    }
    w.nvalid = kThreads;
    __syncthreads();
    // further passes of 256 until a pass's last boundary has reached the span's
    // end (they do not decrease; past the table every entry is the end)
    while (bnd[w.nvalid - 1] < w.len && w.nvalid < kRaggedLdsEntries) {
        const uint64_t m = (uint64_t)w.p0 + 1 + w.nvalid + t;
        int64_t v = a.starts[m <= a.npieces ? m : a.npieces] - (int64_t)e0;
        v = m > a.npieces || v > (int64_t)w.len ? (int64_t)w.len : v < 0 ? 0 : v;
        bnd[w.nvalid + t] = (uint32_t)v;
        w.nvalid += kThreads;
        __syncthreads();
    }

    // bit j: the lane's unit j is still to do
    uint32_t todo = 0;
#pragma unroll
    for (int j = 0; j < per_lane; ++j) todo |= (uint32_t)((t + (uint32_t)j * kThreads) * V < w.len) << j;

    if constexpr (sizeof(T) <= 16) {
        // the chunks that can go as vectors: each unit's piece from LDS, then
        // both sides' displacement loads in one run (a packed side loads nothing),
        // then the data loads of the chunks that qualify
        RaggedPiece p[per_lane];
        uintptr_t pi[per_lane], po[per_lane];
        u32x4 x[per_lane], y[per_lane];
        bool vec[per_lane];
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uint32_t r = (t + (uint32_t)j * kThreads) * V;
            // inside one piece (whose end is clipped to the span's, and so to count)
            vec[j] = ragged_piece_lds(w, r < w.len ? r : w.len - 1, p[j]) && (todo >> j & 1) &&
                     (int32_t)(r + V) <= p[j].e;
        }
#pragma unroll
        for (int j = 0; j < per_lane; ++j) po[j] = ragged_off(w, a.io_displs, off_io, a.disp_unit, p[j], sizeof(T));
#pragma unroll
        for (int j = 0; j < per_lane; ++j) pi[j] = ragged_off(w, a.in_displs, off_in, a.disp_unit, p[j], sizeof(T));
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uint32_t r = (t + (uint32_t)j * kThreads) * V;
            const uint64_t d = (uint64_t)(int64_t)((int32_t)r - p[j].s) * sizeof(T);    // bytes into the piece
            pi[j] += reinterpret_cast<uintptr_t>(a.in) + d;
            po[j] += reinterpret_cast<uintptr_t>(a.io) + d;
            vec[j] = vec[j] && ((pi[j] | po[j]) & 15) == 0;
        }
        // No branch around the loads, so that all of a lane's leave together and
        // it waits once: a chunk that goes by elements loads the first 16 bytes
        // of starts instead (two entries, which every table has) and drops them.
        // Only the stores are guarded.
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uintptr_t spare = reinterpret_cast<uintptr_t>(a.starts);
            x[j] = __builtin_nontemporal_load(reinterpret_cast<const global_u32x4 *>(vec[j] ? po[j] : spare));
            y[j] = __builtin_nontemporal_load(reinterpret_cast<const global_u32x4 *>(vec[j] ? pi[j] : spare));
        }
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            if (vec[j]) {
                __builtin_nontemporal_store(combine16<Op, T>(x[j], y[j]), reinterpret_cast<global_u32x4 *>(po[j]));
                todo &= ~(1u << j);
            }
        }
    }
    // the other units, element by element: an element at or past its piece's end
    // steps to the next piece that holds one (empty pieces fall through)
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)per_lane; ++j) {
        if (!(todo >> j & 1)) continue;
        const uint32_t r = (t + j * kThreads) * V;
        RaggedPiece q;
        if (!ragged_piece_lds(w, r, q)) ragged_piece_far(w, r, q);
        uint64_t qi = ragged_off(w, a.in_displs, off_in, a.disp_unit, q, sizeof(T));
        uint64_t qo = ragged_off(w, a.io_displs, off_io, a.disp_unit, q, sizeof(T));
        for (uint32_t i = 0; i < V && r + i < w.len; ++i) {
            const int32_t e = (int32_t)(r + i);
            if (e >= q.e) {
                // (past the table every bound is the span's length, above e: the walk ends)
                do {
                    ++q.k;
                    q.s = q.e;
                    q.e = ragged_bound(w, (uint64_t)q.k + 1);
                } while (e >= q.e);
                qi = ragged_off(w, a.in_displs, off_in, a.disp_unit, q, sizeof(T));
                qo = ragged_off(w, a.io_displs, off_io, a.disp_unit, q, sizeof(T));
            }
            batch_elem_at<Op, T>(a.in + qi, a.io + qo, (uint64_t)(int64_t)(e - q.s));
        }
    }
}

// one launch, always: the grid is the packed elements' spans
template <class Op, class T>
hipError_t launch_ragged(const RaggedArgs *a, hipStream_t s) {
    const uint64_t groups = ragged_groups(a->count, sizeof(T));
    if (!a->npieces || !a->count || !a->disp_unit || !a->starts || groups < 1 || groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_ragged<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Fetching reductions (MPIR_Hip_reduce_fetch): fetch[i] = the bytes io[i] held,
// io[i] = op(io[i], in[i]), in ONE pass -- the target side of MPI_Get_accumulate
// and MPI_Fetch_and_op, which copies the target's old contents into the response
// buffer and then combines the origin's data into the target
// (ch3u_rma_pkthandler.c:899-917: "NOTE: 'copy data + ACC' needs to be atomic").
// A device copy followed by the single call reads inoutbuf twice, five streams
// through HBM; here the tile already holds each 16-byte vector of inoutbuf in
// registers before it combines, and storing that vector to a third buffer first
// adds no load and no arithmetic: four streams, one launch.
//
//   * One read of inoutbuf: the value stored to fetchbuf and the value combined
//     are the SAME registers, filled by one load of io[i] -- on the tile path
//     the vector a[u], on the element path the bytes `old`.  No second read of
//     inoutbuf exists in the kernel, so the reference's "copy + ACC is atomic"
//     holds by construction (nothing can come between a copy and a combine that
//     are one load).
//   * The fetched bytes are a byte copy: whole 16-byte vectors on the tile path,
//     an element's raw bytes on the element path (never a value of type T: NaN
//     payloads and the padding of the x87 slots and of the pair types arrive as
//     they were).
//   * Tile path: all three pointers naturally aligned and at one offset mod 16
//     (fetch_split: seg_split's condition and arithmetic, extended to the third
//     pointer).  reduce_fetch_tile is reduce_tile with a third buffer descriptor
//     at the same lo / nrec: the 16 KiB grid is inoutbuf's address grid, and
//     fetchbuf shares inoutbuf's offset mod 16, not necessarily mod 16 KiB, as
//     inbuf does.  Both stores are nt (keep = 0, as the batch and the strided
//     call store).  Tile 0 also takes the head and tail elements.
//   * Every other alignment, and the 32-byte classes: the element form,
//     workgroup g owning elements [g, g + 1) x kTileBytes / sizeof(T).
//   * fetch_split / batch_seg_groups are the one source of the split and the
//     workgroup count, on the host (fetch_plan) and on the device.
// 256 threads, 32 bytes of kernel arguments, no LDS, no scratch, no gridDim.
// ============================================================================
struct FetchArgs {
    const char *in;
    char *io;
    char *fetch;
    uint64_t count;     // elements, > 0
};

// count is an int at the public entry point: at most (2^31 - 1) elements of at
// most 32 bytes is below 2^36 bytes, so 2^22 tiles of 16 KiB plus the one a
// start off the grid adds -- one launch always stays below kBatchMaxGroups.
static_assert(((uint64_t)INT32_MAX * 32 + 2 * (uint64_t)kTileBytes) / kTileBytes < kBatchMaxGroups,
              "a fetching reduction of INT_MAX elements must fit one launch");

// seg_split of (in, io, count), and the tile path only if fetch sits at io's
// offset mod 16 as well (it is then naturally aligned where io is)
template <class T>
__host__ __device__ inline SegSplit fetch_split(const void *in, const void *io, const void *fetch, uint64_t count) {
    SegSplit s = seg_split<T>(in, io, count);
    if (s.tile && ((reinterpret_cast<uintptr_t>(fetch) ^ reinterpret_cast<uintptr_t>(io)) & 15) != 0)
        s = SegSplit{false, 0, 0, 0, 0};
    return s;
}

// element i: its bytes read once, stored to fetch as they are, then combined
template <class Op, class T>
__device__ __forceinline__ void fetch_elem_at(const char *in, char *io, char *fetch, uint64_t i) {
    struct Raw { unsigned char b[sizeof(T)]; };
    Op op;
    Raw old;
    T y;
    __builtin_memcpy(&old, io + i * sizeof(T), sizeof(T));
    __builtin_memcpy(&y, in + i * sizeof(T), sizeof(T));
    __builtin_memcpy(fetch + i * sizeof(T), &old, sizeof(T));
    const T x = op(__builtin_bit_cast(T, old), y);
    __builtin_memcpy(io + i * sizeof(T), &x, sizeof(T));
}

// reduce_tile with the loaded inoutbuf vectors also stored to fetch, through a
// descriptor of its own clipped where the other two are
template <class Op, class T>
__device__ __forceinline__ void reduce_fetch_tile(const char *in, char *io, char *fetch, uint64_t tile, uint64_t vbytes) {
    const int64_t start = (int64_t)(tile * kTileBytes) - (int64_t)tile_shift(io);
    const uint64_t lo = start > 0 ? (uint64_t)start : 0;
    if (lo >= vbytes) return;
    const uint64_t end = (uint64_t)(start + kTileBytes);
    const int nrec = (int)((end < vbytes ? end : vbytes) - lo);
    const int cut = (int)(lo - start);       // 0, or s for tile 0: lanes below it wrap out of range
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *)(in + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rio = __builtin_amdgcn_make_buffer_rsrc((void *)(io + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rfe = __builtin_amdgcn_make_buffer_rsrc((void *)(fetch + lo), 0, nrec, 0x00020000);
    const int t = (int)threadIdx.x;
    const int wb = (t >> 6) * (kVecPerLane * 1024) + (t & 63) * 16 - cut;
    u32x4 a[kVecPerLane], b[kVecPerLane];
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) {
        a[u] = __builtin_amdgcn_raw_buffer_load_b128(rio, wb + u * 1024, 0, kCachePolicyNT);
        b[u] = __builtin_amdgcn_raw_buffer_load_b128(rin, wb + u * 1024, 0, kCachePolicyNT);
        if (u + 1 < kVecPerLane) issue_gap();
    }
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) store16(a[u], rfe, wb + u * 1024, false);
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) store16(combine16<Op, T>(a[u], b[u]), rio, wb + u * 1024, false);
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_fetch(FetchArgs a) {
    const uint64_t tile = blockIdx.x;
    const SegSplit s = fetch_split<T>(a.in, a.io, a.fetch, a.count);
    if (tile >= batch_seg_groups<T>(s, a.io, a.count)) return;
    if constexpr (sizeof(T) <= 16) {
        if (s.tile) {
            reduce_fetch_tile<Op, T>(a.in + s.head_bytes, a.io + s.head_bytes, a.fetch + s.head_bytes, tile, s.vbytes);
            if (tile == 0) {
                const unsigned t = threadIdx.x;
                const uint64_t tail0 = (s.head_bytes + s.vbytes) / sizeof(T);
                if (t < s.nhead) fetch_elem_at<Op, T>(a.in, a.io, a.fetch, t);
                else if (t >= 64 && t - 64 < s.ntail) fetch_elem_at<Op, T>(a.in, a.io, a.fetch, tail0 + (t - 64));
            }
            return;
        }
    }
    constexpr uint64_t per = kTileBytes / sizeof(T);
    const uint64_t base = tile * per;
    const uint64_t end = base + per < a.count ? base + per : a.count;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads) fetch_elem_at<Op, T>(a.in, a.io, a.fetch, i);
}

// The plan of one fetching reduction: the path, the grid and tile 0's elements
// (MPIR_Hip_fetch_plan_info reports it, launch_fetch launches it)
struct FetchPlan {
    bool tile;
    uint64_t groups;
    uint32_t nhead, ntail;
};
template <class T>
void fetch_plan(const FetchArgs *a, FetchPlan *p) {
    const SegSplit s = fetch_split<T>(a->in, a->io, a->fetch, a->count);
    *p = FetchPlan{s.tile, batch_seg_groups<T>(s, a->io, a->count), s.nhead, s.ntail};
}

template <class Op, class T>
hipError_t launch_fetch(const FetchArgs *a, hipStream_t s) {
    FetchPlan p;
    fetch_plan<T>(a, &p);
    if (!a->count || p.groups < 1 || p.groups > kBatchMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_fetch<Op, T>), dim3((unsigned)p.groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Fetching ragged reductions (MPIR_Hip_reduce_fetch_ragged): the fetching
// reduction on a ragged target -- the shape of the reference's MPI_Get_accumulate
// target handler (ch3u_handle_recv_req.c:326-358, :1391-1423), which packs the
// derived-type target into the contiguous response buffer (MPIR_Segment_pack,
// :339-351) and then runs do_accumulate_op over the same target, piece by piece
// against the packed origin data (mpidrma.h:930-1021), under "NOTE: 'copy data +
// ACC' needs to be atomic".  in and fetch are packed (piece k at starts[k]
// elements), io has the displacement table:
//     fetch[starts[k] + i] = the bytes io_k[i] held,  io_k[i] = op(io_k[i], in[starts[k] + i])
// with io_k = io + io_displs[k] * disp_unit, i < starts[k + 1] - starts[k].
//
// k_reduce_ragged's machinery unchanged (ragged_first_piece, the LDS boundary
// passes, ragged_piece_lds / ragged_piece_far / ragged_bound / ragged_off) and
// its division of work: workgroup g owns packed elements [g, g + 1) x kTileBytes
// / sizeof(T), ragged_groups workgroups, one launch always.  One side has a
// table, so LDS holds the boundaries (11 KiB) and one array of offsets (2 KiB).
//
//   * One read of io: the value stored to fetch and the value combined are the
//     SAME registers, filled by one load of the target -- the vector x[j] of a
//     vector chunk, the bytes `old` of fetch_ragged_elem.  The kernel holds no
//     second load of io, as k_reduce_fetch holds none.
//   * The fetched bytes are a byte copy (whole vectors, or an element's raw
//     bytes; never a value of type T).
//   * A 16-byte chunk of packed space inside one piece and not past count moves
//     as a vector when its three byte addresses are multiples of 16.  The two
//     packed ones are base + a multiple of 16, so the host decides them once
//     (packed_aligned); the target's is decided here, per chunk.  A vector chunk
//     is one nt 16-byte load of io, one of in, an nt store of io's registers to
//     fetch and an nt store of combine16 to io.  No branch around the loads: a
//     chunk that goes by elements loads the first 16 bytes of starts instead.
//   * Every other chunk, and the 32-byte classes, element by element through
//     fetch_ragged_elem, each element stepping forward to its own piece.
//   * MPI_NO_OP and MPI_REPLACE are the byte functors OpFetchNoOp and
//     OpFetchSwap over RawBytes<size>, one kernel per element SIZE: NO_OP loads
//     no in and stores no io (a pack of the pieces into fetch), REPLACE stores
//     in's bytes (a swap).
//
// 256 threads, 64 bytes of kernel arguments, 13 KiB of static LDS, no scratch,
// no gridDim.
// ============================================================================
struct FetchRaggedArgs {
    const char *in;             // packed; never looked at by OpFetchNoOp
    char *io;                   // the target's base
    char *fetch;                // packed
    const int64_t *io_displs;   // npieces entries
    const int64_t *starts;      // npieces + 1 entries
    uint64_t disp_unit;         // bytes per displacement unit, > 0
    uint32_t npieces;           // > 0
    uint32_t count;             // packed elements, > 0
    uint32_t packed_aligned;    // in (where it is read) and fetch are multiples of 16
    uint32_t pad_;
};

static_assert(((uint64_t)INT32_MAX * 32 + kTileBytes - 1) / kTileBytes < kBatchMaxGroups,
              "a fetching ragged reduction of INT_MAX elements must fit one launch");
static_assert(kRaggedLdsEntries * sizeof(uint32_t) + kRaggedLdsOffsets * sizeof(uint64_t) == (13u << 10),
              "13 KiB of static LDS: the boundaries and one side's offsets");

// the two byte ops, and the element they move: size bytes of no type
struct OpFetchNoOp {};
struct OpFetchSwap {};
template <int N>
struct RawBytes { uint32_t __attribute__((ext_vector_type(N / 4))) v; };   // (one register value, no byte array)
template <>
struct RawBytes<1> { uint8_t v; };
template <>
struct RawBytes<2> { uint16_t v; };
template <>
struct RawBytes<4> { uint32_t v; };

template <class Op, class T>
__device__ __forceinline__ u32x4 fetch_ragged_combine16(u32x4 x, u32x4 y) {
    if constexpr (__is_same(Op, OpFetchSwap)) return y;
    else return combine16<Op, T>(x, y);
}

// one element: its bytes read once, stored to fetch as they are, then combined
// (NO_OP: nothing more; REPLACE: in's bytes stored)
template <class Op, class T>
__device__ __forceinline__ void fetch_ragged_elem(const char *in, char *io, char *fetch) {
    typedef RawBytes<(int)sizeof(T)> Raw;
    Raw old;
    __builtin_memcpy(&old, io, sizeof(T));
    if constexpr (__is_same(Op, OpFetchNoOp)) {
        __builtin_memcpy(fetch, &old, sizeof(T));
    } else if constexpr (__is_same(Op, OpFetchSwap)) {
        Raw y;
        __builtin_memcpy(&y, in, sizeof(T));
        __builtin_memcpy(fetch, &old, sizeof(T));
        __builtin_memcpy(io, &y, sizeof(T));
    } else {
        Op op;
        T y;
        __builtin_memcpy(&y, in, sizeof(T));
        __builtin_memcpy(fetch, &old, sizeof(T));
        const T x = op(__builtin_bit_cast(T, old), y);
        __builtin_memcpy(io, &x, sizeof(T));
    }
}

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_reduce_fetch_ragged(FetchRaggedArgs a) {
    constexpr bool no_op = __is_same(Op, OpFetchNoOp);
    constexpr uint32_t per = kTileBytes / sizeof(T);                    // the span's elements
    constexpr uint32_t V = sizeof(T) <= 16 ? 16 / sizeof(T) : 1;        // a unit's elements
    constexpr int per_lane = (int)(per / V / kThreads);
    __shared__ uint32_t bnd[kRaggedLdsEntries];
    __shared__ uint64_t off_io[kRaggedLdsOffsets];
    const unsigned t = threadIdx.x;
    const uint64_t e0 = (uint64_t)blockIdx.x * per;
    if (e0 >= a.count) return;
    RaggedSpan w;
    w.starts = a.starts;
    w.bnd = bnd;
    w.off_in = nullptr;         // (the packed sides have no offsets)
    w.off_io = off_io;
    w.npieces = a.npieces;
    w.e0 = (uint32_t)e0;
    w.len = a.count - w.e0 < per ? a.count - w.e0 : per;
    w.p0 = ragged_first_piece(a.starts, a.npieces, e0);
    w.s0 = (int32_t)(a.starts[w.p0] - (int64_t)e0);
    // the first 256 boundaries after starts[p0] and the byte offsets of pieces
    // p0 ... p0 + 255, two loads at indices kept inside the tables, none behind
    // a branch (k_reduce_ragged's first pass with one displacement side)
    {
        const uint64_t k = (uint64_t)w.p0 + t < a.npieces ? (uint64_t)w.p0 + t : a.npieces - 1;
        const uint64_t m = (uint64_t)w.p0 + 1 + t;
        const int64_t dj = a.io_displs[k];
        int64_t v = a.starts[m <= a.npieces ? m : a.npieces] - (int64_t)e0;
        v = m > a.npieces || v > (int64_t)w.len ? (int64_t)w.len : v < 0 ? 0 : v;
        off_io[t] = (uint64_t)dj * a.disp_unit;
        bnd[t] = (uint32_t)v;
    }
    w.nvalid = kThreads;
    __syncthreads();
    // further passes of 256 until a pass's last boundary has reached the span's end
    while (bnd[w.nvalid - 1] < w.len && w.nvalid < kRaggedLdsEntries) {
        const uint64_t m = (uint64_t)w.p0 + 1 + w.nvalid + t;
        int64_t v = a.starts[m <= a.npieces ? m : a.npieces] - (int64_t)e0;
        v = m > a.npieces || v > (int64_t)w.len ? (int64_t)w.len : v < 0 ? 0 : v;
        bnd[w.nvalid + t] = (uint32_t)v;
        w.nvalid += kThreads;
        __syncthreads();
    }

    // bit j: the lane's unit j is still to do
    uint32_t todo = 0;
#pragma unroll
    for (int j = 0; j < per_lane; ++j) todo |= (uint32_t)((t + (uint32_t)j * kThreads) * V < w.len) << j;
    // the span's first byte on the two packed sides
    const uint64_t pk0 = e0 * sizeof(T);

    if constexpr (sizeof(T) <= 16) {
        RaggedPiece p[per_lane];
        uintptr_t po[per_lane];
        u32x4 x[per_lane], y[per_lane];
        bool vec[per_lane];
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uint32_t r = (t + (uint32_t)j * kThreads) * V;
            // inside one piece (whose end is clipped to the span's, and so to count)
            vec[j] = ragged_piece_lds(w, r < w.len ? r : w.len - 1, p[j]) && (todo >> j & 1) &&
                     (int32_t)(r + V) <= p[j].e && a.packed_aligned;
        }
#pragma unroll
        for (int j = 0; j < per_lane; ++j) po[j] = ragged_off(w, a.io_displs, off_io, a.disp_unit, p[j], sizeof(T));
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uint32_t r = (t + (uint32_t)j * kThreads) * V;
            const uint64_t d = (uint64_t)(int64_t)((int32_t)r - p[j].s) * sizeof(T);    // bytes into the piece
            po[j] += reinterpret_cast<uintptr_t>(a.io) + d;
            vec[j] = vec[j] && (po[j] & 15) == 0;
        }
        // No branch around the loads (k_reduce_ragged's arrangement): a chunk that
        // goes by elements loads the first 16 bytes of starts and drops them.
        // x[j] is the ONE load of the target: it is stored to fetch and combined.
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            const uintptr_t spare = reinterpret_cast<uintptr_t>(a.starts);
            const uint64_t pk = pk0 + (uint64_t)(t + (uint32_t)j * kThreads) * 16;
            x[j] = __builtin_nontemporal_load(reinterpret_cast<const global_u32x4 *>(vec[j] ? po[j] : spare));
            if constexpr (!no_op)
                y[j] = __builtin_nontemporal_load(reinterpret_cast<const global_u32x4 *>(
                    vec[j] ? reinterpret_cast<uintptr_t>(a.in) + pk : spare));
        }
#pragma unroll
        for (int j = 0; j < per_lane; ++j) {
            if (vec[j]) {
                const uint64_t pk = pk0 + (uint64_t)(t + (uint32_t)j * kThreads) * 16;
                __builtin_nontemporal_store(x[j], reinterpret_cast<global_u32x4 *>(reinterpret_cast<uintptr_t>(a.fetch) + pk));
                if constexpr (!no_op)
                    __builtin_nontemporal_store(fetch_ragged_combine16<Op, T>(x[j], y[j]),
                                                reinterpret_cast<global_u32x4 *>(po[j]));
                todo &= ~(1u << j);
            }
        }
    }
    // the other units, element by element: an element at or past its piece's end
    // steps to the next piece that holds one (empty pieces fall through)
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)per_lane; ++j) {
        if (!(todo >> j & 1)) continue;
        const uint32_t r = (t + j * kThreads) * V;
        RaggedPiece q;
        if (!ragged_piece_lds(w, r, q)) ragged_piece_far(w, r, q);
        uint64_t qo = ragged_off(w, a.io_displs, off_io, a.disp_unit, q, sizeof(T));
        for (uint32_t i = 0; i < V && r + i < w.len; ++i) {
            const int32_t e = (int32_t)(r + i);
            if (e >= q.e) {
                // (past the table every bound is the span's length, above e: the walk ends)
                do {
                    ++q.k;
                    q.s = q.e;
                    q.e = ragged_bound(w, (uint64_t)q.k + 1);
                } while (e >= q.e);
                qo = ragged_off(w, a.io_displs, off_io, a.disp_unit, q, sizeof(T));
            }
            const uint64_t pk = pk0 + (uint64_t)(uint32_t)e * sizeof(T);
            fetch_ragged_elem<Op, T>(a.in + pk, a.io + qo + (uint64_t)(int64_t)(e - q.s) * sizeof(T), a.fetch + pk);
        }
    }
}

// one launch, always: the grid is the packed elements' spans
template <class Op, class T>
hipError_t launch_fetch_ragged(const FetchRaggedArgs *a, hipStream_t s) {
    const uint64_t groups = ragged_groups(a->count, sizeof(T));
    if (!a->npieces || !a->count || !a->disp_unit || !a->starts || !a->io_displs || groups < 1 ||
        groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_reduce_fetch_ragged<Op, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// ============================================================================
// Multi-operand combines: the log2(p) / (p-1) MPIR_Reduce_local steps of a
// reduction schedule fused into ONE pass over HBM, in the schedule's exact
// association and operand order (so results are bit-identical to running the
// reference schedule step by step).
//
//   TREE  (recursive halving: reduce_intra_reduce_scatter_gather.c:186-249,
//          allreduce_intra_reduce_scatter_allgather.c:150-215):
//          v_j = y_j; for l = 0..L-1: v_j = v_j (+) v_{j + 2^l}, j % 2^(l+1) == 0
//          i.e. ((y0+y1)+(y2+y3))+((y4+y5)+(y6+y7)), left operand = inout.
//          The caller orders y_j = contribution of newrank (owner ^ j).
//   CHAIN (pairwise: reduce_scatter_block_intra_pairwise.c:97-134):
//          acc = y0; acc = acc (+) y1; ...; acc = acc (+) y_{P-1}.
//
// One workgroup reads P x TILE bytes and writes TILE bytes; the lane keeps
// P 16-byte loads in flight (P x 1 KiB per wave-instruction group).
// ============================================================================
constexpr int kMaxOperands = 16;

struct MultiArgs {
    const char *in[kMaxOperands];   // 16 B-aligned vector regions, same alignment as out
    char *out;
    uint64_t vbytes;                // multiple of 16
    uint32_t nhead, ntail;          // scalar elements before / after the vector region
    int64_t head_off, tail_off;     // byte offsets of head / tail from the region starts
    uint64_t keep;                  // keep_for(vbytes)
};

template <class Op, class T, int P, bool TREE, bool RAW = false>
__device__ __forceinline__ void fold_elems(T (&v)[P]) {
    Op op;
    if constexpr (TREE) {
#pragma unroll
        for (int step = 1; step < P; step *= 2)
#pragma unroll
            for (int j = 0; j < P; j += 2 * step) {
                if constexpr (RAW) v[j] = Op::raw(v[j], v[j + step]);
                else v[j] = op(v[j], v[j + step]);
            }
    } else {
#pragma unroll
        for (int j = 1; j < P; ++j) {
            if constexpr (RAW) v[0] = Op::raw(v[0], v[j]);
            else v[0] = op(v[0], v[j]);
        }
    }
}

// fold with the fast path: plain arithmetic, then the exact x86-rule fold only
// if the result is NaN (a NaN anywhere in an add/mul tree reaches the root)
template <class Op, class T, int P, bool TREE>
__device__ __forceinline__ T fold_fast(const T (&v0)[P]) {
    T v[P];
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = v0[j];
    if constexpr (nan_fast<Op, T>::value) {
        fold_elems<Op, T, P, TREE, true>(v);
        if (__builtin_expect(!isnan_(v[0]), 1)) return v[0];
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = v0[j];
    }
    fold_elems<Op, T, P, TREE>(v);
    return v[0];
}

// tile `blk` of the fused fold (TH threads, U vectors per lane per operand)
template <class Op, class T, int P, bool TREE, int U, int TH>
__device__ __forceinline__ void combine_multi_tile(const MultiArgs &a, uint64_t blk) {
    constexpr uint32_t tile = TH * U * 16;
    const uint64_t base = blk * tile;
    if (base < a.vbytes) {
        const uint64_t left = a.vbytes - base;
        const int nrec = (int)(left < tile ? left : tile);
        // each wave owns a contiguous U KiB of every operand's tile (as in the
        // two-operand kernel); the loads go vector by vector across the P
        // operands with an issue gap after every (P == 2 ? 2 : 4) of them
        const int t = (int)threadIdx.x;
        const int wb = (t >> 6) * (U * 1024) + (t & 63) * 16;
        constexpr int GAP = P == 2 ? 2 : 4;
        u32x4 x[P][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < P; ++j) {
                __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)(a.in[j] + base), 0, nrec, 0x00020000);
                x[j][u] = __builtin_amdgcn_raw_buffer_load_b128(r, wb + u * 1024, 0, kCachePolicyNT);
                if ((u * P + j + 1) % GAP == 0 && u * P + j + 1 < U * P) issue_gap();
            }
        __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)(a.out + base), 0, nrec, 0x00020000);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            Pack16<T> pk[P];
#pragma unroll
            for (int j = 0; j < P; ++j) pk[j] = __builtin_bit_cast(Pack16<T>, x[j][u]);
            Pack16<T> res;
#pragma unroll
            for (int k = 0; k < (int)(16 / sizeof(T)); ++k) {
                T v[P];
#pragma unroll
                for (int j = 0; j < P; ++j) v[j] = pk[j].e[k];
                res.e[k] = fold_fast<Op, T, P, TREE>(v);
            }
            store16(__builtin_bit_cast(u32x4, res), ro, wb + u * 1024, keep_tile(base, a.vbytes, a.keep));
        }
    }
}

template <class Op, class T, int P, bool TREE, int U, int TH>
__global__ __launch_bounds__(TH) void k_combine_multi(MultiArgs a) {
    combine_multi_tile<Op, T, P, TREE, U, TH>(a, blockIdx.x);
    if (blockIdx.x == 0) {
        const unsigned t = threadIdx.x;
        int64_t off = 0;
        bool act = false;
        if (t < a.nhead) { off = a.head_off + (int64_t)(t * sizeof(T)); act = true; }
        else if (t >= 64 && t - 64 < a.ntail) { off = a.tail_off + (int64_t)((t - 64) * sizeof(T)); act = true; }
        if (act) {
            T v[P];
#pragma unroll
            for (int j = 0; j < P; ++j) v[j] = *reinterpret_cast<const T *>(a.in[j] + off);
            fold_elems<Op, T, P, TREE>(v);
            *reinterpret_cast<T *>(a.out + off) = v[0];
        }
    }
}

// Misaligned operands: element-granular grid-stride fallback.
template <class Op, class T, int P, bool TREE>
__global__ __launch_bounds__(kThreads) void k_combine_multi_elems(MultiArgs a, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        T v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) __builtin_memcpy(&v[j], a.in[j] + i * sizeof(T), sizeof(T));
        fold_elems<Op, T, P, TREE>(v);
        __builtin_memcpy(a.out + i * sizeof(T), &v[0], sizeof(T));
    }
}

// Fewer loads in flight per CU for the many-operand folds: a dynamic LDS
// reservation the kernel never touches caps the workgroups a CU holds.
//   * P = 8 (1024-thread workgroups): 96 KiB, one per CU instead of two, 128 KiB
//     of loads in flight per CU instead of 256.  The eight reads alone do not
//     gain: the write stream among them does (tools/fused_write_ab.hip,
//     tools/multi_occ_ab.hip, profiles/r04/fused_*.log, multi_occ_ab*.log).
//   * P = 4 (256 threads x 4 vectors): 53 KiB, three per CU (192 KiB in flight;
//     shape sweep: tools/multi_p24_occ_ab.hip, profiles/r04/multi_p24_occ_ab.log).
//   * P = 2: no cap (TREE2 loses 2 points under one, CHAIN2 moves by 0.3).
// Two library builds alternated (tools/multi_cap_ab.sh, profiles/r04/
// multi_cap_ab.log, four pairs per case, outputs identical), without -> with:
// TREE8 fp32 over 8 x 32 MiB 0.744-0.749 -> 0.750-0.757, CHAIN8 fp16 over
// 8 x 128 MiB 0.745-0.749 -> 0.762-0.764, TREE4 fp32 over 4 x 64 MiB
// 0.726-0.735 -> 0.756-0.758, CHAIN4 fp16 over 4 x 256 MiB 0.760-0.763 -> 0.809-0.813.
// 0 (no reservation) if the runtime refuses the attribute.
#ifndef MPIR_MULTI_CAP_LDS
#define MPIR_MULTI_CAP_LDS 1    // 0: no reservation (a build-time override for tools/multi_cap_ab.sh only)
#endif
template <int P, int TH>
constexpr int multi_cap_bytes() {
    // P = 5-7 (CHAIN folds of non-power-of-two rank counts) take P = 8's shape
    // and cap, P = 3 P = 4's: with the operands in one staging slab at
    // stage_stride() apart, as the collectives lay them, 1024 x 1 at one per CU
    // runs CHAIN5-7 0.765-0.773 against 0.749-0.762 for 256 x 4 at three per CU,
    // and CHAIN3 0.779 against 0.816 (tools/archive/chain_shape.hip chainslab,
    // profiles/r05/chainslab_shape.log).  (With one allocation per operand the
    // order reverses, also for P = 8 below 128 MiB: chain_shape.log,
    // p8_shape*.log against slab_shape.log; the library follows its collectives.)
    return !MPIR_MULTI_CAP_LDS ? 0
           : (P >= 5 && TH == 1024) ? (96 << 10)
           : ((P == 4 || P == 3) && TH == kThreads) ? (53 << 10) : 0;
}
// Per call (MPIR_Hip_combine_set_flags, MPIR_HIP_COMBINE_UNCAPPED): a fold
// that runs beside other kernels -- the device collectives' pipelined fold,
// overlapping RCCL's transfer kernels -- goes without the reservation, which
// would hold every CU to one of its workgroups and slow the kernels beside it
// (tools/archive/lds_cap_cost.hip).
bool multi_uncapped();      // the calling thread's flag (hip_reduce.hip)
template <class Op, class T, int P, bool TREE, int U, int TH>
size_t multi_lds_cap() {
    constexpr int cap = multi_cap_bytes<P, TH>();
    if constexpr (cap == 0) {
        return 0;
    } else {
        static const size_t v = hipFuncSetAttribute((const void *)k_combine_multi<Op, T, P, TREE, U, TH>,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    cap) == hipSuccess ? (size_t)cap : 0;
        return v;
    }
}

// The fused fold's split of `count` elements at `out`: head elements (to
// 16 B-align out) / a 16 B vector body / tail elements when every operand is
// naturally aligned and shares out's alignment mod 16 (vec_ok: k_combine_multi),
// else the element kernel over all of them (k_combine_multi_elems).
// launch_combine_pu launches it; MPIR_Hip_combine_plan_info reports it
// (Entry::split, kernel_table.hpp).
struct CombineSplit {
    bool vec_ok;
    uint64_t head;          // bytes before the vector region (at most the payload)
    uint64_t vbytes;        // multiple of 16
    uint32_t nhead, ntail;  // elements
};
template <class T>
void combine_split(const void *const *ins, int P, const void *out, uint64_t count, CombineSplit *c) {
    const uintptr_t ao = reinterpret_cast<uintptr_t>(out);
    const uint64_t nbytes = count * sizeof(T);
    bool vec_ok = (ao % alignof(T) == 0) && (((16 - (ao & 15)) & 15) % sizeof(T) == 0);
    for (int j = 0; j < P; ++j) {
        const uintptr_t ai = reinterpret_cast<uintptr_t>(ins[j]);
        vec_ok = vec_ok && (ai % alignof(T) == 0) && (((ai ^ ao) & 15) == 0);
    }
    c->vec_ok = vec_ok;
    c->head = c->vbytes = 0;
    c->nhead = c->ntail = 0;
    if (!vec_ok) return;
    uint64_t head = (16 - (ao & 15)) & 15;
    if (head > nbytes) head = nbytes;
    const uint64_t rest = nbytes - head, vbytes = rest & ~(uint64_t)15;
    c->head = head;
    c->vbytes = vbytes;
    c->nhead = (uint32_t)(head / sizeof(T));
    c->ntail = (uint32_t)((rest - vbytes) / sizeof(T));
}

template <class Op, class T, int P, bool TREE, int U, int TH>
hipError_t launch_combine_pu(const void *const *ins, void *out_, uint64_t count, hipStream_t s) {
    constexpr uint32_t tile = TH * U * 16;
    char *out = static_cast<char *>(out_);
    CombineSplit c;
    combine_split<T>(ins, P, out_, count, &c);
    MultiArgs a;
    for (int j = 0; j < kMaxOperands; ++j) a.in[j] = j < P ? static_cast<const char *>(ins[j]) : nullptr;
    if (c.vec_ok) {
        for (int j = 0; j < P; ++j) a.in[j] += c.head;
        a.out = out + c.head;
        a.vbytes = c.vbytes;
        a.keep = keep_for(c.vbytes);
        a.nhead = c.nhead;
        a.head_off = -(int64_t)c.head;              // head elements sit before the region start
        a.ntail = c.ntail;
        a.tail_off = (int64_t)c.vbytes;
        uint64_t grid = (c.vbytes + tile - 1) / tile;
        if (grid == 0) grid = 1;
        const size_t lds = multi_uncapped() ? 0 : multi_lds_cap<Op, T, P, TREE, U, TH>();
        hipLaunchKernelGGL((k_combine_multi<Op, T, P, TREE, U, TH>), dim3((unsigned)grid), dim3(TH), lds, s, a);
    } else {
        a.out = out;
        a.vbytes = 0;
        a.keep = 0;
        uint64_t grid = (count + kThreads - 1) / kThreads;
        if (grid > 4096) grid = 4096;
        if (grid == 0) grid = 1;
        hipLaunchKernelGGL((k_combine_multi_elems<Op, T, P, TREE>), dim3((unsigned)grid), dim3(kThreads), 0, s, a, count);
    }
    return hipGetLastError();
}

// Any (op, element class), any n <= 64, either order, in ONE pass with no
// device temporaries: the combine for the (op, type) pairs the fused
// k_combine_multi is not instantiated for (logical / bitwise ops, MAXLOC /
// MINLOC pairs, complex PROD, long double) and for n > 8.  Element-granular
// and grid-stride; the tree is evaluated left to right with a per-thread
// stack (a binary counter of partial results), which is the association
// ((y0+y1)+(y2+y3))+... with the earlier partial always the left operand.
// out may alias in[0]: every input of element i is read before out[i] is written.
constexpr int kMaxAnyOperands = 64;
struct AnyArgs {
    const char *in[kMaxAnyOperands];
    char *out;
    int n;
    int tree;
};

template <class Op, class T>
__global__ __launch_bounds__(kThreads) void k_combine_any(AnyArgs a, uint64_t count) {
    Op op;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride) {
        const uint64_t off = i * sizeof(T);
        T acc;
        __builtin_memcpy(&acc, a.in[0] + off, sizeof(T));
        if (!a.tree) {
            for (int j = 1; j < a.n; ++j) {
                T v;
                __builtin_memcpy(&v, a.in[j] + off, sizeof(T));
                acc = op(acc, v);
            }
        } else {
            T st[7];
            int lv[7];
            int sp = 0;
            for (int j = 0; j < a.n; ++j) {
                T v = acc;
                if (j) __builtin_memcpy(&v, a.in[j] + off, sizeof(T));
                int l = 0;
                while (sp > 0 && lv[sp - 1] == l) {
                    v = op(st[sp - 1], v);
                    --sp;
                    ++l;
                }
                st[sp] = v;
                lv[sp] = l;
                ++sp;
            }
            acc = st[0];
        }
        __builtin_memcpy(a.out + off, &acc, sizeof(T));
    }
}

template <class Op, class T>
hipError_t launch_combine_any(const void *const *ins, int n, int tree, void *out, uint64_t count, hipStream_t s) {
    if (n < 1 || n > kMaxAnyOperands || (tree && (n & (n - 1)))) return hipErrorInvalidValue;
    AnyArgs a;
    for (int j = 0; j < kMaxAnyOperands; ++j) a.in[j] = j < n ? static_cast<const char *>(ins[j]) : nullptr;
    a.out = static_cast<char *>(out);
    a.n = n;
    a.tree = tree;
    uint64_t grid = (count + kThreads - 1) / kThreads;
    if (grid > 8192) grid = 8192;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL((k_combine_any<Op, T>), dim3((unsigned)grid), dim3(kThreads), 0, s, a, count);
    return hipGetLastError();
}

template <class Op, class T, int P, bool TREE>
hipError_t launch_combine_p(const void *const *ins, void *out_, uint64_t count, hipStream_t s) {
    // (2, 4, 8 for TREE; every P of 2-8 for CHAIN: 5-7 in P = 8's shape, 3 in
    // P = 4's).  rocprofv3 trace, 32 MiB blocks (profiles/archive/r01s3_multi_shape_p24.log):
    // P = 8 on 1024-thread WGs (0.76-0.80 of peak); P = 4 with 4 vectors per lane
    // 0.78-0.80 (2 vectors: 0.72-0.74); P = 2 with 4 vectors per lane 0.74-0.76
    // P = 2 over blocks of 256 MiB or more (config 5's 2 x 512 MiB at 2 ranks) on
    // 1024 x 1, uncapped: 0.798-0.808 against 0.784-0.788 for 256 x 4 in the
    // staging slab; over 128 MiB the two tie (tools/archive/chain_shape.hip p2slab,
    // profiles/r05/p2slab*.log)
    if constexpr (P == 2) {
        if (count * sizeof(T) >= (256ull << 20))
            return launch_combine_pu<Op, T, 2, TREE, 1, 1024>(ins, out_, count, s);
    }
    return launch_combine_pu<Op, T, P, TREE, (P >= 5 ? 1 : 4), (P >= 5 ? 1024 : kThreads)>(ins, out_, count, s);
}

// ============================================================================
// Ordered compare-and-swap (MPIR_Hip_cas_indexed_ordered): `count` entries of
// ONE element each, the target side of MPI_Compare_and_swap many times over --
// the reference's handlers copy the old value out, call MPIR_Compare_equal and,
// where it is true, copy the origin value in, under the window lock
// (ch3u_rma_pkthandler.c:1166-1178, ch3u_handle_recv_req.c:1677,
// mpid_rma_shm.h:625-632).  origin, compare and result are packed by entry
// number; entry k's target is target + displs[k] * disp_unit.  For k = 0 ..
// count - 1 in that order:
//     result[k] = the bytes target_k holds;  if they equal compare[k]: target_k = origin[k]
// Equality is equality of the element's N bytes (every type MPIR_Compare_equal
// accepts is an integer, _Bool or a byte), so the kernels are per element SIZE
// over RawBytes<N>, N = 1, 2, 4, 8, never per type.
//
// k_cas_indexed_ordered<N>: one lane per sorted position, kCasPerGroup
// positions a workgroup (a lane's kCasPerLane positions a wave apart, their
// order and displacement loads issued in straight runs).
//   * Head test, clamping of every index read from a device `order`, and the
//     pos0 / nrows / count launch split are reduce_ordered_narrow's: position p
//     heads a run iff p == 0 or displs[order[p - 1]] != displs[order[p]]; a
//     run belongs entirely to its head, across workgroup and launch boundaries;
//     a null `order` is the identity.  Non-heads load two entries of each table
//     and nothing else.
//   * The head loads the target element ONCE into a register.  For each entry of
//     the run it stores the register to result[k] (nt), and where the register
//     equals compare[k] takes origin[k].  It stores the target once at the end
//     of the run, and only if some entry of the run swapped (a run of failed
//     compares writes no target byte; nothing can observe the difference).
//   * The run is walked kCasAhead positions at a time: the order entries of the
//     next positions load together, then their displacements, compare values
//     and origin values together (all three depend on the order entry alone),
//     and the selects follow in order -- two dependent round trips per
//     kCasAhead entries where an element-at-a-time loop pays three per entry.
//   * Every element access is memcpy-style: any target alignment works (odd byte
//     displacements with disp_unit 1), and unaligned packed bases.
// No LDS, no scratch, no gridDim.  72 bytes of kernel arguments.
//
// k_cas_contig<N> (displs null: element k is entry k, no entry repeats):
// k_reduce_fetch's structure with two more streams.  The 16 KiB tile grid sits
// on the target's address; the tile path is taken only where origin, compare
// and result all share the target's offset mod 16 and the target is naturally
// aligned (cas_split: fetch_split extended to the fourth pointer).  A lane loads
// the target, compare and origin vectors, stores the target vector to result and
// a per-element blend to the target; tile 0 takes the head and tail elements.
// Every other alignment: the element form, workgroup g owning elements [g, g +
// 1) x kTileBytes / N.  cas_split / batch_seg_groups are the one source of the
// split and the workgroup count for the planner (cas_plan) and the kernel.
// 256 threads, 40 bytes of kernel arguments, no LDS, no scratch, no gridDim.
// All stores nt.
// ============================================================================
// (a build-time override for tools/cas_ab.py's look-ahead comparison only)
#ifndef MPIR_CAS_AHEAD
#define MPIR_CAS_AHEAD 4
#endif
constexpr int kCasAhead = MPIR_CAS_AHEAD;
constexpr int kCasPerLane = 4;
constexpr uint32_t kCasPerGroup = kThreads * kCasPerLane;
static_assert(kCasAhead >= 1 && kCasAhead <= 8, "positions looked ahead of a run's current end");

struct CasArgs {
    const char *origin;         // packed: entry k at k * N
    const char *compare;        // packed
    char *target;
    const int64_t *displs;      // never null
    char *result;               // packed
    const int *order;           // sorted position -> entry number; null: the identity
    uint64_t disp_unit;         // bytes per displacement unit, > 0
    uint32_t count;             // entries of the whole call
    uint32_t pos0;              // this launch's first sorted position
    uint32_t nrows;             // sorted positions of this launch, > 0
    uint32_t pad_;
};

struct CasContigArgs {
    const char *origin;
    const char *compare;
    char *target;
    char *result;
    uint64_t count;             // elements, > 0
};

template <int N>
__device__ __forceinline__ bool cas_equal(const RawBytes<N> &x, const RawBytes<N> &y) {
    if constexpr (N == 8) return x.v[0] == y.v[0] && x.v[1] == y.v[1];     // all 64 bits
    else return x.v == y.v;
}

// the entry at sorted position p (p < count), clamped into the tables
__device__ __forceinline__ uint32_t cas_entry(const CasArgs &a, uint32_t p) {
    if (!a.order) return p;                                 // (uniform: a kernel argument)
    const uint32_t k = (uint32_t)a.order[p];
    return k < a.count ? k : a.count - 1;
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_cas_indexed_ordered(CasArgs a) {
    typedef RawBytes<N> Raw;
    const unsigned t = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * kCasPerGroup;
    // a position past the launch's last is clamped into it: its table loads need no branch
    const uint64_t last = a.nrows - 1;
    uint32_t pos[kCasPerLane], k[kCasPerLane], kp[kCasPerLane], kn[kCasPerLane];
    int64_t d[kCasPerLane], dp[kCasPerLane], dn[kCasPerLane];
    bool head[kCasPerLane];
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) {
        const uint64_t r = r0 + t + (uint64_t)j * kThreads;
        head[j] = r <= last;
        pos[j] = a.pos0 + (uint32_t)(head[j] ? r : last);
    }
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) k[j] = cas_entry(a, pos[j]);
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) kp[j] = cas_entry(a, pos[j] ? pos[j] - 1 : 0);
    // (the position after, with the same loads: a run of one ends without another round trip)
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) kn[j] = cas_entry(a, pos[j] + 1 < a.count ? pos[j] + 1 : pos[j]);
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) d[j] = a.displs[k[j]];
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) dp[j] = a.displs[kp[j]];
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) dn[j] = a.displs[kn[j]];
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) head[j] = head[j] && (pos[j] == 0 || d[j] != dp[j]);
    // only heads touch data: the target's element once, and their own entry's two values
    Raw x[kCasPerLane], c[kCasPerLane], o[kCasPerLane];
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) {
        if (!head[j]) continue;
        __builtin_memcpy(&x[j], a.target + (uint64_t)d[j] * a.disp_unit, N);
        __builtin_memcpy(&c[j], a.compare + (uint64_t)k[j] * N, N);
        __builtin_memcpy(&o[j], a.origin + (uint64_t)k[j] * N, N);
    }
#pragma unroll
    for (int j = 0; j < kCasPerLane; ++j) {
        if (!head[j]) continue;
        Raw v = x[j];
        ordered_fetch_store(a.result + (uint64_t)k[j] * N, v);
        bool swapped = cas_equal<N>(v, c[j]);
        if (swapped) v = o[j];
        bool more = dn[j] == d[j];
        for (uint32_t q = pos[j] + 1; more && q < a.count; q += kCasAhead) {
            uint32_t kq[kCasAhead];
            int64_t dq[kCasAhead];
            Raw cq[kCasAhead], oq[kCasAhead];
            // (a position past the table is clamped into it and not counted)
#pragma unroll
            for (int i = 0; i < kCasAhead; ++i) kq[i] = cas_entry(a, q + i < a.count ? q + i : a.count - 1);
#pragma unroll
            for (int i = 0; i < kCasAhead; ++i) dq[i] = a.displs[kq[i]];
#pragma unroll
            for (int i = 0; i < kCasAhead; ++i) __builtin_memcpy(&cq[i], a.compare + (uint64_t)kq[i] * N, N);
#pragma unroll
            for (int i = 0; i < kCasAhead; ++i) __builtin_memcpy(&oq[i], a.origin + (uint64_t)kq[i] * N, N);
#pragma unroll
            for (int i = 0; i < kCasAhead; ++i) {
                more = more && q + i < a.count && dq[i] == d[j];
                if (more) {
                    ordered_fetch_store(a.result + (uint64_t)kq[i] * N, v);
                    if (cas_equal<N>(v, cq[i])) {
                        v = oq[i];
                        swapped = true;
                    }
                }
            }
        }
        if (swapped) __builtin_memcpy(a.target + (uint64_t)d[j] * a.disp_unit, &v, N);
    }
}

// one launch: `groups` workgroups over sorted positions [pos0, pos0 + nrows)
template <int N>
hipError_t launch_cas_indexed_ordered(const CasArgs *a, uint64_t groups, hipStream_t s) {
    if (!a->nrows || !a->disp_unit || !a->displs || !a->origin || !a->compare || !a->target || !a->result ||
        (uint64_t)a->pos0 + a->nrows > a->count || groups != (a->nrows + kCasPerGroup - 1) / kCasPerGroup ||
        groups > kBatchMaxGroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_cas_indexed_ordered<N>), dim3((unsigned)groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

// fetch_split of (origin, target, result, count), and the tile path only if
// compare sits at the target's offset mod 16 as well
template <int N>
__host__ __device__ inline SegSplit cas_split(const void *origin, const void *compare, const void *target,
                                              const void *result, uint64_t count) {
    SegSplit s = fetch_split<RawBytes<N>>(origin, target, result, count);
    if (s.tile && ((reinterpret_cast<uintptr_t>(compare) ^ reinterpret_cast<uintptr_t>(target)) & 15) != 0)
        s = SegSplit{false, 0, 0, 0, 0};
    return s;
}

// element i: the target's bytes read once, stored to result as they are, then the select
template <int N>
__device__ __forceinline__ void cas_elem_at(const CasContigArgs &a, uint64_t i) {
    RawBytes<N> x, c;
    __builtin_memcpy(&x, a.target + i * N, N);
    __builtin_memcpy(&c, a.compare + i * N, N);
    ordered_fetch_store(a.result + i * N, x);
    if (cas_equal<N>(x, c)) {
        RawBytes<N> o;
        __builtin_memcpy(&o, a.origin + i * N, N);
        __builtin_memcpy(a.target + i * N, &o, N);
    }
}

// 16 bytes of N-byte elements: o's element where x's equals c's, else x's
template <int N>
__device__ __forceinline__ u32x4 cas_blend16(u32x4 x, u32x4 c, u32x4 o) {
    u32x4 r;
    if constexpr (N == 8) {
#pragma unroll
        for (int w = 0; w < 4; w += 2) {
            const bool eq = x[w] == c[w] && x[w + 1] == c[w + 1];
            r[w] = eq ? o[w] : x[w];
            r[w + 1] = eq ? o[w + 1] : x[w + 1];
        }
    } else if constexpr (N == 4) {
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] = x[w] == c[w] ? o[w] : x[w];
    } else {
        constexpr uint32_t field = (1u << (8 * N)) - 1;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t diff = x[w] ^ c[w];
            uint32_t m = 0;
#pragma unroll
            for (int b = 0; b < 4 / N; ++b) m |= (diff & (field << (8 * N * b))) ? 0u : field << (8 * N * b);
            r[w] = (o[w] & m) | (x[w] & ~m);
        }
    }
    return r;
}

// reduce_fetch_tile with a fourth descriptor: tile `tile` of the grid on the
// target's address, all four clipped alike
template <int N>
__device__ __forceinline__ void cas_tile(const char *origin, const char *compare, char *target, char *result,
                                         uint64_t tile, uint64_t vbytes) {
    const int64_t start = (int64_t)(tile * kTileBytes) - (int64_t)tile_shift(target);
    const uint64_t lo = start > 0 ? (uint64_t)start : 0;
    if (lo >= vbytes) return;
    const uint64_t end = (uint64_t)(start + kTileBytes);
    const int nrec = (int)((end < vbytes ? end : vbytes) - lo);
    const int cut = (int)(lo - start);       // 0, or s for tile 0: lanes below it wrap out of range
    __amdgpu_buffer_rsrc_t ror = __builtin_amdgcn_make_buffer_rsrc((void *)(origin + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rco = __builtin_amdgcn_make_buffer_rsrc((void *)(compare + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rta = __builtin_amdgcn_make_buffer_rsrc((void *)(target + lo), 0, nrec, 0x00020000);
    __amdgpu_buffer_rsrc_t rre = __builtin_amdgcn_make_buffer_rsrc((void *)(result + lo), 0, nrec, 0x00020000);
    const int t = (int)threadIdx.x;
    const int wb = (t >> 6) * (kVecPerLane * 1024) + (t & 63) * 16 - cut;
    u32x4 x[kVecPerLane], c[kVecPerLane], o[kVecPerLane];
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) {
        x[u] = __builtin_amdgcn_raw_buffer_load_b128(rta, wb + u * 1024, 0, kCachePolicyNT);
        c[u] = __builtin_amdgcn_raw_buffer_load_b128(rco, wb + u * 1024, 0, kCachePolicyNT);
        o[u] = __builtin_amdgcn_raw_buffer_load_b128(ror, wb + u * 1024, 0, kCachePolicyNT);
        if (u + 1 < kVecPerLane) issue_gap();
    }
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) store16(x[u], rre, wb + u * 1024, false);
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) store16(cas_blend16<N>(x[u], c[u], o[u]), rta, wb + u * 1024, false);
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_cas_contig(CasContigArgs a) {
    const uint64_t tile = blockIdx.x;
    const SegSplit s = cas_split<N>(a.origin, a.compare, a.target, a.result, a.count);
    if (tile >= batch_seg_groups<RawBytes<N>>(s, a.target, a.count)) return;
    if (s.tile) {
        cas_tile<N>(a.origin + s.head_bytes, a.compare + s.head_bytes, a.target + s.head_bytes, a.result + s.head_bytes,
                    tile, s.vbytes);
        if (tile == 0) {
            const unsigned t = threadIdx.x;
            const uint64_t tail0 = (s.head_bytes + s.vbytes) / N;
            if (t < s.nhead) cas_elem_at<N>(a, t);
            else if (t >= 64 && t - 64 < s.ntail) cas_elem_at<N>(a, tail0 + (t - 64));
        }
        return;
    }
    constexpr uint64_t per = kTileBytes / N;
    const uint64_t base = tile * per;
    const uint64_t end = base + per < a.count ? base + per : a.count;
    for (uint64_t i = base + threadIdx.x; i < end; i += kThreads) cas_elem_at<N>(a, i);
}

// The plan of one contiguous call: the path, the grid and tile 0's elements
// (MPIR_Hip_cas_plan_info reports it, launch_cas_contig launches it)
template <int N>
void cas_plan(const CasContigArgs *a, FetchPlan *p) {
    const SegSplit s = cas_split<N>(a->origin, a->compare, a->target, a->result, a->count);
    *p = FetchPlan{s.tile, batch_seg_groups<RawBytes<N>>(s, a->target, a->count), s.nhead, s.ntail};
}

template <int N>
hipError_t launch_cas_contig(const CasContigArgs *a, hipStream_t s) {
    FetchPlan p;
    cas_plan<N>(a, &p);
    if (!a->count || p.groups < 1 || p.groups > kBatchMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_cas_contig<N>), dim3((unsigned)p.groups), dim3(kThreads), 0, s, *a);
    return hipGetLastError();
}

}  // namespace mpir_hip
