// kernel_table.hpp -- the (op, element class) kernel tables of the C-ABI shim.
//
// g_table[op][elem].fn : the single-operand MPIR_Reduce_local launcher
//                        (k_reduce_tile / k_reduce_shift / k_reduce_elems, or the
//                        32-byte LDS-transpose kernel);
// g_table[op][elem].any: the one-pass n-operand combine (k_combine_any), the
//                        general path of MPIR_Hip_combine; REPLACE has none;
// g_table[op][elem].host: the same combine as a host loop over the same
//                        functors (reduce_ops.hpp), for small operands that
//                        both live in host memory (MPIR_Hip_reduce);
// g_multi[op][elem][order][P - 2]: the fused schedule combines
//                        (k_combine_multi) for the ops the collectives use most:
//                        TREE folds of P = 2, 4, 8 operands, CHAIN folds of every
//                        P from 2 to 8 (a pairwise chain over p ranks is one pass
//                        for any p <= 8).
// Storage lives in hip_reduce.hip (zero-initialised); the reg_*.hip units fill
// it from static constructors.  Which ops a class admits (src/include/
// mpir_op_util.h:263-364) is stated once, in the four MPIR_PAIRS_* lists at the
// end of this file, one per op group.  A unit is one macro call, MPIR_REG_UNIT or
// MPIR_REG_FAMILY_UNIT: one kernel family's reg_*<> template over one list, so a
// family is four units that compile in parallel, each its own code object.
// direct_tiles.hip expands the same lists into its kernels.  The fused folds
// (reg_multi*.hip), the byte ops of the fetching families and the CAS kernels
// are partitioned by size, not by op group, and keep lists of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpir_hip_reduce.h"
#include "reduce_kernels.hpp"

namespace mpir_hip {

typedef hipError_t (*launch_fn)(const void *, void *, uint64_t, hipStream_t);
typedef hipError_t (*any_fn)(const void *const *, int, int, void *, uint64_t, hipStream_t);
typedef hipError_t (*multi_fn)(const void *const *, void *, uint64_t, hipStream_t);
typedef void (*host_fn)(const void *, void *, uint64_t);
typedef void (*plan_fn)(const void *, void *, uint64_t, ReducePlan *);
typedef void (*split_fn)(const void *const *, int, const void *, uint64_t, CombineSplit *);
typedef hipError_t (*batch_fn)(const BatchArgs *, uint64_t, hipStream_t);
typedef uint64_t (*bgroups_fn)(const void *, const void *, uint64_t, int *);
typedef hipError_t (*strided_fn)(const StridedArgs *, uint64_t, hipStream_t);
typedef hipError_t (*subarray_fn)(const SubarrayArgs *, uint64_t, hipStream_t);
typedef hipError_t (*fetch_fn)(const FetchArgs *, hipStream_t);
typedef hipError_t (*indexed_fn)(const IndexedArgs *, uint64_t, hipStream_t);
typedef hipError_t (*ordered_fn)(const OrderedArgs *, uint64_t, hipStream_t);
typedef hipError_t (*chunked_fn)(const ChunkedArgs *, int, uint64_t, hipStream_t);
typedef hipError_t (*ragged_fn)(const RaggedArgs *, hipStream_t);
typedef void (*fplan_fn)(const FetchArgs *, FetchPlan *);
typedef hipError_t (*fetch_ragged_fn)(const FetchRaggedArgs *, hipStream_t);
typedef hipError_t (*fetch_ordered_fn)(const FetchOrderedArgs *, uint64_t, hipStream_t);
typedef hipError_t (*cas_fn)(const CasArgs *, uint64_t, hipStream_t);
typedef hipError_t (*cas_contig_fn)(const CasContigArgs *, hipStream_t);
typedef void (*cas_plan_fn)(const CasContigArgs *, FetchPlan *);

// plan: plan_reduce<T> (reduce_kernels.hpp) for the classes whose launcher is
// launch_reduce -- the kernel, grid and argument bytes the direct AQL dispatch
// launches from its code object; null for the 32-byte classes (LDS transpose)
// and REPLACE (a byte copy), which take the HIP launch.
// wide: plan_reduce_wide<T, EPL> for the 32-byte classes (what launch_reduce_wide
// launches); split: combine_split<T> for the pairs with fused folds (what
// launch_combine_pu launches).  Both are read by the plan introspection only.
struct Entry { launch_fn fn; any_fn any; host_fn host; plan_fn plan; plan_fn wide; split_fn split; };
// g_batch[op][elem], a table of its own beside g_table (whose layout stays as
// it was): launch = launch_batch<Op, T>, one launch of k_reduce_batch over a
// segment table (MPIR_Hip_reduce_batch), for every pair with fn but REPLACE;
// groups = batch_groups_any<T>, a segment's path and workgroup count for the
// batch's planner.
struct BatchEntry { batch_fn launch; bgroups_fn groups; };
// g_strided[op][elem], likewise a table of its own: launch_strided<Op, T>, one
// launch of k_reduce_strided over a range of rows (MPIR_Hip_reduce_strided), for
// the pairs g_batch holds (reg_strided<>, from the reg_strided_*.hip units); a
// row's path and workgroups are g_batch's `groups`.
struct StridedEntry { strided_fn launch; };
// g_subarray[op][elem], likewise: launch_subarray<Op, T>, one launch of
// k_reduce_subarray over a range of rows of a sub-box (MPIR_Hip_reduce_subarray),
// for the pairs g_strided holds (reg_subarray<>, from the reg_subarray_*.hip units).
struct SubarrayEntry { subarray_fn launch; };
// g_fetch[op][elem], likewise: launch_fetch<Op, T>, the one launch of
// k_reduce_fetch (MPIR_Hip_reduce_fetch), for the pairs g_batch holds
// (reg_fetch<>, from the reg_fetch_*.hip units); plan = fetch_plan<T>, the plan
// that launch makes, for MPIR_Hip_fetch_plan_info.  MPI_NO_OP and MPI_REPLACE
// are device copies and have no entry.
struct FetchEntry { fetch_fn launch; fplan_fn plan; };
// g_indexed[op][elem], likewise: launch_indexed<Op, T>, one launch of
// k_reduce_indexed over a range of blocks (MPIR_Hip_reduce_indexed), for the
// pairs g_batch holds (reg_indexed<>, from the reg_indexed_*.hip units).
struct IndexedEntry { indexed_fn launch; };
// g_ordered[op][elem], likewise: launch_indexed_ordered<Op, T>, one launch of
// k_reduce_indexed_ordered over a range of sorted positions
// (MPIR_Hip_reduce_indexed_ordered), for the pairs g_indexed holds
// (reg_ordered<>, from the reg_ordered_*.hip units).
struct OrderedEntry { ordered_fn launch; };
// g_chunked[op][elem], likewise: launch_indexed_chunked<Op, T>, one launch of
// k_chunk_partials or (fold != 0) k_fold_partials over a range of sorted
// positions (MPIR_Hip_reduce_indexed_chunked), for the pairs g_ordered holds
// (reg_chunked<>, from the reg_chunked_*.hip units).
struct ChunkedEntry { chunked_fn launch; };
// g_ragged[op][elem], likewise: launch_ragged<Op, T>, the one launch of
// k_reduce_ragged (MPIR_Hip_reduce_ragged), for the pairs g_indexed holds
// (reg_ragged<>, from the reg_ragged_*.hip units).
struct RaggedEntry { ragged_fn launch; };
// g_fetch_ragged[op][elem], likewise: launch_fetch_ragged<Op, T>, the one launch
// of k_reduce_fetch_ragged (MPIR_Hip_reduce_fetch_ragged), for the pairs g_ragged
// holds (reg_fetch_ragged<>, from the reg_fetch_ragged_*.hip units).
// g_fetch_ragged_bytes[which][log2 size]: the same kernel over the two byte
// functors, MPI_NO_OP (0) and MPI_REPLACE (1), one per element size from 1 to 32
// bytes (reg_fetch_ragged_bytes.hip): they take every element class of that size.
struct FetchRaggedEntry { fetch_ragged_fn launch; };
constexpr int kFetchRaggedSizes = 6;
// g_fetch_ordered[op][elem], likewise: launch_fetch_indexed_ordered<Op, T>, one
// launch of k_reduce_fetch_indexed_ordered over a range of sorted positions
// (MPIR_Hip_reduce_fetch_indexed_ordered), for the pairs g_ordered holds
// (reg_fetch_ordered<>, from the reg_fetch_ordered_*.hip units).
// g_fetch_ordered_bytes[which][log2 size]: the same kernel over the two byte
// functors, laid out as g_fetch_ragged_bytes is (reg_fetch_ordered_bytes.hip).
struct FetchOrderedEntry { fetch_ordered_fn launch; };
// g_cas[log2 size]: the ordered compare-and-swap kernels of one element size, 1 to
// 8 bytes (MPIR_Hip_cas_indexed_ordered; reg_cas.hip): launch =
// launch_cas_indexed_ordered<N>, one launch of k_cas_indexed_ordered over a range
// of sorted positions; contig = launch_cas_contig<N>, the one launch of
// k_cas_contig for a call with no table; plan = cas_plan<N>, the plan that launch
// makes, for MPIR_Hip_cas_plan_info.
struct CasEntry { cas_fn launch; cas_contig_fn contig; cas_plan_fn plan; };
constexpr int kCasSizes = 4;

// float / double SUM and PROD on the host: the SSE instruction itself.  The
// reference's loop `a[i] = a[i] + b[i]` (opsum.c:21-76, gcc -O2) is an
// addss/addsd (addps/addpd when vectorised) with a[i] -- inout -- as the first
// source, and x86 applies exactly the NaN rule that x86_result restates for
// the GPU: the first source if it is a NaN, else the second, quieted; the
// indefinite for an invalid operation; denormals kept (MXCSR default).  The
// operand order is pinned with inline asm because the compiler treats
// addpd/mulpd as commutative.  4 floats / 2 doubles per instruction instead
// of the functor's per-element NaN checks: 1024 doubles 1.0 -> 0.4 us
// (tools/host_small_latency.c).  Unaligned operands: movups/movupd.
template <bool Prod, class T>
inline bool host_sse(const char *pi, char *po, uint64_t n) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    typedef float v4f __attribute__((vector_size(16), aligned(1)));
    uint64_t i = 0;
    constexpr uint64_t per = 16 / sizeof(T);
    for (; i + per <= n; i += per) {
        v4f a, b;
        __builtin_memcpy(&a, po + i * sizeof(T), 16);
        __builtin_memcpy(&b, pi + i * sizeof(T), 16);
        if constexpr (sizeof(T) == 4) {
            if constexpr (Prod) asm("mulps %1, %0" : "+x"(a) : "x"(b));
            else asm("addps %1, %0" : "+x"(a) : "x"(b));
        } else {
            if constexpr (Prod) asm("mulpd %1, %0" : "+x"(a) : "x"(b));
            else asm("addpd %1, %0" : "+x"(a) : "x"(b));
        }
        __builtin_memcpy(po + i * sizeof(T), &a, 16);
    }
    for (; i < n; ++i) {
        T a, b;
        __builtin_memcpy(&a, po + i * sizeof(T), sizeof(T));
        __builtin_memcpy(&b, pi + i * sizeof(T), sizeof(T));
        if constexpr (sizeof(T) == 4) {
            if constexpr (Prod) asm("mulss %1, %0" : "+x"(a) : "x"(b));
            else asm("addss %1, %0" : "+x"(a) : "x"(b));
        } else {
            if constexpr (Prod) asm("mulsd %1, %0" : "+x"(a) : "x"(b));
            else asm("addsd %1, %0" : "+x"(a) : "x"(b));
        }
        __builtin_memcpy(po + i * sizeof(T), &a, sizeof(T));
    }
    return true;
#else
    return false;
#endif
}

// inout[i] = Op(inout[i], in[i]) on the host, element by element, through the
// device functors compiled for x86 (unaligned operands: memcpy'd elements)
template <class Op, class T>
void host_loop(const void *in, void *io, uint64_t n) {
    Op op;
    const char *pi = static_cast<const char *>(in);
    char *po = static_cast<char *>(io);
    if constexpr ((__is_same(T, float) || __is_same(T, double)) && (__is_same(Op, OpSum) || __is_same(Op, OpProd)))
        if (host_sse<__is_same(Op, OpProd), T>(pi, po, n)) return;
    for (uint64_t i = 0; i < n; ++i) {
        T a, b;
        __builtin_memcpy(&a, po + i * sizeof(T), sizeof(T));
        __builtin_memcpy(&b, pi + i * sizeof(T), sizeof(T));
        a = op(a, b);
        __builtin_memcpy(po + i * sizeof(T), &a, sizeof(T));
    }
}
extern Entry g_table[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern BatchEntry g_batch[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern StridedEntry g_strided[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern SubarrayEntry g_subarray[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern FetchEntry g_fetch[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern IndexedEntry g_indexed[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern OrderedEntry g_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern ChunkedEntry g_chunked[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern RaggedEntry g_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern FetchRaggedEntry g_fetch_ragged[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern FetchRaggedEntry g_fetch_ragged_bytes[2][kFetchRaggedSizes];
extern FetchOrderedEntry g_fetch_ordered[MPIR_HIP_NOPS][MPIR_HIP_NELEMS];
extern FetchOrderedEntry g_fetch_ordered_bytes[2][kFetchRaggedSizes];
extern CasEntry g_cas[kCasSizes];
constexpr int kMultiMaxP = 8;
extern multi_fn g_multi[MPIR_HIP_NOPS][MPIR_HIP_NELEMS][2][kMultiMaxP - 1];

template <class Op, class T>
void reg(int op, int elem) {
    g_table[op][elem].fn = &launch_reduce<Op, T>;
    g_table[op][elem].host = &host_loop<Op, T>;
    if constexpr (!__is_same(Op, OpReplace)) {
        g_table[op][elem].any = &launch_combine_any<Op, T>;
        g_table[op][elem].plan = &plan_reduce_any<T>;
        g_batch[op][elem] = BatchEntry{&launch_batch<Op, T>, &batch_groups_any<T>};
    }
}
template <class Op, class T, int EPL = 2>
void reg_wide(int op, int elem) {
    g_table[op][elem].fn = &launch_reduce_wide<Op, T, EPL>;
    g_table[op][elem].wide = &plan_reduce_wide<T, EPL>;
    g_table[op][elem].host = &host_loop<Op, T>;
    g_table[op][elem].any = &launch_combine_any<Op, T>;
    g_batch[op][elem] = BatchEntry{&launch_batch<Op, T>, &batch_groups_any<T>};
}
// the strided kernel of a pair reg<> / reg_wide<> registers (REPLACE has none).
// Called from units of their own, reg_strided_*.hip, one beside each reg_*.hip
// with that unit's list of pairs: the code objects of the single call's, the
// batch's and the folds' kernels stay what they were without this entry point.
template <class Op, class T>
void reg_strided(int op, int elem) {
    g_strided[op][elem] = StridedEntry{&launch_strided<Op, T>};
}
// the subarray kernel of the same pairs, from the reg_subarray_*.hip units
template <class Op, class T>
void reg_subarray(int op, int elem) {
    g_subarray[op][elem] = SubarrayEntry{&launch_subarray<Op, T>};
}
// the fetching kernel of the same pairs, from the reg_fetch_*.hip units
template <class Op, class T>
void reg_fetch(int op, int elem) {
    g_fetch[op][elem] = FetchEntry{&launch_fetch<Op, T>, &fetch_plan<T>};
}
// the indexed kernel of the same pairs, from the reg_indexed_*.hip units
template <class Op, class T>
void reg_indexed(int op, int elem) {
    g_indexed[op][elem] = IndexedEntry{&launch_indexed<Op, T>};
}
// the ordered indexed kernel of the same pairs, from the reg_ordered_*.hip units
template <class Op, class T>
void reg_ordered(int op, int elem) {
    g_ordered[op][elem] = OrderedEntry{&launch_indexed_ordered<Op, T>};
}
// the two chunked indexed kernels of the same pairs, from the reg_chunked_*.hip units
template <class Op, class T>
void reg_chunked(int op, int elem) {
    g_chunked[op][elem] = ChunkedEntry{&launch_indexed_chunked<Op, T>};
}
// the ragged kernel of the same pairs, from the reg_ragged_*.hip units
template <class Op, class T>
void reg_ragged(int op, int elem) {
    g_ragged[op][elem] = RaggedEntry{&launch_ragged<Op, T>};
}
// the fetching ragged kernel of the same pairs, from the reg_fetch_ragged_*.hip units
template <class Op, class T>
void reg_fetch_ragged(int op, int elem) {
    g_fetch_ragged[op][elem] = FetchRaggedEntry{&launch_fetch_ragged<Op, T>};
}
// ... and of MPI_NO_OP and MPI_REPLACE on elements of 1 << LOG2 bytes
template <int LOG2>
void reg_fetch_ragged_bytes() {
    static_assert(LOG2 >= 0 && LOG2 < kFetchRaggedSizes, "element sizes 1 to 32 bytes");
    g_fetch_ragged_bytes[0][LOG2] = FetchRaggedEntry{&launch_fetch_ragged<OpFetchNoOp, RawBytes<(1 << LOG2)>>};
    g_fetch_ragged_bytes[1][LOG2] = FetchRaggedEntry{&launch_fetch_ragged<OpFetchSwap, RawBytes<(1 << LOG2)>>};
}
// the fetching ordered indexed kernel of the pairs reg_ordered<> registers, from
// the reg_fetch_ordered_*.hip units
template <class Op, class T>
void reg_fetch_ordered(int op, int elem) {
    g_fetch_ordered[op][elem] = FetchOrderedEntry{&launch_fetch_indexed_ordered<Op, T>};
}
// ... and of MPI_NO_OP and MPI_REPLACE on elements of 1 << LOG2 bytes
template <int LOG2>
void reg_fetch_ordered_bytes() {
    static_assert(LOG2 >= 0 && LOG2 < kFetchRaggedSizes, "element sizes 1 to 32 bytes");
    g_fetch_ordered_bytes[0][LOG2] = FetchOrderedEntry{&launch_fetch_indexed_ordered<OpFetchNoOp, RawBytes<(1 << LOG2)>>};
    g_fetch_ordered_bytes[1][LOG2] = FetchOrderedEntry{&launch_fetch_indexed_ordered<OpFetchSwap, RawBytes<(1 << LOG2)>>};
}
// the ordered compare-and-swap kernels of elements of 1 << LOG2 bytes, from reg_cas.hip
template <int LOG2>
void reg_cas() {
    static_assert(LOG2 >= 0 && LOG2 < kCasSizes, "element sizes 1 to 8 bytes");
    g_cas[LOG2] = CasEntry{&launch_cas_indexed_ordered<(1 << LOG2)>, &launch_cas_contig<(1 << LOG2)>, &cas_plan<(1 << LOG2)>};
}
template <class Op, class T>
void reg_multi(int op, int elem) {
    g_table[op][elem].split = &combine_split<T>;
    g_multi[op][elem][0][2 - 2] = &launch_combine_p<Op, T, 2, true>;
    g_multi[op][elem][0][4 - 2] = &launch_combine_p<Op, T, 4, true>;
    g_multi[op][elem][0][8 - 2] = &launch_combine_p<Op, T, 8, true>;
    g_multi[op][elem][1][2 - 2] = &launch_combine_p<Op, T, 2, false>;
    g_multi[op][elem][1][3 - 2] = &launch_combine_p<Op, T, 3, false>;
    g_multi[op][elem][1][4 - 2] = &launch_combine_p<Op, T, 4, false>;
    g_multi[op][elem][1][5 - 2] = &launch_combine_p<Op, T, 5, false>;
    g_multi[op][elem][1][6 - 2] = &launch_combine_p<Op, T, 6, false>;
    g_multi[op][elem][1][7 - 2] = &launch_combine_p<Op, T, 7, false>;
    g_multi[op][elem][1][8 - 2] = &launch_combine_p<Op, T, 8, false>;
}

}  // namespace mpir_hip

// Element classes and their device types: X(E, T) for each class of the group;
// whatever follows X in the call is handed on to it as further arguments.
#define FOR_INTS(X, ...) \
    X(MPIR_HIP_I8, int8_t, ##__VA_ARGS__) X(MPIR_HIP_U8, uint8_t, ##__VA_ARGS__) \
    X(MPIR_HIP_I16, int16_t, ##__VA_ARGS__) X(MPIR_HIP_U16, uint16_t, ##__VA_ARGS__) \
    X(MPIR_HIP_I32, int32_t, ##__VA_ARGS__) X(MPIR_HIP_U32, uint32_t, ##__VA_ARGS__) \
    X(MPIR_HIP_I64, int64_t, ##__VA_ARGS__) X(MPIR_HIP_U64, uint64_t, ##__VA_ARGS__)
#define FOR_REALS(X, ...) \
    X(MPIR_HIP_F16, f16, ##__VA_ARGS__) X(MPIR_HIP_F32, float, ##__VA_ARGS__) X(MPIR_HIP_F64, double, ##__VA_ARGS__)
#define FOR_CPLX(X, ...) X(MPIR_HIP_CF32, cf32, ##__VA_ARGS__) X(MPIR_HIP_CF64, cf64, ##__VA_ARGS__)
#define FOR_PAIRS(X, ...) \
    X(MPIR_HIP_P2INT, p2int, ##__VA_ARGS__) X(MPIR_HIP_PFLOATINT, pfloatint, ##__VA_ARGS__) \
    X(MPIR_HIP_PLONGINT, plongint, ##__VA_ARGS__) X(MPIR_HIP_PSHORTINT, pshortint, ##__VA_ARGS__) \
    X(MPIR_HIP_PDOUBLEINT, pdoubleint, ##__VA_ARGS__)

// The (op, class) pairs that have kernels, stated once: four lists, one per op
// group, which is also one registration unit per kernel family (they compile in
// parallel).  Each list calls, in the order the kernels are instantiated,
//   R(Op, OPN, E, T)       for a pair on the ordinary launcher,
//   W(Op, OPN, E, T, EPL)  for a pair of the 32-byte classes on the wide one;
// Op is the functor, OPN its bare name (MPIR_HIP_OP_##OPN is the op's index,
// and direct_tiles.hip pastes OPN into its kernels' names), E the class, T its
// device type.  118 pairs, 114 of them on R.  MPI_REPLACE, a byte copy of every
// class and of the single call alone, is in no list (reg_pairs_x87.hip).
#define MPIR_OPS_SUM_PROD_(E, T, R) R(OpSum, SUM, E, T) R(OpProd, PROD, E, T)
#define MPIR_OPS_MAX_MIN_(E, T, R) R(OpMax, MAX, E, T) R(OpMin, MIN, E, T)
#define MPIR_OPS_LOGICAL_(E, T, R) R(OpLand, LAND, E, T) R(OpLor, LOR, E, T) R(OpLxor, LXOR, E, T)
#define MPIR_OPS_LXOR_(E, T, R) R(OpLxor, LXOR, E, T)
#define MPIR_OPS_BITWISE_(E, T, R) R(OpBand, BAND, E, T) R(OpBor, BOR, E, T) R(OpBxor, BXOR, E, T)
#define MPIR_OPS_LOC_(E, T, R) R(OpMaxloc, MAXLOC, E, T) R(OpMinloc, MINLOC, E, T)
// MPI_SUM / MPI_PROD (opsum.c:21-76, opprod.c:21-96): C_INTEGER, FORTRAN_INTEGER,
// FLOATING_POINT (+EXTRA: char, _Float16), COMPLEX
#define MPIR_PAIRS_SUM_PROD(R, W) \
    FOR_INTS(MPIR_OPS_SUM_PROD_, R) FOR_REALS(MPIR_OPS_SUM_PROD_, R) FOR_CPLX(MPIR_OPS_SUM_PROD_, R)
// MPI_MAX / MPI_MIN (opmax.c:20-55, opmin.c:19-54): integers and reals, no complex
#define MPIR_PAIRS_MAX_MIN(R, W) FOR_INTS(MPIR_OPS_MAX_MIN_, R) FOR_REALS(MPIR_OPS_MAX_MIN_, R)
// LAND / LOR (opland.c, oplor.c: integers and _Bool as u8), LXOR (oplxor.c: also
// the reals, :66-67), BAND / BOR / BXOR (opband.c, opbor.c, opbxor.c: integers and byte)
#define MPIR_PAIRS_LOGIC(R, W) \
    FOR_INTS(MPIR_OPS_LOGICAL_, R) FOR_REALS(MPIR_OPS_LXOR_, R) FOR_INTS(MPIR_OPS_BITWISE_, R)
// MAXLOC / MINLOC on the pair types (opmaxloc.c:79, opminloc.c:78) and the long
// double rows computed as x87 in software (FLOATING_POINT: SUM, PROD, MAX, MIN,
// LXOR; its _Complex: SUM, PROD; MPI_LONG_DOUBLE_INT: MAXLOC, MINLOC)
#define MPIR_PAIRS_PAIRS_X87(R, W) \
    FOR_PAIRS(MPIR_OPS_LOC_, R) \
    MPIR_OPS_SUM_PROD_(MPIR_HIP_F80, x80, R) MPIR_OPS_MAX_MIN_(MPIR_HIP_F80, x80, R) MPIR_OPS_LXOR_(MPIR_HIP_F80, x80, R) \
    W(OpSum, SUM, MPIR_HIP_CF80, cx80, 2) W(OpProd, PROD, MPIR_HIP_CF80, cx80, 1) \
    W(OpMaxloc, MAXLOC, MPIR_HIP_PLDOUBLEINT, pldint, 2) W(OpMinloc, MINLOC, MPIR_HIP_PLDOUBLEINT, pldint, 2)

// A registration unit: the static constructor that fills one family's table from
// one list.  MPIR_REG_UNIT(reg, reg_wide, LIST) is the single call's unit;
// MPIR_REG_FAMILY_UNIT(reg_strided, LIST) a unit of a family with one launcher,
// which takes the wide pairs as it takes the others (EPL is the wide launcher's
// alone).  The callbacks handed to the list are a template's name followed by the
// macro that writes its arguments.
#define MPIR_REG_R_(Op, OPN, E, T) <Op, T>(MPIR_HIP_OP_##OPN, E);
#define MPIR_REG_W_(Op, OPN, E, T, EPL) <Op, T, EPL>(MPIR_HIP_OP_##OPN, E);
#define MPIR_REG_W1_(Op, OPN, E, T, EPL) <Op, T>(MPIR_HIP_OP_##OPN, E);
#define MPIR_REG_INIT_(R, W, LIST) \
    namespace {                    \
    struct Init {                  \
        Init() { LIST(R, W) }      \
    } init;                        \
    }
#define MPIR_REG_UNIT(narrow, wide, LIST) MPIR_REG_INIT_(narrow MPIR_REG_R_, wide MPIR_REG_W_, LIST)
#define MPIR_REG_FAMILY_UNIT(family, LIST) MPIR_REG_INIT_(family MPIR_REG_R_, family MPIR_REG_W1_, LIST)
