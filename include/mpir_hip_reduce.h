/*
 * mpir_hip_reduce.h -- the thin C-ABI shim between MPICH's host C op layer
 * and the gfx950 HIP kernels.  Plain pointers and sizes only.
 *
 * The host C layer (the C files under mpich-pip_amd/csrc/host) keeps the reference's
 * structure: MPIR_SUM(invec, inoutvec, len, type) switches over the MPI
 * datatype exactly like src/mpi/coll/op/opsum.c:21-76, and where the
 * reference runs its scalar loop (MPIR_OP_TYPE_REDUCE_CASE,
 * src/include/mpir_op_util.h:48-55) it calls MPIR_Hip_reduce() with the
 * resolved (op, element class) pair instead.
 */
#ifndef MPIR_HIP_REDUCE_H_INCLUDED
#define MPIR_HIP_REDUCE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* op codes == the reference's MPIR_Op_table index (allreduce.c:121-129) */
enum MPIR_Hip_op {
    MPIR_HIP_OP_MAX = 1,
    MPIR_HIP_OP_MIN = 2,
    MPIR_HIP_OP_SUM = 3,
    MPIR_HIP_OP_PROD = 4,
    MPIR_HIP_OP_LAND = 5,
    MPIR_HIP_OP_BAND = 6,
    MPIR_HIP_OP_LOR = 7,
    MPIR_HIP_OP_BOR = 8,
    MPIR_HIP_OP_LXOR = 9,
    MPIR_HIP_OP_BXOR = 10,
    MPIR_HIP_OP_MINLOC = 11,
    MPIR_HIP_OP_MAXLOC = 12,
    MPIR_HIP_OP_REPLACE = 13,
    MPIR_HIP_NOPS = 14
};

/* element classes: the device storage type an MPI basic type maps to */
enum MPIR_Hip_elem {
    MPIR_HIP_I8 = 1, MPIR_HIP_U8, MPIR_HIP_I16, MPIR_HIP_U16,
    MPIR_HIP_I32, MPIR_HIP_U32, MPIR_HIP_I64, MPIR_HIP_U64,
    MPIR_HIP_F16, MPIR_HIP_F32, MPIR_HIP_F64,
    MPIR_HIP_CF32, MPIR_HIP_CF64,                 /* C float/double _Complex */
    MPIR_HIP_P2INT, MPIR_HIP_PFLOATINT, MPIR_HIP_PLONGINT,
    MPIR_HIP_PSHORTINT, MPIR_HIP_PDOUBLEINT,      /* MAXLOC/MINLOC pairs */
    MPIR_HIP_F80, MPIR_HIP_CF80,                  /* x87 long double (16 B slot), its _Complex */
    MPIR_HIP_PLDOUBLEINT,                         /* MPI_LONG_DOUBLE_INT pair (32 B) */
    MPIR_HIP_NELEMS
};

/* return codes */
#define MPIR_HIP_OK        0
#define MPIR_HIP_EBUFFER   1   /* host-only pointer where device memory is required */
#define MPIR_HIP_ERUNTIME  2   /* HIP runtime failure; see MPIR_Hip_error_string() */
#define MPIR_HIP_ENOKERNEL 3   /* (op, elem) pair has no kernel */
#define MPIR_HIP_ENODEV    4   /* no usable GPU */
#define MPIR_HIP_EARG      5   /* an argument out of range (MPIR_Hip_reduce_strided's strides, MPIR_Hip_reduce_indexed's and MPIR_Hip_reduce_ragged's disp_unit, offsets and tables, MPIR_Hip_reduce_indexed_ordered's order table, MPIR_Hip_reduce_indexed_chunked's tables and work_bytes, MPIR_Hip_order_build's work_bytes) */

/* Combine inoutbuf[i] = op(inoutbuf[i], inbuf[i]) for i < count elements of
 * class `elem`.  Pointers may be device, pinned-host or pageable-host memory
 * in any mix (host operands are staged through device scratch).
 * hip_stream: a hipStream_t, or NULL for the calling thread's library stream
 * on the device that owns inoutbuf.  sync != 0: wait for completion (and for
 * the copy-back of a host inoutbuf) before returning.  sync == 0 requires
 * both buffers device-resident on one device (else MPIR_HIP_EBUFFER). */
int MPIR_Hip_reduce(const void *inbuf, void *inoutbuf, uint64_t count, int op, int elem,
                    void *hip_stream, int sync);

/* Multi-operand combine: outbuf = fold(inbufs[0..n-1]) in one pass, in the
 * association of a reduction schedule (the schedule's MPIR_Reduce_local steps
 * fused; left operand = the step's inoutbuf):
 *   MPIR_HIP_ORDER_TREE  (n a power of two <= 64; one fused pass for n <= 8):
 *       ((y0+y1)+(y2+y3))+((y4+y5)+(y6+y7)),
 *       the recursive-halving order of reduce_intra_reduce_scatter_gather.c;
 *   MPIR_HIP_ORDER_CHAIN (1 <= n <= 64): ((y0+y1)+y2)+..., the pairwise order
 *       of reduce_scatter_block_intra_pairwise.c.
 * All buffers device-resident on one device; outbuf may alias inbufs[0]. */
#define MPIR_HIP_ORDER_TREE  0
#define MPIR_HIP_ORDER_CHAIN 1
int MPIR_Hip_combine(const void *const *inbufs, int n, void *outbuf, uint64_t count, int op, int elem,
                     int order, void *hip_stream, int sync);

/* For tests and tools: the launch plan MPIR_Hip_reduce would take for device
 * operands at these addresses, from the same planner the launch calls -- host
 * arithmetic on the pointer values only (they are never dereferenced or
 * classified; no GPU is needed).  out = {kind, groups, nhead, ntail, vbytes,
 * keep}: the plan kind below, its grid in workgroups, the elements workgroup 0
 * combines before / after the 16-byte vector region, that region's bytes, and
 * the bytes of it stored sc1 (0: all nt; MPIR_Hip_set_keep_bytes).  The element
 * kinds report nhead = ntail = vbytes = keep = 0.  MPIR_HIP_ENOKERNEL where
 * (op, elem) has no planned kernel (REPLACE's byte copy included). */
#define MPIR_HIP_PLAN_LEAN        0   /* tile kernel, no head / tail */
#define MPIR_HIP_PLAN_FULL        1   /* tile kernel with head / tail elements */
#define MPIR_HIP_PLAN_SHIFT       2   /* inbuf at another offset mod 16 than inoutbuf, >= 2 tiles */
#define MPIR_HIP_PLAN_ELEMS       3   /* element kernel, naturally aligned */
#define MPIR_HIP_PLAN_ELEMS_U     4   /* element kernel, unaligned elements */
#define MPIR_HIP_PLAN_WIDE_TILE   5   /* 32-byte classes: LDS-transpose tile kernel */
#define MPIR_HIP_PLAN_WIDE_ELEMS  6   /* 32-byte classes off 16 B alignment: element kernel */
int MPIR_Hip_plan_info(const void *inbuf, const void *inoutbuf, uint64_t count, int op, int elem, uint64_t out[6]);

/* For tests and tools: the same for MPIR_Hip_combine.  out = {path, passes,
 * nhead, ntail}: the path below; the kernel launches (1, or 2-9 for a CHAIN of
 * more than 8 operands with a fused fold); the head / tail elements of the
 * fused vector kernel (0 on the other paths).  A multi-pass CHAIN reports
 * fused-elements if any of its passes takes the element kernel. */
#define MPIR_HIP_COMBINE_PATH_COPY           0   /* n == 1, or REPLACE: a device copy (none if in place) */
#define MPIR_HIP_COMBINE_PATH_FUSED_VECTOR   1   /* k_combine_multi */
#define MPIR_HIP_COMBINE_PATH_FUSED_ELEMENTS 2   /* k_combine_multi_elems: an operand off the output's alignment */
#define MPIR_HIP_COMBINE_PATH_ANY            3   /* k_combine_any */
int MPIR_Hip_combine_plan_info(const void *const *inbufs, int n, const void *outbuf, uint64_t count, int op, int elem,
                               int order, uint64_t out[4]);

/* Batched reduction: io[i] = op(io[i], in[i]), i < count, for each of nsegs
 * independent segments under one (op, elem), in one kernel launch per
 * MPIR_Hip_batch_plan_info's "max segments per launch" non-empty segments
 * (back-to-back launches on the same stream beyond that).  Each segment's
 * result is bit-identical to MPIR_Hip_reduce on it.  Every non-empty segment's
 * two buffers must be device-resident, all on one device (else
 * MPIR_HIP_EBUFFER); every pointer is classified before the first launch, so a
 * call that fails has written nothing.  count == 0 segments are skipped, their
 * pointers never looked at.  Segments may share or overlap inputs; overlapping
 * outputs, or an input overlapping another segment's output, are undefined.
 * A batch with exactly one non-empty segment is MPIR_Hip_reduce on it.
 * hip_stream / sync as for MPIR_Hip_reduce.  The segment table travels in the
 * kernel arguments: `segs` may be reused as soon as the call returns. */
typedef struct { const void *in; void *io; uint64_t count; } MPIR_Hip_seg;
int MPIR_Hip_reduce_batch(const MPIR_Hip_seg *segs, int nsegs, int op, int elem, void *hip_stream, int sync);

/* For tests and tools: the launches MPIR_Hip_reduce_batch would make for
 * device segments at these addresses, from the same planner the launch calls
 * (host arithmetic on the pointer values only).  out = {launches, workgroups
 * over all launches, tile-path segments, element-path segments, empty
 * segments, max segments per launch}; seg_kind / seg_groups (each nsegs
 * entries, or NULL) receive every segment's path below and its workgroups.  A
 * launch also closes before its workgroups pass MPIR_HIP_BATCH_MAX_GROUPS.
 * MPIR_HIP_ENOKERNEL for REPLACE and for pairs with no kernel. */
#define MPIR_HIP_BATCH_SEG_EMPTY  0   /* count == 0: skipped */
#define MPIR_HIP_BATCH_SEG_TILE   1   /* naturally aligned, equal offsets mod 16: the 16 KiB tile grid */
#define MPIR_HIP_BATCH_SEG_ELEMS  2   /* any other alignment, and the 32-byte classes: element runs */
#define MPIR_HIP_BATCH_SEG_SINGLE 3   /* the only non-empty segment: MPIR_Hip_reduce's own plan */
#define MPIR_HIP_BATCH_MAX_GROUPS (1ull << 23)
int MPIR_Hip_batch_plan_info(const MPIR_Hip_seg *segs, int nsegs, int op, int elem,
                             uint64_t out[6], uint32_t *seg_kind, uint32_t *seg_groups);

/* Strided reduction: for r < nblocks, io_r[i] = op(io_r[i], in_r[i]), i <
 * blocklen, where in_r = inbuf + r * in_stride and io_r = inoutbuf + r *
 * io_stride (strides in bytes) -- the rows of an MPI_Type_vector operand under
 * one (op, elem), in one kernel launch however many rows there are (further
 * launches on the same stream take later row ranges once a launch would pass
 * MPIR_HIP_BATCH_MAX_GROUPS workgroups).  Each row's result is bit-identical to
 * MPIR_Hip_reduce on it; bytes between rows are never read or written.
 * nblocks == 0 or blocklen == 0 succeeds with no pointer looked at.  With
 * nblocks > 1, io_stride below the row's bytes (output rows would overlap), or
 * a span past the end of the address space, is MPIR_HIP_EARG; in_stride may be
 * anything, 0 combines one input row into every output row.  The first and the
 * last byte of each operand's span must be device memory, all on one device
 * (else MPIR_HIP_EBUFFER); they are classified before the first launch, so a
 * call that fails has written nothing.  nblocks == 1, or both strides equal to
 * the row's bytes, is MPIR_Hip_reduce on nblocks * blocklen elements.
 * hip_stream / sync as for MPIR_Hip_reduce; the launch carries everything in
 * its kernel arguments.  MPIR_HIP_ENOKERNEL for REPLACE and pairs with no kernel. */
int MPIR_Hip_reduce_strided(const void *inbuf, uint64_t in_stride, void *inoutbuf, uint64_t io_stride,
                            uint64_t nblocks, uint64_t blocklen, int op, int elem, void *hip_stream, int sync);

/* For tests and tools: the launches MPIR_Hip_reduce_strided would make for
 * device operands at these addresses, from the same planner the launch calls
 * (host arithmetic on the pointer values only).  out = {form, launches,
 * workgroups over all launches, G (WIDE: workgroups per row) or units per
 * workgroup (NARROW), rows on the tile path, rows on the element path (both
 * WIDE only, else 0), the wide / narrow threshold in force (bytes), rows per
 * launch}.  SINGLE reports MPIR_Hip_plan_info's grid as its workgroups.
 * Returns as MPIR_Hip_reduce_strided does for the same arguments, residency
 * apart. */
#define MPIR_HIP_STRIDED_EMPTY        0   /* nblocks or blocklen 0: nothing to do */
#define MPIR_HIP_STRIDED_SINGLE       1   /* one row, or contiguous rows: MPIR_Hip_reduce's own plan */
#define MPIR_HIP_STRIDED_WIDE         2   /* row bytes >= the threshold: nblocks x G workgroups, the batch's segment code */
#define MPIR_HIP_STRIDED_NARROW_VEC   3   /* flattened 16-byte units: row bytes, strides and bases all multiples of 16 */
#define MPIR_HIP_STRIDED_NARROW_ELEMS 4   /* flattened elements, any alignment */
int MPIR_Hip_strided_plan_info(const void *inbuf, uint64_t in_stride, const void *inoutbuf, uint64_t io_stride,
                               uint64_t nblocks, uint64_t blocklen, int op, int elem, uint64_t out[8]);
/* Rows of at least this many bytes take the WIDE form
 * (MPIR_CVAR_REDUCE_LOCAL_STRIDED_WIDE_KB, default 16 KiB; 0: every row; at most
 * 1 GiB).  The setter changes it at run time (tools/strided_ab.py forces each
 * form with it) and returns the previous value. */
uint64_t MPIR_Hip_set_strided_wide_bytes(uint64_t bytes);
/* Test hook: the calling thread's strided launches close before `groups`
 * workgroups instead of MPIR_HIP_BATCH_MAX_GROUPS (never inside a row of the
 * WIDE form), so that the row-range split runs at a small size
 * (tests/test_strided_gpu.py).  0, or more than the real cap: the real cap.
 * Returns the previous value. */
uint64_t MPIR_Hip_strided_test_max_groups(uint64_t groups);

/* Subarray reduction: every row of a sub-box of an N-dimensional array combined
 * as MPIR_Hip_reduce combines it, no table and, for boxes of up to three outer
 * dimensions, one launch.  Each operand is what MPI_Type_create_subarray(ndims,
 * X_sizes, subsizes, X_starts, order, ...) describes at X buf, the origin of the
 * whole array (c_order != 0: MPI_ORDER_C, the last dimension the fastest; else
 * MPI_ORDER_FORTRAN); X_sizes NULL: that operand is packed (sizes = subsizes,
 * starts 0, X_starts not looked at).  The planner brings the box to a normal
 * form -- the fastest dimension first; a dimension of subsize 1 dropped;
 * dimension d + 1 merged into d where the box spans all of d on both sides (an
 * outer dimension's merged count stays below 2^31) -- a row of blocklen
 * contiguous elements under k outer dimensions, each a count and one byte stride
 * per side.  k == 0 is MPIR_Hip_reduce, k == 1 MPIR_Hip_reduce_strided, both
 * with everything they do; k == 2 or 3 is k_reduce_subarray, in the strided
 * call's three forms at the strided call's threshold and per-launch cap
 * (MPIR_Hip_set_strided_wide_bytes, MPIR_Hip_strided_test_max_groups); the
 * dimensions past the third are looped on the host, back-to-back launches on the
 * same stream.  The first and the last byte of each box must be device memory
 * on one device (MPIR_HIP_EBUFFER), settled before the first launch.  ndims
 * outside 1..MPIR_HIP_SUBARRAY_MAXDIMS, subsizes NULL, sizes without starts, a
 * dimension the reference refuses (size < 1, subsize < 1, start < 0, subsize >
 * size, start > size - subsize) or an array whose bytes pass 63 bits:
 * MPIR_HIP_EARG.  MPIR_HIP_ENOKERNEL for REPLACE and pairs with no kernel.
 * Nothing of the caller's arrays is read after the call returns. */
#define MPIR_HIP_SUBARRAY_MAXDIMS 8
int MPIR_Hip_reduce_subarray(const void *inbuf, const int *in_sizes, const int *in_starts, void *inoutbuf,
                             const int *io_sizes, const int *io_starts, int ndims, const int *subsizes, int c_order,
                             int op, int elem, void *hip_stream, int sync);

/* For tests and tools: the normal form and the launches of MPIR_Hip_reduce_subarray
 * for device operands at these addresses (host arithmetic on the arguments only).
 * out[0] form; out[1] launches; out[2] workgroups over all launches; out[3] G
 * (WIDE) or units per workgroup (NARROW); out[4] units per row (NARROW); out[5]
 * the wide / narrow threshold in force; out[6] rows per launch; out[7] k; out[8]
 * blocklen; out[9] / out[10] the byte offsets of the input and output box in
 * their arrays; STRIDED only: out[11] the strided call's form, out[12] / out[13]
 * its rows on the tile and the element path, and out[1..3], out[5], out[6] as
 * MPIR_Hip_strided_plan_info reports them; out[16 + d], out[24 + d], out[32 + d]
 * for d < k: outer dimension d's count and its byte stride in the input and the
 * output.  SINGLE reports MPIR_Hip_plan_info's grid as its workgroups.  Returns
 * as MPIR_Hip_reduce_subarray does for the same arguments, residency apart. */
#define MPIR_HIP_SUBARRAY_SINGLE       1   /* k == 0: MPIR_Hip_reduce's own plan */
#define MPIR_HIP_SUBARRAY_WIDE         2   /* the forms of k >= 2: MPIR_HIP_STRIDED_WIDE, ... */
#define MPIR_HIP_SUBARRAY_NARROW_VEC   3
#define MPIR_HIP_SUBARRAY_NARROW_ELEMS 4
#define MPIR_HIP_SUBARRAY_STRIDED      5   /* k == 1: MPIR_Hip_reduce_strided's own plan */
#define MPIR_HIP_SUBARRAY_PLAN_WORDS  40
int MPIR_Hip_subarray_plan_info(const void *inbuf, const int *in_sizes, const int *in_starts, const void *inoutbuf,
                                const int *io_sizes, const int *io_starts, int ndims, const int *subsizes, int c_order,
                                int op, int elem, uint64_t out[MPIR_HIP_SUBARRAY_PLAN_WORDS]);

/* Fetching reduction: for i < count, fetchbuf[i] = the bytes inoutbuf[i] held on
 * entry and inoutbuf[i] = op(inoutbuf[i], inbuf[i]), in one kernel launch that
 * reads inoutbuf once -- the target side of MPI_Get_accumulate / MPI_Fetch_and_op
 * (ch3u_rma_pkthandler.c:899-917, :1354; ch3u_handle_recv_req.c:207, 274, 356,
 * 441, 494, 1350, 1423, 1567), whose "copy data + ACC" the reference requires to
 * be atomic: the value fetched and the value combined come from the same load.
 * inoutbuf's result is bit-identical to MPIR_Hip_reduce's; the fetched bytes are
 * a byte copy of count * MPIR_Hip_elem_size(elem) bytes.
 * op: an MPIR_Hip_op with a kernel for elem, or one of the two copy ops, which
 * need no kernel and take any element class:
 *   MPIR_HIP_OP_NO_OP    fetchbuf <- inoutbuf: one stream-ordered device copy;
 *                        inbuf is never looked at (it may be NULL), inoutbuf
 *                        is not written;
 *   MPIR_HIP_OP_REPLACE  fetchbuf <- inoutbuf, then inoutbuf <- inbuf: two such
 *                        copies on the same stream.
 * count == 0 succeeds with no pointer looked at.  Every buffer that is looked at
 * must be device-resident, all on one device (else MPIR_HIP_EBUFFER; host
 * operands are not taken); they are classified before the first launch, so a
 * call that fails has written nothing.  fetchbuf overlapping either operand is
 * undefined here (MPIX_Reduce_local_fetch refuses it).  hip_stream / sync as for
 * MPIR_Hip_reduce; the launch carries everything in its kernel arguments.
 * MPIR_HIP_ENOKERNEL for pairs with no kernel. */
#define MPIR_HIP_OP_NO_OP 14   /* MPI_NO_OP's table index; the fetching calls (MPIR_Hip_reduce_fetch, _fetch_ragged, _fetch_indexed_ordered) alone take it (no kernel table slot) */
int MPIR_Hip_reduce_fetch(const void *inbuf, void *inoutbuf, void *fetchbuf, uint64_t count, int op, int elem,
                          void *hip_stream, int sync);

/* For tests and tools: the plan MPIR_Hip_reduce_fetch would take for device
 * operands at these addresses, from the planner the launch runs (host
 * arithmetic on the pointer values only).  out = {path, workgroups, nhead,
 * ntail}: the path below, the grid of the one launch (0 for EMPTY and COPY), and
 * the elements workgroup 0 takes before / after the 16-byte vector region on the
 * tile path (0 on the others). */
#define MPIR_HIP_FETCH_EMPTY 0   /* count == 0: nothing to do */
#define MPIR_HIP_FETCH_COPY  1   /* MPI_NO_OP / MPI_REPLACE: device copies, no kernel */
#define MPIR_HIP_FETCH_TILE  2   /* all three pointers naturally aligned, one offset mod 16: the 16 KiB tile grid */
#define MPIR_HIP_FETCH_ELEMS 3   /* any other alignment, and the 32-byte classes: element runs */
int MPIR_Hip_fetch_plan_info(const void *inbuf, const void *inoutbuf, const void *fetchbuf, uint64_t count, int op,
                             int elem, uint64_t out[4]);

/* Indexed reduction: for k < nblocks, io_k[i] = op(io_k[i], in_k[i]), i <
 * blocklen, where in_k = inbuf + in_displs[k] * disp_unit and io_k = inoutbuf +
 * io_displs[k] * disp_unit bytes (signed displacements); a side whose table is
 * NULL is packed, block k at k * blocklen * the element's size.  The blocks of
 * an MPI_Type_create_indexed_block / hindexed_block operand under one (op,
 * elem) -- a scatter-add with io_displs, a gather-reduce with in_displs -- in
 * one kernel launch however many blocks there are (further launches on the
 * same stream take later block ranges, their table pointers and packed bases
 * advanced, once a launch would pass MPIR_HIP_BATCH_MAX_GROUPS workgroups).
 * Each block's result is bit-identical to MPIR_Hip_reduce on it; no byte outside
 * the blocks is read or written.  Output blocks that overlap each other or an
 * input block are undefined (not checked: the blocks run concurrently); a
 * repeated in_displs entry is fine.
 * disp_unit == 0, or more than INT64_MAX, is MPIR_HIP_EARG, whatever the
 * counts (MPIX_Reduce_local_indexed answers MPI_ERR_ARG likewise).  Otherwise
 * nblocks == 0 or blocklen == 0 succeeds with no pointer looked at, tables
 * included.  Both
 * tables NULL is MPIR_Hip_reduce on nblocks * blocklen elements.
 * Residency: both bases must be device memory on one device, and the first and
 * the last byte of a packed side's span (else MPIR_HIP_EBUFFER).  A table is
 * device memory on that device, read by the kernel: it must stay unchanged until
 * the work completes.  With sync != 0 and hip_stream NULL a table may be host
 * memory instead: it is copied into a per-(thread, device) table buffer of the
 * library's, stream-ordered ahead of the kernel; as the library reads such a
 * table anyway, it also checks displs[k] * disp_unit for overflow
 * (MPIR_HIP_EARG) and classifies the first byte of the lowest block and the
 * last byte of the highest.  A host table in any other call is
 * MPIR_HIP_EBUFFER.  Everything is classified before the first launch, so a
 * call that fails has written nothing.  With device tables the launch carries
 * everything else in its kernel arguments (graph-capturable).
 * The wide / narrow threshold is the strided call's
 * (MPIR_Hip_set_strided_wide_bytes), and so are the per-launch workgroup cap
 * and its test hook (MPIR_Hip_strided_test_max_groups).
 * Narrow blocks move as 16-byte vectors only where every address is provably a
 * multiple of 16 without reading a table: blocklen * size and both bases
 * multiples of 16, and disp_unit a multiple of 16 for each side with a table.
 * A caller whose blocks are 16-byte aligned should therefore pass disp_unit 16
 * (or a multiple) with displacements scaled to it, not byte displacements with
 * disp_unit 1, which take the element form.
 * MPIR_HIP_ENOKERNEL for REPLACE and pairs with no kernel. */
int MPIR_Hip_reduce_indexed(const void *inbuf, const int64_t *in_displs, void *inoutbuf, const int64_t *io_displs,
                            uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                            void *hip_stream, int sync);

/* For tests and tools: the launches MPIR_Hip_reduce_indexed would make for
 * device operands and tables at these addresses, from the same planner the
 * launch runs (host arithmetic on the pointer values only: the tables are never
 * read, only compared with NULL; no GPU is needed).  out = {form, launches,
 * workgroups over all launches, G (WIDE: workgroups per block, the most a block
 * can need at any address) or units per workgroup (NARROW), the wide / narrow
 * threshold in force (bytes), blocks per launch}.  SINGLE reports
 * MPIR_Hip_plan_info's grid as its workgroups.  Returns as
 * MPIR_Hip_reduce_indexed does for the same arguments, residency apart. */
#define MPIR_HIP_INDEXED_EMPTY        0   /* nblocks or blocklen 0: nothing to do */
#define MPIR_HIP_INDEXED_SINGLE       1   /* both tables NULL: MPIR_Hip_reduce's own plan */
#define MPIR_HIP_INDEXED_WIDE         2   /* block bytes >= the threshold: nblocks x G workgroups, the batch's segment code */
#define MPIR_HIP_INDEXED_NARROW_VEC   3   /* flattened 16-byte units: every address provably a multiple of 16 */
#define MPIR_HIP_INDEXED_NARROW_ELEMS 4   /* flattened elements, any alignment */
int MPIR_Hip_indexed_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                               const int64_t *io_displs, uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen,
                               int op, int elem, uint64_t out[6]);

/* Ordered indexed reduction: MPIR_Hip_reduce_indexed whose output table may name
 * one block any number of times, with the result of the blocks applied one after
 * another in table order: for k = 0 .. nblocks - 1 in that order, io_k[i] =
 * op(io_k[i], in_k[i]), bit-identical to that sequence of MPIR_Hip_reduce calls.
 * Two output blocks must have equal io_displs entries or be disjoint (partial
 * overlap is undefined, as is an input block that overlaps an output block).
 * `order` (nblocks ints) puts the blocks of one target side by side: a
 * permutation of [0, nblocks) with io_displs[order[p]] non-decreasing in p and,
 * within equal displacements, order[p] ascending -- a stable argsort of
 * io_displs, which MPIR_Hip_order_build makes.  The kernel
 * (k_reduce_indexed_ordered, reduce_kernels.hpp) gives each run of equal
 * displacements to the workgroups (WIDE) or lanes (NARROW) of its first sorted
 * position, which load the target once, fold the run's input blocks into
 * registers serially, in order, and store once; the plan, the forms, the
 * threshold and the per-launch cap are the indexed call's, rows read as sorted
 * positions.  Later launches get the same tables and bases with their first
 * position: a run may cross a launch boundary and still has one owner.
 * order NULL is MPIR_Hip_reduce_indexed unchanged (a promise of no repeats).
 * Otherwise the indexed call's argument checks, then io_displs NULL or nblocks >
 * INT32_MAX: MPIR_HIP_EARG (counts of 0 succeed before that, no pointer looked
 * at).  Residency as the indexed call's, `order` a third table under the same
 * rules.  A host order table is checked (MPIR_HIP_EARG): every entry in range,
 * no entry twice and, where io_displs is a host table too, the two ordering
 * conditions.  A device order table is not, and one that breaks the conditions
 * gives an undefined result; every index the kernel reads from it is clamped
 * into [0, nblocks), so its reads of all three tables stay inside them.
 * A call that fails has written nothing; no table is ever written.  With device
 * tables the launch carries everything in its kernel arguments (no library
 * buffer, graph-capturable). */
int MPIR_Hip_reduce_indexed_ordered(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                    const int64_t *io_displs, const int *order, uint64_t disp_unit, uint64_t nblocks,
                                    uint64_t blocklen, int op, int elem, void *hip_stream, int sync);

/* For tests and tools: MPIR_Hip_indexed_plan_info's six outputs for the launches
 * MPIR_Hip_reduce_indexed_ordered would make (rows are sorted positions; `order`
 * is only compared with NULL).  Returns as that call does, residency apart. */
int MPIR_Hip_indexed_ordered_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                       const int64_t *io_displs, const int *order, uint64_t disp_unit,
                                       uint64_t nblocks, uint64_t blocklen, int op, int elem, uint64_t out[6]);

/* The order table of `displs` (nblocks signed 64-bit displacements): order[p]
 * the block at sorted position p, a stable sort by displacement.
 * *work_bytes = the scratch MPIR_Hip_order_build may use for nblocks, from
 * nblocks alone (host arithmetic, non-decreasing, no GPU needed): room for the
 * sorted keys plus a bound on what rocPRIM's radix_sort_pairs asks for on any
 * device.  nblocks > INT32_MAX: MPIR_HIP_EARG (both functions).
 * Build: both tables device memory on one device: the sort is enqueued on
 * hip_stream, or on the library stream and waited for with sync != 0 and
 * hip_stream NULL.  `work` is device memory there of at least *work_bytes
 * (work_bytes less: MPIR_HIP_EARG; not device memory: MPIR_HIP_EBUFFER); bytes
 * past the reported size are never touched.  work NULL without a stream: the
 * thread's table buffer serves; with a stream: MPIR_HIP_EBUFFER.  In a
 * synchronous call either table may be host memory (with a stream:
 * MPIR_HIP_EBUFFER): both on the host is a host stable sort that does not open
 * the GPU runtime; one of them is copied through the table buffer.  nblocks 0
 * succeeds and looks at nothing.  The build allocates nothing on a stream but
 * makes several launches whose number depends on nblocks, and asks the runtime
 * for the device's properties: capture into a graph is not promised. */
int MPIR_Hip_order_worksize(uint64_t nblocks, uint64_t *work_bytes);
int MPIR_Hip_order_build(const int64_t *displs, uint64_t nblocks, int *order, void *work, uint64_t work_bytes,
                         void *hip_stream, int sync);

/* Chunked indexed reduction: MPIR_Hip_reduce_indexed_ordered's operands and
 * tables, but the blocks of one target are not folded one after another: the
 * run's blocks, in ascending block number, are cut into chunks of
 * MPIR_HIP_REDUCE_CHUNK counted from the run's first; each chunk is folded into
 * a partial that starts as a byte copy of the chunk's first input block; the
 * partials are then combined into the target in order.  The association depends
 * on the run's own length alone: the same tables and data always give the same
 * bits, and a hot row's serial depth is 64 + L / 64, not L.  On floating types
 * the result is NOT the ordered call's.
 * `runstart` (nblocks ints) is a fourth table: runstart[p] the smallest sorted
 * position q with io_displs[order[q]] == io_displs[order[p]]
 * (MPIR_Hip_runs_build makes it).  order and runstart both NULL is
 * MPIR_Hip_reduce_indexed unchanged; one of them NULL, or either given with
 * io_displs NULL, MPIR_HIP_EARG.  The argument checks are the ordered call's in
 * its order, residency too, runstart a fourth table under the same rules --
 * but the tables are placed first, as the ragged call places them, and a host
 * order or runstart is read and checked before the operands' residency is.  A
 * host runstart is checked (MPIR_HIP_EARG): against its definition where order
 * and io_displs are host tables too, else 0 <= runstart[p] <= p.  A device
 * runstart is not, and a wrong one gives an undefined result; the kernels clamp
 * what they read from it, so reads stay inside the tables and writes inside
 * the target blocks and `work`.
 * `work`: device scratch for the partials of runs longer than a chunk, at least
 * MPIR_Hip_chunked_worksize's bytes (2 * ceil(nblocks / 64) slots of the block's
 * bytes rounded up to 16 plus 16, and 256 to align; from the three arguments
 * alone, non-decreasing in nblocks and blocklen, no GPU needed; a size past 63
 * bits: MPIR_HIP_EARG).  work_bytes less: MPIR_HIP_EARG; not device memory on
 * the operands' device: MPIR_HIP_EBUFFER; bytes past the reported size are never
 * touched.  work NULL without a stream: the thread's table buffer serves; with
 * a stream: MPIR_HIP_EBUFFER.
 * Two kernels (k_chunk_partials, k_fold_partials; reduce_kernels.hpp), each
 * over the ordered call's plan, every launch of the first before any of the
 * second: with device tables and the caller's work nothing is allocated and the
 * call is a linear chain of launches that can be captured into a graph.  A call
 * that fails has written nothing. */
#define MPIR_HIP_REDUCE_CHUNK 64
int MPIR_Hip_chunked_worksize(uint64_t nblocks, uint64_t blocklen, int elem, uint64_t *work_bytes);
int MPIR_Hip_reduce_indexed_chunked(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                    const int64_t *io_displs, const int *order, const int *runstart,
                                    uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                    void *work, uint64_t work_bytes, void *hip_stream, int sync);

/* For tests and tools: the launches MPIR_Hip_reduce_indexed_chunked would make
 * (the tables are only compared with NULL).  out[0..5]: as
 * MPIR_Hip_indexed_ordered_plan_info reports them, for ONE of the two kernels
 * (both have the same form, launches and workgroups); out[6] = launches of the
 * whole call (twice out[1]; with no table the indexed call's); out[7] = the
 * work bytes.  Returns as that call does, residency apart. */
int MPIR_Hip_indexed_chunked_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                       const int64_t *io_displs, const int *order, const int *runstart,
                                       uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                       uint64_t out[8]);

/* The runstart table of a displacement table and its order table: runstart[p] =
 * the smallest sorted position q with displs[order[q]] == displs[order[p]].
 * All three device memory on one device: ONE kernel (a lower-bound binary search
 * per position over displs[order[.]], every order entry clamped) enqueued on
 * hip_stream, or on the library stream and waited for with sync != 0 and
 * hip_stream NULL; no scratch, nothing allocated, and it can be captured into a
 * graph.  In a synchronous call any table may be host memory (with a stream:
 * MPIR_HIP_EBUFFER): all on the host is a host loop that does not open the GPU
 * runtime; otherwise the host ones are copied through the table buffer.
 * nblocks > INT32_MAX: MPIR_HIP_EARG; nblocks 0 succeeds and looks at nothing. */
int MPIR_Hip_runs_build(const int64_t *displs, const int *order, uint64_t nblocks, int *runstart, void *hip_stream,
                        int sync);

/* Ragged reduction: npieces pieces of unequal length.  starts (npieces + 1
 * entries) holds the pieces' element offsets in packed order, CSR row pointers:
 * starts[0] == 0, non-decreasing, starts[npieces] == count; piece k has
 * starts[k + 1] - starts[k] elements (none is fine) and is
 * io_k[i] = op(io_k[i], in_k[i]) with in_k = inbuf + in_displs[k] * disp_unit
 * and io_k = inoutbuf + io_displs[k] * disp_unit bytes (signed displacements);
 * a side whose table is NULL is packed, piece k at starts[k] * the element's
 * size.  The pieces of an MPI_Type_indexed / MPI_Type_create_hindexed operand,
 * or of any IOV, under one (op, elem), in ONE kernel launch always: the grid
 * goes by packed element (ceil(count * size / 16 KiB) workgroups), not by piece.
 * Each piece's result is bit-identical to MPIR_Hip_reduce on it; no byte outside
 * the pieces is read or written, no table is written.  Output pieces that
 * overlap each other or an input piece are undefined (not checked); a repeated
 * input piece is fine.
 * disp_unit == 0, or more than INT64_MAX, is MPIR_HIP_EARG, whatever the
 * counts.  Otherwise count == 0 succeeds with no pointer looked at, tables
 * included.  count > 0 with npieces == 0, npieces or count above INT32_MAX, and
 * starts NULL beside a displacement table are MPIR_HIP_EARG.  Both displacement
 * tables NULL is MPIR_Hip_reduce on count elements; starts is not looked at.
 * Residency: both bases must be device memory on one device, and the last byte
 * of a packed side (else MPIR_HIP_EBUFFER).  Each of the three tables is device
 * memory on that device, read by the kernel: it must stay unchanged until the
 * work completes.  A device starts that breaks its three conditions is the
 * caller's error and what is then combined is undefined; the kernel's table
 * indices stay inside [0, npieces] all the same.  With sync != 0 and hip_stream
 * NULL each table may be host memory instead: the library reads it -- starts
 * for its three conditions (MPIR_HIP_EARG), a displacement table for the
 * overflow of displs[k] * disp_unit (MPIR_HIP_EARG), both before the operands'
 * residency is looked at, and, where starts is a host table too so that the
 * lengths are known, the first byte of the lowest non-empty piece and the last
 * byte of the highest (MPIR_HIP_EBUFFER) -- and copies it into the per-(thread, device) table buffer, stream-ordered ahead of
 * the kernel.  A host table in any other call is MPIR_HIP_EBUFFER.  Everything is
 * checked before anything is enqueued, so a call that fails has written nothing.
 * With device tables the launch carries everything else in its kernel arguments
 * (graph-capturable).
 * A 16-byte chunk of packed space moves as one vector where it lies inside one
 * piece and both its addresses are multiples of 16, decided per chunk on the
 * device; other chunks move element by element.
 * MPIR_HIP_ENOKERNEL for REPLACE and pairs with no kernel. */
int MPIR_Hip_reduce_ragged(const void *inbuf, const int64_t *in_displs, void *inoutbuf, const int64_t *io_displs,
                           const int64_t *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count, int op,
                           int elem, void *hip_stream, int sync);

/* For tests and tools: the launch MPIR_Hip_reduce_ragged would make, from the
 * same planner the launch runs (host arithmetic on the pointer values and
 * counts only: the tables are never read, only compared with NULL; no GPU is
 * needed).  out = {form, launches (1), workgroups, packed elements per
 * workgroup, rounds of the wave-wide search for a workgroup's first piece
 * (ceil(log64(npieces + 1))), piece boundaries a workgroup holds in LDS (4
 * bytes each)}.  SINGLE reports MPIR_Hip_plan_info's grid as its workgroups.
 * Returns as MPIR_Hip_reduce_ragged does for the same arguments, residency and
 * the tables' contents apart. */
#define MPIR_HIP_RAGGED_EMPTY   0   /* count 0: nothing to do */
#define MPIR_HIP_RAGGED_SINGLE  1   /* both displacement tables NULL: MPIR_Hip_reduce's own plan */
#define MPIR_HIP_RAGGED_RAGGED  2   /* one launch of k_reduce_ragged */
int MPIR_Hip_ragged_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                              const int64_t *io_displs, const int64_t *starts, uint64_t disp_unit, uint64_t npieces,
                              uint64_t count, int op, int elem, uint64_t out[6]);

/* Fetching ragged reduction: MPIR_Hip_reduce_fetch on a ragged target, the shape
 * of the reference's MPI_Get_accumulate target handler
 * (ch3u_handle_recv_req.c:326-358, :1391-1423: MPIR_Segment_pack of the
 * derived-type target into the response buffer, :339-351, then do_accumulate_op
 * over the same target, mpidrma.h:930-1021, "copy data + ACC needs to be
 * atomic").  inbuf (the origin's streamed data) and fetchbuf (the response
 * buffer) are packed; inoutbuf (the target) has the displacement table.  starts,
 * disp_unit, npieces and count are MPIR_Hip_reduce_ragged's.  For piece k of
 * len = starts[k + 1] - starts[k] elements at io_k = inoutbuf + io_displs[k] *
 * disp_unit: the len * size bytes of fetchbuf at starts[k] * size receive the
 * bytes io_k held on entry, a byte copy (never a value of the type), and io_k
 * becomes what MPIR_Hip_reduce(inbuf + starts[k] * size, io_k, len) would leave,
 * bit for bit.  ONE kernel launch always, which reads the target once: the value
 * fetched and the value combined come from the same load of each target element.
 * No byte outside the pieces is read or written, no byte of fetchbuf outside
 * [0, count * size), no table.
 * op: an MPIR_Hip_op MPIR_Hip_reduce_ragged has a kernel for, or
 *   MPIR_HIP_OP_NO_OP    a pack: the pieces gathered into fetchbuf; inbuf is
 *                        never looked at (it may be NULL), the target is not
 *                        written;
 *   MPIR_HIP_OP_REPLACE  a swap: the pieces out to fetchbuf, inbuf's bytes in;
 * both byte operations with a kernel per element size, for every element class.
 * The argument rules are MPIR_Hip_reduce_ragged's (disp_unit, count == 0,
 * npieces, starts NULL beside a table: MPIR_HIP_EARG likewise), and so are the
 * tables' residency and the checks of host tables (synchronous call on the
 * library stream only, through the per-(thread, device) table buffer).
 * io_displs NULL is MPIR_Hip_reduce_fetch on count elements; starts is not looked
 * at.  Residency: inoutbuf's base, and the first and the last byte of fetchbuf's
 * and (but for NO_OP) inbuf's count * size bytes, device memory on one device
 * (else MPIR_HIP_EBUFFER).  Where both tables are host tables, the pieces'
 * extremes are classified as MPIR_Hip_reduce_ragged does, and a fetchbuf range
 * that meets any byte from the lowest piece's first to the highest piece's last
 * is MPIR_HIP_EBUFFER.  With a device table fetchbuf overlapping a target piece
 * is undefined; so is fetchbuf overlapping inbuf (MPIX_Reduce_local_fetch_ragged
 * refuses that one).  Everything is checked before anything is enqueued, so a
 * call that fails has written nothing.  With device tables the launch carries
 * everything else in its kernel arguments (graph-capturable).
 * A 16-byte chunk of packed space moves as one vector where it lies inside one
 * piece and its three addresses are multiples of 16 (the packed two known on the
 * host, the target's decided per chunk on the device); other chunks move element
 * by element.  MPIR_HIP_ENOKERNEL for pairs with no kernel. */
int MPIR_Hip_reduce_fetch_ragged(const void *inbuf, void *inoutbuf, const int64_t *io_displs, void *fetchbuf,
                                 const int64_t *starts, uint64_t disp_unit, uint64_t npieces, uint64_t count, int op,
                                 int elem, void *hip_stream, int sync);

/* For tests and tools: the launch MPIR_Hip_reduce_fetch_ragged would make, from
 * the same planner the launch runs (host arithmetic on the pointer values and
 * counts only; no table is read, no GPU is needed).  out = {form (the
 * MPIR_HIP_RAGGED_* forms), launches, workgroups, packed elements per workgroup,
 * rounds of the wave-wide search, piece boundaries a workgroup holds in LDS, 1
 * if the two packed sides are at multiples of 16 (NO_OP: fetchbuf alone) so that
 * chunks can move as vectors}.  SINGLE reports MPIR_Hip_fetch_plan_info's grid as
 * its workgroups and that call's launches (2 copies for REPLACE, else 1). */
int MPIR_Hip_fetch_ragged_plan_info(const void *inbuf, const void *inoutbuf, const int64_t *io_displs,
                                    const void *fetchbuf, const int64_t *starts, uint64_t disp_unit, uint64_t npieces,
                                    uint64_t count, int op, int elem, uint64_t out[7]);

/* Fetching ordered indexed reduction: MPIR_Hip_reduce_indexed_ordered with every
 * intermediate value handed out -- MPIR_Hip_reduce_fetch block by block in table
 * order.  For k = 0 .. nblocks - 1 in that order, with in_k and io_k the indexed
 * call's blocks: the blocklen * size bytes of fetchbuf at k * blocklen * size
 * (fetchbuf is packed by block number) receive the bytes io_k holds after
 * contributions 0 .. k - 1 and before contribution k, and io_k = op(io_k, in_k).
 * What each of the MPI_Fetch_and_op / MPI_Get_accumulate operations a target has
 * queued for one location must answer.  The kernel
 * (k_reduce_fetch_indexed_ordered, reduce_kernels.hpp) is the ordered kernel's
 * code storing its running registers before each combine: the value fetched and
 * the value combined are one, the target is loaded once and stored once per run
 * of equal displacements.  The first block of a run receives a byte copy of the
 * old target (never a value of the type); a later one the bytes the ordered call
 * would have stored had the run ended before it.  The target ends as
 * MPIR_Hip_reduce_indexed_ordered leaves it.  No byte outside the blocks, outside
 * fetchbuf's nblocks * blocklen * size, or in any table is written.
 * op: an MPIR_Hip_op the ordered call has a kernel for, or
 *   MPIR_HIP_OP_NO_OP    every block of a run receives the old target; inbuf and
 *                        in_displs are never looked at (they may be NULL), the
 *                        target is not written;
 *   MPIR_HIP_OP_REPLACE  fetchbuf block k receives the previous contribution's
 *                        input block (the head of a run: the old target); the
 *                        target ends holding the run's last input block;
 * both byte operations with a kernel per element size, for every element class.
 * Tables: `order` as for the ordered call (MPIR_Hip_order_build makes it).
 * order NULL with io_displs given: sorted position p is block p, the caller's
 * promise that equal entries of io_displs, if any, are adjacent in the table (in
 * particular: no repeats, the fetching indexed call); a host io_displs is held to
 * it (an entry equal to a non-adjacent earlier one: MPIR_HIP_EARG).  io_displs
 * NULL: with order or in_displs given MPIR_HIP_EARG (a packed target has no
 * repeats, and gathering the origin side is not this call's job), with neither
 * MPIR_Hip_reduce_fetch on nblocks * blocklen elements.
 * The argument checks and their order are the ordered call's (disp_unit, counts
 * of 0 succeed looking at no pointer, nblocks > INT32_MAX), the op looked up as
 * MPIR_Hip_reduce_fetch_ragged looks it up.  Residency as the ordered call's,
 * fetchbuf's first and last byte on the same device (else MPIR_HIP_EBUFFER);
 * host tables in a synchronous call on the library stream only, checked as the
 * ordered call checks them; and with a host io_displs a fetchbuf range that meets
 * any byte from the lowest block's first to the highest block's last is
 * MPIR_HIP_EBUFFER.  With a device io_displs that overlap is undefined, as is
 * fetchbuf overlapping an input block (MPIX_Reduce_local_fetch_indexed_ordered
 * refuses a packed inbuf's range).  Every index read from a device order table
 * is clamped into [0, nblocks), so the stores to fetchbuf stay inside it too.
 * A call that fails has written nothing.  With device tables everything travels
 * in the kernel arguments (no allocation, no library buffer: graph-capturable).
 * The plan is the ordered call's with fetchbuf joining the alignment test:
 * NARROW_VEC needs fetchbuf at a multiple of 16 as well, else NARROW_ELEMS. */
int MPIR_Hip_reduce_fetch_indexed_ordered(const void *inbuf, const int64_t *in_displs, void *inoutbuf,
                                          const int64_t *io_displs, void *fetchbuf, const int *order, uint64_t disp_unit,
                                          uint64_t nblocks, uint64_t blocklen, int op, int elem, void *hip_stream,
                                          int sync);

/* For tests and tools: MPIR_Hip_indexed_ordered_plan_info's six outputs for the
 * launches MPIR_Hip_reduce_fetch_indexed_ordered would make (the tables are only
 * compared with NULL; for NO_OP inbuf and in_displs are not looked at).  No
 * table at all (SINGLE) reports MPIR_Hip_fetch_plan_info's launches and grid.
 * Returns as that call does, residency and the tables' contents apart. */
int MPIR_Hip_fetch_indexed_ordered_plan_info(const void *inbuf, const int64_t *in_displs, const void *inoutbuf,
                                             const int64_t *io_displs, const void *fetchbuf, const int *order,
                                             uint64_t disp_unit, uint64_t nblocks, uint64_t blocklen, int op, int elem,
                                             uint64_t out[6]);

/* Ordered compare-and-swap: `count` entries of ONE element each, the target side of
 * MPI_Compare_and_swap many times over.  origin, compare and result are packed
 * by entry number; entry k's target is target + displs[k] * disp_unit bytes
 * (signed displacements).  For k = 0 .. count - 1 in that order: result[k]
 * receives the bytes the target holds (a byte copy), and where those bytes equal
 * compare[k]'s the target receives origin[k]'s.  Equality is equality of the
 * element's bytes, so the kernels (k_cas_indexed_ordered, k_cas_contig;
 * reduce_kernels.hpp) are chosen by the element class's SIZE, 1, 2, 4 or 8 bytes
 * (any other class: MPIR_HIP_ENOKERNEL).  One register value per run of equal
 * displacements: loaded from the target once, handed to result before every
 * step, stored back once if some step swapped.
 * Tables: `order` as for MPIR_Hip_reduce_fetch_indexed_ordered -- the ordered
 * call's table, or NULL with displs given for the caller's promise that equal
 * entries of displs are adjacent (a host displs is held to it).  displs NULL: a
 * contiguous target, element k is entry k (order given then: MPIR_HIP_EARG).
 * The argument checks are that call's in its order (disp_unit, a count of 0
 * succeeds looking at no pointer, count > INT32_MAX), as are residency (all four
 * buffers device memory on one device, the first and last byte of each packed
 * one), host tables (a synchronous call on the library stream only; overflow of
 * displs[k] * disp_unit and an invalid order MPIR_HIP_EARG; result meeting any
 * byte from the lowest target's first to the highest target's last
 * MPIR_HIP_EBUFFER) and the clamping of every index read from a device order.
 * A call that fails has written nothing.  With device tables everything travels
 * in the kernel arguments (no allocation, no library buffer: graph-capturable). */
#define MPIR_HIP_CAS_EMPTY        0   /* count == 0: nothing to do */
#define MPIR_HIP_CAS_CONTIG_TILE  1   /* no table; the four pointers at one offset mod 16, the target naturally aligned: the 16 KiB tile grid */
#define MPIR_HIP_CAS_CONTIG_ELEMS 2   /* no table, any other alignment: element runs */
#define MPIR_HIP_CAS_INDEXED      3   /* a displacement table: one lane per sorted position */
int MPIR_Hip_cas_indexed_ordered(const void *origin, const void *compare, void *target, const int64_t *displs,
                                 void *result, const int *order, uint64_t disp_unit, uint64_t count, int elem,
                                 void *hip_stream, int sync);

/* For tests and tools: the launches MPIR_Hip_cas_indexed_ordered would make for
 * device operands at these addresses (never dereferenced, the tables only
 * compared with NULL; no GPU needed).  out[0] the form (MPIR_HIP_CAS_*), out[1]
 * launches, out[2] workgroups over the whole call, out[3] rows_per_launch (sorted
 * positions of a full launch; MPIR_Hip_strided_test_max_groups lowers the
 * per-launch workgroup cap behind it), out[4] the entries one workgroup owns,
 * out[5] kCasAhead (the positions a run is walked at a time), out[6] / out[7]
 * the head and tail elements workgroup 0 of the tile form takes.  Returns as the
 * call does, residency and the tables' contents apart. */
int MPIR_Hip_cas_plan_info(const void *origin, const void *compare, const void *target, const int64_t *displs,
                           const void *result, const int *order, uint64_t disp_unit, uint64_t count, int elem,
                           uint64_t out[8]);

/* Flags for the calling thread's later MPIR_Hip_combine calls; returns the
 * previous flags.  MPIR_HIP_COMBINE_UNCAPPED: the fused folds run without the
 * LDS reservation that caps a CU at one (P >= 5) or three (P = 3, 4) of their
 * workgroups -- for a fold that overlaps other work on the device (the
 * collectives' pipelined folds beside RCCL's transfers). */
#define MPIR_HIP_COMBINE_UNCAPPED 1
int MPIR_Hip_combine_set_flags(int flags);

/* byte size of an element class (0 if unknown) */
size_t MPIR_Hip_elem_size(int elem);
/* 1 if a kernel exists for (op, elem) */
int MPIR_Hip_has_kernel(int op, int elem);
/* 1 if p is device-accessible memory (hipMalloc / managed), 0 otherwise */
int MPIR_Hip_is_device_ptr(const void *p);
/* how a reduction of `bytes` sees p: 0 pageable host memory, 1 device memory,
 * 2 pinned host memory (hipHostMalloc / hipHostRegister).  A call within the
 * mixed slot's and the host combine's limits (MPIR_Hip_mixed_max_bytes,
 * MPIR_Hip_host_max_bytes) may take this thread's kept verdict for p's page; a
 * larger one asks HIP again (pointer classification) */
int MPIR_Hip_pointer_kind(const void *p, uint64_t bytes);
/* synchronous copy between any two pointers (device/host in any mix) */
int MPIR_Hip_memcpy(void *dst, const void *src, size_t bytes);
/* last runtime error text for this thread ("" if none) */
const char *MPIR_Hip_error_string(void);
/* number of visible devices (0 if none / runtime unavailable) */
int MPIR_Hip_device_count(void);
/* per-thread contexts (streams, completion word, scratch) created so far; a
   context returns to a pool when its thread exits and is reused, so this stays
   at the peak number of threads calling at once (diagnostic) */
/* Largest operand (bytes) combined on the host when both operands are host
 * memory (MPIR_CVAR_REDUCE_LOCAL_HOST_MAX_KB; default no limit, 0 = always
 * stage through the GPU).  The setter changes it at run time (an MPI_T-style
 * cvar write; bench.py uses it to time the staging pipeline) and returns the
 * previous value. */
uint64_t MPIR_Hip_host_max_bytes(void);
uint64_t MPIR_Hip_set_host_max_bytes(uint64_t bytes);

/* Results of at most this many bytes are stored into the Infinity Cache (sc1)
 * for their next reader, larger ones bypass it (nt): MPIR_CVAR_REDUCE_LOCAL_KEEP_MB,
 * default 64 MiB.  The setter changes it at run time and returns the previous
 * value (bench.py reports config 2 both ways). */
uint64_t MPIR_Hip_set_keep_bytes(uint64_t bytes);
/* Results of at most `bytes` are stored nt whatever MPIR_Hip_set_keep_bytes says
 * (MPIR_CVAR_REDUCE_LOCAL_KEEP_MIN_MB, default 16 MiB: below it sc1 costs the
 * call more than its next reader gains); returns the previous value. */
uint64_t MPIR_Hip_set_keep_min_bytes(uint64_t bytes);

/* One operand host memory, the other on a device, at most this many bytes
 * (MPIR_CVAR_REDUCE_LOCAL_MIXED_MAX_KB, default 1 MiB): the host operand is
 * copied into the calling thread's pinned, device-mapped slot and the kernel
 * reads (writes) it there directly; larger calls use the staging pipeline. */
uint64_t MPIR_Hip_mixed_max_bytes(void);

/* Synchronous device-resident reductions completed through the direct AQL
 * dispatch (direct_dispatch.hip) so far in this process (0 with
 * MPIR_CVAR_REDUCE_LOCAL_DISPATCH=hip or where the path is unavailable). */
uint64_t MPIR_Hip_direct_dispatches(void);

/* Kernel timing of the direct dispatch: with profiling on, the CP's start /
 * end timestamps of each dispatch (as rocprofv3 reads them); the calling
 * thread's last direct dispatch in ns (0 if none or profiling off). */
void MPIR_Hip_direct_profile(int on);
uint64_t MPIR_Hip_direct_last_kernel_ns(void);

/* Direct-dispatch diagnostics: the device's state (0 not yet tried, 1 ready,
 * 2 ready with every kernarg write made visible by a flush read back before
 * the doorbell -- the queue's dispatch ids are not its packet indices, as
 * under a tool that intercepts queues such as rocprofv3 --kernel-trace;
 * -1..-12 the initialisation step that failed: properties, hsa_init, agents,
 * VRAM pool, HDP register, code-object file, code-object load, kernel
 * symbols, kernarg memory, queue, error word, and (-12) a code object built
 * from other sources than this library (MPIR_Hip_build_id); -20 disabled by
 * MPIR_CVAR_REDUCE_LOCAL_DISPATCH=hip), and the number of direct calls that
 * first synchronised with work reported pending on the legacy null stream. */
int MPIR_Hip_direct_state(int dev);
/* Initialise device `dev`'s direct path now -- its HSA queue, the device-only
 * code object, the kernarg slots, the dispatch-id probe (2-10 ms) -- rather
 * than inside the first synchronous call on that device; meant for MPI_Init
 * (Option 1).  Idempotent and thread-safe; returns
 * MPIR_Hip_direct_state(dev). */
int MPIR_Hip_direct_prepare(int dev);

/* The library's load-time default HSA_ALLOCATE_QUEUE_DEV_MEM=1 (AQL rings in
 * VRAM), applied on request: 1 set now, 0 the environment already holds a
 * value (kept), -1 the HSA runtime has started (too late, nothing done), -2 the
 * process runs other threads and threads_ok is 0.  The constructor applies it
 * with threads_ok 0; the Python package's load() with 1. */
int MPIR_Hip_default_rings_in_vram(int threads_ok);
/* With profiling on, the calling thread's last direct call on the system
 * clock, ns from entering the dispatch: doorbell rung, CP start, CP end,
 * completion seen by the host.  The CP's two stamps reach the system clock
 * through the runtime's translation, so they carry its offset (a few us at
 * most) and are two's-complement int64 values in the uint64 slots. */
void MPIR_Hip_direct_last_split(uint64_t out[4]);
uint64_t MPIR_Hip_direct_busy_skips(void);
/* Direct calls whose kernel arguments missed the kernarg cache (written into a
 * VRAM slot before the doorbell, with an HDP flush; read back under a queue-
 * intercepting tool). */
uint64_t MPIR_Hip_direct_kernarg_writes(void);
/* Test hook: with us > 0, a checked dispatch's kernarg write moves behind the
 * doorbell and is held back `us` microseconds, as if it had lost the race to
 * the CP; the dispatched workgroups wait for it
 * (tests/test_parity_gpu.py::test_direct_dispatch_preempted_writer,
 * tests/test_direct_timeout_gpu.py, tools/late_write_probe.py).  0, the
 * default: the write precedes the doorbell.  Returns the previous value. */
uint32_t MPIR_Hip_direct_test_write_delay_us(uint32_t us);
/* Test hook: the next probe of a newly created timestamped (profiled) queue
 * reports that dispatch ids are not packet indices, as under a tool that
 * intercepts the queue; the first profiled call then switches the device to
 * read-back flushes (MPIR_Hip_direct_state 2) and must still complete
 * (tests/test_direct_prepare_gpu.py). */
void MPIR_Hip_direct_test_fail_probe(void);
/* Where the synchronous call's host side runs relative to device `dev`
 * (diagnostic; bench.py records it per rank): out[0] the calling thread's CPU
 * (sched_getcpu), out[1] that CPU's NUMA node, out[2] the device's NUMA node
 * (its PCI function's sysfs numa_node), out[3] the node of the page holding
 * this thread's completion signal for dev, out[4] the node of the device's
 * error word; -1 where unknown or not yet created. */
void MPIR_Hip_direct_placement(int dev, int out[5]);
/* Where device dev's direct-path queue keeps its AQL ring (diagnostic): 1 device
 * memory (HSA_ALLOCATE_QUEUE_DEV_MEM=1, the library's default), 0 host memory,
 * -1 no queue yet / unknown. */
int MPIR_Hip_direct_ring_location(int dev);
int MPIR_Hip_thread_contexts(void);

/* The build id of this library: "src=<hash of csrc/ and include/> tiles=<hash
 * of the direct path's code object sources> git=<commit>[+dirty]" (Makefile),
 * so a run can show which sources its binaries came from. */
const char *MPIR_Hip_build_id(void);

/* Ranks of this job on this node, for sizing the host combine's threads: the
 * node's CPUs are shared by every local rank, and all of them reach the
 * combine of a host-buffer MPI_Allreduce together.  Inside libmpi the op layer
 * passes MPICH's node communicator size (mpich_glue.c) before its first
 * combine; otherwise MPI_LOCALNRANKS / MPIR_PIP_SIZE / LOCAL_WORLD_SIZE /
 * OMPI_COMM_WORLD_LOCAL_SIZE, else 1.  Takes effect if called before the first
 * host combine sizes the pool; returns the previous value (0 = unset). */
int MPIR_Hip_set_local_ranks(int n);
/* Threads one host combine uses, the caller included (1 = the caller alone):
 * this rank's share of the node's CPUs, at most 16, or
 * MPIR_CVAR_REDUCE_LOCAL_STAGE_THREADS.  Sizes the pool without starting it. */
int MPIR_Hip_host_threads(void);

#ifdef __cplusplus
}
#endif
#endif /* MPIR_HIP_REDUCE_H_INCLUDED */
