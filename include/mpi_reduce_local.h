/*
 * mpi_reduce_local.h -- drop-in C ABI for MPICH's local reduction hot path,
 * implemented on MI355X (gfx950) HIP kernels.
 *
 * Every declaration here replaces the symbol of the same name in the
 * reference (pmodels/mpich-pip, MPICH 3.3).  Handle values, error classes and
 * calling conventions are identical to an x86-64 MPICH 3.3 build configured
 * with --disable-fortran --disable-cxx (long double included: the x87 80-bit
 * format is computed in software on the GPU), so the existing collective
 * schedules and the RMA accumulate path can call these functions unchanged.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   MPI_Reduce_local / PMPI_Reduce_local  src/include/mpi.h.in:1359,
 *                                          src/mpi/coll/reduce_local/reduce_local.c:11-20,155-219
 *   MPIR_Reduce_local                      src/include/mpir_coll.h:1542,
 *                                          src/mpi/coll/reduce_local/reduce_local.c:35-122
 *   MPIR_Op_table / MPIR_Op_check_dtype_table
 *                                          src/mpi/coll/allreduce/allreduce.c:121-139,
 *                                          src/include/mpir_op.h:183-189
 *   MPIR_MAXF ... MPIR_NO_OP (+ _check_dtype)
 *                                          src/include/mpir_op.h:131-159, src/mpi/coll/op/op*.c
 *   MPI_Op_create / MPI_Op_free / MPI_Op_commutative
 *                                          src/mpi/coll/op/op_create.c:73-140,
 *                                          src/mpi/coll/op/op_free.c, op_commutative.c
 *   MPIR_Op_is_commutative                 src/mpi/coll/op/op_commutative.c:39
 *   MPI_Error_class / MPI_Error_string     src/mpi/errhan/error_class.c, error_string.c
 *
 * Extensions (MPIX_ prefix, not in the reference):
 *   MPIX_Reduce_local_stream  -- stream-ordered, non-synchronising variant for
 *                                device-resident buffers (what this library's
 *                                own schedules and benchmarks use).
 *   MPIX_Reduce_local_set_errhandler / _get_errhandler -- the reference routes
 *                                MPI_Reduce_local errors through
 *                                MPIR_Err_return_comm(NULL, ...) (errutil.c:238),
 *                                i.e. COMM_WORLD's handler; this library has no
 *                                communicators, so the handler is set here.
 */
#ifndef MPI_REDUCE_LOCAL_H_INCLUDED
#define MPI_REDUCE_LOCAL_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

/* The public API stays exported when these sources are compiled into a
 * libmpi built with -fvisibility=hidden (MPICH's configure.ac:1443 adds it;
 * mpi.h.in:13 marks the public prototypes the same way); the MPIR_ internals
 * follow the build's visibility, as MPICH's do. */
#ifndef MPICH_API_PUBLIC
#if defined(__GNUC__) || defined(__clang__)
#define MPICH_API_PUBLIC __attribute__((visibility("default")))
#else
#define MPICH_API_PUBLIC
#endif
#endif

/* ---- handle types (mpi.h.in:104,310) ---------------------------------- */
typedef int MPI_Datatype;
typedef int MPI_Op;
typedef int MPI_Errhandler;
typedef long MPI_Aint;          /* x86-64: MPI_AINT is 8 bytes */
typedef long long MPI_Offset;
typedef long long MPI_Count;

typedef void (MPI_User_function) (void *invec, void *inoutvec, int *len, MPI_Datatype * datatype);

#define MPI_IN_PLACE ((void *) -1)      /* mpi.h.in:544 */

/* ---- error classes (mpi.h.in:784-811) --------------------------------- */
#define MPI_SUCCESS          0
#define MPI_ERR_BUFFER       1
#define MPI_ERR_COUNT        2
#define MPI_ERR_TYPE         3
#define MPI_ERR_OP           9
#define MPI_ERR_ARG         12
#define MPI_ERR_UNKNOWN     13
#define MPI_ERR_OTHER       15
#define MPI_ERR_INTERN      16
#define MPI_ERR_NO_MEM      34

/* ---- error handlers (mpi.h.in: MPI_ERRORS_ARE_FATAL / MPI_ERRORS_RETURN) */
#define MPI_ERRHANDLER_NULL  ((MPI_Errhandler)0x14000000)
#define MPI_ERRORS_ARE_FATAL ((MPI_Errhandler)0x54000000)
#define MPI_ERRORS_RETURN    ((MPI_Errhandler)0x54000001)

/* ---- predefined ops (mpi.h.in:310-325): 0x58000000 | table index ------- */
#define MPI_OP_NULL ((MPI_Op)0x18000000)
#define MPI_MAX     ((MPI_Op)0x58000001)
#define MPI_MIN     ((MPI_Op)0x58000002)
#define MPI_SUM     ((MPI_Op)0x58000003)
#define MPI_PROD    ((MPI_Op)0x58000004)
#define MPI_LAND    ((MPI_Op)0x58000005)
#define MPI_BAND    ((MPI_Op)0x58000006)
#define MPI_LOR     ((MPI_Op)0x58000007)
#define MPI_BOR     ((MPI_Op)0x58000008)
#define MPI_LXOR    ((MPI_Op)0x58000009)
#define MPI_BXOR    ((MPI_Op)0x5800000a)
#define MPI_MINLOC  ((MPI_Op)0x5800000b)
#define MPI_MAXLOC  ((MPI_Op)0x5800000c)
#define MPI_REPLACE ((MPI_Op)0x5800000d)
#define MPI_NO_OP   ((MPI_Op)0x5800000e)

/* ---- predefined datatypes, x86-64 values (configure.ac:3442-3705,5077-5408)
 * bits 8-15 hold the size in bytes (mpir_datatype.h:172). */
#define MPI_DATATYPE_NULL       ((MPI_Datatype)0x0c000000)
#define MPI_CHAR                ((MPI_Datatype)0x4c000101)
#define MPI_UNSIGNED_CHAR       ((MPI_Datatype)0x4c000102)
#define MPI_SHORT               ((MPI_Datatype)0x4c000203)
#define MPI_UNSIGNED_SHORT      ((MPI_Datatype)0x4c000204)
#define MPI_INT                 ((MPI_Datatype)0x4c000405)
#define MPI_UNSIGNED            ((MPI_Datatype)0x4c000406)
#define MPI_LONG                ((MPI_Datatype)0x4c000807)
#define MPI_UNSIGNED_LONG       ((MPI_Datatype)0x4c000808)
#define MPI_LONG_LONG_INT       ((MPI_Datatype)0x4c000809)
#define MPI_LONG_LONG           MPI_LONG_LONG_INT
#define MPI_FLOAT               ((MPI_Datatype)0x4c00040a)
#define MPI_DOUBLE              ((MPI_Datatype)0x4c00080b)
#define MPI_LONG_DOUBLE         ((MPI_Datatype)0x4c00100c)   /* x87 80-bit in a 16-byte slot */
#define MPI_BYTE                ((MPI_Datatype)0x4c00010d)
#define MPI_WCHAR               ((MPI_Datatype)0x4c00040e)
#define MPI_PACKED              ((MPI_Datatype)0x4c00010f)
#define MPI_LB                  ((MPI_Datatype)0x4c000010)
#define MPI_UB                  ((MPI_Datatype)0x4c000011)
#define MPI_2INT                ((MPI_Datatype)0x4c000816)
#define MPI_SIGNED_CHAR         ((MPI_Datatype)0x4c000118)
#define MPI_UNSIGNED_LONG_LONG  ((MPI_Datatype)0x4c000819)
#define MPI_FLOAT_INT           ((MPI_Datatype)0x8c000000)
#define MPI_DOUBLE_INT          ((MPI_Datatype)0x8c000001)
#define MPI_LONG_INT            ((MPI_Datatype)0x8c000002)
#define MPI_SHORT_INT           ((MPI_Datatype)0x8c000003)
#define MPI_LONG_DOUBLE_INT     ((MPI_Datatype)0x8c000004)   /* {long double; int}, 32 B */
#define MPI_INT8_T              ((MPI_Datatype)0x4c000137)
#define MPI_INT16_T             ((MPI_Datatype)0x4c000238)
#define MPI_INT32_T             ((MPI_Datatype)0x4c000439)
#define MPI_INT64_T             ((MPI_Datatype)0x4c00083a)
#define MPI_UINT8_T             ((MPI_Datatype)0x4c00013b)
#define MPI_UINT16_T            ((MPI_Datatype)0x4c00023c)
#define MPI_UINT32_T            ((MPI_Datatype)0x4c00043d)
#define MPI_UINT64_T            ((MPI_Datatype)0x4c00083e)
#define MPI_C_BOOL              ((MPI_Datatype)0x4c00013f)
#define MPI_C_FLOAT_COMPLEX     ((MPI_Datatype)0x4c000840)
#define MPI_C_COMPLEX           MPI_C_FLOAT_COMPLEX
#define MPI_C_DOUBLE_COMPLEX    ((MPI_Datatype)0x4c001041)
#define MPI_C_LONG_DOUBLE_COMPLEX ((MPI_Datatype)0x4c002042) /* long double _Complex, 32 B */
#define MPIX_C_FLOAT16          ((MPI_Datatype)0x4c000246)
#define MPI_AINT                ((MPI_Datatype)0x4c000843)
#define MPI_OFFSET              ((MPI_Datatype)0x4c000844)
#define MPI_COUNT               ((MPI_Datatype)0x4c000845)

/* ---- the hot path ------------------------------------------------------ */

/* MPI_Reduce_local (reduce_local.c:155): inoutbuf[i] = op(inbuf[i], inoutbuf[i]),
 * i in [0,count).  Buffers may be HIP device memory, pinned host memory or
 * pageable host memory, in any combination; the combine always runs on the
 * GPU.  Synchronous: the result is complete in inoutbuf on return. */
MPICH_API_PUBLIC int MPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op);
MPICH_API_PUBLIC int PMPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op);

/* MPIR_Reduce_local (reduce_local.c:35): no argument validation; builtin ops
 * dispatch through MPIR_Op_table[op & 0xf], user ops through their function. */
int MPIR_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op);

/* ---- op kernels and tables (mpir_op.h:131-189, allreduce.c:121-139) --- */
void MPIR_MAXF(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_MINF(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_SUM(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_PROD(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_LAND(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_BAND(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_LOR(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_BOR(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_LXOR(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_BXOR(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_MAXLOC(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_MINLOC(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_REPLACE(void *invec, void *inoutvec, int *len, MPI_Datatype * type);
void MPIR_NO_OP(void *invec, void *inoutvec, int *len, MPI_Datatype * type);

int MPIR_MAXF_check_dtype(MPI_Datatype type);
int MPIR_MINF_check_dtype(MPI_Datatype type);
int MPIR_SUM_check_dtype(MPI_Datatype type);
int MPIR_PROD_check_dtype(MPI_Datatype type);
int MPIR_LAND_check_dtype(MPI_Datatype type);
int MPIR_BAND_check_dtype(MPI_Datatype type);
int MPIR_LOR_check_dtype(MPI_Datatype type);
int MPIR_BOR_check_dtype(MPI_Datatype type);
int MPIR_LXOR_check_dtype(MPI_Datatype type);
int MPIR_BXOR_check_dtype(MPI_Datatype type);
int MPIR_MAXLOC_check_dtype(MPI_Datatype type);
int MPIR_MINLOC_check_dtype(MPI_Datatype type);
int MPIR_REPLACE_check_dtype(MPI_Datatype type);
int MPIR_NO_OP_check_dtype(MPI_Datatype type);

#define MPIR_OP_N_BUILTIN 15
typedef int (MPIR_Op_check_dtype_fn) (MPI_Datatype);
extern MPI_User_function *MPIR_Op_table[MPIR_OP_N_BUILTIN];
extern MPIR_Op_check_dtype_fn *MPIR_Op_check_dtype_table[MPIR_OP_N_BUILTIN];
#define MPIR_OP_HDL_TO_FN(op) MPIR_Op_table[((op)&0xf)]
#define MPIR_OP_HDL_TO_DTYPE_FN(op) MPIR_Op_check_dtype_table[((op)&0xf)]

/* ---- user ops (op_create.c, op_free.c, op_commutative.c) ------------- */
MPICH_API_PUBLIC int MPI_Op_create(MPI_User_function * user_fn, int commute, MPI_Op * op);
MPICH_API_PUBLIC int PMPI_Op_create(MPI_User_function * user_fn, int commute, MPI_Op * op);
MPICH_API_PUBLIC int MPI_Op_free(MPI_Op * op);
MPICH_API_PUBLIC int PMPI_Op_free(MPI_Op * op);
MPICH_API_PUBLIC int MPI_Op_commutative(MPI_Op op, int *commute);
MPICH_API_PUBLIC int PMPI_Op_commutative(MPI_Op op, int *commute);
int MPIR_Op_is_commutative(MPI_Op op);

/* ---- errors ------------------------------------------------------------ */
#define MPI_MAX_ERROR_STRING 512
MPICH_API_PUBLIC int MPI_Error_class(int errorcode, int *errorclass);
MPICH_API_PUBLIC int MPI_Error_string(int errorcode, char *string, int *resultlen);

/* ---- extensions -------------------------------------------------------- */
/* Stream-ordered variant: enqueue the combine on `hip_stream` (a hipStream_t,
 * NULL = the calling thread's library stream) and return without waiting.
 * Both buffers must be device-accessible (hipMalloc / managed / mapped);
 * host-only pointers give MPI_ERR_BUFFER.  Same validation and error classes
 * as MPI_Reduce_local; user ops give MPI_ERR_OP (they run on the host). */
MPICH_API_PUBLIC int MPIX_Reduce_local_stream(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype,
                             MPI_Op op, void *hip_stream);
/* Multi-operand local reduction: outbuf = fold of n device buffers, in the
 * association a reduction schedule would produce by calling MPIR_Reduce_local
 * step by step (bit-identical to doing exactly that):
 *   MPIX_ORDER_TREE  (n a power of two <= 64): ((b0+b1)+(b2+b3))+((b4+b5)+(b6+b7)) --
 *       recursive halving, reduce_intra_reduce_scatter_gather.c:186-249;
 *   MPIX_ORDER_CHAIN (1 <= n <= 64): ((b0+b1)+b2)+... -- pairwise,
 *       reduce_scatter_block_intra_pairwise.c:97-134.
 * Passes over HBM: one for TREE (any n) and for CHAIN with n <= 8; CHAIN with
 * n > 8 folds 7 more operands per pass into outbuf, ceil((n-1)/7) passes.
 * In each step the left operand is the step's inoutbuf.  outbuf may be
 * inbufs[0] exactly; any other overlap of outbuf with an operand is
 * MPI_ERR_BUFFER.  hip_stream NULL: synchronous on the library stream;
 * otherwise enqueued on that stream without waiting.  Builtin ops and basic
 * types with the same validation as MPI_Reduce_local. */
#define MPIX_ORDER_TREE  0
#define MPIX_ORDER_CHAIN 1
MPICH_API_PUBLIC int MPIX_Reduce_local_multi(const void *const *inbufs, int n, void *outbuf, int count,
                            MPI_Datatype datatype, MPI_Op op, int order, void *hip_stream);
/* Batched local reduction: nsegs independent MPI_Reduce_local's under one
 * (op, datatype) in one kernel launch -- a bucket of gradient tensors, the
 * per-block combines of an accumulate on a derived target type, the blocks of
 * a ragged reduce-scatter, the sub-ranges of a schedule step.  Each segment's
 * result is bit-identical to MPI_Reduce_local(inbuf, inoutbuf, count, ...).
 *   hip_stream NULL: synchronous on the calling thread's library stream, every
 *       result complete on return; otherwise enqueued on that stream without
 *       waiting (the segment table is copied into the launch: `segs` may be
 *       reused at once).
 *   Builtin ops and basic types, each segment validated as MPI_Reduce_local
 *       validates (MPI_REPLACE, MPI_NO_OP, null and invalid ops: MPI_ERR_OP;
 *       inbuf == inoutbuf: MPI_ERR_BUFFER under MPIR_CVAR_COLL_ALIAS_CHECK;
 *       MPI_IN_PLACE: MPI_ERR_BUFFER); user ops give MPI_ERR_OP (they run on
 *       the host), MPI_LAND / MPI_LOR on floating types MPI_ERR_OP.
 *   nsegs == 0 succeeds; nsegs < 0, or segs == NULL with nsegs > 0, is
 *       MPI_ERR_ARG.  A segment with count == 0 is skipped and its pointers
 *       are not looked at; count < 0 is MPI_ERR_COUNT.
 *   Every non-empty segment's two buffers must be device-resident, all on one
 *       device (else MPI_ERR_BUFFER).
 *   Everything is validated and classified before the first launch: a call
 *       that returns an error has modified nothing.
 *   Segments may share or overlap inbufs.  Two segments whose inoutbuf ranges
 *       overlap, or an inbuf overlapping another segment's inoutbuf, are
 *       undefined (not checked): the segments run concurrently.
 *   A batch with exactly one non-empty segment is the single call.
 * More non-empty segments than fit one launch's kernel arguments (127) run as
 * back-to-back launches on the same stream.  Many pieces of two operands (an
 * indexed type, an IOV) are MPIX_Reduce_local_ragged's, one launch however
 * many: measured ahead of this call from 128 pieces on, behind it below that
 * (by 1 to 3.6 us on pieces around 16 KiB; see there). */
typedef struct MPIX_Reduce_local_seg { const void *inbuf; void *inoutbuf; int count; } MPIX_Reduce_local_seg;
MPICH_API_PUBLIC int MPIX_Reduce_local_batch(const MPIX_Reduce_local_seg *segs, int nsegs,
                            MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Strided local reduction: the rows of a vector-shaped operand in one launch --
 * the target of an accumulate on an MPI_Type_vector / hvector type, a
 * sub-matrix, a halo face, a column.  For r in [0, nblocks):
 *   MPI_Reduce_local((char *) inbuf + r * in_stride, (char *) inoutbuf + r * inout_stride,
 *                    blocklen, datatype, op)
 * every row bit-identical to that call; the bytes between rows are never read
 * or written.  Strides are in bytes (MPI_Type_create_hvector's unit).
 *   hip_stream NULL: synchronous on the calling thread's library stream, every
 *       row complete on return; otherwise enqueued on that stream without
 *       waiting.  The launch carries the five numbers that describe the operands
 *       in its kernel arguments: nothing of the caller's is read afterwards.
 *   Builtin ops and basic types, validated as the batch validates a segment
 *       (MPI_REPLACE, MPI_NO_OP, null and invalid ops: MPI_ERR_OP; inbuf ==
 *       inoutbuf: MPI_ERR_BUFFER under MPIR_CVAR_COLL_ALIAS_CHECK; MPI_IN_PLACE:
 *       MPI_ERR_BUFFER); user ops give MPI_ERR_OP (they run on the host),
 *       MPI_LAND / MPI_LOR on floating types MPI_ERR_OP.
 *   nblocks < 0 or blocklen < 0 is MPI_ERR_COUNT.  Either one 0 succeeds, and
 *       the pointers are not looked at.
 *   A negative stride is MPI_ERR_ARG.  With nblocks > 1, inout_stride below the
 *       row's bytes (blocklen x the datatype's size) is MPI_ERR_ARG: output rows
 *       would overlap.  in_stride may be anything >= 0; 0 combines the same
 *       input row into every output row.
 *   The first and the last byte of each operand's span must be device memory,
 *       all on one device (else MPI_ERR_BUFFER); what lies between is the
 *       caller's, as with any MPI buffer.  Host operands are not taken (the
 *       batch refuses them too): MPI_Reduce_local row by row serves them.
 *   Everything is validated and classified before the first launch: a call
 *       that returns an error has modified nothing.
 *   An input span overlapping the output span is undefined (not checked, but
 *       for inbuf == inoutbuf above): the rows run concurrently.
 *   nblocks == 1, or both strides equal to the row's bytes (contiguous rows),
 *       is the single call on nblocks x blocklen elements.
 * Equal rows at irregular places are MPIX_Reduce_local_indexed's, ragged rows
 * MPIX_Reduce_local_ragged's. */
MPICH_API_PUBLIC int MPIX_Reduce_local_strided(const void *inbuf, MPI_Aint in_stride,
                              void *inoutbuf, MPI_Aint inout_stride, int nblocks, int blocklen,
                              MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Subarray local reduction: a sub-box of an N-dimensional array on either side,
 * with no table -- ghost cells folded back onto the owner's interior, a packed
 * halo buffer accumulated into an interior region, a periodic boundary wrapped
 * inside one array.  Each operand is what
 *   MPI_Type_create_subarray(ndims, X_sizes, subsizes, X_starts, order, datatype, &t)
 * describes, applied once to X buf, the origin of the whole array; layout and
 * the meaning of `order` (MPI_ORDER_C: the last dimension the fastest,
 * MPI_ORDER_FORTRAN: the first) are the reference's
 * (src/mpi/datatype/type_create_subarray.c:185-258).  X_sizes NULL: that operand
 * is packed -- its sizes are subsizes, its starts 0, X_starts is not looked at.
 * For every index tuple of the box the element of inoutbuf becomes what
 * MPI_Reduce_local on that one pair of elements leaves, bit for bit; every
 * contiguous row of the box is bit-identical to MPI_Reduce_local on it; no byte
 * of either array outside its box is read or written.
 *   hip_stream NULL: synchronous on the calling thread's library stream;
 *       otherwise enqueued on that stream without waiting.  Everything travels
 *       in the kernel arguments: no argument array is read after the call
 *       returns, and a call on a stream is captured into a graph as a linear
 *       chain with nothing to keep alive.
 *   Checked in this order, all before the first launch, so that a call that
 *   returns an error has modified nothing:
 *   1. Builtin ops and basic types as the strided call validates them
 *       (MPI_REPLACE, MPI_NO_OP, null, invalid and user ops: MPI_ERR_OP;
 *       MPI_LAND / MPI_LOR on floating types: MPI_ERR_OP).
 *   2. ndims < 1 or > MPIX_REDUCE_LOCAL_SUBARRAY_MAXDIMS: MPI_ERR_DIMS.  subsizes
 *       NULL, or X_sizes given with X_starts NULL: MPI_ERR_ARG.  order neither
 *       constant: MPI_ERR_ARG.
 *   3. Per dimension in ascending order, inbuf's side then inoutbuf's, as
 *       type_create_subarray.c:104-133 checks them: size < 1, subsize < 1,
 *       start < 0, subsize > size, start > size - subsize: each MPI_ERR_ARG.  An
 *       empty box is refused, as the reference refuses it.
 *   4. The product of an operand's sizes times the datatype's size not fitting
 *       an MPI_Aint: MPI_ERR_ARG.
 *   5. MPI_IN_PLACE for either buffer: MPI_ERR_BUFFER.
 *   6. inbuf == inoutbuf under MPIR_CVAR_COLL_ALIAS_CHECK: MPI_ERR_BUFFER, unless
 *       both sides give sizes, the two size arrays are equal and the boxes are
 *       disjoint: some dimension has |in_starts[d] - inout_starts[d]| >=
 *       subsizes[d].  That is the periodic wrap inside one array.  Any other
 *       overlap of the input box with the output box is undefined and not checked.
 *   7. The first and the last byte of each operand's box must be device memory
 *       on one device (MPI_ERR_BUFFER).  Host operands are not taken.
 * The box is brought to a row of contiguous elements under k outer dimensions
 * (dimensions of subsize 1 dropped; a dimension the box spans on both sides
 * merged into the next).  k == 0 is the single call and k == 1
 * MPIX_Reduce_local_strided, each with everything it does; k == 2 or 3 is one
 * launch of a kernel of its own (more only past 2^23 workgroups); from k == 4 on
 * the outermost k - 3 dimensions are looped on the host as back-to-back launches
 * on the same stream.  The wide / narrow threshold is the strided call's.
 * Measured (tools/subarray_ab.py; DESIGN.md, Subarray reductions): the 254^3
 * interior of a 256^3 array of doubles in 102 us against 4.6 ms for the loop of
 * 254 strided calls and 105 us for MPIX_Reduce_local_indexed over a device table
 * of the 64,516 rows; its one-cell face across the fast axis in 18.8 us against
 * 2.6 ms and 22.7 us.  One call costs what 1.1 to 5.9 planes of the loop cost; it
 * was ahead of the indexed call at every shape tried, by 1.4-3.7 % on 2 KiB rows
 * and 12-21 % on rows of one or two elements.  A box that collapses to one outer
 * dimension runs 0.3-0.5 us above the strided call it becomes. */
#define MPI_ERR_DIMS      11     /* mpi.h.in:802 */
#define MPI_ORDER_C       56     /* mpi.h.in:537-538 */
#define MPI_ORDER_FORTRAN 57
#define MPIX_REDUCE_LOCAL_SUBARRAY_MAXDIMS 8
MPICH_API_PUBLIC int MPIX_Reduce_local_subarray(const void *inbuf, const int in_sizes[], const int in_starts[],
                              void *inoutbuf, const int inout_sizes[], const int inout_starts[],
                              int ndims, const int subsizes[], int order,
                              MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Fetching local reduction: the old value out and the combine in one pass -- the
 * target side of MPI_Get_accumulate / MPI_Fetch_and_op, which copies the target's
 * old contents into the response buffer and then combines the origin's data into
 * the target (src/mpid/ch3/src/ch3u_rma_pkthandler.c:899-917 "NOTE: 'copy data +
 * ACC' needs to be atomic", :1354; ch3u_handle_recv_req.c:207, 274, 356, 441, 494,
 * 1350, 1423, 1567), and any schedule step that must keep the previous partial
 * result while it folds the next operand into it.  For i in [0, count):
 *   fetchbuf[i] receives the bytes inoutbuf[i] held on entry;
 *   inoutbuf[i] becomes what MPI_Reduce_local(inbuf, inoutbuf, count, datatype, op)
 *       would have left there, bit for bit.
 * One kernel launch and four streams through memory, where a device copy followed
 * by MPI_Reduce_local is two launches and reads inoutbuf twice.
 *   The fetched bytes are a byte copy of count x the datatype's size bytes, never
 *       passed through an arithmetic type: NaN payloads and the six padding bytes
 *       of each x87 long double slot arrive as they were.
 *   The value combined and the value fetched come from one and the same read of
 *       inoutbuf[i]: the reference's atomicity requirement holds by construction.
 *   Ops: the builtin ops on basic types, validated as MPIR_ERRTEST_OP_GACC
 *       (src/include/mpir_err.h:528-539) plus MPI_Reduce_local's datatype check.
 *       MPI_OP_NULL and invalid handles: MPI_ERR_OP; user ops: MPI_ERR_OP (not
 *       predefined); MPI_LAND / MPI_LOR on floating types: MPI_ERR_OP, as
 *       everywhere in this library.  MPI_NO_OP and MPI_REPLACE, which every other
 *       entry point but MPIX_Reduce_local_fetch_ragged refuses, are accepted on
 *       every basic type; on a derived
 *       handle they are MPI_ERR_TYPE, as MPIR_REPLACE answers.
 *   MPI_NO_OP (an atomic get) never looks at inbuf, which may be NULL; inoutbuf is
 *       not written; fetchbuf receives the copy.  MPI_REPLACE (a swap) puts the old
 *       bytes in fetchbuf and sets inoutbuf = inbuf.  Both are stream-ordered
 *       device copies, no kernel.
 *   count < 0 is MPI_ERR_COUNT.  count == 0 succeeds and no pointer is looked at.
 *   inbuf == inoutbuf: MPI_ERR_BUFFER under MPIR_CVAR_COLL_ALIAS_CHECK.
 *       MPI_IN_PLACE for any of the three buffers: MPI_ERR_BUFFER.  fetchbuf NULL
 *       with count > 0: MPI_ERR_BUFFER.  fetchbuf's byte range overlapping
 *       inoutbuf's, or inbuf's unless the op is MPI_NO_OP: MPI_ERR_BUFFER, checked
 *       whatever the alias check says, as MPIX_Reduce_local_multi checks its output
 *       against its operands.  An inbuf range partly overlapping inoutbuf stays
 *       undefined, as elsewhere.
 *   All buffers that are looked at must be device-resident on one device (else
 *       MPI_ERR_BUFFER).  Host operands are not taken, as the batch and the strided
 *       call refuse them.
 *   Everything is validated and classified before the first launch: a call that
 *       returns an error has written nothing.
 *   hip_stream NULL: synchronous on the calling thread's library stream, both
 *       results complete on return; otherwise enqueued on that stream without
 *       waiting.  The call is self-contained in its kernel arguments and can be
 *       captured into a HIP graph. */
MPICH_API_PUBLIC int MPIX_Reduce_local_fetch(const void *inbuf, void *inoutbuf, void *fetchbuf, int count,
                            MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Indexed local reduction: equal blocks at the places a displacement table
 * names, in one launch -- the target of an accumulate on an
 * MPI_Type_create_indexed_block / hindexed_block type (a scatter-add: embedding
 * row gradients, sparse updates), or the gather-reduce the other way round.
 * For k in [0, nblocks):
 *   MPI_Reduce_local((char *) inbuf + in_off(k), (char *) inoutbuf + io_off(k),
 *                    blocklen, datatype, op)
 * every block bit-identical to that call; no byte outside the blocks is read or
 * written.  X_off(k) = X_displs[k] * disp_unit bytes where the table is given,
 * k * blocklen * the datatype's size where it is NULL (a packed operand).
 *   disp_unit 1 is hindexed_block (byte displacements), the type's extent
 *       indexed_block, a row's bytes makes the table row indices.  in_displs
 *       NULL with inout_displs given is the scatter (the accumulate target),
 *       the reverse the gather; both may be given.  Both NULL is the single
 *       call on nblocks x blocklen elements.
 *   Displacements may be negative.  A repeated in_displs entry is fine (input
 *       is only read).  Output blocks that overlap each other, or an input
 *       block, are undefined and not checked: MPI forbids overlapping target
 *       entries in an accumulate, and the blocks run concurrently.  A table with
 *       repeated targets (embedding rows hit twice, several accumulates queued
 *       to one location) is MPIX_Reduce_local_indexed_ordered's.  The old
 *       target blocks out as well (a Get_accumulate on this shape) is
 *       MPIX_Reduce_local_fetch_indexed_ordered with order NULL.
 *   Ops and types as the strided call validates them, in its order: MPI_REPLACE,
 *       MPI_NO_OP, null, invalid and user ops, and MPI_LAND / MPI_LOR on
 *       floating types: MPI_ERR_OP; nblocks < 0 or blocklen < 0: MPI_ERR_COUNT;
 *       MPI_IN_PLACE: MPI_ERR_BUFFER; inbuf == inoutbuf: MPI_ERR_BUFFER under
 *       MPIR_CVAR_COLL_ALIAS_CHECK; disp_unit <= 0: MPI_ERR_ARG.  Either count 0
 *       succeeds, and no pointer is looked at, the tables included; the op and
 *       disp_unit are still checked then, as the strided call still checks its
 *       op and the sign of its strides.
 *   Both base pointers must be device memory on one device (MPI_ERR_BUFFER).
 *       A table may be device memory on that device: the kernel reads it, and
 *       it must stay unchanged until the work completes.  With hip_stream NULL
 *       a table may also be host memory: the library copies it to a buffer of
 *       its own ahead of the kernel, and, reading it anyway, checks every
 *       displs[k] * disp_unit for overflow (MPI_ERR_ARG) and that the lowest
 *       block's first byte and the highest block's last byte are device memory
 *       (MPI_ERR_BUFFER).  A host table with a stream is MPI_ERR_BUFFER.
 *   hip_stream NULL: synchronous, every block complete on return; otherwise
 *       enqueued on that stream without waiting; with device tables everything
 *       else travels in the kernel arguments, so the call can be captured into
 *       a graph.
 *   Everything is validated and classified before the first launch: a call
 *       that returns an error has modified nothing.
 *   Blocks shorter than the strided call's wide threshold move as 16-byte
 *       vectors only where the library can tell without reading a table that
 *       every address is a multiple of 16: blocklen x size and both bases
 *       multiples of 16, and disp_unit a multiple of 16.  Callers with 16-byte
 *       aligned blocks should pass disp_unit 16 (or a multiple) and scale the
 *       displacements, not byte displacements with disp_unit 1, which move
 *       element by element.
 * Ragged blocks (MPI_Type_indexed proper) are MPIX_Reduce_local_ragged's, which
 * also takes equal ones but reads a third table and searches it: 4 to 7 % more
 * time than this call on 4096 blocks of 64 KiB, about 20 % (3.6 to 3.9 us) on
 * 65,536 blocks of 256 bytes.  Against MPIX_Reduce_local_batch
 * over the same equal blocks this call was measured a little behind it at two
 * blocks (by the spread between runs) and ahead from eight on.  Blocks at a constant stride are
 * MPIX_Reduce_local_strided's: it reads no table and plans its grid exactly, and
 * takes somewhat less time on the same operands (Indexed reductions,
 * has the figures for both). */
MPICH_API_PUBLIC int MPIX_Reduce_local_indexed(const void *inbuf, const MPI_Aint * in_displs,
                              void *inoutbuf, const MPI_Aint * inout_displs, MPI_Aint disp_unit,
                              int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Ordered indexed local reduction: MPIX_Reduce_local_indexed whose output table
 * may name the same block any number of times -- a scatter-add with repeated
 * rows (embedding gradients), many contributions assembled into one node, or the
 * accumulates an RMA target has queued for one location, which MPI orders
 * (MPI-3.1 11.7.2, accumulate_ordering).  The call is exactly
 *   for k = 0 .. nblocks - 1, one after another in that order:
 *     MPI_Reduce_local((char *) inbuf + in_off(k), (char *) inoutbuf + io_off(k),
 *                      blocklen, datatype, op)
 * bit for bit (in_off, io_off: the indexed call's), deterministic where atomics
 * are not; each distinct target block is read once and written once, however
 * many contributions it gets.  No byte outside the blocks is read or written,
 * and no table is written.  The value the target held before each contribution
 * (MPI_Fetch_and_op, MPI_Get_accumulate) is MPIX_Reduce_local_fetch_indexed_ordered's.
 *   Two output blocks must have equal inout_displs entries or be disjoint;
 *       partial overlap stays undefined, as does an input block that overlaps
 *       an output block.
 *   order has nblocks ints and puts the blocks of one target side by side: a
 *       permutation of [0, nblocks) such that inout_displs[order[p]] is
 *       non-decreasing in p and, within equal displacements, order[p] is
 *       ascending (ties keep table order).  That is a stable argsort of
 *       inout_displs by signed value; any framework's will do, and
 *       MPIX_Reduce_local_order makes one.  Build it once per index pattern and
 *       combine many times.
 *   order NULL is a promise of no repeats: the call is
 *       MPIX_Reduce_local_indexed unchanged.  order with inout_displs NULL is
 *       MPI_ERR_ARG: a packed target has no repeats.
 *   Validation is the indexed call's, in its order: ops (MPI_REPLACE and
 *       MPI_NO_OP stay MPI_ERR_OP), counts, MPI_IN_PLACE, the alias check,
 *       disp_unit; either count 0 succeeds and looks at no pointer.
 *   Bases and tables have the indexed call's residency rules, order a third
 *       table under them: device memory on the operands' device, or, with
 *       hip_stream NULL, host memory (with a stream: MPI_ERR_BUFFER).  A host
 *       order is checked: every entry in range, none twice, and, where
 *       inout_displs is a host table too, the two ordering conditions
 *       (MPI_ERR_ARG).  A device order that breaks its conditions is the
 *       caller's error and the result is undefined; the kernel still clamps
 *       every index it reads from it, so its reads of all three tables stay
 *       inside them.
 *   A call that returns an error has written nothing.
 *   hip_stream as in the indexed call; with device tables everything travels in
 *       the kernel arguments: nothing is allocated, no library scratch is used,
 *       and the call can be captured into a graph.
 *   The blocks of one target are folded serially by one slice of one workgroup
 *       (one lane per 16 bytes of a narrow block, one workgroup per 16 KiB tile
 *       of a wide one): the order is the contract, and a tree would change
 *       floating-point results.  A hot row costs time in proportion to its
 *       contributions; distinct targets run concurrently.
 *   Measured: fp32 MPI_SUM, medians of alternated rounds (Ordered
 *       indexed reductions, has the table).  65,536 blocks of 256 bytes: with
 *       no repeats 22.7 us against the indexed call's 19.2 (1.18 x: the order
 *       entry and the neighbours' displacements are read before any data); 4
 *       blocks per target 36 us against 51 for four duplicate-free rounds of
 *       the indexed call, 64 per target 52 us against 745.  4096 blocks of 64
 *       KiB: 142 us against the indexed call's 162 with no repeats, 97 against
 *       196 at 4 per target, 340 against 840 at 64.  A hot row: all 65,536
 *       blocks of 256 bytes on one target take 29 ms (0.44 us a contribution),
 *       all 4096 of 64 KiB 4.2 ms (1 us): keep such a row out of the table, or
 *       pre-reduce it, where the order of its sum may be chosen.  Where only
 *       determinism is asked of a row's sum, not table order,
 *       MPIX_Reduce_local_indexed_chunked folds a hot row in chunks of 64.
 *       MPIX_Reduce_local_order: 56 us for 65,536 entries, 31 us for 4096. */
MPICH_API_PUBLIC int MPIX_Reduce_local_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs,
                              void *inoutbuf, const MPI_Aint * inout_displs, const int *order,
                              MPI_Aint disp_unit, int nblocks, int blocklen,
                              MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* The order table of a displacement table, for MPIX_Reduce_local_indexed_ordered:
 * order[p] = the block at sorted position p, a stable sort of (displs[k], k) by
 * the signed displacement.  nblocks < 0: MPI_ERR_COUNT; nblocks 0 succeeds and
 * looks at nothing.
 *   work is scratch of at least MPIX_Reduce_local_order_worksize(nblocks) bytes
 *       in device memory on the device of displs (fewer work_bytes:
 *       MPI_ERR_ARG); no byte past that size is touched.  With hip_stream NULL
 *       work may be NULL and the library uses a buffer of its own; with a
 *       stream a NULL work is MPI_ERR_BUFFER.  The size depends on nblocks
 *       alone, never decreases with it, and needs no GPU to ask.
 *   displs and order in device memory: the build is enqueued on the stream, or
 *       synchronous when hip_stream is NULL.  A synchronous call also takes
 *       either table in host memory (copied through the library's table
 *       buffer); with both on the host it is a host stable sort and the GPU
 *       runtime is not opened.  A host table with a stream is MPI_ERR_BUFFER.
 *   The build makes several launches, their number depending on nblocks, and
 *       asks the runtime about the device: capture into a graph is NOT promised.
 *       Build outside the capture, and capture the combine. */
MPICH_API_PUBLIC int MPIX_Reduce_local_order_worksize(int nblocks, MPI_Aint * work_bytes);
MPICH_API_PUBLIC int MPIX_Reduce_local_order(const MPI_Aint * displs, int nblocks, int *order,
                              void *work, MPI_Aint work_bytes, void *hip_stream);
/* Chunked indexed local reduction: MPIX_Reduce_local_indexed_ordered's operands
 * and tables for the caller who may choose the order of a row's sum but wants
 * the same bits every time -- accumulate_ordering=none, gradients (a padding
 * token's embedding row), assembly (a boundary node): the workloads whose
 * tables have hot rows.  The contributions of one target are cut into chunks of
 * MPIX_REDUCE_LOCAL_CHUNK = 64, each chunk is folded on its own, and the
 * partials are then folded into the target.  Exactly: for one distinct target
 * displacement d, let its blocks in ascending table number be k_0 < ... <
 * k_{L-1}, C = 64 and m = ceil(L / C).  Then
 *   for j = 0 .. m-1:   P_j := a byte copy of input block k_{jC}
 *     for i = jC+1 .. min((j+1)C, L)-1:
 *       MPI_Reduce_local(input block k_i, P_j, blocklen, datatype, op)
 *   for j = 0 .. m-1:   MPI_Reduce_local(P_j, target block at d, blocklen, datatype, op)
 * bit for bit.  Everything follows from those calls: operand order, the x86 NaN
 * rule, x87 slot padding, pair padding, integer wrap.  A run of one block is
 * the indexed call on it; every longer run, short ones included, goes through
 * its partial, so on floating types this call is NOT the ordered call.  The
 * association of a row depends on that row's own contributions alone: never on
 * what other rows receive, on the launch geometry or on the block size.  C is
 * part of the contract (it fixes the bits), a public constant and not a tuning
 * knob; 64 was chosen, not measured: it makes the two serial levels equal at
 * 4096 contributions and is one wave of positions.
 *   in_off(k), io_off(k), order, the equal-or-disjoint rule for output blocks,
 *       the residency rules and the validation order are the ordered call's.
 *   runstart has nblocks ints: runstart[p] is the smallest sorted position q
 *       with inout_displs[order[q]] == inout_displs[order[p]].  The format is
 *       public, like order's; MPIX_Reduce_local_runs builds it.
 *   order and runstart both NULL: MPIX_Reduce_local_indexed unchanged.  Exactly
 *       one of them NULL, or either given with inout_displs NULL: MPI_ERR_ARG.
 *   A host runstart (hip_stream NULL) is checked against its definition where
 *       order and inout_displs are host tables too, otherwise for 0 <=
 *       runstart[p] <= p (MPI_ERR_ARG); a host order or runstart is read and
 *       checked before the operands' residency.  A device runstart is not checked and a
 *       wrong one gives an undefined result; the kernels still clamp what they
 *       read from it: reads stay inside the tables, writes inside the target
 *       blocks and work.
 *   work is device scratch for the partials of runs longer than one chunk, at
 *       least MPIX_Reduce_local_chunked_worksize(nblocks, blocklen, datatype)
 *       bytes on the operands' device (fewer work_bytes: MPI_ERR_ARG); no byte
 *       past that size is touched.  With hip_stream NULL work may be NULL and
 *       the library uses a buffer of its own; with a stream a NULL work is
 *       MPI_ERR_BUFFER.  The size depends on its three arguments alone, never
 *       decreases in nblocks or blocklen, and needs no GPU to ask.
 *   A call that returns an error has written nothing, in the target or in work.
 *   Two launches per call (several of each where a launch's workgroup cap asks
 *       for it), all of the first kernel before any of the second; no workgroup
 *       waits for another.  With device tables and the caller's work nothing is
 *       allocated and the call can be captured into a graph: a linear chain.
 *   Measured: fp32 MPI_SUM against MPIX_Reduce_local_indexed_ordered on the same
 *       operands, medians of alternated rounds (tools/indexed_chunked_ab.py,
 *       profiles/indexed_chunked/indexed_chunked_ab.log; DESIGN.md, Chunked
 *       indexed reductions, has the table).  A hot row: all 65,536 blocks of 256
 *       bytes on one target take 494 us against the ordered call's 29.1 ms
 *       (59 x), all 4096 of 64 KiB 345 us against 4.19 ms (12 x).  64 per
 *       target: 50.8 us against 52.0, and 287 against 341 on 64 KiB blocks.
 *       Without hot rows the fourth table and the second launch cost: 27.6 us
 *       against 22.7 with no repeats on 256-byte blocks (1.22 x), 154 against
 *       143 on 64 KiB blocks (1.08 x); 4 per target 30.3 against 35.7 and 97.9
 *       against 96.6.  A caller whose tables have no hot rows keeps the indexed
 *       or the ordered call.  MPIX_Reduce_local_runs: 14 us for 65,536 entries,
 *       12 us for 4096. */
#define MPIX_REDUCE_LOCAL_CHUNK 64
MPICH_API_PUBLIC int MPIX_Reduce_local_indexed_chunked(const void *inbuf, const MPI_Aint * in_displs,
                              void *inoutbuf, const MPI_Aint * inout_displs, const int *order,
                              const int *runstart, MPI_Aint disp_unit, int nblocks, int blocklen,
                              MPI_Datatype datatype, MPI_Op op, void *work, MPI_Aint work_bytes,
                              void *hip_stream);
MPICH_API_PUBLIC int MPIX_Reduce_local_chunked_worksize(int nblocks, int blocklen, MPI_Datatype datatype,
                              MPI_Aint * work_bytes);
/* The runstart table of MPIX_Reduce_local_indexed_chunked from displs and its
 * order table.  nblocks < 0: MPI_ERR_COUNT; nblocks 0 succeeds and looks at
 * nothing; a NULL table: MPI_ERR_ARG.
 *   All three tables in device memory on one device: one kernel (a lower-bound
 *       binary search per position), enqueued on the stream or synchronous when
 *       hip_stream is NULL; no scratch, nothing allocated, and it can be
 *       captured into a graph.
 *   A synchronous call also takes any of the tables in host memory (copied
 *       through the library's table buffer); with all three on the host it is a
 *       host loop and the GPU runtime is not opened (an order entry out of
 *       range: MPI_ERR_ARG).  A host table with a stream is MPI_ERR_BUFFER. */
MPICH_API_PUBLIC int MPIX_Reduce_local_runs(const MPI_Aint * displs, const int *order, int nblocks,
                              int *runstart, void *hip_stream);
/* Ragged local reduction: many pieces of unequal length in one launch -- the
 * target of an accumulate on an MPI_Type_indexed / MPI_Type_create_hindexed
 * type, a sub-array with a ragged edge, any list of (location, length) pieces
 * the segment code makes of a derived type; on a GPU also a CSR-shaped
 * scatter-add or gather-reduce (variable-length rows, embedding bags, halo
 * lists per neighbour).  starts has npieces + 1 entries, the pieces' element
 * offsets in packed order (CSR row pointers): starts[0] == 0, non-decreasing,
 * starts[npieces] == count.  Piece k has len(k) = starts[k + 1] - starts[k]
 * elements; none is fine.  For k in [0, npieces):
 *   MPI_Reduce_local((char *) inbuf + in_off(k), (char *) inoutbuf + io_off(k),
 *                    len(k), datatype, op)
 * every piece bit-identical to that call; no byte outside the pieces is read or
 * written, and no table is written.  X_off(k) = X_displs[k] * disp_unit bytes
 * where the table is given, starts[k] * the datatype's size where it is NULL (a
 * packed operand; the size is the one MPIX_Reduce_local_indexed uses there).
 * count is the packed side's element count.
 *   disp_unit, NULL tables, signed displacements, repeated input pieces and
 *       overlapping output pieces (undefined, not checked) are as in
 *       MPIX_Reduce_local_indexed.  Both tables NULL is the single call on count
 *       elements, and starts is not looked at.  Equal pieces whose targets
 *       repeat are MPIX_Reduce_local_indexed_ordered's.
 *   Ops and types as the indexed call validates them, in its order; npieces < 0
 *       or count < 0: MPI_ERR_COUNT; MPI_IN_PLACE: MPI_ERR_BUFFER; inbuf ==
 *       inoutbuf: MPI_ERR_BUFFER under MPIR_CVAR_COLL_ALIAS_CHECK; disp_unit <=
 *       0: MPI_ERR_ARG.  count 0 succeeds, and no pointer is looked at, the
 *       tables included; the op and disp_unit are still checked then.  count >
 *       0 with npieces 0, and starts NULL while a table is given: MPI_ERR_ARG.
 *   Both base pointers must be device memory on one device, and a packed
 *       side's last byte (MPI_ERR_BUFFER).  Each of the three tables may be
 *       device memory on that device: the kernel reads it, and it must stay
 *       unchanged until the work completes.  A device starts that breaks its
 *       three conditions is the caller's error: what the call then combines is
 *       undefined (the library's own reads of the tables stay inside them).
 *       With hip_stream NULL each table may also be host memory: the library
 *       copies it to a buffer of its own ahead of the kernel, and, reading it
 *       anyway, checks starts' three conditions (MPI_ERR_ARG), every displs[k] *
 *       disp_unit for overflow (MPI_ERR_ARG) and, where starts is a host table
 *       too, that the first byte of the lowest non-empty piece and the last
 *       byte of the highest are device memory (MPI_ERR_BUFFER).  A host table
 *       with a stream is MPI_ERR_BUFFER.
 *   hip_stream NULL: synchronous, every piece complete on return; otherwise
 *       enqueued on that stream without waiting; with device tables everything
 *       else travels in the kernel arguments, so the call can be captured into
 *       a graph.
 *   Everything is validated before anything is enqueued: a call that returns
 *       an error has modified nothing.
 *   Always one launch: the work is divided by packed element, 16 KiB to a
 *       workgroup, never by piece, so one long piece among many short ones
 *       costs nothing extra.  A 16-byte chunk of packed space moves as one
 *       vector where it lies inside one piece and both its addresses are
 *       multiples of 16 (decided on the device, chunk by chunk: disp_unit 1
 *       with aligned byte displacements is as good as disp_unit 16); other
 *       chunks move element by element.  Pieces of 16-byte multiples at
 *       16-byte-aligned places on both sides are all vectors.
 * Against MPIX_Reduce_local_batch on the same pieces (Ragged
 * reductions, has the figures and their spread): this call takes less time from
 * 128 pieces on, where the batch needs its second launch -- about 15.2 against
 * 16.6 us at 128 pieces around 16 KiB, 15.9 against 23.5 at 256, 177 against 340 us
 * at 4096 pieces of 32 to 96 KiB, 26 to 45 us against 3.1 to 3.5 ms at 65,536
 * short pieces -- by far more than the rounds' spread (0.1 to 0.3 us at the small
 * shapes).  Up to 127 pieces around 16 KiB the batch, whose pieces travel in the
 * kernel arguments, takes less: about 10.5 against 13.7 to 14.2 us at 2 pieces,
 * 14.3 against 15.2 at 127.  That shape stays the batch's where a host-side pointer pair per
 * piece is at hand; a table that lives on the device, or a call to be captured
 * in a graph with more pieces than one batch launch holds, is this call's at
 * any piece count.  Equal pieces are MPIX_Reduce_local_indexed's (no starts to
 * read, nothing to search: this call took 4 to 7 % more time on 4096 pieces of
 * 64 KiB and about 20 % more on 65,536 of 256 bytes), pieces at a constant stride
 * MPIX_Reduce_local_strided's. */
MPICH_API_PUBLIC int MPIX_Reduce_local_ragged(const void *inbuf, const MPI_Aint * in_displs,
                             void *inoutbuf, const MPI_Aint * inout_displs, const MPI_Aint * starts,
                             MPI_Aint disp_unit, int npieces, int count, MPI_Datatype datatype, MPI_Op op,
                             void *hip_stream);
/* Fetching ragged local reduction: MPIX_Reduce_local_fetch on a ragged target,
 * in one launch -- the shape of the reference's MPI_Get_accumulate target
 * handler (src/mpid/ch3/src/ch3u_handle_recv_req.c:326-358, also :1391-1423),
 * which under "NOTE: 'copy data + ACC' needs to be atomic" packs the
 * derived-type target into the contiguous response buffer (MPIR_Segment_pack,
 * :339-351) and then runs do_accumulate_op over the same target, piece by piece
 * against the packed origin data (src/mpid/ch3/include/mpidrma.h:930-1021).
 * inbuf is the streamed origin data, packed; fetchbuf is the response buffer,
 * packed; inoutbuf is the target and has the displacement table.  starts,
 * disp_unit, npieces and count mean what they mean in MPIX_Reduce_local_ragged:
 * npieces + 1 packed element offsets, starts[0] == 0, non-decreasing,
 * starts[npieces] == count, empty pieces allowed, signed displacements.  For
 * piece k of len(k) = starts[k + 1] - starts[k] elements at
 * piece = (char *) inoutbuf + inout_displs[k] * disp_unit:
 *   the len(k) x size bytes of fetchbuf at starts[k] x size receive the bytes the
 *       piece held on entry: a byte copy that never passes through a value of the
 *       type, as MPIX_Reduce_local_fetch promises (NaN payloads, x87 slot padding
 *       and pair-type padding arrive as they were);
 *   the piece becomes what MPI_Reduce_local((char *) inbuf + starts[k] x size,
 *       piece, len(k), datatype, op) would leave, bit for bit.
 * No byte outside the pieces is read or written, no byte of fetchbuf outside
 * [0, count x size), and no table.
 *   One read of the target: the value fetched and the value combined come from
 *       one and the same load of each target element; the kernel holds no second
 *       load of inoutbuf, so the reference's atomicity requirement holds by
 *       construction, without a lock.
 *   Ops: validated as MPIX_Reduce_local_fetch validates them
 *       (MPIR_ERRTEST_OP_GACC, src/include/mpir_err.h:528-539, plus
 *       MPI_Reduce_local's datatype check; user ops, and MPI_LAND / MPI_LOR on
 *       floating types: MPI_ERR_OP).  MPI_NO_OP and MPI_REPLACE are accepted on
 *       every basic type, and here both are kernels, byte operations chosen by
 *       the element's size: MPI_NO_OP is a pack, a gather of the pieces into
 *       fetchbuf (MPI_Get of an indexed type; an atomic get): inbuf is not looked
 *       at and may be NULL, the target is not written.  MPI_REPLACE is a swap
 *       (MPI_Put as an unpack, with the old contents out).
 *   Arguments: MPIX_Reduce_local_ragged's rules in its order -- npieces < 0 or
 *       count < 0: MPI_ERR_COUNT; then the op; inbuf == inoutbuf under
 *       MPIR_CVAR_COLL_ALIAS_CHECK and MPI_IN_PLACE for any of the three
 *       buffers: MPI_ERR_BUFFER; disp_unit <= 0: MPI_ERR_ARG; count 0 succeeds
 *       and no pointer or table is looked at (the op and disp_unit are still
 *       checked); count > 0 with npieces 0, and starts NULL while the table is
 *       given: MPI_ERR_ARG.  On top, MPIX_Reduce_local_fetch's rules for
 *       fetchbuf: NULL with count > 0 is MPI_ERR_BUFFER; its packed range
 *       overlapping inbuf's packed range is MPI_ERR_BUFFER whatever the alias
 *       check says, unless the op is MPI_NO_OP.
 *   Tables: device memory at any time, read by the kernel (they must stay
 *       unchanged until the work completes).  With hip_stream NULL either may be
 *       host memory: it is copied to a buffer of the library's ahead of the
 *       kernel and gets the ragged call's checks, starts' three conditions and
 *       the overflow of inout_displs[k] * disp_unit (MPI_ERR_ARG); with both on
 *       the host also the residency of the lowest piece's first byte and the
 *       highest piece's last, and a fetchbuf range that meets ANY byte between
 *       those two is MPI_ERR_BUFFER.  With a device table the library cannot see
 *       the pieces: fetchbuf overlapping a target piece is then undefined, as is
 *       a device starts that breaks its conditions (the library's own table
 *       reads stay inside the tables all the same).  A host table with a stream
 *       is MPI_ERR_BUFFER.
 *   inbuf (unless MPI_NO_OP), inoutbuf and fetchbuf must be device memory on one
 *       device (MPI_ERR_BUFFER); host operands are not taken.
 *   Everything is validated before anything is enqueued: a call that returns an
 *       error has written nothing.
 *   inout_displs NULL (a contiguous target) is MPIX_Reduce_local_fetch on count
 *       elements; starts is not looked at.
 *   hip_stream NULL: synchronous; otherwise enqueued on that stream without
 *       waiting.  With device tables the call is self-contained in its kernel
 *       arguments and can be captured into a graph.  Always ONE launch: the
 *       work is divided by packed element, 16 KiB to a workgroup.  A 16-byte
 *       chunk of packed space inside one piece moves as one vector where the
 *       target's address, inbuf's and fetchbuf's are all multiples of 16 (the
 *       target's is decided on the device, chunk by chunk); other chunks move
 *       element by element.
 *   Equal-block and constant-stride targets (MPI_Type_create_indexed_block,
 *       MPI_Type_vector) are expressed with a uniform starts, starts[k] = k x
 *       blocklen; a starts == NULL shortcut for equal pieces is deliberately not
 *       part of this call.  Equal blocks whose targets repeat, each contribution
 *       fetching what the one before left, are MPIX_Reduce_local_fetch_indexed_ordered's.
 * Measured (Fetching ragged reductions, has the tables and the spread
 * of the rounds): against what a caller did before, a device copy per piece into
 * fetchbuf followed by MPIX_Reduce_local_ragged, this call takes less time at
 * every piece count measured -- about 14.5 against 54 us at 2 pieces around 16
 * KiB, 15.0 against 158 to 161 at 32, 16.6 against 912 at 256 (the rounds' medians
 * spread by 0.1 us for this call, by up to 20 us for the copies).  Against
 * MPIX_Reduce_local_ragged alone, which moves three streams where this call moves
 * four, it takes 1.00 to 1.04 times as long up to 256 pieces and 1.10 to 1.23
 * times at 4096 pieces of 32 to 96 KiB (195 to 214 against 175 to 177 us), below
 * the 4/3 that memory bandwidth alone would make it.  Against
 * MPIX_Reduce_local_fetch on the same bytes in contiguous buffers it takes 1.16 to
 * 1.23 times as long at 256 MiB and 4.2 to 4.8 us more up to 256 pieces: a
 * contiguous target stays that call's (inout_displs NULL is that call). */
MPICH_API_PUBLIC int MPIX_Reduce_local_fetch_ragged(const void *inbuf, void *inoutbuf,
                             const MPI_Aint * inout_displs, void *fetchbuf, const MPI_Aint * starts,
                             MPI_Aint disp_unit, int npieces, int count, MPI_Datatype datatype, MPI_Op op,
                             void *hip_stream);
/* Fetching ordered indexed local reduction: an ordered fetch-and-op.
 * MPIX_Reduce_local_indexed_ordered with every intermediate value handed out --
 * what the MPI_Fetch_and_op / MPI_Get_accumulate operations an RMA target has
 * queued for one location must each answer, the value the target held just
 * before that operation ("'copy data + ACC' needs to be atomic",
 * src/mpid/ch3/src/ch3u_rma_pkthandler.c:899-917); also a deterministic
 * fetch-and-add (slot or ticket allocation, histograms that hand out positions),
 * an exclusive running reduction per key in table order (a segmented scan by
 * key), and with MPI_REPLACE a chain of swaps.  The call is exactly
 *   for k = 0 .. nblocks - 1, one after another in that order:
 *     MPIX_Reduce_local_fetch((char *) inbuf + in_off(k), (char *) inoutbuf + io_off(k),
 *                             (char *) fetchbuf + k * blocklen * size, blocklen, datatype, op, ...)
 * (in_off, io_off: the indexed call's; fetchbuf is packed by block number), in
 * the ordered call's launches: fetchbuf block k receives the bytes the target
 * block held after contributions 0 .. k - 1 and before contribution k, and the
 * target ends as MPIX_Reduce_local_indexed_ordered would leave it.
 *   One value: what is stored to fetchbuf and what is combined is one and the
 *       same register value.  The target is loaded once per run of equal
 *       displacements and stored once per run; for MPI_NO_OP it is never stored.
 *   The first block of a run is a byte copy of the old target (NaN payloads, x87
 *       slot padding and pair padding arrive untouched); later blocks of a run
 *       are the bytes the ordered call would have stored at that step.
 *   No byte outside the blocks, outside fetchbuf[0, nblocks x blocklen x size),
 *       or in any table is written.
 *   Ops: validated as MPIX_Reduce_local_fetch validates them
 *       (MPIR_ERRTEST_OP_GACC plus MPI_Reduce_local's datatype check; user ops,
 *       and MPI_LAND / MPI_LOR on floating types: MPI_ERR_OP).  MPI_NO_OP and
 *       MPI_REPLACE are accepted on every basic type, both kernels here, byte
 *       operations chosen by the element's size.  MPI_NO_OP makes every block of
 *       a run receive the same old bytes; inbuf and in_displs are not looked at
 *       and may be NULL; the target is not written.  MPI_REPLACE gives fetchbuf
 *       block k the previous contribution's block (the head of a run: the old
 *       target), and the target ends holding the run's last input block.
 *   order given: the ordered call's table under its rules, from
 *       MPIX_Reduce_local_order unchanged.  order NULL with inout_displs given:
 *       the positions are the table's own -- the caller's promise that equal
 *       entries of inout_displs, if any, are adjacent in the table; in
 *       particular that there are none, which makes this the fetching indexed
 *       call, a Get_accumulate on an indexed_block target, with no sort.  A host
 *       inout_displs is held to the promise: an entry equal to a non-adjacent
 *       earlier one is MPI_ERR_ARG.  inout_displs NULL with order given is
 *       MPI_ERR_ARG, as in the ordered call; with in_displs given too: a packed
 *       target has no repeats, and a gather on the origin side is not this
 *       call's job.  Both NULL is MPIX_Reduce_local_fetch on nblocks x blocklen
 *       elements.
 *   Arguments: the ordered call's checks in its order, the fetch call's op rule
 *       in the op's place.  After the alias check (inbuf == inoutbuf, unless
 *       MPI_NO_OP) the fetch call's rules for fetchbuf: MPI_IN_PLACE for any of
 *       the three buffers is MPI_ERR_BUFFER; fetchbuf NULL with both counts
 *       positive is MPI_ERR_BUFFER; its range overlapping a packed inbuf's range
 *       (in_displs NULL) is MPI_ERR_BUFFER whatever the alias check says, unless
 *       the op is MPI_NO_OP.  Either count 0 succeeds and looks at no pointer or
 *       table; the op and disp_unit are still checked.
 *   Bases and tables have the ordered call's residency rules: device memory on
 *       one device, or, with hip_stream NULL, a table in host memory, which gets
 *       the ordered call's checks; with a stream a host table is MPI_ERR_BUFFER.
 *       With a host inout_displs, fetchbuf meeting ANY byte from the lowest
 *       block's first to the highest block's last is MPI_ERR_BUFFER (the
 *       fetching ragged call's rule); with device tables those overlaps are
 *       undefined.  Every index read from a device order stays clamped, so the
 *       stores to fetchbuf stay inside it too.
 *   A call that returns an error has written nothing.
 *   With device tables everything travels in the kernel arguments: no
 *       allocation and no library scratch, so the call can be captured into a
 *       graph.
 *   Blocks below the wide threshold move as 16-byte vectors under the indexed
 *       call's conditions with fetchbuf a multiple of 16 as well; else element
 *       by element.  A run is folded serially, as in the ordered call: a hot
 *       row costs time in proportion to its contributions.
 *   Measured: fp32 MPI_SUM, synchronous calls, medians of alternated rounds, the
 *       rounds' medians within 1 % of these but where noted
 *       (tools/fetch_ordered_ab.py, profiles/fetch_ordered/fetch_ordered_ab.log;
 *       DESIGN.md, Fetching ordered indexed reductions, has the table).  Against
 *       MPIX_Reduce_local_indexed_ordered on the same operands, the cost of the
 *       extra store stream: 65,536 blocks of 256 bytes 27.0 against 22.6 us with
 *       no repeats (1.19 x), 47.5 against 35.6 at 4 blocks per target (1.34 x),
 *       65.7 against 52.0 at 64 (1.26 x); 4096 blocks of 64 KiB 178 against 143
 *       us (1.25 x; 177 to 184 between rounds), 127 against 96 (1.32 x), 499
 *       against 340 (1.47 x) -- below what the bytes alone would make it (1.33,
 *       1.67 and 1.97 x).  Against what a caller had before, one
 *       MPIX_Reduce_local_fetch_ragged per duplicate-free round (the split and
 *       the packing of each round not timed): at 4 per target 47.5 against 66.5
 *       us and 127 against 234, at 64 per target 65.7 against 925 and 499
 *       against 1036.  With NO repeats that way is a single fetch_ragged call
 *       and takes LESS time than this call with an order table on 256-byte
 *       blocks, 24.5 against 27.0 us (64 KiB blocks: 189 against 178): a table
 *       known to be free of repeats should pass order NULL, which reads no order
 *       table and takes 24.0 us (0.97 x fetch_ragged) and 173 us (0.92 x).  A
 *       hot row, every block on one target: 29.4 ms for 65,536 blocks of 256
 *       bytes (0.45 us a contribution; 29.0 to 30.3 between rounds), 4.6 ms for
 *       4096 of 64 KiB (1.1 us), 1.04 and 1.09 x the ordered call. */
MPICH_API_PUBLIC int MPIX_Reduce_local_fetch_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs,
                             void *inoutbuf, const MPI_Aint * inout_displs, void *fetchbuf, const int *order,
                             MPI_Aint disp_unit, int nblocks, int blocklen,
                             MPI_Datatype datatype, MPI_Op op, void *hip_stream);
/* Ordered compare-and-swap: many MPI_Compare_and_swap targets in one call, in
 * table order -- the one RMA atomic that is not an MPI_Op, so no MPIX_Reduce_local
 * call expresses it (MPI_REPLACE through the fetching ordered call swaps
 * unconditionally).  The reference's target handlers copy the old value out, call
 * MPIR_Compare_equal and, where it is true, copy the origin value in, under the
 * window lock (src/mpid/ch3/src/ch3u_rma_pkthandler.c:1166-1178,
 * ch3u_handle_recv_req.c:1677, src/mpid/ch3/include/mpid_rma_shm.h:625-632).
 * This call is the CASes a target has queued, a deterministic lock or slot
 * claim, a hash-table insert whose winner is the earliest table position
 * instead of whoever wins an atomic's race.
 * count entries of ONE element each (MPI_Compare_and_swap has no count, so
 * there is no blocklen).  origin, compare and result are packed by entry number;
 * entry k's target is (char *) target + target_displs[k] * disp_unit, signed
 * displacements as in the indexed calls.  The call is exactly
 *   for k = 0 .. count - 1, one after another in that order:
 *     result[k] receives the bytes the target holds (a byte copy);
 *     if MPIR_Compare_equal(&compare[k], target_k, datatype): target_k receives
 *         the bytes of origin[k].
 * result[k] is what the target held after entries 0 .. k - 1 and before entry k;
 * a successful swap makes a later compare against the new value succeed, a failed
 * one leaves the value for the next entry.  No byte outside the targets, outside
 * result[0, count x size), or in any table is written.
 *   One value: a run of entries on one target is folded by one lane, the target
 *       loaded once into a register that is handed to result before every step.
 *       The target is stored once at the end of a run, and only when some entry
 *       of the run swapped (a run of failed compares writes no target byte;
 *       nothing can observe the difference from storing the unchanged value).
 *   Types: exactly MPIR_Type_is_rma_atomic (src/mpi/rma/rmatypeutil.c:23-43) for
 *       this build -- the C integer group (mpir_op_util.h:263-281), MPI_CHAR,
 *       MPI_AINT, MPI_OFFSET, MPI_COUNT, MPI_C_BOOL and MPI_BYTE.  Every other
 *       basic or pair type (MPI_WCHAR, the floating, complex and pair types,
 *       MPIX_C_FLOAT16) is MPI_ERR_TYPE, "Datatype (...) not permitted for atomic
 *       operations" (errnames.txt:206-207); a null or invalid handle is
 *       MPI_ERR_TYPE.  For every accepted type MPIR_Compare_equal
 *       (rmatypeutil.c:53-76) is `==` on an integer type, _Bool or unsigned char,
 *       which is equality of the element's bytes (_Bool is compared as its byte,
 *       as this library treats it everywhere; MPI_BYTE as unsigned char,
 *       rmatypeutil.c:65 -- of the validity test's groups the compare leaves out
 *       BYTE_EXTRA alone, which is empty, mpir_op_util.h:346).  The kernels
 *       therefore go by the element's size, 1, 2, 4 or 8 bytes, not by type.
 *   order: MPIX_Reduce_local_order's table under
 *       MPIX_Reduce_local_indexed_ordered's rules, unchanged.  order NULL with
 *       target_displs given promises that equal entries are adjacent (a host
 *       table is held to it, as in MPIX_Reduce_local_fetch_indexed_ordered).
 *       target_displs NULL is a contiguous target, element k entry k: no entry
 *       repeats, and order given then is MPI_ERR_ARG.
 *   Arguments, in this order: count < 0 MPI_ERR_COUNT; the datatype; disp_unit
 *       <= 0 MPI_ERR_ARG; count 0 succeeds and looks at no pointer or table; NULL
 *       origin, compare or result MPI_ERR_ARG (MPIR_ERRTEST_ARGNULL,
 *       src/mpi/rma/compare_and_swap.c:115-117); MPI_IN_PLACE for any of the four
 *       buffers MPI_ERR_BUFFER; origin == target or compare == target
 *       MPI_ERR_BUFFER under MPIR_CVAR_COLL_ALIAS_CHECK; order without
 *       target_displs MPI_ERR_ARG; result's packed range overlapping origin's,
 *       compare's or a contiguous target's MPI_ERR_BUFFER whatever the alias
 *       check says (origin and compare are only read and may overlap or be equal).
 *   Residency and host tables are MPIX_Reduce_local_fetch_indexed_ordered's:
 *       everything device memory on one device; with hip_stream NULL a table may
 *       be host memory and gets that call's checks (displacement overflow and an
 *       order that is no stable sort MPI_ERR_ARG, with no order the adjacency
 *       promise; the residency of the lowest and highest target, and result
 *       meeting ANY byte of the targets' span, MPI_ERR_BUFFER); a host table with
 *       a stream is MPI_ERR_BUFFER.  A device order that breaks its conditions
 *       gives an undefined result, but every index read from it is clamped: reads
 *       stay inside the tables and stores inside result and the named targets.
 *   A call that returns an error has written nothing.
 *   hip_stream NULL: synchronous; otherwise enqueued on that stream without
 *       waiting.  With device tables everything travels in the kernel arguments:
 *       no allocation, no library scratch, so the call can be captured into a
 *       graph on one stream.
 *   Element access is byte-wise where it must be: any target alignment works, odd
 *       byte displacements with disp_unit 1 included.  A contiguous target moves
 *       as 16-byte vectors on a 16 KiB tile grid where all four pointers share
 *       one offset mod 16 and the target is naturally aligned, else by elements.
 *   Measured: synchronous calls, medians of alternated rounds, the rounds' medians
 *       within 1 % of these (tools/cas_ab.py, profiles/cas/cas_ab.log; DESIGN.md,
 *       Ordered compare-and-swap, has the tables); values from three words, a third
 *       of the compares succeeding.  Against the unconditional swap a caller had
 *       before, MPIX_Reduce_local_fetch_indexed_ordered with MPI_REPLACE and
 *       blocklen 1 on the same tables (by the bytes per entry this call moves at
 *       most 5 : 4 of it): 65,536 entries of MPI_LONG in 16.8 against 21.1 us with
 *       no repeats, 20.1 against 27.7 at 4 entries per target, 89 against 182 at
 *       64; MPI_INT 18.3 against 30.5, 20.8 against 42.6, 84 against 328.  Every
 *       entry on one target, the serial worst case: 13.0 ms (0.2 us an entry)
 *       against 14.7.  Walking a run four positions at a time against one at a
 *       time (the same sources built both ways, alternated): 20.1 against 21.3 us
 *       at 4 per target, 89 against 115 at 64, 13.0 against 17.5 ms on one target,
 *       equal with no repeats.  A contiguous MPI_LONG target against
 *       MPIX_Reduce_local_fetch with MPI_BXOR, four streams where this call moves
 *       five: 10.4 against 9.9 us at 16 KiB, 222 against 191 us at 256 MiB (1.17 x,
 *       byte bound 1.25; the five streams over the whole call's time are 0.755 of
 *       the 8 TB/s peak; the kernel alone was not measured). */
MPICH_API_PUBLIC int MPIX_Compare_and_swap_indexed_ordered(const void *origin, const void *compare,
                             void *target, const MPI_Aint * target_displs, void *result, const int *order,
                             MPI_Aint disp_unit, int count, MPI_Datatype datatype, void *hip_stream);
MPICH_API_PUBLIC int MPIX_Reduce_local_set_errhandler(MPI_Errhandler errhandler);
MPICH_API_PUBLIC int MPIX_Reduce_local_get_errhandler(MPI_Errhandler * errhandler);

#ifdef __cplusplus
}
#endif
#endif /* MPI_REDUCE_LOCAL_H_INCLUDED */
