/*
 * reduce_local.c -- MPI_Reduce_local / PMPI_Reduce_local / MPIR_Reduce_local,
 * the stream-ordered MPIX variant, user-defined ops and error reporting.
 *
 * Reference: src/mpi/coll/reduce_local/reduce_local.c (MPIR_Reduce_local
 * :35-122, MPI_Reduce_local :155-219), src/include/mpir_err.h (ERRTEST_OP
 * :499-510, ERRTEST_ALIAS_COLL :277-285, ERRTEST_NAMED_BUF_INPLACE :440-446),
 * src/mpi/coll/op/op_create.c, op_free.c, op_commutative.c.
 *
 * Validation order, error classes, the count==0 early exit, the op_errno
 * reset/read protocol and the builtin/user dispatch are the reference's.
 * Differences, all documented in DESIGN.md:
 *   - the library is always "initialized" (no MPI_Init in this drop-in);
 *   - error codes are MPICH-format codes with an error stack (errutil.c; libmpi's
 *     own MPIR_Err_* routines when compiled into it);
 *   - the error handler that MPI_Reduce_local reaches through
 *     MPIR_Err_return_comm(NULL, ...) is set by MPIX_Reduce_local_set_errhandler
 *     (default MPI_ERRORS_ARE_FATAL, as for COMM_WORLD in the reference);
 *   - a builtin-kind op handle with table index 0 or 15 returns MPI_ERR_OP
 *     instead of calling through the table's NULL slot.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mpir_op_objects.h"
#include "mpir_op_types.h"

/* ---- handles and user ops: the MPIR_Op object store (op_objects.c) ----- */
#define HANDLE_KIND_INVALID  MPIR_HANDLE_KIND_INVALID
#define HANDLE_KIND_BUILTIN  MPIR_HANDLE_KIND_BUILTIN
#define HANDLE_GET_KIND(a)     MPIR_HANDLE_GET_KIND(a)
#define HANDLE_GET_MPI_KIND(a) MPIR_HANDLE_GET_MPI_KIND(a)

/* A live user-defined op: MPIR_Op_get_ptr + MPIR_Op_valid_ptr
 * (reduce_local.c:172-177), plus a check the reference does not make --
 * that the object is allocated (its handle is this handle, its reference
 * count positive) -- so a freed or never-created handle returns
 * MPI_ERR_OP instead of calling through a stale function pointer. */
static MPIR_Op *user_op_get(MPI_Op op)
{
    MPIR_Op *p;
    if (HANDLE_GET_MPI_KIND(op) != MPIR_OP_OBJ_KIND || HANDLE_GET_KIND(op) == HANDLE_KIND_BUILTIN)
        return NULL;
    p = MPIR_Op_get_ptr_fn(op);
    if (!p || p->handle != op || __atomic_load_n(&p->ref_count, __ATOMIC_ACQUIRE) <= 0 ||
        p->kind < MPIR_OP_KIND__USER_NONCOMMUTE)
        return NULL;
    return p;
}

/* ---- error handling ----------------------------------------------------- */
/* COMM_WORLD's handler as MPIR_Err_return_comm(NULL, ...) sees it: fatal,
 * unless MPIR_CVAR_REDUCE_LOCAL_ERRHANDLER=return (for the LD_PRELOAD shim,
 * whose MPIX_ setter the application cannot reach) or the setter says so */
static MPI_Errhandler reduce_local_errhandler = 0;

static MPI_Errhandler default_errhandler(void)
{
    const char *e = getenv("MPIR_CVAR_REDUCE_LOCAL_ERRHANDLER");
    return (e && !strcmp(e, "return")) ? MPI_ERRORS_RETURN : MPI_ERRORS_ARE_FATAL;
}

int MPIX_Reduce_local_set_errhandler(MPI_Errhandler errhandler)
{
    if (errhandler != MPI_ERRORS_ARE_FATAL && errhandler != MPI_ERRORS_RETURN)
        return MPI_ERR_ARG;
    __atomic_store_n(&reduce_local_errhandler, errhandler, __ATOMIC_RELAXED);
    return MPI_SUCCESS;
}

int MPIX_Reduce_local_get_errhandler(MPI_Errhandler * errhandler)
{
    MPI_Errhandler h = __atomic_load_n(&reduce_local_errhandler, __ATOMIC_RELAXED);
    *errhandler = h ? h : default_errhandler();
    return MPI_SUCCESS;
}

/* The innermost level of an error stack: a bare class raised inside this
 * library (its text in the thread's detail slot) becomes an MPICH error code
 * (MPIR_Err_create_code, errutil.c here or libmpi's own).  A code that already
 * carries a stack passes through. */
int MPIR_Err_wrap_detail(const char *fcname, int line, int mpi_errno)
{
    const char *detail;
    if (mpi_errno == MPI_SUCCESS || (mpi_errno & ~0x7f) != 0)
        return mpi_errno;
    detail = MPIR_Err_last_detail();
    if (!detail[0])
        return MPIR_Err_create_code(MPI_SUCCESS, MPIR_ERR_RECOVERABLE, fcname, line, mpi_errno, "**other", NULL);
    return MPIR_Err_create_code(MPI_SUCCESS, MPIR_ERR_RECOVERABLE, fcname, line, mpi_errno, "**other", "%s", detail);
}

/* The MPI-level error exit of every entry point but MPI_Reduce_local's own:
 * wrap, then MPIR_Err_return_comm(NULL, ...) (errutil.c:238) -- COMM_WORLD's
 * handler, fatal by default. */
int MPIR_Err_return_at(const char *fcname, int line, int mpi_errno)
{
    return MPIR_Err_return_comm(NULL, fcname, MPIR_Err_wrap_detail(fcname, line, mpi_errno));
}

#define err_return MPIR_Err_return

static int alias_check_enabled(void)
{
    /* MPIR_CVAR_COLL_ALIAS_CHECK (mpir_err.h:157-171), default 1.  Racing
     * first calls store the same value; the atomics make that well defined. */
    static int cached = -1;
    int c = __atomic_load_n(&cached, __ATOMIC_RELAXED);
    if (c < 0) {
        const char *v = getenv("MPIR_CVAR_COLL_ALIAS_CHECK");
        c = v ? (atoi(v) != 0) : 1;
        __atomic_store_n(&cached, c, __ATOMIC_RELAXED);
    }
    return c;
}

/* The validation block of MPI_Reduce_local (reduce_local.c:166-191). */
static int validate(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op)
{
    int mpi_errno;
    /* MPIR_ERRTEST_OP (mpir_err.h:499-510) */
    if (op == MPI_OP_NULL) {
        MPIR_Err_set_detail("Null MPI_Op");
        return MPI_ERR_OP;
    }
    if (op == MPI_NO_OP || op == MPI_REPLACE) {
        MPIR_Err_set_detail("MPI_Op operation is not allowed in this routine");
        return MPI_ERR_OP;
    }
    if (HANDLE_GET_MPI_KIND(op) != MPIR_OP_OBJ_KIND || HANDLE_GET_KIND(op) == HANDLE_KIND_INVALID) {
        MPIR_Err_set_detail("Invalid MPI_Op");
        return MPI_ERR_OP;
    }
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        if (!user_op_get(op)) {         /* MPIR_Op_valid_ptr */
            MPIR_Err_set_detail("Invalid MPI_Op");
            return MPI_ERR_OP;
        }
    } else {
        MPIR_Op_check_dtype_fn *chk = MPIR_OP_HDL_TO_DTYPE_FN(op);
        if (!chk) {
            MPIR_Err_set_detail("Invalid MPI_Op");
            return MPI_ERR_OP;
        }
        mpi_errno = chk(datatype);
        if (mpi_errno != MPI_SUCCESS)
            return mpi_errno;
    }
    if (count != 0 && alias_check_enabled() && inbuf == inoutbuf) {
        MPIR_Err_set_detail("Buffers must not be aliased");
        return MPI_ERR_BUFFER;
    }
    if (count > 0 && inbuf == MPI_IN_PLACE) {
        MPIR_Err_set_detail("buffer 'inbuf' cannot be MPI_IN_PLACE");
        return MPI_ERR_BUFFER;
    }
    if (count > 0 && inoutbuf == MPI_IN_PLACE) {
        MPIR_Err_set_detail("buffer 'inoutbuf' cannot be MPI_IN_PLACE");
        return MPI_ERR_BUFFER;
    }
    return MPI_SUCCESS;
}

/* ---- user op on device buffers: the function is host code, so device ----
 * ---- operands are staged through host memory around the call.      ---- */
static int call_user_op(MPI_User_function * fn, const void *inbuf, void *inoutbuf, int count,
                        MPI_Datatype datatype)
{
    int in_dev = MPIR_Hip_is_device_ptr(inbuf);
    int io_dev = MPIR_Hip_is_device_ptr(inoutbuf);
    const MPIR_Type_desc *d;
    size_t bytes;
    void *hin = NULL, *hio = NULL;
    int rc = MPI_SUCCESS;

    if (!in_dev && !io_dev) {
        fn((void *) inbuf, inoutbuf, &count, &datatype);
        return MPI_SUCCESS;
    }
    d = MPIR_Type_lookup(datatype);
    if (!d || count < 0) {
        MPIR_Err_set_detail("user MPI_Op on device buffers needs a basic datatype");
        return MPI_ERR_TYPE;
    }
    bytes = (size_t) count * MPIR_Hip_elem_size(d->elem);
    hin = in_dev ? malloc(bytes ? bytes : 1) : (void *) inbuf;
    hio = io_dev ? malloc(bytes ? bytes : 1) : inoutbuf;
    if (!hin || !hio) {
        rc = MPI_ERR_NO_MEM;
        goto done;
    }
    if ((in_dev && MPIR_Hip_memcpy(hin, inbuf, bytes)) || (io_dev && MPIR_Hip_memcpy(hio, inoutbuf, bytes))) {
        MPIR_Err_set_detail("staging for user MPI_Op: %s", MPIR_Hip_error_string());
        rc = MPI_ERR_OTHER;
        goto done;
    }
    fn(hin, hio, &count, &datatype);
    if (io_dev && MPIR_Hip_memcpy(inoutbuf, hio, bytes)) {
        MPIR_Err_set_detail("staging for user MPI_Op: %s", MPIR_Hip_error_string());
        rc = MPI_ERR_OTHER;
    }
  done:
    if (in_dev && hin)
        free(hin);
    if (io_dev && hio)
        free(hio);
    return rc;
}

/* ---- MPIR_Reduce_local (reduce_local.c:35-122) -------------------------- */
int MPIR_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op)
{
    int mpi_errno = MPI_SUCCESS;
    int *op_errno;
    MPI_User_function *uop;

    if (count == 0)
        return MPI_SUCCESS;

    op_errno = MPIR_Op_errno_ptr();
    *op_errno = MPI_SUCCESS;

    if (HANDLE_GET_KIND(op) == HANDLE_KIND_BUILTIN) {
        uop = MPIR_OP_HDL_TO_FN(op);
        if (!uop) {
            MPIR_Err_set_detail("Invalid MPI_Op");
            return MPI_ERR_OP;
        }
        (*uop) ((void *) inbuf, inoutbuf, &count, &datatype);
    } else {
        /* MPIR_Op_get_ptr; a C-language op calls function.c_function (:65-82) */
        MPIR_Op *op_ptr = user_op_get(op);
        uop = op_ptr ? (MPI_User_function *) op_ptr->function.c_function : NULL;
        if (!uop) {
            MPIR_Err_set_detail("Invalid MPI_Op");
            return MPI_ERR_OP;
        }
        mpi_errno = call_user_op(uop, inbuf, inoutbuf, count, datatype);
        if (mpi_errno)
            return mpi_errno;
    }

    if (*op_errno)
        mpi_errno = *op_errno;
    return mpi_errno;
}

/* ---- MPI_Reduce_local (reduce_local.c:155-219) -------------------------- */
/* The body of PMPI_Reduce_local, under an internal name the LD_PRELOAD shim
 * (preload.c) also calls. */
int MPIR_Reduce_local_checked(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op)
{
    static const char FCNAME[] = "PMPI_Reduce_local";
    int mpi_errno;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);         /* reduce_local.c:162 */
    mpi_errno = validate(inbuf, inoutbuf, count, datatype, op);
    if (mpi_errno == MPI_SUCCESS)
        mpi_errno = MPIR_Reduce_local(inbuf, inoutbuf, count, datatype, op);
    if (mpi_errno != MPI_SUCCESS) {
        /* fn_fail (reduce_local.c:208-217) */
        mpi_errno = MPIR_Err_wrap_detail(FCNAME, __LINE__, mpi_errno);
        mpi_errno = MPIR_Err_create_code(mpi_errno, MPIR_ERR_RECOVERABLE, FCNAME, __LINE__, MPI_ERR_OTHER,
                                         "**mpi_reduce_local", "**mpi_reduce_local %p %p %d %D %O", inbuf,
                                         inoutbuf, count, datatype, op);
        mpi_errno = MPIR_Err_return_comm(NULL, FCNAME, mpi_errno);
    }
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);          /* reduce_local.c:205 */
    return mpi_errno;
}

#ifndef MPIR_PRELOAD_SHIM
int PMPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op)
{
    return MPIR_Reduce_local_checked(inbuf, inoutbuf, count, datatype, op);
}

/* profiling interface: MPI_ is a weak alias of PMPI_ (reduce_local.c:10-20) */
int MPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype, MPI_Op op)
    __attribute__ ((weak, alias("PMPI_Reduce_local")));
#endif

/* ---- MPIX_Reduce_local_stream: enqueue on a HIP stream, no wait -------- */
static int reduce_local_stream(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype,
                               MPI_Op op, void *hip_stream);

/* the MPIX entry points validate user-op handles like MPI_Reduce_local does,
 * so they hold the same GLOBAL section */
int MPIX_Reduce_local_stream(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype,
                             MPI_Op op, void *hip_stream)
{
    int rc;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);
    rc = reduce_local_stream(inbuf, inoutbuf, count, datatype, op, hip_stream);
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);
    return rc;
}

static int reduce_local_stream(const void *inbuf, void *inoutbuf, int count, MPI_Datatype datatype,
                               MPI_Op op, void *hip_stream)
{
    int mpi_errno = validate(inbuf, inoutbuf, count, datatype, op);
    int opidx, elem, rc;
    if (mpi_errno != MPI_SUCCESS)
        return err_return("MPIX_Reduce_local_stream", mpi_errno);
    if (count <= 0)
        return MPI_SUCCESS;
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        MPIR_Err_set_detail("user MPI_Op functions run on the host; use MPI_Reduce_local");
        return err_return("MPIX_Reduce_local_stream", MPI_ERR_OP);
    }
    opidx = op & 0xf;
    elem = MPIR_Op_resolve_elem(opidx, datatype);
    if (!elem) {        /* compute switch `default:` (LAND/LOR on floats) */
        MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
        return err_return("MPIX_Reduce_local_stream", MPI_ERR_OP);
    }
    rc = MPIR_Hip_reduce(inbuf, inoutbuf, (uint64_t) count, opidx, elem, hip_stream, 0);
    if (rc == MPIR_HIP_EBUFFER) {
        MPIR_Err_set_detail("MPIX_Reduce_local_stream needs device-resident buffers on one device");
        return err_return("MPIX_Reduce_local_stream", MPI_ERR_BUFFER);
    }
    if (rc != MPIR_HIP_OK) {
        MPIR_Op_report_hip_error("MPIX_Reduce_local_stream", rc);
        return err_return("MPIX_Reduce_local_stream", *MPIR_Op_errno_ptr());
    }
    return MPI_SUCCESS;
}

/* ---- MPIX_Reduce_local_multi: fused schedule steps (see the header) ---- */
static int reduce_local_multi(const void *const *inbufs, int n, void *outbuf, int count,
                              MPI_Datatype datatype, MPI_Op op, int order, void *hip_stream);

int MPIX_Reduce_local_multi(const void *const *inbufs, int n, void *outbuf, int count,
                            MPI_Datatype datatype, MPI_Op op, int order, void *hip_stream)
{
    int rc;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);
    rc = reduce_local_multi(inbufs, n, outbuf, count, datatype, op, order, hip_stream);
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);
    return rc;
}

static int reduce_local_multi(const void *const *inbufs, int n, void *outbuf, int count,
                              MPI_Datatype datatype, MPI_Op op, int order, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_multi";
    int mpi_errno, opidx, elem, rc, j;
    if (n < 1 || n > 64 || !inbufs || (order != MPIX_ORDER_TREE && order != MPIX_ORDER_CHAIN)) {
        MPIR_Err_set_detail("invalid operand count or order");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (order == MPIX_ORDER_TREE && (n & (n - 1))) {
        MPIR_Err_set_detail("MPIX_ORDER_TREE needs a power-of-two operand count");
        return err_return(fc, MPI_ERR_ARG);
    }
    for (j = 0; j < n; j++) {
        mpi_errno = validate(inbufs[j], outbuf, j == 0 ? 0 : count, datatype, op);
        if (mpi_errno != MPI_SUCCESS)
            return err_return(fc, mpi_errno);
    }
    if (count <= 0)
        return MPI_SUCCESS;
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        MPIR_Err_set_detail("user MPI_Op functions run on the host; use MPI_Reduce_local");
        return err_return(fc, MPI_ERR_OP);
    }
    opidx = op & 0xf;
    elem = MPIR_Op_resolve_elem(opidx, datatype);
    if (!elem) {
        MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
        return err_return(fc, MPI_ERR_OP);
    }
    /* outbuf may be inbufs[0] exactly; any other overlap is refused whatever
     * MPIR_CVAR_COLL_ALIAS_CHECK says: the CHAIN path for n > 8 writes outbuf
     * between passes, before later operands are read */
    {
        const uintptr_t ob = (uintptr_t) outbuf;
        const uintptr_t nb = (uintptr_t) count * MPIR_Hip_elem_size(elem);
        for (j = 0; j < n; j++) {
            const uintptr_t ib = (uintptr_t) inbufs[j];
            if ((j > 0 || ib != ob) && ib < ob + nb && ob < ib + nb) {
                MPIR_Err_set_detail("inbufs[%d] overlaps outbuf (only inbufs[0] may be outbuf, exactly)", j);
                return err_return(fc, MPI_ERR_BUFFER);
            }
        }
    }
    rc = MPIR_Hip_combine(inbufs, n, outbuf, (uint64_t) count, opidx, elem,
                          order == MPIX_ORDER_TREE ? MPIR_HIP_ORDER_TREE : MPIR_HIP_ORDER_CHAIN,
                          hip_stream, hip_stream == NULL);
    if (rc == MPIR_HIP_EBUFFER) {
        MPIR_Err_set_detail("%s needs device-resident buffers on one device", fc);
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (rc != MPIR_HIP_OK) {
        MPIR_Op_report_hip_error(fc, rc);
        return err_return(fc, *MPIR_Op_errno_ptr());
    }
    return MPI_SUCCESS;
}

/* ---- what the MPIX calls on many blocks share --------------------------- */
/* Each of them is a static body under the GLOBAL critical section (they
 * validate user-op handles like MPI_Reduce_local does): the public entry
 * returns CS_RETURN(body(...)). */
#define CS_RETURN(call) do { \
        int cs_rc_; \
        MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL); \
        cs_rc_ = (call); \
        MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL); \
        return cs_rc_; \
    } while (0)

/* A predefined op and its element class for the datatype in *opidx and *elem, or
 * MPI_ERR_OP with the detail set: a user op, or the compute switch's `default:`
 * (LAND / LOR on floats) */
static int builtin_op_elem(MPI_Datatype datatype, MPI_Op op, int *opidx, int *elem)
{
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        MPIR_Err_set_detail("user MPI_Op functions run on the host; use MPI_Reduce_local");
        return MPI_ERR_OP;
    }
    *opidx = op & 0xf;
    *elem = MPIR_Op_resolve_elem(*opidx, datatype);
    if (!*elem) {
        MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
        return MPI_ERR_OP;
    }
    return MPI_SUCCESS;
}

/* The shim's entries are bound weakly, so that a program which links this file
 * against a partial shim of its own (a harness that stubs only the MPIR_Hip_*
 * entries its collectives reach) still links; without the entry the call fails
 * with MPI_ERR_OTHER. */
static int shim_has(int bound, const char *entry)
{
    if (bound)
        return MPI_SUCCESS;
    MPIR_Err_set_detail("the HIP shim linked here has no %s", entry);
    return MPI_ERR_OTHER;
}

/* The shim's return code as the MPI error of the call `fc`: MPIR_HIP_EBUFFER is
 * MPI_ERR_BUFFER with the text `ebuffer`, MPIR_HIP_EARG (where the call has a
 * text for it) MPI_ERR_ARG with `earg`, both formats of fc; anything else as
 * MPIR_Op_report_hip_error reports it. */
static int shim_result(const char *fc, int rc, const char *ebuffer, const char *earg)
{
    if (rc == MPIR_HIP_OK)
        return MPI_SUCCESS;
    if (rc == MPIR_HIP_EBUFFER) {
        MPIR_Err_set_detail(ebuffer, fc);
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (rc == MPIR_HIP_EARG && earg) {
        MPIR_Err_set_detail(earg, fc);
        return err_return(fc, MPI_ERR_ARG);
    }
    MPIR_Op_report_hip_error(fc, rc);
    return err_return(fc, *MPIR_Op_errno_ptr());
}

static const char EBUF_BUFFERS[] = "%s needs device-resident buffers on one device";
static const char EBUF_TABLES[] = "%s needs device-resident operands on one device, and its tables there too "
    "(host tables: the synchronous call only)";
static const char EARG_RAGGED[] = "%s: starts is not 0, non-decreasing and ending at count, or a piece's offset does "
    "not fit the address space";

/* ---- MPIX_Reduce_local_batch: many segments, one launch (see the header) */
#pragma weak MPIR_Hip_reduce_batch
static int reduce_local_batch(const MPIX_Reduce_local_seg * segs, int nsegs, MPI_Datatype datatype,
                              MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_batch";
    MPIR_Hip_seg small[64], *hs = small;
    int mpi_errno, opidx, elem, rc, j, nonempty = 0;
    if (nsegs < 0 || (nsegs > 0 && !segs)) {
        MPIR_Err_set_detail("invalid segment count or segment array");
        return err_return(fc, MPI_ERR_ARG);
    }
    /* everything is validated before anything is launched */
    for (j = 0; j < nsegs; j++) {
        if (segs[j].count < 0) {
            MPIR_Err_set_detail("segment %d: negative count %d", j, segs[j].count);
            return err_return(fc, MPI_ERR_COUNT);
        }
        /* an empty segment's pointers are not looked at (the op still is) */
        mpi_errno = segs[j].count ? validate(segs[j].inbuf, segs[j].inoutbuf, segs[j].count, datatype, op)
            : validate(NULL, NULL, 0, datatype, op);
        if (mpi_errno != MPI_SUCCESS)
            return err_return(fc, mpi_errno);
        nonempty += segs[j].count != 0;
    }
    if (!nonempty)
        return MPI_SUCCESS;
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS ||
        (mpi_errno = shim_has(MPIR_Hip_reduce_batch != NULL, "MPIR_Hip_reduce_batch")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (nsegs > (int) (sizeof small / sizeof small[0])) {
        hs = (MPIR_Hip_seg *) malloc((size_t) nsegs * sizeof *hs);
        if (!hs) {
            MPIR_Err_set_detail("out of memory for %d segments", nsegs);
            return err_return(fc, MPI_ERR_NO_MEM);
        }
    }
    for (j = 0; j < nsegs; j++) {
        hs[j].in = segs[j].inbuf;
        hs[j].io = segs[j].inoutbuf;
        hs[j].count = (uint64_t) segs[j].count;
    }
    rc = MPIR_Hip_reduce_batch(hs, nsegs, opidx, elem, hip_stream, hip_stream == NULL);
    if (hs != small)
        free(hs);
    return shim_result(fc, rc, EBUF_BUFFERS, NULL);
}

int MPIX_Reduce_local_batch(const MPIX_Reduce_local_seg * segs, int nsegs, MPI_Datatype datatype,
                            MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_batch(segs, nsegs, datatype, op, hip_stream));
}

/* ---- MPIX_Reduce_local_strided: equal rows at one stride (see the header) */
#pragma weak MPIR_Hip_reduce_strided
static int reduce_local_strided(const void *inbuf, MPI_Aint in_stride, void *inoutbuf, MPI_Aint inout_stride,
                                int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_strided";
    int mpi_errno, opidx, elem, rc;
    const int empty = nblocks == 0 || blocklen == 0;
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* as the batch validates a segment: an empty call's pointers are not looked
     * at (the op still is) */
    mpi_errno = empty ? validate(NULL, NULL, 0, datatype, op) : validate(inbuf, inoutbuf, blocklen, datatype, op);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (in_stride < 0 || inout_stride < 0) {
        MPIR_Err_set_detail("negative %s", in_stride < 0 ? "in_stride" : "inout_stride");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (empty)
        return MPI_SUCCESS;
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (nblocks > 1 && (uint64_t) inout_stride < (uint64_t) blocklen * MPIR_Hip_elem_size(elem)) {
        MPIR_Err_set_detail("inout_stride %ld is below the row's %lu bytes: output rows would overlap",
                            (long) inout_stride, (unsigned long) blocklen * MPIR_Hip_elem_size(elem));
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((mpi_errno = shim_has(MPIR_Hip_reduce_strided != NULL, "MPIR_Hip_reduce_strided")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_strided(inbuf, (uint64_t) in_stride, inoutbuf, (uint64_t) inout_stride, (uint64_t) nblocks,
                                 (uint64_t) blocklen, opidx, elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_BUFFERS, "%s: the rows' span does not fit the address space");
}

int MPIX_Reduce_local_strided(const void *inbuf, MPI_Aint in_stride, void *inoutbuf, MPI_Aint inout_stride,
                              int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_strided(inbuf, in_stride, inoutbuf, inout_stride, nblocks, blocklen, datatype, op,
                                   hip_stream));
}

/* ---- MPIX_Reduce_local_subarray: sub-boxes of N-d arrays (see the header) */
#pragma weak MPIR_Hip_reduce_subarray
/* one dimension of one operand as type_create_subarray.c:105-133 checks it */
static int subarray_dim_ok(const char *side, int d, int size, int subsize, int start)
{
    if (size < 1 || subsize < 1 || start < 0) {
        MPIR_Err_set_detail("%s dimension %d: %s %d", side, d,
                            size < 1 ? "size" : subsize < 1 ? "subsize" : "negative start",
                            size < 1 ? size : subsize < 1 ? subsize : start);
        return 0;
    }
    if (subsize > size || start > size - subsize) {
        MPIR_Err_set_detail("%s dimension %d: %s %d is above %d", side, d, subsize > size ? "subsize" : "start",
                            subsize > size ? subsize : start, subsize > size ? size : size - subsize);
        return 0;
    }
    return 1;
}

static int reduce_local_subarray(const void *inbuf, const int in_sizes[], const int in_starts[], void *inoutbuf,
                                 const int inout_sizes[], const int inout_starts[], int ndims, const int subsizes[],
                                 int order, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_subarray";
    int mpi_errno, opidx, elem, rc, d, side;
    /* the op and the type first, as the strided call validates them */
    if ((mpi_errno = validate(NULL, NULL, 0, datatype, op)) != MPI_SUCCESS ||
        (mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (ndims < 1 || ndims > MPIX_REDUCE_LOCAL_SUBARRAY_MAXDIMS) {
        MPIR_Err_set_detail("ndims %d is not in 1..%d", ndims, MPIX_REDUCE_LOCAL_SUBARRAY_MAXDIMS);
        return err_return(fc, MPI_ERR_DIMS);
    }
    if (!subsizes || (in_sizes && !in_starts) || (inout_sizes && !inout_starts)) {
        MPIR_Err_set_detail("Null pointer in parameter %s", !subsizes ? "subsizes" : in_sizes &&
                            !in_starts ? "in_starts" : "inout_starts");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (order != MPI_ORDER_C && order != MPI_ORDER_FORTRAN) {
        MPIR_Err_set_detail("Invalid argument order");
        return err_return(fc, MPI_ERR_ARG);
    }
    for (d = 0; d < ndims; d++)
        if (!subarray_dim_ok("inbuf", d, in_sizes ? in_sizes[d] : subsizes[d], subsizes[d], in_sizes ? in_starts[d] : 0) ||
            !subarray_dim_ok("inoutbuf", d, inout_sizes ? inout_sizes[d] : subsizes[d], subsizes[d],
                             inout_sizes ? inout_starts[d] : 0))
            return err_return(fc, MPI_ERR_ARG);
    /* the reference's **subarrayoflow: the whole array's bytes in an MPI_Aint */
    for (side = 0; side < 2; side++) {
        const int *sizes = side ? inout_sizes : in_sizes;
        MPI_Aint bytes = (MPI_Aint) MPIR_Hip_elem_size(elem);
        for (d = 0; d < ndims; d++)
            if (__builtin_mul_overflow(bytes, (MPI_Aint) (sizes ? sizes[d] : subsizes[d]), &bytes)) {
                MPIR_Err_set_detail("the size of %s's array does not fit an MPI_Aint", side ? "inoutbuf" : "inbuf");
                return err_return(fc, MPI_ERR_ARG);
            }
    }
    if (inbuf == MPI_IN_PLACE || inoutbuf == MPI_IN_PLACE) {
        MPIR_Err_set_detail("buffer '%s' cannot be MPI_IN_PLACE", inbuf == MPI_IN_PLACE ? "inbuf" : "inoutbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (inbuf == inoutbuf && alias_check_enabled()) {
        /* one array on both sides is the periodic wrap: legal where the two
         * boxes are disjoint, which the starts of one dimension show */
        int apart = 0;
        if (in_sizes && inout_sizes && !memcmp(in_sizes, inout_sizes, (size_t) ndims * sizeof(int)))
            for (d = 0; d < ndims; d++) {
                const long gap = (long) in_starts[d] - (long) inout_starts[d];
                apart |= (gap < 0 ? -gap : gap) >= (long) subsizes[d];
            }
        if (!apart) {
            MPIR_Err_set_detail("Buffers must not be aliased (one array on both sides needs equal sizes and disjoint boxes)");
            return err_return(fc, MPI_ERR_BUFFER);
        }
    }
    if ((mpi_errno = shim_has(MPIR_Hip_reduce_subarray != NULL, "MPIR_Hip_reduce_subarray")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_subarray(inbuf, in_sizes, in_starts, inoutbuf, inout_sizes, inout_starts, ndims, subsizes,
                                  order == MPI_ORDER_C, opidx, elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_BUFFERS, "%s: the arrays' sizes, subsizes or starts are out of range");
}

int MPIX_Reduce_local_subarray(const void *inbuf, const int in_sizes[], const int in_starts[], void *inoutbuf,
                               const int inout_sizes[], const int inout_starts[], int ndims, const int subsizes[],
                               int order, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_subarray(inbuf, in_sizes, in_starts, inoutbuf, inout_sizes, inout_starts, ndims, subsizes,
                                    order, datatype, op, hip_stream));
}

/* ---- MPIX_Reduce_local_fetch: old value out, combine in (see the header) */
#pragma weak MPIR_Hip_reduce_fetch
static int ranges_overlap(const void *a, const void *b, uint64_t bytes)
{
    const uintptr_t pa = (uintptr_t) a, pb = (uintptr_t) b;
    return pa < pb + bytes && pb < pa + bytes;
}

static int reduce_local_fetch(const void *inbuf, void *inoutbuf, void *fetchbuf, int count, MPI_Datatype datatype,
                              MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_fetch";
    const int no_op = op == MPI_NO_OP, copy = no_op || op == MPI_REPLACE;
    int mpi_errno, opidx, elem, rc;
    uint64_t n = count > 0 ? (uint64_t) count : 0, bytes;
    if (count < 0) {
        MPIR_Err_set_detail("negative count %d", count);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* MPIR_ERRTEST_OP_GACC (mpir_err.h:528-539): MPI_NO_OP and MPI_REPLACE pass,
     * a user op does not */
    if (op == MPI_OP_NULL) {
        MPIR_Err_set_detail("Null MPI_Op");
        return err_return(fc, MPI_ERR_OP);
    }
    if (HANDLE_GET_MPI_KIND(op) != MPIR_OP_OBJ_KIND || HANDLE_GET_KIND(op) == HANDLE_KIND_INVALID ||
        (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN && !user_op_get(op)) ||
        (HANDLE_GET_KIND(op) == HANDLE_KIND_BUILTIN &&
         ((op & 0xf) >= MPIR_OP_N_BUILTIN || !MPIR_OP_HDL_TO_DTYPE_FN(op)))) {
        MPIR_Err_set_detail("Invalid MPI_Op");
        return err_return(fc, MPI_ERR_OP);
    }
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        MPIR_Err_set_detail("MPI_Op is not a predefined operation; user MPI_Op functions run on the host");
        return err_return(fc, MPI_ERR_OP);
    }
    opidx = op & 0xf;
    if (copy) {
        /* every predefined datatype is count * size contiguous bytes, as for
         * MPIR_REPLACE (op_kernels.c); a derived one needs MPICH's datatype engine */
        const MPIR_Type_desc *d = MPIR_Type_lookup(datatype);
        const unsigned h = (unsigned) datatype;
        if (d) {
            elem = d->elem;
        } else if ((h >> 30) == 1u && ((h >> 26) & 0xfu) == 0x3u) {     /* builtin-kind datatype */
            elem = MPIR_HIP_U8;
            n *= (h >> 8) & 0xffu;
        } else {
            MPIR_Err_set_detail("%s: derived datatypes are not supported by this library", no_op ? "MPI_NO_OP" : "MPI_REPLACE");
            return err_return(fc, MPI_ERR_TYPE);
        }
    } else {
        /* MPI_Reduce_local's datatype check (reduce_local.c:179-183), then the
         * compute switch's `default:` (LAND / LOR on floats) */
        mpi_errno = MPIR_OP_HDL_TO_DTYPE_FN(op) (datatype);
        if (mpi_errno != MPI_SUCCESS)
            return err_return(fc, mpi_errno);
        elem = MPIR_Op_resolve_elem(opidx, datatype);
        if (!elem) {
            MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
            return err_return(fc, MPI_ERR_OP);
        }
    }
    if (n == 0)         /* no pointer is looked at */
        return MPI_SUCCESS;
    bytes = n * MPIR_Hip_elem_size(elem);
    /* MPI_NO_OP never looks at inbuf */
    if (!no_op && alias_check_enabled() && inbuf == inoutbuf) {
        MPIR_Err_set_detail("Buffers must not be aliased");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if ((!no_op && inbuf == MPI_IN_PLACE) || inoutbuf == MPI_IN_PLACE || fetchbuf == MPI_IN_PLACE) {
        MPIR_Err_set_detail("buffer '%s' cannot be MPI_IN_PLACE",
                            !no_op && inbuf == MPI_IN_PLACE ? "inbuf" : inoutbuf == MPI_IN_PLACE ? "inoutbuf" : "fetchbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (!fetchbuf) {
        MPIR_Err_set_detail("Null buffer pointer 'fetchbuf'");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    /* whatever MPIR_CVAR_COLL_ALIAS_CHECK says, as MPIX_Reduce_local_multi checks
     * its output against its operands: the old bytes must not land on either */
    if (ranges_overlap(fetchbuf, inoutbuf, bytes) || (!no_op && ranges_overlap(fetchbuf, inbuf, bytes))) {
        MPIR_Err_set_detail("fetchbuf overlaps %s", ranges_overlap(fetchbuf, inoutbuf, bytes) ? "inoutbuf" : "inbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if ((mpi_errno = shim_has(MPIR_Hip_reduce_fetch != NULL, "MPIR_Hip_reduce_fetch")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_fetch(inbuf, inoutbuf, fetchbuf, n, opidx, elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_BUFFERS, NULL);
}

int MPIX_Reduce_local_fetch(const void *inbuf, void *inoutbuf, void *fetchbuf, int count, MPI_Datatype datatype,
                            MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_fetch(inbuf, inoutbuf, fetchbuf, count, datatype, op, hip_stream));
}

/* ---- MPIX_Reduce_local_indexed: equal blocks at a displacement table (see the header) */
#pragma weak MPIR_Hip_reduce_indexed
static int reduce_local_indexed(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                const MPI_Aint * inout_displs, MPI_Aint disp_unit, int nblocks, int blocklen,
                                MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_indexed";
    int mpi_errno, opidx, elem, rc;
    const int empty = nblocks == 0 || blocklen == 0;
    _Static_assert(sizeof(MPI_Aint) == sizeof(int64_t), "the shim's tables are 64-bit displacements");
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* the strided call's order: an empty call's pointers are not looked at (the
     * op still is) */
    mpi_errno = empty ? validate(NULL, NULL, 0, datatype, op) : validate(inbuf, inoutbuf, blocklen, datatype, op);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (empty)
        return MPI_SUCCESS;
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS ||
        (mpi_errno = shim_has(MPIR_Hip_reduce_indexed != NULL, "MPIR_Hip_reduce_indexed")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_indexed(inbuf, (const int64_t *) in_displs, inoutbuf, (const int64_t *) inout_displs,
                                 (uint64_t) disp_unit, (uint64_t) nblocks, (uint64_t) blocklen, opidx, elem,
                                 hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_TABLES, "%s: a block's offset does not fit the address space");
}

int MPIX_Reduce_local_indexed(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                              const MPI_Aint * inout_displs, MPI_Aint disp_unit, int nblocks, int blocklen,
                              MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_indexed(inbuf, in_displs, inoutbuf, inout_displs, disp_unit, nblocks, blocklen, datatype,
                                   op, hip_stream));
}

/* ---- MPIX_Reduce_local_indexed_ordered: repeated targets in table order (see the header) */
#pragma weak MPIR_Hip_reduce_indexed_ordered
#pragma weak MPIR_Hip_order_build
#pragma weak MPIR_Hip_order_worksize
static int reduce_local_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                        const MPI_Aint * inout_displs, const int *order, MPI_Aint disp_unit,
                                        int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op,
                                        void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_indexed_ordered";
    int mpi_errno, opidx, elem, rc;
    const int empty = nblocks == 0 || blocklen == 0;
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* the indexed call's order: an empty call's pointers are not looked at (the
     * op still is) */
    mpi_errno = empty ? validate(NULL, NULL, 0, datatype, op) : validate(inbuf, inoutbuf, blocklen, datatype, op);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (empty)
        return MPI_SUCCESS;
    if (inout_displs == NULL) {
        MPIR_Err_set_detail("an order table with no inout_displs: a packed target has no repeats to order");
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS ||
        (mpi_errno = shim_has(MPIR_Hip_reduce_indexed_ordered != NULL, "MPIR_Hip_reduce_indexed_ordered")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_indexed_ordered(inbuf, (const int64_t *) in_displs, inoutbuf, (const int64_t *) inout_displs,
                                         order, (uint64_t) disp_unit, (uint64_t) nblocks, (uint64_t) blocklen, opidx,
                                         elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_TABLES, "%s: a block's offset does not fit the address space, or the order table "
                       "is not a stable sort of inout_displs");
}

int MPIX_Reduce_local_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                      const MPI_Aint * inout_displs, const int *order, MPI_Aint disp_unit,
                                      int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    /* no order table: the indexed call unchanged, its own name on the error stack */
    if (order == NULL)
        return MPIX_Reduce_local_indexed(inbuf, in_displs, inoutbuf, inout_displs, disp_unit, nblocks, blocklen,
                                         datatype, op, hip_stream);
    CS_RETURN(reduce_local_indexed_ordered(inbuf, in_displs, inoutbuf, inout_displs, order, disp_unit, nblocks,
                                           blocklen, datatype, op, hip_stream));
}

int MPIX_Reduce_local_order_worksize(int nblocks, MPI_Aint * work_bytes)
{
    static const char *fc = "MPIX_Reduce_local_order_worksize";
    uint64_t bytes = 0;
    int rc = MPI_SUCCESS;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);
    if (nblocks < 0) {
        MPIR_Err_set_detail("negative nblocks %d", nblocks);
        rc = err_return(fc, MPI_ERR_COUNT);
    } else if (work_bytes == NULL) {
        MPIR_Err_set_detail("work_bytes is NULL");
        rc = err_return(fc, MPI_ERR_ARG);
    } else if ((rc = shim_has(MPIR_Hip_order_worksize != NULL, "MPIR_Hip_order_worksize")) != MPI_SUCCESS) {
        rc = err_return(fc, rc);
    } else {
        (void) MPIR_Hip_order_worksize((uint64_t) nblocks, &bytes);     /* (an int is always in its range) */
        *work_bytes = (MPI_Aint) bytes;
    }
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);
    return rc;
}

static int reduce_local_order(const MPI_Aint * displs, int nblocks, int *order, void *work, MPI_Aint work_bytes,
                              void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_order";
    int rc;
    if (nblocks < 0) {
        MPIR_Err_set_detail("negative nblocks %d", nblocks);
        return err_return(fc, MPI_ERR_COUNT);
    }
    if (nblocks == 0)
        return MPI_SUCCESS;
    if (displs == NULL || order == NULL) {
        MPIR_Err_set_detail("%s is NULL", displs == NULL ? "displs" : "order");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (work != NULL && work_bytes < 0) {
        MPIR_Err_set_detail("negative work_bytes %ld", (long) work_bytes);
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((rc = shim_has(MPIR_Hip_order_build != NULL, "MPIR_Hip_order_build")) != MPI_SUCCESS)
        return err_return(fc, rc);
    rc = MPIR_Hip_order_build((const int64_t *) displs, (uint64_t) nblocks, order, work, (uint64_t) work_bytes,
                              hip_stream, hip_stream == NULL);
    if (rc == MPIR_HIP_EARG) {  /* (its text has an argument of its own) */
        MPIR_Err_set_detail("%s: work_bytes %ld is less than MPIX_Reduce_local_order_worksize reports", fc,
                            (long) work_bytes);
        return err_return(fc, MPI_ERR_ARG);
    }
    return shim_result(fc, rc, "%s needs its tables and work in device memory on one device (host tables, or no "
                       "work: the synchronous call only)", NULL);
}

int MPIX_Reduce_local_order(const MPI_Aint * displs, int nblocks, int *order, void *work, MPI_Aint work_bytes,
                            void *hip_stream)
{
    CS_RETURN(reduce_local_order(displs, nblocks, order, work, work_bytes, hip_stream));
}

/* ---- MPIX_Reduce_local_indexed_chunked: hot rows folded in chunks of 64 (see the header) */
#pragma weak MPIR_Hip_reduce_indexed_chunked
#pragma weak MPIR_Hip_chunked_worksize
#pragma weak MPIR_Hip_runs_build
static int reduce_local_indexed_chunked(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                        const MPI_Aint * inout_displs, const int *order, const int *runstart,
                                        MPI_Aint disp_unit, int nblocks, int blocklen, MPI_Datatype datatype,
                                        MPI_Op op, void *work, MPI_Aint work_bytes, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_indexed_chunked";
    int mpi_errno, opidx, elem, rc;
    uint64_t need = 0;
    const int empty = nblocks == 0 || blocklen == 0;
    _Static_assert(MPIX_REDUCE_LOCAL_CHUNK == MPIR_HIP_REDUCE_CHUNK, "the public chunk length is the kernels'");
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* the ordered call's order: an empty call's pointers are not looked at (the
     * op still is) */
    mpi_errno = empty ? validate(NULL, NULL, 0, datatype, op) : validate(inbuf, inoutbuf, blocklen, datatype, op);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (empty)
        return MPI_SUCCESS;
    if (order == NULL || runstart == NULL) {
        MPIR_Err_set_detail("%s is NULL and %s is not: the two tables come together", order == NULL ? "order" : "runstart",
                            order == NULL ? "runstart" : "order");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (inout_displs == NULL) {
        MPIR_Err_set_detail("order and runstart with no inout_displs: a packed target has no repeats to fold");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (work != NULL && work_bytes < 0) {
        MPIR_Err_set_detail("negative work_bytes %ld", (long) work_bytes);
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS ||
        (mpi_errno = shim_has(MPIR_Hip_reduce_indexed_chunked != NULL && MPIR_Hip_chunked_worksize != NULL,
                              "MPIR_Hip_reduce_indexed_chunked")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (work != NULL && MPIR_Hip_chunked_worksize((uint64_t) nblocks, (uint64_t) blocklen, elem, &need) == MPIR_HIP_OK &&
        (uint64_t) work_bytes < need) {
        MPIR_Err_set_detail("%s: work_bytes %ld is less than MPIX_Reduce_local_chunked_worksize reports", fc,
                            (long) work_bytes);
        return err_return(fc, MPI_ERR_ARG);
    }
    rc = MPIR_Hip_reduce_indexed_chunked(inbuf, (const int64_t *) in_displs, inoutbuf, (const int64_t *) inout_displs,
                                         order, runstart, (uint64_t) disp_unit, (uint64_t) nblocks, (uint64_t) blocklen,
                                         opidx, elem, work, (uint64_t) work_bytes, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, "%s needs device-resident operands on one device, and its tables and work there too "
                       "(host tables, or no work: the synchronous call only)",
                       "%s: a block's offset does not fit the address space, the order table is not a stable sort of "
                       "inout_displs, or the runstart table is not the first positions of its runs");
}

int MPIX_Reduce_local_indexed_chunked(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                      const MPI_Aint * inout_displs, const int *order, const int *runstart,
                                      MPI_Aint disp_unit, int nblocks, int blocklen, MPI_Datatype datatype, MPI_Op op,
                                      void *work, MPI_Aint work_bytes, void *hip_stream)
{
    /* neither table: the indexed call unchanged, its own name on the error stack */
    if (order == NULL && runstart == NULL)
        return MPIX_Reduce_local_indexed(inbuf, in_displs, inoutbuf, inout_displs, disp_unit, nblocks, blocklen,
                                         datatype, op, hip_stream);
    CS_RETURN(reduce_local_indexed_chunked(inbuf, in_displs, inoutbuf, inout_displs, order, runstart, disp_unit,
                                           nblocks, blocklen, datatype, op, work, work_bytes, hip_stream));
}

int MPIX_Reduce_local_chunked_worksize(int nblocks, int blocklen, MPI_Datatype datatype, MPI_Aint * work_bytes)
{
    static const char *fc = "MPIX_Reduce_local_chunked_worksize";
    uint64_t bytes = 0;
    int rc = MPI_SUCCESS, elem = 0;
    const MPIR_Type_desc *d;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);
    /* (the size needs the datatype's element bytes alone: the described type's class) */
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        rc = err_return(fc, MPI_ERR_COUNT);
    } else if ((d = MPIR_Type_lookup(datatype)) == NULL || (elem = d->elem) == 0) {
        MPIR_Err_set_detail("datatype 0x%x has no device element class", (unsigned) datatype);
        rc = err_return(fc, MPI_ERR_TYPE);
    } else if (work_bytes == NULL) {
        MPIR_Err_set_detail("work_bytes is NULL");
        rc = err_return(fc, MPI_ERR_ARG);
    } else if ((rc = shim_has(MPIR_Hip_chunked_worksize != NULL, "MPIR_Hip_chunked_worksize")) != MPI_SUCCESS) {
        rc = err_return(fc, rc);
    } else if (MPIR_Hip_chunked_worksize((uint64_t) nblocks, (uint64_t) blocklen, elem, &bytes) != MPIR_HIP_OK) {
        MPIR_Err_set_detail("the work of %d blocks of %d elements does not fit an MPI_Aint", nblocks, blocklen);
        rc = err_return(fc, MPI_ERR_ARG);
    } else {
        *work_bytes = (MPI_Aint) bytes;
    }
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);
    return rc;
}

static int reduce_local_runs(const MPI_Aint * displs, const int *order, int nblocks, int *runstart, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_runs";
    int rc;
    if (nblocks < 0) {
        MPIR_Err_set_detail("negative nblocks %d", nblocks);
        return err_return(fc, MPI_ERR_COUNT);
    }
    if (nblocks == 0)
        return MPI_SUCCESS;
    if (displs == NULL || order == NULL || runstart == NULL) {
        MPIR_Err_set_detail("%s is NULL", displs == NULL ? "displs" : order == NULL ? "order" : "runstart");
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((rc = shim_has(MPIR_Hip_runs_build != NULL, "MPIR_Hip_runs_build")) != MPI_SUCCESS)
        return err_return(fc, rc);
    rc = MPIR_Hip_runs_build((const int64_t *) displs, order, (uint64_t) nblocks, runstart, hip_stream,
                             hip_stream == NULL);
    return shim_result(fc, rc, "%s needs its three tables in device memory on one device (host tables: the "
                       "synchronous call only)", "%s: an entry of a host order table is out of range");
}

int MPIX_Reduce_local_runs(const MPI_Aint * displs, const int *order, int nblocks, int *runstart, void *hip_stream)
{
    CS_RETURN(reduce_local_runs(displs, order, nblocks, runstart, hip_stream));
}

/* ---- MPIX_Reduce_local_ragged: unequal pieces from a table of packed offsets (see the header) */
#pragma weak MPIR_Hip_reduce_ragged
static int reduce_local_ragged(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                               const MPI_Aint * inout_displs, const MPI_Aint * starts, MPI_Aint disp_unit,
                               int npieces, int count, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_ragged";
    int mpi_errno, opidx, elem, rc;
    _Static_assert(sizeof(MPI_Aint) == sizeof(int64_t), "the shim's tables are 64-bit entries");
    /* the indexed call's checks in the indexed call's order, npieces and count
     * where it has nblocks and blocklen */
    if (npieces < 0 || count < 0) {
        MPIR_Err_set_detail("negative %s %d", npieces < 0 ? "npieces" : "count", npieces < 0 ? npieces : count);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* an empty call's pointers are not looked at (the op still is) */
    mpi_errno = count == 0 ? validate(NULL, NULL, 0, datatype, op) : validate(inbuf, inoutbuf, count, datatype, op);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (count == 0)
        return MPI_SUCCESS;
    if (npieces == 0) {
        MPIR_Err_set_detail("count %d with no pieces", count);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (starts == NULL && (in_displs != NULL || inout_displs != NULL)) {
        MPIR_Err_set_detail("a displacement table needs starts");
        return err_return(fc, MPI_ERR_ARG);
    }
    if ((mpi_errno = builtin_op_elem(datatype, op, &opidx, &elem)) != MPI_SUCCESS ||
        (mpi_errno = shim_has(MPIR_Hip_reduce_ragged != NULL, "MPIR_Hip_reduce_ragged")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_ragged(inbuf, (const int64_t *) in_displs, inoutbuf, (const int64_t *) inout_displs,
                                (const int64_t *) starts, (uint64_t) disp_unit, (uint64_t) npieces, (uint64_t) count,
                                opidx, elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, EBUF_TABLES, EARG_RAGGED);
}

int MPIX_Reduce_local_ragged(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                             const MPI_Aint * inout_displs, const MPI_Aint * starts, MPI_Aint disp_unit,
                             int npieces, int count, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_ragged(inbuf, in_displs, inoutbuf, inout_displs, starts, disp_unit, npieces, count,
                                  datatype, op, hip_stream));
}

/* ---- MPIX_Reduce_local_fetch_ragged: the fetching reduction on a ragged target (see the header) */
#pragma weak MPIR_Hip_reduce_fetch_ragged

/* The op rule of the fetching calls whose byte ops are kernels (the ragged and
 * the ordered indexed one): *opidx and *elem of (datatype, op), or the error
 * class with the detail set. */
static int fetch_op_elem(MPI_Datatype datatype, MPI_Op op, int *opidx, int *elem)
{
    const int no_op = op == MPI_NO_OP, copy = no_op || op == MPI_REPLACE;
    int mpi_errno;
    /* MPIR_ERRTEST_OP_GACC (mpir_err.h:528-539): MPI_NO_OP and MPI_REPLACE pass,
     * a user op does not */
    if (op == MPI_OP_NULL) {
        MPIR_Err_set_detail("Null MPI_Op");
        return MPI_ERR_OP;
    }
    if (HANDLE_GET_MPI_KIND(op) != MPIR_OP_OBJ_KIND || HANDLE_GET_KIND(op) == HANDLE_KIND_INVALID ||
        (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN && !user_op_get(op)) ||
        (HANDLE_GET_KIND(op) == HANDLE_KIND_BUILTIN &&
         ((op & 0xf) >= MPIR_OP_N_BUILTIN || !MPIR_OP_HDL_TO_DTYPE_FN(op)))) {
        MPIR_Err_set_detail("Invalid MPI_Op");
        return MPI_ERR_OP;
    }
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN) {
        MPIR_Err_set_detail("MPI_Op is not a predefined operation; user MPI_Op functions run on the host");
        return MPI_ERR_OP;
    }
    *opidx = op & 0xf;
    if (copy) {
        /* the tables count elements of the datatype, so the byte ops need its
         * element size: the described type's class, or for another builtin handle
         * (MPI_WCHAR) a class of its size; a derived one needs MPICH's datatype engine */
        const MPIR_Type_desc *d = MPIR_Type_lookup(datatype);
        const unsigned h = (unsigned) datatype;
        *elem = 0;
        if (d) {
            *elem = d->elem;
        } else if ((h >> 30) == 1u && ((h >> 26) & 0xfu) == 0x3u) {     /* builtin-kind datatype: a class of its size */
            switch ((h >> 8) & 0xffu) {
                case 1: *elem = MPIR_HIP_U8; break;
                case 2: *elem = MPIR_HIP_U16; break;
                case 4: *elem = MPIR_HIP_U32; break;
                case 8: *elem = MPIR_HIP_U64; break;
                case 16: *elem = MPIR_HIP_CF64; break;
                case 32: *elem = MPIR_HIP_CF80; break;
            }
        }
        if (!*elem) {
            MPIR_Err_set_detail("%s: derived datatypes are not supported by this library", no_op ? "MPI_NO_OP" : "MPI_REPLACE");
            return MPI_ERR_TYPE;
        }
    } else {
        /* MPI_Reduce_local's datatype check (reduce_local.c:179-183), then the
         * compute switch's `default:` (LAND / LOR on floats) */
        mpi_errno = MPIR_OP_HDL_TO_DTYPE_FN(op) (datatype);
        if (mpi_errno != MPI_SUCCESS)
            return mpi_errno;
        *elem = MPIR_Op_resolve_elem(*opidx, datatype);
        if (!*elem) {
            MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
            return MPI_ERR_OP;
        }
    }
    return MPI_SUCCESS;
}

static int reduce_local_fetch_ragged(const void *inbuf, void *inoutbuf, const MPI_Aint * inout_displs,
                                     void *fetchbuf, const MPI_Aint * starts, MPI_Aint disp_unit, int npieces,
                                     int count, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_fetch_ragged";
    const int no_op = op == MPI_NO_OP;
    int mpi_errno, opidx, elem, rc;
    uint64_t bytes;
    _Static_assert(sizeof(MPI_Aint) == sizeof(int64_t), "the shim's tables are 64-bit entries");
    /* the ragged call's checks in the ragged call's order; where that call runs
     * MPI_Reduce_local's validation block, this one runs the fetch call's */
    if (npieces < 0 || count < 0) {
        MPIR_Err_set_detail("negative %s %d", npieces < 0 ? "npieces" : "count", npieces < 0 ? npieces : count);
        return err_return(fc, MPI_ERR_COUNT);
    }
    mpi_errno = fetch_op_elem(datatype, op, &opidx, &elem);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    /* the buffer rules of the validation block, where the ragged call has them
     * (an empty call's pointers are not looked at), MPI_NO_OP never looking at inbuf */
    if (count != 0 && !no_op && alias_check_enabled() && inbuf == inoutbuf) {
        MPIR_Err_set_detail("Buffers must not be aliased");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (count != 0 && ((!no_op && inbuf == MPI_IN_PLACE) || inoutbuf == MPI_IN_PLACE || fetchbuf == MPI_IN_PLACE)) {
        MPIR_Err_set_detail("buffer '%s' cannot be MPI_IN_PLACE",
                            !no_op && inbuf == MPI_IN_PLACE ? "inbuf" : inoutbuf == MPI_IN_PLACE ? "inoutbuf" : "fetchbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (count == 0)     /* no pointer or table is looked at */
        return MPI_SUCCESS;
    if (npieces == 0) {
        MPIR_Err_set_detail("count %d with no pieces", count);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (starts == NULL && inout_displs != NULL) {
        MPIR_Err_set_detail("a displacement table needs starts");
        return err_return(fc, MPI_ERR_ARG);
    }
    /* the fetch call's rules for fetchbuf */
    if (!fetchbuf) {
        MPIR_Err_set_detail("Null buffer pointer 'fetchbuf'");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    bytes = (uint64_t) count *MPIR_Hip_elem_size(elem);
    /* the two packed ranges, whatever MPIR_CVAR_COLL_ALIAS_CHECK says; a contiguous
     * target is a range too */
    if ((!no_op && ranges_overlap(fetchbuf, inbuf, bytes)) || (!inout_displs && ranges_overlap(fetchbuf, inoutbuf, bytes))) {
        MPIR_Err_set_detail("fetchbuf overlaps %s", !no_op && ranges_overlap(fetchbuf, inbuf, bytes) ? "inbuf" : "inoutbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if ((mpi_errno = shim_has(MPIR_Hip_reduce_fetch_ragged != NULL, "MPIR_Hip_reduce_fetch_ragged")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_fetch_ragged(inbuf, inoutbuf, (const int64_t *) inout_displs, fetchbuf,
                                      (const int64_t *) starts, (uint64_t) disp_unit, (uint64_t) npieces,
                                      (uint64_t) count, opidx, elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, "%s needs device-resident buffers on one device, its tables there too (host tables: "
                       "the synchronous call only), and fetchbuf outside the pieces' extent", EARG_RAGGED);
}

int MPIX_Reduce_local_fetch_ragged(const void *inbuf, void *inoutbuf, const MPI_Aint * inout_displs,
                                   void *fetchbuf, const MPI_Aint * starts, MPI_Aint disp_unit, int npieces,
                                   int count, MPI_Datatype datatype, MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_fetch_ragged(inbuf, inoutbuf, inout_displs, fetchbuf, starts, disp_unit, npieces, count,
                                        datatype, op, hip_stream));
}

/* ---- MPIX_Reduce_local_fetch_indexed_ordered: the ordered fetch-and-op (see the header) */
#pragma weak MPIR_Hip_reduce_fetch_indexed_ordered
static int reduce_local_fetch_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                              const MPI_Aint * inout_displs, void *fetchbuf, const int *order,
                                              MPI_Aint disp_unit, int nblocks, int blocklen, MPI_Datatype datatype,
                                              MPI_Op op, void *hip_stream)
{
    static const char *fc = "MPIX_Reduce_local_fetch_indexed_ordered";
    const int no_op = op == MPI_NO_OP;
    const int empty = nblocks == 0 || blocklen == 0;
    int mpi_errno, opidx, elem, rc;
    uint64_t bytes;
    /* the ordered call's checks in the ordered call's order; where that call runs
     * MPI_Reduce_local's validation block, this one runs the fetch call's */
    if (nblocks < 0 || blocklen < 0) {
        MPIR_Err_set_detail("negative %s %d", nblocks < 0 ? "nblocks" : "blocklen", nblocks < 0 ? nblocks : blocklen);
        return err_return(fc, MPI_ERR_COUNT);
    }
    mpi_errno = fetch_op_elem(datatype, op, &opidx, &elem);
    if (mpi_errno != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    /* the buffer rules of the validation block (an empty call's pointers are not
     * looked at), MPI_NO_OP never looking at inbuf */
    if (!empty && !no_op && alias_check_enabled() && inbuf == inoutbuf) {
        MPIR_Err_set_detail("Buffers must not be aliased");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (!empty && ((!no_op && inbuf == MPI_IN_PLACE) || inoutbuf == MPI_IN_PLACE || fetchbuf == MPI_IN_PLACE)) {
        MPIR_Err_set_detail("buffer '%s' cannot be MPI_IN_PLACE",
                            !no_op && inbuf == MPI_IN_PLACE ? "inbuf" : inoutbuf == MPI_IN_PLACE ? "inoutbuf" : "fetchbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (empty)          /* no pointer or table is looked at */
        return MPI_SUCCESS;
    if (inout_displs == NULL && order != NULL) {
        MPIR_Err_set_detail("an order table with no inout_displs: a packed target has no repeats to order");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (inout_displs == NULL && !no_op && in_displs != NULL) {
        MPIR_Err_set_detail("in_displs with no inout_displs: a packed target has no repeats, and a gather on the "
                            "origin side is not this call's job");
        return err_return(fc, MPI_ERR_ARG);
    }
    /* the fetch call's rules for fetchbuf */
    if (!fetchbuf) {
        MPIR_Err_set_detail("Null buffer pointer 'fetchbuf'");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    bytes = (uint64_t) nblocks *(uint64_t) blocklen *MPIR_Hip_elem_size(elem);
    /* the packed ranges, whatever MPIR_CVAR_COLL_ALIAS_CHECK says; a contiguous
     * target is a range too */
    if ((!no_op && !in_displs && ranges_overlap(fetchbuf, inbuf, bytes)) ||
        (!inout_displs && ranges_overlap(fetchbuf, inoutbuf, bytes))) {
        MPIR_Err_set_detail("fetchbuf overlaps %s",
                            !no_op && !in_displs && ranges_overlap(fetchbuf, inbuf, bytes) ? "inbuf" : "inoutbuf");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if ((mpi_errno = shim_has(MPIR_Hip_reduce_fetch_indexed_ordered != NULL,
                              "MPIR_Hip_reduce_fetch_indexed_ordered")) != MPI_SUCCESS)
        return err_return(fc, mpi_errno);
    rc = MPIR_Hip_reduce_fetch_indexed_ordered(inbuf, no_op ? NULL : (const int64_t *) in_displs, inoutbuf,
                                               (const int64_t *) inout_displs, fetchbuf, order, (uint64_t) disp_unit,
                                               (uint64_t) nblocks, (uint64_t) blocklen, opidx, elem, hip_stream,
                                               hip_stream == NULL);
    return shim_result(fc, rc, "%s needs device-resident buffers on one device, its tables there too (host tables: "
                       "the synchronous call only), and fetchbuf outside the target blocks' extent",
                       "%s: a block's offset does not fit the address space, the order table is not a stable sort of "
                       "inout_displs, or with no order table equal entries of inout_displs are not adjacent");
}

int MPIX_Reduce_local_fetch_indexed_ordered(const void *inbuf, const MPI_Aint * in_displs, void *inoutbuf,
                                            const MPI_Aint * inout_displs, void *fetchbuf, const int *order,
                                            MPI_Aint disp_unit, int nblocks, int blocklen, MPI_Datatype datatype,
                                            MPI_Op op, void *hip_stream)
{
    CS_RETURN(reduce_local_fetch_indexed_ordered(inbuf, in_displs, inoutbuf, inout_displs, fetchbuf, order, disp_unit,
                                                 nblocks, blocklen, datatype, op, hip_stream));
}

/* ---- MPIX_Compare_and_swap_indexed_ordered: batched CAS in table order (see the header) */
#pragma weak MPIR_Hip_cas_indexed_ordered
#pragma weak MPIR_Hip_cas_plan_info
/* MPIR_Type_is_rma_atomic (src/mpi/rma/rmatypeutil.c:23-43) for a build with no
 * Fortran and no C++: the C integer group and MPI_CHAR, MPI_AINT / MPI_OFFSET /
 * MPI_COUNT, MPI_C_BOOL and MPI_BYTE */
#define RMA_ATOMIC_GROUPS (G_C_INTEGER | G_C_INTEGER_EXTRA | G_FORTRAN_INTEGER | G_LOGICAL | G_BYTE)

static int compare_and_swap_indexed_ordered(const void *origin, const void *compare, void *target,
                                            const MPI_Aint * target_displs, void *result, const int *order,
                                            MPI_Aint disp_unit, int count, MPI_Datatype datatype, void *hip_stream)
{
    static const char *fc = "MPIX_Compare_and_swap_indexed_ordered";
    const MPIR_Type_desc *d;
    const unsigned h = (unsigned) datatype;
    uint64_t bytes;
    int rc;
    _Static_assert(sizeof(MPI_Aint) == sizeof(int64_t), "the shim's tables are 64-bit entries");
    if (count < 0) {
        MPIR_Err_set_detail("negative count %d", count);
        return err_return(fc, MPI_ERR_COUNT);
    }
    /* MPIR_ERRTEST_DATATYPE, then MPIR_ERRTEST_TYPE_RMA_ATOMIC (compare_and_swap.c:119-123) */
    d = MPIR_Type_lookup(datatype);
    if (!d) {
        if (datatype == MPI_DATATYPE_NULL)
            MPIR_Err_set_detail("Null datatype");
        else if ((h >> 30) == 1u && ((h >> 26) & 0xfu) == 0x3u)        /* another builtin-kind datatype (MPI_WCHAR) */
            MPIR_Err_set_detail("Datatype (0x%x) not permitted for atomic operations", h);
        else
            MPIR_Err_set_detail("Invalid datatype");
        return err_return(fc, MPI_ERR_TYPE);
    }
    if (!(d->groups & RMA_ATOMIC_GROUPS)) {
        MPIR_Err_set_detail("Datatype (%s) not permitted for atomic operations", d->name);
        return err_return(fc, MPI_ERR_TYPE);
    }
    if (disp_unit <= 0) {
        MPIR_Err_set_detail("disp_unit %ld is not positive", (long) disp_unit);
        return err_return(fc, MPI_ERR_ARG);
    }
    if (count == 0)     /* no pointer or table is looked at */
        return MPI_SUCCESS;
    /* MPIR_ERRTEST_ARGNULL (compare_and_swap.c:115-117) */
    if (!origin || !compare || !result) {
        MPIR_Err_set_detail("Null pointer in parameter %s", !origin ? "origin" : !compare ? "compare" : "result");
        return err_return(fc, MPI_ERR_ARG);
    }
    if (origin == MPI_IN_PLACE || compare == MPI_IN_PLACE || target == MPI_IN_PLACE || result == MPI_IN_PLACE) {
        MPIR_Err_set_detail("buffer '%s' cannot be MPI_IN_PLACE",
                            origin == MPI_IN_PLACE ? "origin" : compare == MPI_IN_PLACE ? "compare" :
                            target == MPI_IN_PLACE ? "target" : "result");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (alias_check_enabled() && (origin == target || compare == target)) {
        MPIR_Err_set_detail("Buffers must not be aliased");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if (target_displs == NULL && order != NULL) {
        MPIR_Err_set_detail("an order table with no target_displs: a contiguous target has no repeats to order");
        return err_return(fc, MPI_ERR_ARG);
    }
    bytes = (uint64_t) count *MPIR_Hip_elem_size(d->elem);
    /* result's packed range, whatever MPIR_CVAR_COLL_ALIAS_CHECK says; origin and
     * compare are only read and may overlap each other; a contiguous target is a range too */
    if (ranges_overlap(result, origin, bytes) || ranges_overlap(result, compare, bytes) ||
        (!target_displs && ranges_overlap(result, target, bytes))) {
        MPIR_Err_set_detail("result overlaps %s", ranges_overlap(result, origin, bytes) ? "origin" :
                            ranges_overlap(result, compare, bytes) ? "compare" : "target");
        return err_return(fc, MPI_ERR_BUFFER);
    }
    if ((rc = shim_has(MPIR_Hip_cas_indexed_ordered != NULL, "MPIR_Hip_cas_indexed_ordered")) != MPI_SUCCESS)
        return err_return(fc, rc);
    rc = MPIR_Hip_cas_indexed_ordered(origin, compare, target, (const int64_t *) target_displs, result, order,
                                      (uint64_t) disp_unit, (uint64_t) count, d->elem, hip_stream, hip_stream == NULL);
    return shim_result(fc, rc, "%s needs device-resident buffers on one device, its tables there too (host tables: "
                       "the synchronous call only), and result outside the targets' extent",
                       "%s: a target's offset does not fit the address space, the order table is not a stable sort of "
                       "target_displs, or with no order table equal entries of target_displs are not adjacent");
}

int MPIX_Compare_and_swap_indexed_ordered(const void *origin, const void *compare, void *target,
                                          const MPI_Aint * target_displs, void *result, const int *order,
                                          MPI_Aint disp_unit, int count, MPI_Datatype datatype, void *hip_stream)
{
    CS_RETURN(compare_and_swap_indexed_ordered(origin, compare, target, target_displs, result, order, disp_unit,
                                               count, datatype, hip_stream));
}

/* ---- MPI_Op_create / MPI_Op_free / MPI_Op_commutative ------------------ */
int PMPI_Op_create(MPI_User_function * user_fn, int commute, MPI_Op * op)
{
    int mpi_errno;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);         /* op_create.c:151 */
    mpi_errno = MPIR_Op_create_impl(user_fn, commute, op);
    if (mpi_errno != MPI_SUCCESS)
        mpi_errno = err_return("PMPI_Op_create", mpi_errno);
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);
    return mpi_errno;
}

int MPI_Op_create(MPI_User_function * user_fn, int commute, MPI_Op * op)
    __attribute__ ((weak, alias("PMPI_Op_create")));

/* op_free.c:79-122: a predefined op is "**permop" */
int PMPI_Op_free(MPI_Op * op)
{
    int mpi_errno = MPI_SUCCESS;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);         /* op_free.c:86 */
    if (HANDLE_GET_KIND(*op) == HANDLE_KIND_BUILTIN && HANDLE_GET_MPI_KIND(*op) == MPIR_OP_OBJ_KIND) {
        MPIR_Err_set_detail("Cannot free permanent MPI_Op");       /* "**permop" */
        mpi_errno = err_return("PMPI_Op_free", MPI_ERR_OP);
    } else if (!user_op_get(*op)) {
        MPIR_Err_set_detail("Invalid MPI_Op");
        mpi_errno = err_return("PMPI_Op_free", MPI_ERR_OP);
    } else {
        MPIR_Op_free_impl(op);
    }
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);          /* op_free.c:120 */
    return mpi_errno;
}

int MPI_Op_free(MPI_Op * op) __attribute__ ((weak, alias("PMPI_Op_free")));

/* op_commutative.c:39-53 */
int MPIR_Op_is_commutative(MPI_Op op)
{
    MPIR_Op *op_ptr;
    if (HANDLE_GET_KIND(op) == HANDLE_KIND_BUILTIN)
        return 1;
    op_ptr = MPIR_Op_get_ptr_fn(op);
    return !(op_ptr && op_ptr->kind == MPIR_OP_KIND__USER_NONCOMMUTE);
}

/* op_commutative.c:101-140 */
int PMPI_Op_commutative(MPI_Op op, int *commute)
{
    MPIR_Op *op_ptr = NULL;
    int mpi_errno;
    MPIR_Dropin_cs_enter(MPIR_DROPIN_CS_GLOBAL);         /* op_commutative.c:109 */
    if (HANDLE_GET_KIND(op) != HANDLE_KIND_BUILTIN)
        op_ptr = user_op_get(op);
    else if (HANDLE_GET_MPI_KIND(op) == MPIR_OP_OBJ_KIND)
        op_ptr = MPIR_Op_get_ptr_fn(op);
    if (!op_ptr) {
        MPIR_Err_set_detail("Invalid MPI_Op");
        mpi_errno = err_return("PMPI_Op_commutative", MPI_ERR_OP);
    } else {
        mpi_errno = MPIR_Op_commutative(op_ptr, commute);
    }
    MPIR_Dropin_cs_exit(MPIR_DROPIN_CS_GLOBAL);          /* op_commutative.c:136 */
    return mpi_errno;
}

int MPI_Op_commutative(MPI_Op op, int *commute) __attribute__ ((weak, alias("PMPI_Op_commutative")));
