/*
 * coll_hip.c -- device reduction collectives over RCCL / an in-process
 * loopback, built on the gfx950 MPIR_Reduce_local kernels.  See
 * include/mpix_hip_coll.h for the contract.
 *
 * Reference schedules reproduced (bit-identical results):
 *   Allreduce, one node: allreduce_intra_smp.c (MPIR_Reduce to node root via
 *     reduce_intra_reduce_scatter_gather.c:130-250, then MPIR_Bcast).
 *     Non-power-of-two pre-fold :138-170 (odd rank r < 2*rem sends to r-1,
 *     even computes x_r (+) x_{r+1}); recursive halving :186-249 leaves newrank
 *     n owning block bitrev(n), reduced as ((y0+y1)+(y2+y3))+... with
 *     y_j = contribution of newrank n ^ j (tests/test_schedule_fused_gpu.py).
 *   Reduce_scatter_block: reduce_scatter_block_intra_pairwise.c:75-134:
 *     block r = ((x_r + x_{r-1}) + x_{r-2}) + ... .
 * MI355X form: the log2(p) Sendrecv+Reduce_local rounds become one all-to-all
 * (every xGMI link busy at once) + one fused combine pass + one allgather.
 */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "mpix_hip_coll.h"
#include "mpir_op_types.h"

#define COMM_RCCL 1
#define COMM_LOOPBACK 2
#define MAX_XFER 256
/* Ranks of a communicator: the loopback hub's slots and every per-rank array
 * (cnts / disps / ys / chain).  A combine takes one operand per rank, so this
 * is also MPIR_Hip_combine's operand limit (kMaxAnyOperands = 64 in
 * csrc/hip/reduce_kernels.hpp; mpir_hip_reduce.h documents "n <= 64" but
 * exposes no constant to check against: keep the two equal by hand). */
#define MAX_RANKS 64
#define REDUCE_SHORT_MSG_SIZE 2048            /* reduce.c:14-17 */
#define RSB_COMMUTATIVE_LONG_MSG_SIZE 524288  /* reduce_scatter.c:14-17 */

typedef struct {
    void *buf;
    size_t bytes;
    int peer;
} xfer_t;

/* ------------------------------------------------------------ RCCL (dlopen) */
static struct {
    int loaded;
    void *so;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*ReduceScatter)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                                  hipStream_t);
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                           hipStream_t);
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*GroupStart)(void);
    ncclResult_t (*GroupEnd)(void);
    const char *(*GetErrorString)(ncclResult_t);
} rccl;
static pthread_mutex_t rccl_lock = PTHREAD_MUTEX_INITIALIZER;

static int rccl_load(void)
{
    static const char *names[] = { "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so" };
    /* TEST ONLY: a stand-in library that records the calls
     * (tests/progs/rccl_stub.c, tests/test_rccl_sequence_cpu.py) */
    const char *test_lib = getenv("MPIR_TEST_RCCL_LIBRARY");
    size_t i;
    pthread_mutex_lock(&rccl_lock);
    if (rccl.loaded) {
        pthread_mutex_unlock(&rccl_lock);
        return rccl.loaded > 0;
    }
    if (test_lib && *test_lib)
        rccl.so = dlopen(test_lib, RTLD_NOW | RTLD_GLOBAL);
    for (i = 0; i < sizeof(names) / sizeof(names[0]) && !rccl.so && !(test_lib && *test_lib); i++)
        rccl.so = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (rccl.so) {
#define SYM(f, n) *(void **) (&rccl.f) = dlsym(rccl.so, n)
        SYM(GetUniqueId, "ncclGetUniqueId");
        SYM(CommInitRank, "ncclCommInitRank");
        SYM(CommDestroy, "ncclCommDestroy");
        SYM(AllReduce, "ncclAllReduce");
        SYM(ReduceScatter, "ncclReduceScatter");
        SYM(Reduce, "ncclReduce");
        SYM(Send, "ncclSend");
        SYM(Recv, "ncclRecv");
        SYM(GroupStart, "ncclGroupStart");
        SYM(GroupEnd, "ncclGroupEnd");
        SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    }
    rccl.loaded = (rccl.so && rccl.GetUniqueId && rccl.CommInitRank && rccl.Send && rccl.Recv &&
                   rccl.GroupStart && rccl.GroupEnd && rccl.AllReduce && rccl.ReduceScatter && rccl.Reduce) ? 1 : -1;
    pthread_mutex_unlock(&rccl_lock);
    return rccl.loaded > 0;
}

static long cvar_long(const char *name, long dflt)
{
    const char *v = getenv(name);
    return v && *v ? strtol(v, NULL, 0) : dflt;
}

/* ------------------------------------------------------------ communicators */
typedef struct loop_hub {
    int size;
    int refs;
    pthread_barrier_t bar;
    pthread_mutex_t lock;
    struct {
        int nsend;
        xfer_t sends[MAX_XFER];
        hipEvent_t ready;
    } slot[MAX_RANKS];
} loop_hub_t;
_Static_assert(sizeof(((loop_hub_t *) 0)->slot) / sizeof(((loop_hub_t *) 0)->slot[0]) == MAX_RANKS,
               "one hub slot per rank of the largest communicator");

#define MAX_PIPE 16            /* chunks of a pipelined exchange (pipe_chunks) */

struct MPIX_Hip_comm_s {
    int kind, rank, size, device;
    hipStream_t stream;
    void *scratch;
    size_t scratch_bytes;
    ncclComm_t nccl;
    loop_hub_t *hub;
    /* pipelined schedules (pipe_chunks): the folds' stream, one event per
     * chunk's exchange and one per chunk's fold (created on first use) */
    hipStream_t fold_stream;
    hipEvent_t xev[MAX_PIPE], fev[MAX_PIPE];
};

/* One call of a collective: what coll_begin() settles for every one of them
 * and coll_end() undoes. */
typedef struct {
    const char *fc;             /* the MPIX_ entry point, for error reports */
    struct MPIX_Hip_comm_s *c;
    hipStream_t s;
    int user_stream;            /* s is the caller's: left unsynchronised */
    int saved_device, switched; /* the caller's device, and whether it was left */
    int elem, opidx;
    size_t esz;
} coll_t;

/* ------------------------------------------------------------ error reports:
 * each sets the detail and returns the MPI error class; the entry points turn
 * it into the final code (MPIR_Err_return) */
static int hip_err(const char *fc, hipError_t e)
{
    MPIR_Err_set_detail("%s: HIP error %s", fc, hipGetErrorString(e));
    return MPI_ERR_OTHER;
}

static int rccl_err(const char *what, ncclResult_t r)
{
    MPIR_Err_set_detail("%s: %s", what, rccl.GetErrorString ? rccl.GetErrorString(r) : "?");
    return MPI_ERR_OTHER;
}

#define HIPTRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
        MPIR_Err_set_detail("%s: %s", #x, hipGetErrorString(e_)); return MPI_ERR_OTHER; } } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != MPI_SUCCESS) return rc_; } while (0)

static int comm_init_common(struct MPIX_Hip_comm_s *c)
{
    hipError_t e = hipGetDevice(&c->device);
    if (e == hipSuccess)
        e = hipStreamCreate(&c->stream);
    return e == hipSuccess ? 0 : (int) e;
}

int MPIX_Hip_comm_get_unique_id(void *id)
{
    ncclUniqueId u;
    ncclResult_t r;
    if (!rccl_load()) {
        MPIR_Err_set_detail("RCCL (librccl.so.1) could not be loaded");
        return MPIR_Err_return("MPIX_Hip_comm_get_unique_id", MPI_ERR_OTHER);
    }
    r = rccl.GetUniqueId(&u);
    if (r != ncclSuccess)
        return MPIR_Err_return("MPIX_Hip_comm_get_unique_id", rccl_err("ncclGetUniqueId", r));
    memcpy(id, &u, sizeof(u));
    return MPI_SUCCESS;
}

int MPIX_Hip_comm_create(const void *id, int size, int rank, MPIX_Hip_comm * comm)
{
    static const char *fc = "MPIX_Hip_comm_create";
    struct MPIX_Hip_comm_s *c;
    ncclUniqueId u;
    ncclResult_t r;
    int e;
    if (size < 1 || rank < 0 || rank >= size || size > MAX_RANKS) {
        MPIR_Err_set_detail("%s: invalid size/rank", fc);
        return MPIR_Err_return(fc, MPI_ERR_ARG);
    }
    if (!rccl_load()) {
        MPIR_Err_set_detail("RCCL (librccl.so.1) could not be loaded");
        return MPIR_Err_return(fc, MPI_ERR_OTHER);
    }
    c = calloc(1, sizeof(*c));
    c->kind = COMM_RCCL;
    c->rank = rank;
    c->size = size;
    if ((e = comm_init_common(c)) != 0) {
        free(c);
        return MPIR_Err_return(fc, hip_err(fc, (hipError_t) e));
    }
    memcpy(&u, id, sizeof(u));
    r = rccl.CommInitRank(&c->nccl, size, u, rank);
    if (r != ncclSuccess) {
        (void) hipStreamDestroy(c->stream);
        free(c);
        return MPIR_Err_return(fc, rccl_err("ncclCommInitRank", r));
    }
    *comm = c;
    return MPI_SUCCESS;
}

int MPIX_Hip_comm_create_loopback(int size, MPIX_Hip_comm * comms)
{
    static const char *fc = "MPIX_Hip_comm_create_loopback";
    loop_hub_t *hub;
    int r, e;
    if (size < 1 || size > MAX_RANKS) {
        MPIR_Err_set_detail("%s: size must be 1..%d", fc, MAX_RANKS);
        return MPIR_Err_return(fc, MPI_ERR_ARG);
    }
    hub = calloc(1, sizeof(*hub));
    hub->size = size;
    hub->refs = size;
    pthread_barrier_init(&hub->bar, NULL, (unsigned) size);
    pthread_mutex_init(&hub->lock, NULL);
    for (r = 0; r < size; r++) {
        struct MPIX_Hip_comm_s *c = calloc(1, sizeof(*c));
        c->kind = COMM_LOOPBACK;
        c->rank = r;
        c->size = size;
        c->hub = hub;
        if ((e = comm_init_common(c)) != 0)
            return MPIR_Err_return(fc, hip_err(fc, (hipError_t) e));
        if ((e = hipEventCreateWithFlags(&hub->slot[r].ready, hipEventDisableTiming)) != hipSuccess)
            return MPIR_Err_return(fc, hip_err(fc, (hipError_t) e));
        comms[r] = c;
    }
    return MPI_SUCCESS;
}

int MPIX_Hip_comm_free(MPIX_Hip_comm * comm)
{
    struct MPIX_Hip_comm_s *c = *comm;
    if (!c)
        return MPI_SUCCESS;
    (void) hipStreamSynchronize(c->stream);
    if (c->kind == COMM_RCCL && c->nccl && rccl.CommDestroy)
        rccl.CommDestroy(c->nccl);
    if (c->kind == COMM_LOOPBACK) {
        loop_hub_t *hub = c->hub;
        int last;
        pthread_mutex_lock(&hub->lock);
        last = --hub->refs == 0;
        pthread_mutex_unlock(&hub->lock);
        if (last) {
            int r;
            for (r = 0; r < hub->size; r++)
                (void) hipEventDestroy(hub->slot[r].ready);
            pthread_barrier_destroy(&hub->bar);
            pthread_mutex_destroy(&hub->lock);
            free(hub);
        }
    }
    if (c->scratch)
        (void) hipFree(c->scratch);
    if (c->fold_stream) {
        int k;
        (void) hipStreamSynchronize(c->fold_stream);
        for (k = 0; k < MAX_PIPE; k++) {
            (void) hipEventDestroy(c->xev[k]);
            (void) hipEventDestroy(c->fev[k]);
        }
        (void) hipStreamDestroy(c->fold_stream);
    }
    (void) hipStreamDestroy(c->stream);
    free(c);
    *comm = NULL;
    return MPI_SUCCESS;
}

int MPIX_Hip_comm_rank(MPIX_Hip_comm comm, int *rank)
{
    *rank = comm->rank;
    return MPI_SUCCESS;
}

int MPIX_Hip_comm_size(MPIX_Hip_comm comm, int *size)
{
    *size = comm->size;
    return MPI_SUCCESS;
}

/* the communicator's scratch, grown to `bytes` */
static int comm_scratch(struct MPIX_Hip_comm_s *c, size_t bytes, char **out, const char *fc)
{
    if (c->scratch_bytes < bytes) {
        hipError_t e;
        if (c->scratch) {
            (void) hipStreamSynchronize(c->stream);
            (void) hipDeviceSynchronize();
            (void) hipFree(c->scratch);
        }
        c->scratch = NULL;
        c->scratch_bytes = 0;
        e = hipMalloc(&c->scratch, bytes);
        if (e != hipSuccess) {
            MPIR_Err_set_detail("%s: scratch allocation failed", fc);
            return MPI_ERR_NO_MEM;
        }
        c->scratch_bytes = bytes;
    }
    *out = c->scratch;
    return MPI_SUCCESS;
}

/* ------------------------------------------------------------ transport:
 * one group of point-to-point transfers that progress together (all xGMI
 * links at once); completes in stream order. */
static int group_exchange(struct MPIX_Hip_comm_s *c, const xfer_t *sends, int nsend, const xfer_t *recvs,
                          int nrecv, hipStream_t s)
{
    int i, j;
    if (c->kind == COMM_RCCL) {
        ncclResult_t r = rccl.GroupStart();
        for (i = 0; i < nsend && r == ncclSuccess; i++)
            if (sends[i].bytes)
                r = rccl.Send(sends[i].buf, sends[i].bytes, ncclUint8, sends[i].peer, c->nccl, s);
        for (i = 0; i < nrecv && r == ncclSuccess; i++)
            if (recvs[i].bytes)
                r = rccl.Recv(recvs[i].buf, recvs[i].bytes, ncclUint8, recvs[i].peer, c->nccl, s);
        {
            ncclResult_t r2 = rccl.GroupEnd();
            if (r == ncclSuccess)
                r = r2;
        }
        return r == ncclSuccess ? MPI_SUCCESS : rccl_err("RCCL grouped send/recv", r);
    } else {
        /* loopback: post sends + a ready event; every receiver copies from the
         * matching sender once that event has fired; barrier both sides so no
         * sender reuses a buffer before its readers are done */
        loop_hub_t *hub = c->hub;
        hipError_t e;
        if (nsend > MAX_XFER)
            return MPI_ERR_INTERN;
        hub->slot[c->rank].nsend = nsend;
        memcpy(hub->slot[c->rank].sends, sends, sizeof(xfer_t) * (size_t) nsend);
        e = hipEventRecord(hub->slot[c->rank].ready, s);
        pthread_barrier_wait(&hub->bar);
        for (i = 0; i < nrecv && e == hipSuccess; i++) {
            int peer = recvs[i].peer, found = 0;
            for (j = 0; j < hub->slot[peer].nsend; j++) {
                const xfer_t *x = &hub->slot[peer].sends[j];
                if (x->peer == c->rank) {
                    if (x->bytes != recvs[i].bytes) {
                        MPIR_Err_set_detail("loopback: size mismatch %zu vs %zu", x->bytes, recvs[i].bytes);
                        pthread_barrier_wait(&hub->bar);
                        return MPI_ERR_INTERN;
                    }
                    e = hipStreamWaitEvent(s, hub->slot[peer].ready, 0);
                    if (e == hipSuccess && x->bytes)
                        e = hipMemcpyAsync(recvs[i].buf, x->buf, x->bytes, hipMemcpyDeviceToDevice, s);
                    found = 1;
                    break;
                }
            }
            if (!found && recvs[i].bytes) {
                MPIR_Err_set_detail("loopback: no matching send from %d", peer);
                pthread_barrier_wait(&hub->bar);
                return MPI_ERR_INTERN;
            }
        }
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        pthread_barrier_wait(&hub->bar);
        if (e != hipSuccess) {
            MPIR_Err_set_detail("loopback transfer: %s", hipGetErrorString(e));
            return MPI_ERR_OTHER;
        }
        return MPI_SUCCESS;
    }
}

/* ------------------------------------------------------------ pipelining
 * The reference-order schedules move every block first and fold after (the
 * reference's rounds are step-serial too, allreduce_intra_reduce_scatter_
 * allgather.c:170-260, reduce_scatter_block_intra_pairwise.c:97-134).  For
 * large blocks the exchange is cut into chunks -- byte ranges [k * chunk, ...)
 * of every transfer, one group per chunk on every rank -- and chunk k's fold
 * runs on the communicator's fold stream while chunk k+1 moves: the folds
 * hide behind the transfers.  Element-wise folds over the same operands in the
 * same order: the results are bit-identical to the unchunked schedule.  The
 * pipelined folds keep their LDS cap: beside RCCL's kernel the capped fold
 * leaves it faster than the uncapped one (a one-rank all_reduce 56.9 against
 * 71.2 us, 21.8 alone), and in the pipeline the two are within
 * 1 % (tools/archive/pipeline_overlap.cpp, profiles/r06/pipeline_overlap.log); a caller
 * that wants the other choice has MPIR_Hip_combine_set_flags.
 * MPIR_CVAR_DEVICE_COLL_PIPELINE_KB: the chunk (default 32768 = 32 MiB; 0 =
 * never pipeline); a schedule pipelines when its largest block spans at least
 * two chunks, in at most MAX_PIPE chunks. */
static int pipe_chunks(size_t block_bytes, size_t * chunk)
{
    long kb = cvar_long("MPIR_CVAR_DEVICE_COLL_PIPELINE_KB", 32768);
    size_t ch, n;
    if (kb <= 0)
        return 1;
    ch = ((size_t) kb << 10) & ~(size_t) 255;
    if (ch < 256 || block_bytes < 2 * ch)
        return 1;
    n = (block_bytes + ch - 1) / ch;
    if (n > MAX_PIPE) {
        ch = ((block_bytes + MAX_PIPE - 1) / MAX_PIPE + 255) & ~(size_t) 255;
        n = (block_bytes + ch - 1) / ch;
    }
    *chunk = ch;
    return (int) n;
}

static int pipe_init(struct MPIX_Hip_comm_s *c)
{
    hipError_t e = hipSuccess;
    int k;
    if (c->fold_stream)
        return MPI_SUCCESS;
    for (k = 0; k < MAX_PIPE && e == hipSuccess; k++) {
        e = hipEventCreateWithFlags(&c->xev[k], hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&c->fev[k], hipEventDisableTiming);
    }
    if (e == hipSuccess)
        e = hipStreamCreate(&c->fold_stream);
    if (e != hipSuccess) {
        MPIR_Err_set_detail("pipelined schedule: %s", hipGetErrorString(e));
        return MPI_ERR_OTHER;
    }
    return MPI_SUCCESS;
}

/* chunk k of a transfer list: [k * chunk, min((k + 1) * chunk, bytes)) of each
 * (empty past its end: both sides compute it from the same block size) */
static void chunk_of(const xfer_t *x, int n, int k, size_t chunk, xfer_t *out)
{
    int i;
    for (i = 0; i < n; i++) {
        size_t off = (size_t) k * chunk;
        out[i].peer = x[i].peer;
        out[i].buf = (char *) x[i].buf + (off < x[i].bytes ? off : x[i].bytes);
        out[i].bytes = off < x[i].bytes ? (x[i].bytes - off < chunk ? x[i].bytes - off : chunk) : 0;
    }
}

/* ------------------------------------------------------------ folds
 * the two kernels every schedule is built from, with their error report */
static int kernel_err(const coll_t *f, int rc)
{
    if (rc) {
        MPIR_Op_report_hip_error(f->fc, rc);
        return MPI_ERR_OTHER;
    }
    return MPI_SUCCESS;
}

static int fold_combine(const coll_t *f, const void *const *ys, int n, void *out, long count, int order,
                        hipStream_t s)
{
    return kernel_err(f, MPIR_Hip_combine(ys, n, out, (uint64_t) count, f->opidx, f->elem, order, s, 0));
}

static int fold_tree(const coll_t *f, const void *const *ys, int n, void *out, long count)
{
    return fold_combine(f, ys, n, out, count, MPIR_HIP_ORDER_TREE, f->s);
}

static int fold_step(const coll_t *f, const void *src, void *dst, long count)
{
    return kernel_err(f, MPIR_Hip_reduce(src, dst, (uint64_t) count, f->opidx, f->elem, f->s, 0));
}

/* A pipelined fold: `out_bytes` of output from n operands, folded chunk by
 * chunk with operands and output shifted by the chunk's offset. */
typedef struct {
    const void *const *ys;
    int n, order;
    char *out;
    size_t out_bytes;
} fold_ctx_t;

static int chunk_fold(const coll_t *f, const fold_ctx_t *fo, size_t off, size_t len, hipStream_t fs)
{
    const void *ys[MAX_RANKS];
    int i;
    for (i = 0; i < fo->n; i++)
        ys[i] = (const char *) fo->ys[i] + off;
    return fold_combine(f, ys, fo->n, fo->out + off, (long) (len / f->esz), fo->order, fs);
}

/* chunk k of `sends` / `recvs` as one group on s */
static int exchange_chunk(struct MPIX_Hip_comm_s *c, const xfer_t *sends, int nsend, const xfer_t *recvs, int nrecv,
                          int k, size_t chunk, hipStream_t s)
{
    xfer_t sk[MAX_XFER], rk[MAX_XFER];
    chunk_of(sends, nsend, k, chunk, sk);
    chunk_of(recvs, nrecv, k, chunk, rk);
    return group_exchange(c, sk, nsend, rk, nrecv, s);
}

/* Exchange `sends` / `recvs` in nchunk groups on the call's stream; after
 * group k, chunk k of `fo` (out_bytes 0: this rank folds nothing) on the fold
 * stream, ordered after it by xev[k]; fev[k] marks fold k done. */
static int exchange_fold_pipelined(const coll_t *f, const xfer_t *sends, int nsend, const xfer_t *recvs, int nrecv,
                                   int nchunk, size_t chunk, const fold_ctx_t *fo)
{
    struct MPIX_Hip_comm_s *c = f->c;
    const size_t out_bytes = fo->out_bytes;
    hipStream_t s = f->s;
    int k, rc = MPI_SUCCESS;
    hipError_t e = hipSuccess;
    for (k = 0; k < nchunk && rc == MPI_SUCCESS; k++) {
        size_t off = (size_t) k * chunk;
        if ((rc = exchange_chunk(c, sends, nsend, recvs, nrecv, k, chunk, s)) != MPI_SUCCESS)
            break;
        if ((e = hipEventRecord(c->xev[k], s)) != hipSuccess ||
            (e = hipStreamWaitEvent(c->fold_stream, c->xev[k], 0)) != hipSuccess)
            break;
        if (off < out_bytes &&
            (rc = chunk_fold(f, fo, off, out_bytes - off < chunk ? out_bytes - off : chunk,
                             c->fold_stream)) != MPI_SUCCESS)
            break;
        if ((e = hipEventRecord(c->fev[k], c->fold_stream)) != hipSuccess)
            break;
    }
    if (e != hipSuccess) {
        MPIR_Err_set_detail("pipelined schedule: %s", hipGetErrorString(e));
        return MPI_ERR_OTHER;
    }
    return rc;
}

/* The exchange that follows a pipelined fold, in the same chunks: chunk k
 * leaves once its fold is done (fev[k]). */
static int exchange_after_folds(const coll_t *f, const xfer_t *sends, int nsend, const xfer_t *recvs, int nrecv,
                                int nchunk, size_t chunk)
{
    int k;
    for (k = 0; k < nchunk; k++) {
        HIPTRY(hipStreamWaitEvent(f->s, f->c->fev[k], 0));
        TRY(exchange_chunk(f->c, sends, nsend, recvs, nrecv, k, chunk, f->s));
    }
    return MPI_SUCCESS;
}

/* ------------------------------------------------------------ helpers */
static void xfer_add(xfer_t *list, int *n, const void *buf, size_t bytes, int peer)
{
    list[*n].buf = (void *) buf;
    list[*n].bytes = bytes;
    list[(*n)++].peer = peer;
}

/* Byte stride between staging slots.  Slots at a power-of-two stride (equal
 * blocks of a power-of-two message) put the P operand streams of a fused
 * combine on the same HBM channels at the same moment: 8 x 32 MiB TREE8 fp32
 * ran at 0.689 of the HBM peak with a 32 MiB stride, 0.767 with 32 MiB +
 * 4352 B (4 KiB + 256), 0.717 with + 256 B only (rocprofv3 kernel trace,
 * tools/multi_gap_ab.hip, profiles/archive/r01s3_multi_skew_ab.log).  The best
 * skew depends on the block size (the address bits the blocks themselves set):
 * around 128 MiB blocks (config 5's 8 x 128 MiB CHAIN8) 6400 B ran 1.3-4.5
 * points above 4352 B in seven sweeps on five boxes, at 32 / 64 MiB 0.3-1 point
 * below it, at 256 MiB within a point (tools/archive/fold_skew.hip, chain_shape.hip
 * slabskew; profiles/r05/fold_skew*.log, slabskew.log).  The skew keeps the
 * 256 B alignment (fused kernels need the operands equal mod 16). */
static size_t stage_stride(size_t bytes)
{
    size_t st = (bytes + 255) & ~(size_t) 255;
    if (st >= ((size_t) 96 << 20) && st < ((size_t) 192 << 20))
        return st + 6400;
    return st >= ((size_t) 1 << 20) ? st + 4352 : st;
}

static int pof2_of(int p)
{
    int q = 1;
    while (q * 2 <= p)
        q *= 2;
    return q;
}

static int ilog2(int pof2)
{
    int bits = 0;
    while ((1 << bits) < pof2)
        bits++;
    return bits;
}

static int bitrev(int n, int bits)
{
    int r = 0, i;
    for (i = 0; i < bits; i++)
        if (n & (1 << i))
            r |= 1 << (bits - 1 - i);
    return r;
}

/* MPIR_Allreduce_intra_auto's branch (allreduce.c:145-217) from the CVARs a
 * user can set (defaults in brackets): MPIR_CVAR_ENABLE_SMP_COLLECTIVES [1],
 * MPIR_CVAR_ENABLE_SMP_ALLREDUCE [1], MPIR_CVAR_MAX_SMP_ALLREDUCE_MSG_SIZE [0],
 * MPIR_CVAR_ALLREDUCE_SHORT_MSG_SIZE [2048].  The device communicator is taken
 * as node-aware (one node).  Note the reference's nbytes: it is 0 unless
 * MAX_SMP_ALLREDUCE_MSG_SIZE is set (:159), so the flat branch then always picks
 * recursive doubling. */
#define FLAT_NO 0
#define FLAT_RECURSIVE_DOUBLING 1
#define FLAT_RABENSEIFNER 2
static int allreduce_flat_choice(size_t bytes, long count, int pof2)
{
    const long max_smp = cvar_long("MPIR_CVAR_MAX_SMP_ALLREDUCE_MSG_SIZE", 0);
    const long nbytes = max_smp ? (long) bytes : 0;
    if (cvar_long("MPIR_CVAR_ENABLE_SMP_COLLECTIVES", 1) && cvar_long("MPIR_CVAR_ENABLE_SMP_ALLREDUCE", 1) &&
        nbytes <= max_smp)
        return FLAT_NO;
    if (nbytes <= cvar_long("MPIR_CVAR_ALLREDUCE_SHORT_MSG_SIZE", 2048) || count < pof2)
        return FLAT_RECURSIVE_DOUBLING;
    return FLAT_RABENSEIFNER;
}

/* The pre-fold of a non-power-of-two communicator pairs the ranks below 2*rem:
 * pair m = (2m, 2m+1) continues as newrank m, every rank r >= 2*rem as r - rem. */
static int newrank_of(int rank, int rem)
{
    return rank < 2 * rem ? rank / 2 : rank - rem;
}

/* real rank of newrank m after the pre-fold: the keeper of pair m is the even
 * rank 2m (reduce_intra_reduce_scatter_gather.c) or the odd rank 2m+1
 * (allreduce_intra_reduce_scatter_allgather.c, allreduce_intra_recursive_doubling.c) */
static int real_of(int m, int rem, int odd_keeps)
{
    return m < rem ? 2 * m + (odd_keeps ? 1 : 0) : m + rem;
}

/* ------------------------------------------------------------ short messages
 * MPICH switches algorithm on message size.  For these the device form keeps
 * the reference's association and operand order but not its rounds: ONE
 * exchange brings a rank every operand it needs, then the schedule's fold runs
 * on the device (tests/test_schedule_small_cpu.py pins the fold plans against
 * step-by-step simulations of the reference). */

/* This rank's vector `x` into slot `rank` of p staging slots, then an
 * allgather: slot q holds x_q on every rank. */
static int allgather_slots(const coll_t *f, const void *x, size_t bytes, char **scr)
{
    struct MPIX_Hip_comm_s *c = f->c;
    int p = c->size, q, nsend = 0, nrecv = 0;
    size_t slot = stage_stride(bytes);
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    char *own;
    hipError_t e;
    TRY(comm_scratch(c, (size_t) p * slot, scr, f->fc));
    own = *scr + (size_t) c->rank * slot;
    e = hipMemcpyAsync(own, x, bytes, hipMemcpyDeviceToDevice, f->s);
    if (e != hipSuccess)
        return hip_err(f->fc, e);
    for (q = 0; q < p; q++) {
        if (q == c->rank)
            continue;
        xfer_add(sends, &nsend, own, bytes, q);
        xfer_add(recvs, &nrecv, *scr + (size_t) q * slot, bytes, q);
    }
    return group_exchange(c, sends, nsend, recvs, nrecv, f->s);
}

/* The binomial tree to relrank 0 over p slots (reduce_intra_binomial.c:93-140:
 * relrank r folds in the accumulation of r|mask as the second operand), slot
 * r holding relrank r's vector; the result goes to `out`. */
static int binomial_fold(const coll_t *f, char *scr, size_t slot, void *out, long count)
{
    int p = f->c->size, q, mask;
    hipError_t e;
    if ((p & (p - 1)) == 0) {
        /* power of two: the binomial tree IS the pairwise tree ((x0+x1)+(x2+x3))+... */
        const void *ys[MAX_RANKS];
        for (q = 0; q < p; q++)
            ys[q] = scr + (size_t) q * slot;
        return fold_tree(f, ys, p, out, count);
    }
    for (mask = 1; mask < p; mask <<= 1)
        for (q = 0; q + mask < p; q += 2 * mask)
            TRY(fold_step(f, scr + (size_t) (q + mask) * slot, scr + (size_t) q * slot, count));
    e = hipMemcpyAsync(out, scr, (size_t) count * f->esz, hipMemcpyDeviceToDevice, f->s);
    return e == hipSuccess ? MPI_SUCCESS : hip_err(f->fc, e);
}

/* MPI_Allreduce, count*size <= 2048 or count < pof2: MPIR_Reduce takes the
 * binomial tree to root 0 (reduce.c:214-225, reduce_intra_binomial.c:93-140),
 * then MPIR_Bcast.  Here: an allgather of the p inputs into slots 0..p-1, then
 * every rank folds them in the binomial order itself, so all ranks hold root
 * 0's bytes. */
static int allreduce_short(const coll_t *f, const void *x, void *recvbuf, long count)
{
    size_t bytes = (size_t) count * f->esz;
    char *scr = NULL;
    TRY(allgather_slots(f, x, bytes, &scr));
    return binomial_fold(f, scr, stage_stride(bytes), recvbuf, count);
}

/* MPI_Allreduce, flat branch, recursive doubling
 * (allreduce_intra_recursive_doubling.c): even r < 2*rem sends to r+1, which
 * computes Y = x_{r} (+) x_{r-1}; then at mask 1, 2, 4, ... newrank n folds in
 * the partial of n ^ mask second, so n ends with the tree over z_j = Y_{n ^ j};
 * an excluded even rank receives the result of its odd neighbour.  Here: an
 * allgather of the p inputs, the rem pre-fold steps, one tree combine per rank. */
static int allreduce_recursive_doubling(const coll_t *f, const void *x, void *recvbuf, long count)
{
    int p = f->c->size, pof2 = pof2_of(p), rem = p - pof2, n = newrank_of(f->c->rank, rem), j, m;
    size_t bytes = (size_t) count * f->esz, slot = stage_stride(bytes);
    const void *ys[MAX_RANKS];
    char *scr = NULL;
    TRY(allgather_slots(f, x, bytes, &scr));
    for (m = 0; m < rem; m++)
        TRY(fold_step(f, scr + (size_t) (2 * m) * slot, scr + (size_t) (2 * m + 1) * slot, count));
    for (j = 0; j < pof2; j++)
        ys[j] = scr + (size_t) real_of(n ^ j, rem, 1) * slot;
    return fold_tree(f, ys, pof2, recvbuf, count);
}

/* MPI_Reduce_scatter(_block), total bytes < 524288: recursive halving
 * (reduce_scatter_block_intra_recursive_halving.c; reduce_scatter_intra_
 * recursive_halving.c is the same schedule with per-rank counts).  Block r is
 * finished by newrank n = r/2 (r < 2*rem) or r - rem, as
 *   Y_m = x_{2m+1} (+) x_{2m} for m < rem (pre-fold :163-195), else x_{m+rem};
 *   tree ((z0+z1)+(z2+z3))+... over z_k = Y_{n ^ bitrev(k)} (halving :197-283,
 *   mask = pof2/2 first, received data second).
 * Here: one all-to-all of blocks (every rank gets x_q's block r from each q),
 * the rem pre-fold steps, one tree combine into recvbuf. */
static int reduce_scatter_short(const coll_t *f, const char *src, void *recvbuf, const long *cnts,
                                const long *disps)
{
    struct MPIX_Hip_comm_s *c = f->c;
    int p = c->size, q, nsend = 0, nrecv = 0, pof2 = pof2_of(p), rem = p - pof2, bits = ilog2(pof2);
    int n = newrank_of(c->rank, rem), k, m;
    long rcount = cnts[c->rank];
    size_t esz = f->esz, nb = (size_t) rcount * esz, slot = stage_stride(nb);
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    const void *ys[MAX_RANKS];
    char *scr = NULL;
    hipError_t e;
    TRY(comm_scratch(c, (size_t) p * slot + 256, &scr, f->fc));
    /* own block into its slot: the pre-fold updates slots in place */
    if (nb) {
        e = hipMemcpyAsync(scr + (size_t) c->rank * slot, src + (size_t) disps[c->rank] * esz, nb,
                           hipMemcpyDeviceToDevice, f->s);
        if (e != hipSuccess)
            return hip_err(f->fc, e);
    }
    for (q = 0; q < p; q++) {
        if (q == c->rank)
            continue;
        xfer_add(sends, &nsend, src + (size_t) disps[q] * esz, (size_t) cnts[q] * esz, q);
        xfer_add(recvs, &nrecv, scr + (size_t) q * slot, nb, q);
    }
    TRY(group_exchange(c, sends, nsend, recvs, nrecv, f->s));
    if (!rcount)
        return MPI_SUCCESS;
    for (m = 0; m < rem; m++)
        TRY(fold_step(f, scr + (size_t) (2 * m) * slot, scr + (size_t) (2 * m + 1) * slot, rcount));
    for (k = 0; k < pof2; k++)
        ys[k] = scr + (size_t) real_of(n ^ bitrev(k, bits), rem, 1) * slot;
    return fold_tree(f, ys, pof2, recvbuf, rcount);
}

/* ------------------------------------------------------------ the call frame */
/* validation shared by the collectives (MPIR_ERRTEST_OP + check_dtype) */
static int coll_check(const char *fc, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op,
                      MPIX_Hip_comm comm, int *elem)
{
    unsigned kind = ((unsigned) op & 0xc0000000u) >> 30, mpikind = ((unsigned) op & 0x3c000000u) >> 26;
    int opidx = op & 0xf, rc;
    if (!comm) {
        MPIR_Err_set_detail("%s: null communicator", fc);
        return MPI_ERR_ARG;
    }
    if (count < 0) {
        MPIR_Err_set_detail("%s: negative count", fc);
        return MPI_ERR_COUNT;
    }
    if (op == MPI_OP_NULL || op == MPI_NO_OP || op == MPI_REPLACE || kind != 1 || mpikind != 6 ||
        opidx < 1 || opidx > 12) {
        MPIR_Err_set_detail("%s: builtin reduction MPI_Op required", fc);
        return MPI_ERR_OP;
    }
    if ((rc = MPIR_Op_check_dtype_table[opidx] (dt)) != MPI_SUCCESS)
        return rc;
    *elem = MPIR_Op_resolve_elem(opidx, dt);
    if (!*elem) {
        MPIR_Err_set_detail("MPI_Op operation not defined for this datatype");
        return MPI_ERR_OP;
    }
    if (count > 0 && sendbuf == recvbuf) {
        MPIR_Err_set_detail("%s: Buffers must not be aliased", fc);
        return MPI_ERR_BUFFER;
    }
    return MPI_SUCCESS;
}

/* Opens the call f (fc and c set by the entry point): validates, with
 * `recvbuf` the buffer that takes part in the alias check; then moves to the
 * communicator's device and picks the stream.  Returns 0 when the entry point
 * is to return *rc at once (an error, already final, or nothing to do),
 * else 1: the schedule runs and its result goes through coll_end(). */
static int coll_begin(coll_t *f, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op,
                      void *hip_stream, int *rc)
{
    *rc = coll_check(f->fc, sendbuf, recvbuf, count, dt, op, f->c, &f->elem);
    if (*rc)
        *rc = MPIR_Err_return(f->fc, *rc);
    if (*rc || count == 0)
        return 0;
    f->switched = hipGetDevice(&f->saved_device) == hipSuccess && f->saved_device != f->c->device;
    if (f->switched)
        (void) hipSetDevice(f->c->device);
    f->user_stream = hip_stream != NULL;
    f->s = hip_stream ? (hipStream_t) hip_stream : f->c->stream;
    f->opidx = op & 0xf;
    f->esz = MPIR_Hip_elem_size(f->elem);
    return 1;
}

/* Closes the call with the schedule's result: a successful call on the
 * communicator's own stream is synchronised (a caller's stream never is),
 * the caller's device is put back if it was left. */
static int coll_end(coll_t *f, int rc)
{
    if (rc == MPI_SUCCESS && !f->user_stream) {
        hipError_t e = hipStreamSynchronize(f->s);
        if (e != hipSuccess) {
            MPIR_Err_set_detail("hipStreamSynchronize(s): %s", hipGetErrorString(e));
            rc = MPI_ERR_OTHER;
        }
    }
    if (f->switched)
        (void) hipSetDevice(f->saved_device);
    return rc ? MPIR_Err_return(f->fc, rc) : MPI_SUCCESS;
}

static int want_rccl(const coll_t *f, int algorithm, ncclDataType_t * t, ncclRedOp_t * o)
{
    const char *v;
    if (f->c->kind != COMM_RCCL || algorithm == MPIX_HIP_ALG_REFERENCE_ORDER)
        return 0;
    if (algorithm == MPIX_HIP_ALG_AUTO && (v = getenv("MPIR_CVAR_DEVICE_COLL_ALGORITHM")) &&
        !strcmp(v, "reference"))
        return 0;
    switch (f->elem) {
    case MPIR_HIP_I8: *t = ncclInt8; break;
    case MPIR_HIP_U8: *t = ncclUint8; break;
    case MPIR_HIP_I32: *t = ncclInt32; break;
    case MPIR_HIP_U32: *t = ncclUint32; break;
    case MPIR_HIP_I64: *t = ncclInt64; break;
    case MPIR_HIP_U64: *t = ncclUint64; break;
    case MPIR_HIP_F16: *t = ncclFloat16; break;
    case MPIR_HIP_F32: *t = ncclFloat32; break;
    case MPIR_HIP_F64: *t = ncclFloat64; break;
    default: return 0;
    }
    switch (f->opidx) {
    case MPIR_HIP_OP_SUM: *o = ncclSum; break;
    case MPIR_HIP_OP_PROD: *o = ncclProd; break;
    case MPIR_HIP_OP_MAX: *o = ncclMax; break;
    case MPIR_HIP_OP_MIN: *o = ncclMin; break;
    default: return 0;
    }
    return 1;
}

/* ------------------------------------------------------------ reduce-scatter / gather
 * The layout of reduce_intra_reduce_scatter_gather.c and allreduce_intra_
 * reduce_scatter_allgather.c for one rank: `count` elements in pof2 blocks
 * (the first count % pof2 one element longer), newrank n owning block
 * bitrev(n); the staging for the blocks a rank receives. */
typedef struct {
    int pof2, rem, bits;
    int odd_keeps;              /* the pre-fold's keeper of pair m: 2m+1, else 2m (real_of) */
    int newrank;                /* this rank's; -1: excluded by the pre-fold */
    long cnts[MAX_RANKS], disps[MAX_RANKS];     /* of block b, in elements */
    size_t esz;
    size_t blk;                 /* stride of the staging slots: stage_stride of the largest block, cnts[0] */
    size_t tmp_off;             /* the pre-fold partner's vector in scratch, behind the pof2-1 slots */
    int nchunk;                 /* the all-to-all's pipeline (pipe_chunks): every rank derives */
    size_t chunk;               /* the same chunk count from the largest block */
} rsg_t;

static void rsg_layout(rsg_t *g, int p, int rank, long count, size_t esz, int odd_keeps)
{
    int i;
    g->pof2 = pof2_of(p);
    g->rem = p - g->pof2;
    g->bits = ilog2(g->pof2);
    g->odd_keeps = odd_keeps;
    g->newrank = rank < 2 * g->rem && (rank % 2) != (odd_keeps ? 1 : 0) ? -1 : newrank_of(rank, g->rem);
    for (i = 0; i < g->pof2; i++)
        g->cnts[i] = count / g->pof2 + (i < count % g->pof2 ? 1 : 0);
    g->disps[0] = 0;
    for (i = 1; i < g->pof2; i++)
        g->disps[i] = g->disps[i - 1] + g->cnts[i - 1];
    g->esz = esz;
    g->blk = stage_stride((size_t) g->cnts[0] * esz);
    g->tmp_off = (size_t) (g->pof2 > 1 ? g->pof2 - 1 : 1) * g->blk;
    g->chunk = 0;
    g->nchunk = g->pof2 > 1 ? pipe_chunks((size_t) g->cnts[0] * esz, &g->chunk) : 1;
}

/* block b of a vector laid out by g: its byte offset and length */
static size_t rsg_off(const rsg_t *g, int b)
{
    return (size_t) g->disps[b] * g->esz;
}

static size_t rsg_len(const rsg_t *g, int b)
{
    return (size_t) g->cnts[b] * g->esz;
}

/* what rsg_phase needs in `scr` for a vector of `bytes`: the slots, then the
 * pre-fold partner's vector */
static size_t rsg_scratch_bytes(const rsg_t *g, size_t bytes)
{
    return g->tmp_off + bytes + 256;
}

/* The reduce-scatter phase of reduce_intra_reduce_scatter_gather.c on `work`
 * (count elements, this rank's contribution): the non-power-of-two pre-fold
 * (:138-170: odd r < 2*rem sends everything to r-1, which computes x_r (+) x_{r+1}),
 * then the recursive halving (:186-249) as ONE all-to-all of blocks and ONE
 * fused tree combine: newrank n owns block bitrev(n), reduced as
 * ((y0+y1)+(y2+y3))+... with y_j = the block from newrank n ^ j.
 * `scr` holds rsg_scratch_bytes(): (pof2-1) slots of stage_stride(cnts[0]
 * elements), then `count` elements for the pre-fold partner's vector. */
static int rsg_phase(const coll_t *f, const rsg_t *g, char *work, long count, char *scr)
{
    struct MPIX_Hip_comm_s *c = f->c;
    hipStream_t s = f->s;
    int pof2 = g->pof2, rem = g->rem, n = g->newrank, mb = n >= 0 ? bitrev(n, g->bits) : 0;
    int nsend = 0, nrecv = 0, i, m;
    size_t bytes = (size_t) count * f->esz;
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    const void *ys[MAX_RANKS];
    fold_ctx_t fo = { ys, pof2, MPIR_HIP_ORDER_TREE, NULL, 0 };   /* (an excluded rank folds nothing) */
    /* pre-fold; every rank takes part in the transfer group (empty for ranks >= 2*rem):
     * of the pair (2m, 2m+1) one sends its vector, the keeper receives it and
     * folds it in as the second operand. */
    if (rem > 0) {
        const int paired = c->rank < 2 * rem, keeper = paired && g->newrank >= 0;
        char *tmp = scr + g->tmp_off;
        xfer_t x = { keeper ? tmp : work, bytes, c->rank ^ 1 };
        TRY(group_exchange(c, &x, paired && !keeper, &x, keeper, s));
        if (keeper)
            TRY(fold_step(f, tmp, work, count));
    }

    /* all-to-all of blocks: the owner receives y_j into scratch slot j-1;
     * chunked, with the tree folded chunk by chunk behind it, when the blocks
     * are large (g->nchunk).  A rank the pre-fold excluded matches the group
     * calls of the others with no transfers and folds nothing. */
    if (pof2 == 1)
        return MPI_SUCCESS;
    if (g->nchunk > 1)
        TRY(pipe_init(c));
    if (n >= 0) {
        for (m = 0; m < pof2; m++) {
            int real = real_of(m, rem, g->odd_keeps), b = bitrev(m, g->bits);
            if (m == n)
                continue;
            xfer_add(sends, &nsend, work + rsg_off(g, b), rsg_len(g, b), real);
            xfer_add(recvs, &nrecv, scr + (size_t) ((n ^ m) - 1) * g->blk, rsg_len(g, mb), real);
        }
        ys[0] = fo.out = work + rsg_off(g, mb);
        for (i = 1; i < pof2; i++)
            ys[i] = scr + (size_t) (i - 1) * g->blk;
        fo.out_bytes = rsg_len(g, mb);
    }
    if (g->nchunk > 1)
        return exchange_fold_pipelined(f, sends, nsend, recvs, nrecv, g->nchunk, g->chunk, &fo);
    TRY(group_exchange(c, sends, nsend, recvs, nrecv, s));
    return fo.out_bytes ? fold_tree(f, ys, pof2, fo.out, g->cnts[mb]) : MPI_SUCCESS;
}

/* one receive per reduced block of `buf`, from the rank that owns it */
static void rsg_recv_blocks(const rsg_t *g, char *buf, int rank, xfer_t *recvs, int *nrecv)
{
    int i;
    for (i = 0; i < g->pof2; i++) {
        int real = real_of(i, g->rem, g->odd_keeps), b = bitrev(i, g->bits);
        if (real != rank)
            xfer_add(recvs, nrecv, buf + rsg_off(g, b), rsg_len(g, b), real);
    }
}

/* The allgather of the reduced blocks of `buf` to every rank (the gather +
 * MPIR_Bcast of allreduce_intra_smp.c move data only); chunk k of the owners'
 * blocks leaves once its fold is done. */
static int rsg_allgather(const coll_t *f, const rsg_t *g, char *buf)
{
    struct MPIX_Hip_comm_s *c = f->c;
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    int nsend = 0, nrecv = 0, q;
    if (g->newrank >= 0) {
        int mb = bitrev(g->newrank, g->bits);
        for (q = 0; q < c->size; q++)
            if (q != c->rank)
                xfer_add(sends, &nsend, buf + rsg_off(g, mb), rsg_len(g, mb), q);
    }
    rsg_recv_blocks(g, buf, c->rank, recvs, &nrecv);
    if (g->nchunk > 1)
        return exchange_after_folds(f, sends, nsend, recvs, nrecv, g->nchunk, g->chunk);
    return group_exchange(c, sends, nsend, recvs, nrecv, f->s);
}

/* The gather of the owners' blocks to `root`, into its recvbuf
 * (reduce_intra_reduce_scatter_gather.c:256-410). */
static int rsg_gather(const coll_t *f, const rsg_t *g, char *work, char *recvbuf, int root)
{
    struct MPIX_Hip_comm_s *c = f->c;
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    int nsend = 0, nrecv = 0;
    if (c->rank == root)
        rsg_recv_blocks(g, recvbuf, root, recvs, &nrecv);
    else if (g->newrank >= 0) {
        int mb = bitrev(g->newrank, g->bits);
        xfer_add(sends, &nsend, work + rsg_off(g, mb), rsg_len(g, mb), root);
    }
    return group_exchange(c, sends, nsend, recvs, nrecv, f->s);
}

/* ------------------------------------------------------------ Allreduce */
static int allreduce_schedule(const coll_t *f, const void *sendbuf, void *recvbuf, int count, int algorithm)
{
    struct MPIX_Hip_comm_s *c = f->c;
    const void *own = sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf;
    size_t bytes = (size_t) count * f->esz;
    int p = c->size, pof2 = pof2_of(p), flat;
    ncclDataType_t nt;
    ncclRedOp_t no;
    rsg_t g;
    char *scr = NULL;

    if (want_rccl(f, algorithm, &nt, &no)) {
        ncclResult_t r = rccl.AllReduce(own, recvbuf, (size_t) count, nt, no, c->nccl, f->s);
        return r == ncclSuccess ? MPI_SUCCESS : rccl_err("ncclAllReduce", r);
    }

    /* ---- reference order: MPIR_Allreduce_intra_auto (allreduce.c:145-217).  On one
     * node the SMP branch runs (allreduce_intra_smp.c: MPIR_Reduce with
     * MPIR_Reduce_intra_auto's choice, then MPIR_Bcast); with the SMP CVARs off
     * (or a comm with one rank per node) the flat branch runs */
    if (p == 1) {
        if (sendbuf != MPI_IN_PLACE)
            HIPTRY(hipMemcpyAsync(recvbuf, sendbuf, bytes, hipMemcpyDeviceToDevice, f->s));
        return MPI_SUCCESS;
    }
    flat = allreduce_flat_choice(bytes, count, pof2);
    if (flat == FLAT_RECURSIVE_DOUBLING)
        return allreduce_recursive_doubling(f, own, recvbuf, count);
    if (!flat && (bytes <= REDUCE_SHORT_MSG_SIZE || count < pof2))
        return allreduce_short(f, own, recvbuf, count);
    /* long: the reduce-scatter of reduce_intra_reduce_scatter_gather.c (SMP) or
     * allreduce_intra_reduce_scatter_allgather.c (flat, Rabenseifner) on recvbuf */
    if (sendbuf != MPI_IN_PLACE)
        HIPTRY(hipMemcpyAsync(recvbuf, sendbuf, bytes, hipMemcpyDeviceToDevice, f->s));
    rsg_layout(&g, p, c->rank, count, f->esz, flat == FLAT_RABENSEIFNER);
    TRY(comm_scratch(c, rsg_scratch_bytes(&g, bytes), &scr, f->fc));
    TRY(rsg_phase(f, &g, recvbuf, count, scr));
    return rsg_allgather(f, &g, recvbuf);
}

int MPIX_Allreduce_hip(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                       MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Allreduce_hip", .c = comm };
    int rc;
    if (!coll_begin(&f, sendbuf, recvbuf, count, datatype, op, hip_stream, &rc))
        return rc;
    return coll_end(&f, allreduce_schedule(&f, sendbuf, recvbuf, count, algorithm));
}

/* ------------------------------------------------------------ Reduce
 * MPI_Reduce on one node: MPIR_Reduce_intra_smp (reduce_intra_smp.c) reduces
 * to the root over node_comm with MPIR_Reduce_intra_auto (reduce.c:170-225):
 *   count*size <= 2048 or count < pof2: binomial tree rooted at `root`
 *       (reduce_intra_binomial.c:93-140, commutative: relrank = rank - root);
 *       here a gather to the root, which folds the relranks in binomial order;
 *   else reduce_intra_reduce_scatter_gather.c: the reduce-scatter phase of the
 *       Allreduce (block values do not depend on the root), then the owners'
 *       blocks are gathered to the root. */
static int reduce_schedule(const coll_t *f, const void *sendbuf, void *recvbuf, int count, int root, int algorithm)
{
    struct MPIX_Hip_comm_s *c = f->c;
    const void *own = sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf;
    size_t bytes = (size_t) count * f->esz, slot;
    int p = c->size, pof2 = pof2_of(p), isroot = c->rank == root, i;
    hipStream_t s = f->s;
    ncclDataType_t nt;
    ncclRedOp_t no;
    rsg_t g;
    char *scr = NULL, *work;

    if (want_rccl(f, algorithm, &nt, &no)) {
        ncclResult_t r = rccl.Reduce(own, isroot ? recvbuf : NULL, (size_t) count, nt, no, root, c->nccl, s);
        return r == ncclSuccess ? MPI_SUCCESS : rccl_err("ncclReduce", r);
    }
    if (p == 1) {
        if (sendbuf != MPI_IN_PLACE)
            HIPTRY(hipMemcpyAsync(recvbuf, sendbuf, bytes, hipMemcpyDeviceToDevice, s));
        return MPI_SUCCESS;
    }
    if (bytes <= REDUCE_SHORT_MSG_SIZE || count < pof2) {
        /* binomial: slot rel holds x_{(rel + root) % p}; the tree folds relranks */
        xfer_t recvs[MAX_XFER];
        int nrecv = 0;
        slot = stage_stride(bytes);
        if (!isroot) {
            xfer_t x = { (void *) own, bytes, root };
            return group_exchange(c, &x, 1, NULL, 0, s);
        }
        TRY(comm_scratch(c, (size_t) p * slot, &scr, f->fc));
        HIPTRY(hipMemcpyAsync(scr, own, bytes, hipMemcpyDeviceToDevice, s));
        for (i = 1; i < p; i++)
            xfer_add(recvs, &nrecv, scr + (size_t) i * slot, bytes, (i + root) % p);
        TRY(group_exchange(c, NULL, 0, recvs, nrecv, s));
        return binomial_fold(f, scr, slot, recvbuf, count);
    }

    /* long: reduce-scatter on `work` (recvbuf at the root, scratch elsewhere) */
    rsg_layout(&g, p, c->rank, count, f->esz, 0);
    slot = (rsg_scratch_bytes(&g, bytes) + 255) & ~(size_t) 255;
    TRY(comm_scratch(c, slot + (isroot ? 0 : bytes), &scr, f->fc));
    work = isroot ? (char *) recvbuf : scr + slot;
    if (work != own)
        HIPTRY(hipMemcpyAsync(work, own, bytes, hipMemcpyDeviceToDevice, s));
    TRY(rsg_phase(f, &g, work, count, scr));
    if (g.nchunk > 1)
        HIPTRY(hipStreamWaitEvent(s, c->fev[g.nchunk - 1], 0));     /* every fold done */
    return rsg_gather(f, &g, work, recvbuf, root);
}

int MPIX_Reduce_hip(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op, int root,
                    MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Reduce_hip", .c = comm };
    int rc, isroot;

    if (comm && (root < 0 || root >= comm->size)) {
        MPIR_Err_set_detail("%s: Invalid root (value given was %d)", f.fc, root);
        return MPIR_Err_return(f.fc, MPI_ERR_ROOT);
    }
    isroot = comm && comm->rank == root;
    if (comm && !isroot && sendbuf == MPI_IN_PLACE && count > 0) {
        MPIR_Err_set_detail("%s: MPI_IN_PLACE is only valid at the root", f.fc);
        return MPIR_Err_return(f.fc, MPI_ERR_BUFFER);
    }
    /* recvbuf is significant at the root only (the alias check with it too) */
    if (!coll_begin(&f, sendbuf, isroot ? recvbuf : NULL, count, datatype, op, hip_stream, &rc))
        return rc;
    return coll_end(&f, reduce_schedule(&f, sendbuf, recvbuf, count, root, algorithm));
}

/* ------------------------------------------------------------ Reduce_scatter(_block)
 * One implementation for both: counts[q] elements of the result go to rank q.
 *   RCCL:  ncclReduceScatter (regular counts only).
 *   reference order (MPIR_Reduce_scatter(_block)_intra_auto, builtin ops are
 *   commutative): recursive halving below 524288 total bytes, else pairwise
 *   (reduce_scatter_block_intra_pairwise.c:97-134 /
 *   reduce_scatter_intra_pairwise.c): block r = ((x_r + x_{r-1}) + x_{r-2}) + ...
 *   as one all-to-all + one CHAIN combine. */
static int reduce_scatter_schedule(const coll_t *f, const void *sendbuf, void *recvbuf, const long *cnts,
                                   const long *disps, int regular, int algorithm)
{
    struct MPIX_Hip_comm_s *c = f->c;
    int p = c->size, i, nsend = 0, nrecv = 0, nchunk;
    long total = disps[p - 1] + cnts[p - 1];
    size_t esz = f->esz, nb = (size_t) cnts[c->rank] * esz, slot, maxb = 0, chunk = 0;
    hipStream_t s = f->s;
    ncclDataType_t nt;
    ncclRedOp_t no;
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    const void *ys[MAX_RANKS];
    const char *src = sendbuf == MPI_IN_PLACE ? (const char *) recvbuf : (const char *) sendbuf;
    char *scr = NULL;

    if (regular && want_rccl(f, algorithm, &nt, &no)) {
        /* NCCL's in-place form is recvbuff == sendbuff + rank * recvcount */
        void *dst = sendbuf == MPI_IN_PLACE ? (char *) recvbuf + (size_t) c->rank * nb : recvbuf;
        ncclResult_t r = rccl.ReduceScatter(src, dst, (size_t) cnts[0], nt, no, c->nccl, s);
        if (r != ncclSuccess)
            return rccl_err("ncclReduceScatter", r);
        if (sendbuf == MPI_IN_PLACE && c->rank)
            HIPTRY(hipMemcpyAsync(recvbuf, dst, nb, hipMemcpyDeviceToDevice, s));
        return MPI_SUCCESS;
    }

    if (p > 1 && (size_t) total * esz < RSB_COMMUTATIVE_LONG_MSG_SIZE)
        return reduce_scatter_short(f, src, recvbuf, cnts, disps);
    /* long: pairwise.  y_i = block r from rank r - i into scratch slot i-1; in
     * place, the own block is staged too when it overlaps the output. */
    slot = stage_stride(nb);
    TRY(comm_scratch(c, (size_t) p * slot + 256, &scr, f->fc));
    ys[0] = src + (size_t) disps[c->rank] * esz;
    if (sendbuf == MPI_IN_PLACE && disps[c->rank] > 0 && disps[c->rank] < cnts[c->rank]) {
        HIPTRY(hipMemcpyAsync(scr + (size_t) (p - 1) * slot, ys[0], nb, hipMemcpyDeviceToDevice, s));
        ys[0] = scr + (size_t) (p - 1) * slot;
    }
    for (i = 1; i < p; i++) {
        int dst = (c->rank + i) % p, from = (c->rank - i + p) % p;
        xfer_add(sends, &nsend, src + (size_t) disps[dst] * esz, (size_t) cnts[dst] * esz, dst);
        xfer_add(recvs, &nrecv, scr + (size_t) (i - 1) * slot, nb, from);
        ys[i] = scr + (size_t) (i - 1) * slot;
    }
    /* large blocks: the exchange in chunks, chunk k's chain folded while
     * k+1 moves (pipe_chunks; every rank takes the chunk count from the
     * largest block) */
    for (i = 0; i < p; i++)
        if ((size_t) cnts[i] * esz > maxb)
            maxb = (size_t) cnts[i] * esz;
    nchunk = p > 1 ? pipe_chunks(maxb, &chunk) : 1;
    if (nchunk > 1) {
        fold_ctx_t fo = { ys, p, MPIR_HIP_ORDER_CHAIN, recvbuf, nb };
        TRY(pipe_init(c));
        TRY(exchange_fold_pipelined(f, sends, nsend, recvs, nrecv, nchunk, chunk, &fo));
        HIPTRY(hipStreamWaitEvent(s, c->fev[nchunk - 1], 0));
        return MPI_SUCCESS;
    }
    if (p > 1)
        TRY(group_exchange(c, sends, nsend, recvs, nrecv, s));
    return nb ? fold_combine(f, ys, p, recvbuf, cnts[c->rank], MPIR_HIP_ORDER_CHAIN, s) : MPI_SUCCESS;
}

/* f: fc and c set by the entry point */
static int reduce_scatter_common(coll_t *f, const void *sendbuf, void *recvbuf, const int *counts,
                                 MPI_Datatype datatype, MPI_Op op, int algorithm, void *hip_stream)
{
    int rc, i, regular = 1;
    long cnts[MAX_RANKS] = {0}, disps[MAX_RANKS] = {0}, total = 0;

    if (!f->c) {
        MPIR_Err_set_detail("%s: null communicator", f->fc);
        return MPIR_Err_return(f->fc, MPI_ERR_ARG);
    }
    for (i = 0; i < f->c->size; i++) {
        if (counts[i] < 0) {
            MPIR_Err_set_detail("%s: negative count", f->fc);
            return MPIR_Err_return(f->fc, MPI_ERR_COUNT);
        }
        cnts[i] = counts[i];
        disps[i] = total;
        total += counts[i];
        regular &= counts[i] == counts[0];
    }
    /* op / type validation; the alias check applies when any data moves */
    if (!coll_begin(f, sendbuf, recvbuf, total > 0, datatype, op, hip_stream, &rc))
        return rc;
    return coll_end(f, reduce_scatter_schedule(f, sendbuf, recvbuf, cnts, disps, regular, algorithm));
}

int MPIX_Reduce_scatter_block_hip(const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype datatype,
                                  MPI_Op op, MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Reduce_scatter_block_hip", .c = comm };
    int counts[MAX_RANKS] = { recvcount }, i;
    for (i = 0; comm && recvcount >= 0 && i < comm->size; i++)
        counts[i] = recvcount;
    return reduce_scatter_common(&f, sendbuf, recvbuf, counts, datatype, op, algorithm, hip_stream);
}

int MPIX_Reduce_scatter_hip(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype datatype,
                            MPI_Op op, MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Reduce_scatter_hip", .c = comm };
    if (!recvcounts) {
        MPIR_Err_set_detail("MPIX_Reduce_scatter_hip: recvcounts is NULL");
        return MPIR_Err_return(f.fc, MPI_ERR_ARG);
    }
    return reduce_scatter_common(&f, sendbuf, recvbuf, recvcounts, datatype, op, algorithm, hip_stream);
}

/* ------------------------------------------------------------ Scan / Exscan
 * On one node MPI_Scan is MPIR_Scan_intra_smp over node_comm, i.e. the
 * recursive doubling of scan_intra_recursive_doubling.c:94-147; MPI_Exscan is
 * exscan_intra_recursive_doubling.c:105-170.  At mask m rank r receives the
 * partial scan of r ^ m and, when r > r ^ m, folds it into recvbuf as the
 * second operand.  That partial scan is the full tree T(d) over
 * z_j = x_{d ^ j}, j < m, d = r ^ m (each rank folds its partner's partial
 * scan in second), so rank r's result is the chain
 *     x_r (+) T(r ^ m_1) (+) T(r ^ m_2) ...      (m_i: set bits of r, increasing)
 * and the exscan is the same chain without x_r (tests/test_schedule_small_cpu.py
 * pins the plan against the step-by-step schedules).  MI355X form: every rank
 * sends its vector to all higher ranks in ONE exchange (all xGMI links at
 * once instead of log2(p) dependent rounds), then folds the trees and the
 * chain on the device.  RCCL has no scan; MPIX_HIP_ALG_RCCL runs this too. */
static int scan_schedule(const coll_t *f, const void *sendbuf, void *recvbuf, int count, int exclusive)
{
    struct MPIX_Hip_comm_s *c = f->c;
    const void *own = sendbuf == MPI_IN_PLACE ? recvbuf : sendbuf;
    int p = c->size, r = c->rank, q, m, nsend = 0, nrecv = 0, nchain = 0, nparts = 0;
    size_t bytes = (size_t) count * f->esz, slot = stage_stride(bytes);
    xfer_t sends[MAX_XFER], recvs[MAX_XFER];
    const void *chain[MAX_RANKS], *ys[MAX_RANKS];
    char *scr = NULL;

    for (m = 1; m <= r; m <<= 1)
        nparts += (r & m) != 0;
    if (p > 1)
        TRY(comm_scratch(c, (size_t) (r + nparts + 1) * slot, &scr, f->fc));
    /* every rank's vector to all higher ranks; x_q lands in slot q */
    for (q = 0; q < p; q++) {
        if (q > r)
            xfer_add(sends, &nsend, own, bytes, q);
        else if (q < r)
            xfer_add(recvs, &nrecv, scr + (size_t) q * slot, bytes, q);
    }
    if (p > 1)
        TRY(group_exchange(c, sends, nsend, recvs, nrecv, f->s));
    if (!exclusive)
        chain[nchain++] = own;
    for (m = 1, q = 0; m <= r; m <<= 1) {
        int d, j;
        if (!(r & m))
            continue;
        d = r ^ m;
        if (m == 1) {
            chain[nchain++] = scr + (size_t) d * slot;
        } else {
            char *t = scr + (size_t) (r + q++) * slot;
            for (j = 0; j < m; j++)
                ys[j] = scr + (size_t) (d ^ j) * slot;
            TRY(fold_tree(f, ys, m, t, count));
            chain[nchain++] = t;
        }
    }
    return nchain ? fold_combine(f, chain, nchain, recvbuf, count, MPIR_HIP_ORDER_CHAIN, f->s) : MPI_SUCCESS;
}

/* f: fc and c set by the entry point */
static int scan_common(coll_t *f, const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                       void *hip_stream, int exclusive)
{
    int rc;
    /* the exscan's recvbuf is not significant at rank 0 */
    if (!coll_begin(f, sendbuf, (exclusive && f->c && f->c->rank == 0 && sendbuf != MPI_IN_PLACE) ? NULL : recvbuf,
                    count, datatype, op, hip_stream, &rc))
        return rc;
    return coll_end(f, scan_schedule(f, sendbuf, recvbuf, count, exclusive));
}

int MPIX_Scan_hip(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                  MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Scan_hip", .c = comm };
    (void) algorithm;
    return scan_common(&f, sendbuf, recvbuf, count, datatype, op, hip_stream, 0);
}

int MPIX_Exscan_hip(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op,
                    MPIX_Hip_comm comm, int algorithm, void *hip_stream)
{
    coll_t f = { .fc = "MPIX_Exscan_hip", .c = comm };
    (void) algorithm;
    return scan_common(&f, sendbuf, recvbuf, count, datatype, op, hip_stream, 1);
}
