/*
 * rccl_stub.c -- TEST ONLY: a stand-in librccl that records every call the
 * device collectives make (csrc/host/coll_hip.c loads it through
 * MPIR_TEST_RCCL_LIBRARY), one line per call into $RCCL_STUB_LOG.<rank>, so a
 * CPU test can check that the N ranks' RCCL call sequences match one another
 * (tests/test_rccl_sequence_cpu.py).  It moves no data and touches no buffer.
 *
 * Lines:  init <rank> <nranks>
 *         group_start | group_end
 *         send <bytes> <type> <peer> | recv <bytes> <type> <peer>
 *         allreduce <count> <type> <op> | reduce_scatter <recvcount> <type> <op>
 *         reduce <count> <type> <op> <root> | destroy
 *         note <text>                       (from the harness: memcpy, combine, ...)
 *         note + <call> <name>=<value> ...  (the buffers and the stream of the
 *                                           call on the line before, by the
 *                                           names tests/progs/coll_trace.c gives them)
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>

struct ncclComm {
    int rank, nranks;
};

static FILE *logf_;
static int depth;           /* group nesting, as NCCL allows it */

static void out(const char *fmt, ...)
{
    va_list ap;
    if (!logf_)
        return;
    va_start(ap, fmt);
    vfprintf(logf_, fmt, ap);
    va_end(ap);
    fputc('\n', logf_);
    fflush(logf_);
}

/* the harness's own events, in the same stream */
void rccl_stub_note(const char *text)
{
    out("note %s", text);
}

/* the buffers and the stream of the call just logged, by the harness's names
 * (its lookup functions, found the way its note() finds rccl_stub_note) */
typedef const char *(*name_fn)(const void *, char *, size_t);

static void detail(const char *call, const void *sb, const void *rb, int has_rb, hipStream_t s)
{
    static name_fn ptr_name, stream_name;
    char a[64], b[64], c[32];
    if (!ptr_name) {
        *(void **) (&ptr_name) = dlsym(RTLD_DEFAULT, "coll_trace_ptr_name");
        *(void **) (&stream_name) = dlsym(RTLD_DEFAULT, "coll_trace_stream_name");
    }
    if (!ptr_name || !stream_name)
        return;
    if (has_rb)
        out("note + %s sendbuf=%s recvbuf=%s stream=%s", call, ptr_name(sb, a, sizeof a), ptr_name(rb, b, sizeof b),
            stream_name((const void *) s, c, sizeof c));
    else
        out("note + %s buf=%s stream=%s", call, ptr_name(sb, a, sizeof a), stream_name((const void *) s, c, sizeof c));
}

ncclResult_t ncclGetUniqueId(ncclUniqueId *id)
{
    memset(id, 0, sizeof(*id));
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank)
{
    char path[4096];
    const char *base = getenv("RCCL_STUB_LOG");
    (void) id;
    if (!base || nranks < 1 || rank < 0 || rank >= nranks)
        return ncclInvalidArgument;
    snprintf(path, sizeof path, "%s.%d", base, rank);
    logf_ = fopen(path, "w");
    if (!logf_)
        return ncclSystemError;
    *comm = calloc(1, sizeof(struct ncclComm));
    (*comm)->rank = rank;
    (*comm)->nranks = nranks;
    out("init %d %d", rank, nranks);
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    out("destroy");
    /* the last line of a log: what the harness notes while the rest of the
     * communicator is torn down is not recorded */
    fclose(logf_);
    logf_ = NULL;
    free(comm);
    return ncclSuccess;
}

ncclResult_t ncclGroupStart(void)
{
    if (depth++ == 0)
        out("group_start");
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd(void)
{
    if (depth == 0)
        return ncclInvalidUsage;
    if (--depth == 0)
        out("group_end");
    return ncclSuccess;
}

ncclResult_t ncclSend(const void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t s)
{
    if (peer < 0 || peer >= comm->nranks || peer == comm->rank)
        return ncclInvalidArgument;
    out("send %zu %d %d", count, (int) t, peer);
    detail("send", buf, NULL, 0, s);
    return ncclSuccess;
}

ncclResult_t ncclRecv(void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t s)
{
    if (peer < 0 || peer >= comm->nranks || peer == comm->rank)
        return ncclInvalidArgument;
    out("recv %zu %d %d", count, (int) t, peer);
    detail("recv", buf, NULL, 0, s);
    return ncclSuccess;
}

ncclResult_t ncclAllReduce(const void *sb, void *rb, size_t count, ncclDataType_t t, ncclRedOp_t op,
                           ncclComm_t comm, hipStream_t s)
{
    (void) comm;
    out("allreduce %zu %d %d", count, (int) t, (int) op);
    detail("allreduce", sb, rb, 1, s);
    return ncclSuccess;
}

ncclResult_t ncclReduceScatter(const void *sb, void *rb, size_t recvcount, ncclDataType_t t, ncclRedOp_t op,
                               ncclComm_t comm, hipStream_t s)
{
    (void) comm;
    out("reduce_scatter %zu %d %d", recvcount, (int) t, (int) op);
    detail("reduce_scatter", sb, rb, 1, s);
    return ncclSuccess;
}

ncclResult_t ncclReduce(const void *sb, void *rb, size_t count, ncclDataType_t t, ncclRedOp_t op, int root,
                        ncclComm_t comm, hipStream_t s)
{
    if (root < 0 || root >= comm->nranks)
        return ncclInvalidArgument;
    out("reduce %zu %d %d %d", count, (int) t, (int) op, root);
    detail("reduce", sb, rb, 1, s);
    return ncclSuccess;
}

const char *ncclGetErrorString(ncclResult_t r)
{
    return r == ncclSuccess ? "success" : "stub error";
}
