/*
 * coll_trace.c -- TEST ONLY: one rank of the device collectives
 * (csrc/host/coll_hip.c, the product source, compiled unchanged) with the GPU
 * taken out: the HIP runtime calls coll_hip.c makes and the MPIR_Hip_* kernels
 * it launches are stand-ins defined here that move no data, and librccl is
 * tests/progs/rccl_stub.c (MPIR_TEST_RCCL_LIBRARY), which records every RCCL
 * call.  Device buffers are address ranges reserved with PROT_NONE: coll_hip.c
 * only passes them on, so configs 4 and 5 run at their full sizes in no memory.
 *
 *   coll_trace <rank> <size>   < plan
 * plan lines:  allreduce <count> <type> <op> <alg>
 *              reduce_scatter_block <recvcount> <type> <op> <alg>
 *              reduce_scatter <c0,c1,...> <type> <op> <alg>      (one count per rank)
 *              reduce <count> <type> <op> <alg> <root>
 *              scan <count> <type> <op> | exscan <count> <type> <op>
 *   type: f32 f16 f64 i32    op: sum max min    alg: auto ref rccl
 *              device <d>      (the caller's current device from here on; the
 *                               communicator was created on device 0)
 *   any line may end in `inplace` (sendbuf = MPI_IN_PLACE; for reduce at the
 *   root only) and / or `ustream` (a non-null hip_stream).
 * tests/test_rccl_sequence_cpu.py runs N of these and matches their logs.
 *
 * The log names what coll_hip.c passes on instead of printing addresses, so it
 * is the same in every run: a pointer is <base>+<byte offset> with base `send`
 * / `recv` (the current plan line's two buffers) or `scratch<k>` (the k-th
 * hipMalloc), `null`, or `?` (inside no reservation: the run fails); streams
 * are s<k> in creation order or `user`, events e<k>.  The detail of a call
 * that had a line before (memcpy, reduce_local, combine; in the stub send,
 * recv and the collectives) follows that line as `note + ...`.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <hip/hip_runtime_api.h>

#include "mpi_reduce_local.h"
#include "mpir_hip_reduce.h"
#include "mpix_hip_coll.h"
#include "mpir_op_types.h"

static void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void note(const char *fmt, ...)
{
    static void (*fn)(const char *);
    char buf[2048];
    va_list ap;
    if (!fn)
        *(void **) (&fn) = dlsym(RTLD_DEFAULT, "rccl_stub_note");
    if (!fn)
        return;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fn(buf);
}

/* ---- a reserved, never-touched address range stands in for device memory;
 * a guard page behind it keeps two reservations from touching, so that a
 * pointer one past the end of one is not the start of the next */
#define GUARD 4096
static void *reserve(size_t bytes)
{
    void *p = mmap(NULL, bytes + GUARD, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    return p == MAP_FAILED ? NULL : p;
}

static void release(void *p, size_t bytes)
{
    if (p)
        munmap(p, bytes + GUARD);
}

/* ---- names */
#define MAX_SCRATCH 256
#define USER_STREAM ((hipStream_t) (uintptr_t) 0x75e0)
static struct { const char *base; size_t bytes; } cur_send, cur_recv, scratch[MAX_SCRATCH];
static int nscratch, nstream, nevent, unknown;

static int within(const void *p, const char *base, size_t bytes)
{
    return base && (const char *) p >= base && (const char *) p <= base + bytes;
}

/* both are found by the stub with dlsym, as note() finds the stub */
const char *coll_trace_ptr_name(const void *p, char *buf, size_t len)
{
    int k;
    if (!p)
        return "null";
    if (within(p, cur_send.base, cur_send.bytes))
        snprintf(buf, len, "send+%zu", (size_t) ((const char *) p - cur_send.base));
    else if (within(p, cur_recv.base, cur_recv.bytes))
        snprintf(buf, len, "recv+%zu", (size_t) ((const char *) p - cur_recv.base));
    else {
        for (k = nscratch - 1; k >= 0 && !within(p, scratch[k].base, scratch[k].bytes); k--)
            ;
        if (k < 0) {
            unknown++;
            return "?";
        }
        snprintf(buf, len, "scratch%d+%zu", k, (size_t) ((const char *) p - scratch[k].base));
    }
    return buf;
}

#define STREAM0 0x51000u
#define EVENT0 0xe0000u
const char *coll_trace_stream_name(const void *s, char *buf, size_t len)
{
    uintptr_t v = (uintptr_t) s;
    if (s == (const void *) USER_STREAM)
        return "user";
    if (v < STREAM0 || v >= STREAM0 + (uintptr_t) nstream) {
        unknown++;
        return s ? "?" : "null";
    }
    snprintf(buf, len, "s%d", (int) (v - STREAM0));
    return buf;
}

static const char *event_name(hipEvent_t e, char *buf, size_t len)
{
    uintptr_t v = (uintptr_t) e;
    if (v < EVENT0 || v >= EVENT0 + (uintptr_t) nevent) {
        unknown++;
        return "?";
    }
    snprintf(buf, len, "e%d", (int) (v - EVENT0));
    return buf;
}

#define P(p, b) coll_trace_ptr_name(p, b, sizeof b)
#define S(s, b) coll_trace_stream_name((const void *) (s), b, sizeof b)
#define E(e, b) event_name(e, b, sizeof b)

/* ---- the HIP runtime calls of coll_hip.c */
static int cur_device;      /* plan line `device <d>`: the caller's current device */
hipError_t hipGetDevice(int *d) { *d = cur_device; return hipSuccess; }
hipError_t hipSetDevice(int d) { note("set_device %d", d); cur_device = d; return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t *s)
{
    char b[32];
    *s = (hipStream_t) (uintptr_t) (STREAM0 + (unsigned) nstream++);
    note("stream_create %s", S(*s, b));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { char b[32]; note("stream_destroy %s", S(s, b)); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { char b[32]; note("stream_sync %s", S(s, b)); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { note("device_sync"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int f)
{
    char b[32], c[32];
    note("stream_wait %s %s %u", S(s, b), E(e, c), f);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned f)
{
    char b[32];
    *e = (hipEvent_t) (uintptr_t) (EVENT0 + (unsigned) nevent++);
    note("event_create %s %u", E(*e, b), f);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    char b[32], c[32];
    note("event_record %s %s", E(e, b), S(s, c));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { char b[32]; note("event_destroy %s", E(e, b)); return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { (void) e; return "stand-in"; }
hipError_t hipMalloc(void **p, size_t bytes)
{
    *p = nscratch < MAX_SCRATCH ? reserve(bytes) : NULL;
    note("malloc %zu", bytes);
    if (!*p)
        return hipErrorOutOfMemory;
    scratch[nscratch].base = *p;
    scratch[nscratch].bytes = bytes;
    note("+ malloc scratch%d", nscratch++);
    return hipSuccess;
}
hipError_t hipFree(void *p)     /* (the reservation and its name are left: tiny, short-lived) */
{
    char b[64];
    note("free %s", P(p, b));
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t s)
{
    char b[64], c[64], d[32];
    note("memcpy %zu", bytes);
    note("+ memcpy dst=%s src=%s kind=%d stream=%s", P(dst, b), P(src, c), (int) k, S(s, d));
    return hipSuccess;
}

/* ---- the shim's kernels (mpir_hip_reduce.h) */
static const size_t elem_size[MPIR_HIP_NELEMS] = {
    0, 1, 1, 2, 2, 4, 4, 8, 8, 2, 4, 8, 8, 16, 8, 8, 16, 8, 16, 16, 32, 32,
};
size_t MPIR_Hip_elem_size(int elem) { return elem > 0 && elem < MPIR_HIP_NELEMS ? elem_size[elem] : 0; }
int MPIR_Hip_has_kernel(int op, int elem) { (void) op; return elem > 0 && elem < MPIR_HIP_NELEMS; }
const char *MPIR_Hip_error_string(void) { return ""; }
int MPIR_Hip_is_device_ptr(const void *p) { (void) p; return 1; }
int MPIR_Hip_combine_set_flags(int flags)
{
    static int cur;
    const int prev = cur;
    cur = flags;
    note("set_flags %d", flags);
    return prev;
}
int MPIR_Hip_memcpy(void *d, const void *s, size_t n) { (void) d; (void) s; (void) n; return MPIR_HIP_OK; }
int MPIR_Hip_reduce(const void *in, void *io, uint64_t count, int op, int elem, void *s, int sync)
{
    char b[64], c[64], d[32];
    note("reduce_local %llu %d %d", (unsigned long long) count, op, elem);
    note("+ reduce_local in=%s io=%s stream=%s sync=%d", P(in, b), P(io, c), S(s, d), sync);
    return MPIR_HIP_OK;
}
int MPIR_Hip_combine(const void *const *ins, int n, void *out, uint64_t count, int op, int elem, int order, void *s,
                     int sync)
{
    char text[1800], b[64], d[32];
    int i, len;
    note("combine %d %llu %d %d %s", n, (unsigned long long) count, op, elem,
         order == MPIR_HIP_ORDER_TREE ? "tree" : "chain");
    len = snprintf(text, sizeof text, "+ combine out=%s order=%d stream=%s sync=%d in=", P(out, b), order, S(s, d), sync);
    for (i = 0; i < n && len < (int) sizeof text - 80; i++)
        len += snprintf(text + len, sizeof text - (size_t) len, "%s%s", i ? "," : "", P(ins[i], b));
    note("%s", text);
    return MPIR_HIP_OK;
}

static int type_of(const char *t)
{
    if (!strcmp(t, "f32")) return MPI_FLOAT;
    if (!strcmp(t, "f16")) return MPIX_C_FLOAT16;
    if (!strcmp(t, "f64")) return MPI_DOUBLE;
    if (!strcmp(t, "i32")) return MPI_INT;
    return MPI_DATATYPE_NULL;
}

static int op_of(const char *o)
{
    if (!strcmp(o, "sum")) return MPI_SUM;
    if (!strcmp(o, "max")) return MPI_MAX;
    if (!strcmp(o, "min")) return MPI_MIN;
    return MPI_OP_NULL;
}

static int alg_of(const char *a)
{
    if (!strcmp(a, "ref")) return MPIX_HIP_ALG_REFERENCE_ORDER;
    if (!strcmp(a, "rccl")) return MPIX_HIP_ALG_RCCL;
    return MPIX_HIP_ALG_AUTO;
}

int main(int argc, char **argv)
{
    char id[MPIX_HIP_UNIQUE_ID_BYTES], line[1024];
    MPIX_Hip_comm comm = NULL;
    int rank, size, rc, n = 0;
    if (argc != 3)
        return 2;
    rank = atoi(argv[1]);
    size = atoi(argv[2]);
    MPIX_Reduce_local_set_errhandler(MPI_ERRORS_RETURN);
    if ((rc = MPIX_Hip_comm_get_unique_id(id)) || (rc = MPIX_Hip_comm_create(id, size, rank, &comm))) {
        fprintf(stderr, "comm: %d\n", rc);
        return 3;
    }
    while (fgets(line, sizeof line, stdin)) {
        char *tok[16], *t, *what, *save = NULL;
        const char *alg = "auto";
        int nt = 0, i, root = 0, inplace = 0, counts[64] = {0}, ncounts = 0, dt, op;
        long long count, total = 0;
        size_t esz, bytes, sbytes, rbytes;
        void *sb, *rb, *stream = NULL;
        for (t = strtok_r(line, " \t\n", &save); t && nt < 16; t = strtok_r(NULL, " \t\n", &save))
            tok[nt++] = t;
        if (nt == 2 && !strcmp(tok[0], "device")) {
            cur_device = atoi(tok[1]);
            note("device %d", cur_device);
            continue;
        }
        if (nt < 4)
            continue;
        what = tok[0];
        for (t = strtok_r(tok[1], ",", &save); t && ncounts < 64; t = strtok_r(NULL, ",", &save)) {
            counts[ncounts] = atoi(t);
            total += counts[ncounts++];
        }
        count = atoll(tok[1]);
        dt = type_of(tok[2]);
        op = op_of(tok[3]);
        for (i = 4; i < nt; i++) {
            if (!strcmp(tok[i], "inplace"))
                inplace = 1;
            else if (!strcmp(tok[i], "ustream"))
                stream = (void *) USER_STREAM;
            else if (!strcmp(tok[i], "auto") || !strcmp(tok[i], "ref") || !strcmp(tok[i], "rccl"))
                alg = tok[i];
            else
                root = atoi(tok[i]);
        }
        esz = (size_t) MPIR_Hip_elem_size(MPIR_Op_resolve_elem(op & 0xf, dt));
        esz = esz ? esz : 8;
        bytes = (size_t) count * esz;
        /* what the caller of each collective must provide (mpix_hip_coll.h) */
        sbytes = rbytes = bytes;
        if (!strcmp(what, "reduce_scatter_block")) {
            sbytes = bytes * (size_t) size;
            rbytes = inplace ? sbytes : bytes;
        } else if (!strcmp(what, "reduce_scatter")) {
            if (ncounts != size) {
                fprintf(stderr, "reduce_scatter: %d counts for %d ranks\n", ncounts, size);
                return 4;
            }
            sbytes = (size_t) total * esz;
            rbytes = inplace ? sbytes : (size_t) counts[rank] * esz;
        } else if (!strcmp(what, "reduce")) {
            inplace = inplace && rank == root;
            rbytes = rank == root ? bytes : 0;
        }
        sb = inplace ? NULL : reserve(sbytes);
        rb = !strcmp(what, "reduce") && rank != root ? NULL : reserve(rbytes);
        cur_send.base = sb;
        cur_send.bytes = sbytes;
        cur_recv.base = rb;
        cur_recv.bytes = rbytes;
        note("call %d %s", n++, what);
        note("+ call %s %s %s %s root=%d inplace=%d stream=%s", tok[1], tok[2], tok[3], alg, root, inplace,
             stream ? "user" : "comm");
        if (!strcmp(what, "allreduce")) {
            rc = MPIX_Allreduce_hip(inplace ? MPI_IN_PLACE : sb, rb, (int) count, dt, op, comm, alg_of(alg), stream);
        } else if (!strcmp(what, "reduce_scatter_block")) {
            rc = MPIX_Reduce_scatter_block_hip(inplace ? MPI_IN_PLACE : sb, rb, (int) count, dt, op, comm, alg_of(alg),
                                               stream);
        } else if (!strcmp(what, "reduce_scatter")) {
            rc = MPIX_Reduce_scatter_hip(inplace ? MPI_IN_PLACE : sb, rb, counts, dt, op, comm, alg_of(alg), stream);
        } else if (!strcmp(what, "reduce")) {
            rc = MPIX_Reduce_hip(inplace ? MPI_IN_PLACE : sb, rb, (int) count, dt, op, root, comm, alg_of(alg), stream);
        } else if (!strcmp(what, "scan") || !strcmp(what, "exscan")) {
            rc = (what[0] == 's' ? MPIX_Scan_hip : MPIX_Exscan_hip)(inplace ? MPI_IN_PLACE : sb, rb, (int) count, dt, op,
                                                                   comm, alg_of(alg), stream);
        } else {
            fprintf(stderr, "unknown plan line: %s\n", what);
            return 4;
        }
        release(sb, sbytes);
        release(rb, rbytes);
        cur_send.base = cur_recv.base = NULL;
        if (rc) {
            char msg[512];
            int len = 0;
            MPI_Error_string(rc, msg, &len);
            fprintf(stderr, "%s failed: %s\n", what, msg);
            return 5;
        }
        if (unknown) {
            fprintf(stderr, "%s: %d pointer(s) or handle(s) outside every known reservation\n", what, unknown);
            return 6;
        }
    }
    MPIX_Hip_comm_free(&comm);
    return unknown ? 6 : 0;
}
