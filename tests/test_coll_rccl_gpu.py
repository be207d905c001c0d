"""Device collectives over RCCL (one process per rank): MPI_Allreduce and
MPI_Reduce at small sizes, MPI_Reduce_scatter_block (config 5's collective)
at small sizes, and configs 4 and 5 at their full BASELINE sizes.

Needs one GPU per rank: RCCL refuses two ranks of a communicator on one
device.  With fewer visible GPUs the multi-rank cases skip; the reference-order
algorithm itself is covered on one GPU by test_coll_loopback_gpu.py (same code,
loopback transport).  A 1-rank RCCL communicator always runs here, which
exercises dlopen of librccl, ncclCommInitRank and both algorithms.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

import _types as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rank_main(rank, size, uid, q, cases):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes
    import torch
    import mpich_pip_amd as mpi
    import _types as T
    torch.cuda.set_device(rank)
    lib = mpi.load()
    lib.MPIX_Reduce_local_set_errhandler(mpi.MPI_ERRORS_RETURN)
    comm = ctypes.c_void_p()
    rc = lib.MPIX_Hip_comm_create(ctypes.c_char_p(uid), size, rank, ctypes.byref(comm))
    if rc:
        q.put((rank, "create", rc, mpi.error_string(rc)))
        return
    out = []
    for kind, t, op, count, alg in cases:
        rng = np.random.default_rng(1000 + rank)
        x = T.to_bytes(T.gen(t, count, rng, op, specials=False))
        send = torch.from_numpy(x.copy()).cuda()
        recv = torch.zeros_like(send)
        torch.cuda.synchronize()
        if kind == "rsb":   # count = recvcount; every rank sends count * size elements
            x = T.to_bytes(T.gen(t, count * size, rng, op, specials=False))
            send = torch.from_numpy(x.copy()).cuda()
            recv = torch.zeros(count * T.elem_size(t), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = mpi.reduce_scatter_block(send.data_ptr(), recv.data_ptr(), count, mpi.DATATYPES[t], mpi.OPS[op],
                                          comm.value, alg)
        elif kind == "allreduce":
            rc = mpi.allreduce(send.data_ptr(), recv.data_ptr(), count, mpi.DATATYPES[t], mpi.OPS[op], comm.value,
                               alg)
        else:   # reduce to the last rank; recvbuf NULL elsewhere
            root = size - 1
            rc = mpi.reduce(send.data_ptr(), recv.data_ptr() if rank == root else 0, count, mpi.DATATYPES[t],
                            mpi.OPS[op], root, comm.value, alg)
        torch.cuda.synchronize()
        out.append((rc, x, recv.cpu().numpy()))
    q.put((rank, "ok", 0, out))
    mpi.comm_free(comm.value)


def _run(size, cases):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
    import ctypes
    import mpich_pip_amd as mpi
    uid = ctypes.create_string_buffer(128)
    assert mpi.load().MPIX_Hip_comm_get_unique_id(uid) == 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, size, uid.raw, q, cases)) for r in range(size)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(size):
        r = q.get(timeout=300)
        res[r[0]] = r
    for p in procs:
        p.join(60)
    return res


def _ngpus():
    import torch
    return torch.cuda.device_count()


def _gamma(k, u):
    return k * u / (1 - k * u)


@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_allreduce_and_reduce_over_rccl(mpi, orc, cuda, size):
    from oracle import schedules as S
    if _ngpus() < size:
        pytest.skip(f"needs {size} GPUs, {_ngpus()} visible")
    REF, RCCL = mpi.MPIX_HIP_ALG_REFERENCE_ORDER, mpi.MPIX_HIP_ALG_RCCL
    cases = [("allreduce", "MPI_FLOAT", "MPI_SUM", (1 << 20) + 3, REF),
             ("allreduce", "MPI_FLOAT", "MPI_SUM", (1 << 20) + 3, RCCL),
             ("allreduce", "MPI_INT", "MPI_SUM", 4099, RCCL),
             ("allreduce", "MPIX_C_FLOAT16", "MPI_SUM", 4099, REF),
             ("allreduce", "MPI_DOUBLE", "MPI_MAX", 100, REF),
             ("reduce", "MPI_FLOAT", "MPI_SUM", (1 << 20) + 3, REF),
             ("reduce", "MPI_FLOAT", "MPI_SUM", (1 << 20) + 3, RCCL),
             ("reduce", "MPI_INT", "MPI_SUM", 77, RCCL),
             ("reduce", "MPI_DOUBLE", "MPI_SUM", 77, REF)]
    res = _run(size, cases)
    for r in range(size):
        assert res[r][1] == "ok", res[r]
    for k, (kind, t, op, count, alg) in enumerate(cases):
        xs = [res[r][3][k][1] for r in range(size)]
        esz = T.elem_size(t)
        if kind == "allreduce":
            want = S.allreduce_smp_auto(xs, count, esz, mpi.DATATYPES[t], mpi.OPS[op]) if size > 1 else xs[0]
            checked = range(size)
        else:
            want = S.reduce_auto(xs, count, esz, mpi.DATATYPES[t], mpi.OPS[op], size - 1)
            checked = [size - 1]
        for r in range(size):
            assert res[r][3][k][0] == 0, (kind, t, alg, r)
        for r in checked:
            rc, _, got = res[r][3][k]
            if alg == mpi.MPIX_HIP_ALG_REFERENCE_ORDER or t == "MPI_INT":
                assert np.array_equal(got, want), (t, alg, r)
            else:
                # RCCL's own order: |got - ref| <= gamma_{p-1} * sum|x_i|
                g = got.view(np.float32).astype(np.float64)
                w = want.view(np.float32).astype(np.float64)
                mag = np.sum([np.abs(x.view(np.float32).astype(np.float64)) for x in xs], axis=0)
                u = 2.0 ** -24
                gamma = (size - 1) * u / (1 - (size - 1) * u)
                assert np.all(np.abs(g - w) <= gamma * mag + 1e-45), (t, r)


@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_reduce_scatter_block_over_rccl(mpi, orc, cuda, size):
    """Config 5's collective (reduce_scatter_block_intra_pairwise.c:97-140) at
    N ranks, one per GPU: reference order bit-exact against the oracle's
    step-by-step schedule with MPICH's algorithm choice (pairwise from 512 KiB
    of sendbuf, recursive halving below: reduce_scatter_block.c:136-148);
    RCCL's ncclReduceScatter within 2 gamma_{p-1} of it for fp16 / fp32 (both
    chains round at every step), exact for int32."""
    from oracle import schedules as S
    if _ngpus() < size:
        pytest.skip(f"needs {size} GPUs, {_ngpus()} visible")
    REF, RCCL = mpi.MPIX_HIP_ALG_REFERENCE_ORDER, mpi.MPIX_HIP_ALG_RCCL
    big = (1 << 17) + 3            # size * big * 2 B >= 524288 at every N >= 2: pairwise
    cases = [("rsb", "MPIX_C_FLOAT16", "MPI_SUM", big, REF),
             ("rsb", "MPIX_C_FLOAT16", "MPI_SUM", big, RCCL),
             ("rsb", "MPIX_C_FLOAT16", "MPI_SUM", 1000, REF),          # recursive halving
             ("rsb", "MPI_FLOAT", "MPI_SUM", 4099, REF),
             ("rsb", "MPI_FLOAT", "MPI_SUM", 4099, RCCL),
             ("rsb", "MPI_INT", "MPI_SUM", 77777, RCCL),
             ("rsb", "MPI_DOUBLE", "MPI_MAX", 4099, REF)]
    res = _run(size, cases)
    for r in range(size):
        assert res[r][1] == "ok", res[r]
    for k, (kind, t, op, count, alg) in enumerate(cases):
        xs = [res[r][3][k][1] for r in range(size)]
        esz = T.elem_size(t)
        want = S.reduce_scatter_block_auto(xs, count, esz, mpi.DATATYPES[t], mpi.OPS[op])
        for r in range(size):
            rc, _, got = res[r][3][k]
            assert rc == 0, (t, alg, r)
            if alg == REF or t == "MPI_INT" or size == 1:
                assert np.array_equal(got, want[r]), (t, count, alg, r)
                continue
            ft, u = (np.float16, 2.0 ** -11) if t == "MPIX_C_FLOAT16" else (np.float32, 2.0 ** -24)
            g = got.view(ft).astype(np.float64)
            w = want[r].view(ft).astype(np.float64)
            blk = slice(r * count, (r + 1) * count)
            mag = np.sum([np.abs(x.view(ft)[blk].astype(np.float64)) for x in xs], axis=0)
            tiny = 2.0 ** -24 if ft == np.float16 else 1e-45
            assert np.all(np.abs(g - w) <= 2 * _gamma(size - 1, u) * mag + tiny), (t, r)


def _config_rank_main(rank, size, uid, q, alg):
    """One rank of the config-size cases.  Every rank derives every rank's
    input from seeds -- allreduce: rank j's 256 MiB fp32 buffer is 8 chunks
    seeded (j, c); reduce-scatter: rank j's 1 GiB fp16 sendbuf is `size`
    blocks seeded (j, b) -- so it can check its own result without receiving
    anyone's data.  Expected values (numpy; fp32 / fp16 adds round like the
    reference's, pinned by tests/test_bench_selfcheck_cpu.py): allreduce in
    reduce_intra_reduce_scatter_gather.c's tree order per block (pof2 N), the
    pairwise chain per output block; RCCL against the exact (float64) sum
    within gamma_{p-1} (fp32) / 2 gamma_{p-1} (fp16, both chains round)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    import mpich_pip_amd as mpi
    from bench_coll import expect_allreduce
    torch.cuda.set_device(rank)
    lib = mpi.load()
    lib.MPIX_Reduce_local_set_errhandler(mpi.MPI_ERRORS_RETURN)
    comm = ctypes.c_void_p()
    rc = lib.MPIX_Hip_comm_create(ctypes.c_char_p(uid), size, rank, ctypes.byref(comm))
    if rc:
        q.put((rank, "create", rc, mpi.error_string(rc)))
        return
    out = {}
    # ---- config 4: MPI_Allreduce fp32 SUM, 256 MiB per rank
    n = 64 << 20
    chunks = 8

    def ar_input(j):
        return np.concatenate([np.random.default_rng((j, c, 4)).uniform(-1, 1, n // chunks).astype(np.float32)
                               for c in range(chunks)])
    xs = [ar_input(j) for j in range(size)]
    send = torch.from_numpy(xs[rank]).cuda()
    recv = torch.empty_like(send)
    torch.cuda.synchronize()
    rc = mpi.allreduce(send.data_ptr(), recv.data_ptr(), n, mpi.MPI_FLOAT, mpi.MPI_SUM, comm.value, alg)
    torch.cuda.synchronize()
    got = recv.cpu().numpy()
    del send, recv
    pof2 = size & (size - 1) == 0
    if alg == mpi.MPIX_HIP_ALG_REFERENCE_ORDER and pof2:
        out["allreduce"] = (rc, bool(np.array_equal(got.view(np.uint32), expect_allreduce(xs).view(np.uint32))))
    else:
        exact = np.sum([x.astype(np.float64) for x in xs], axis=0)
        mag = np.sum([np.abs(x.astype(np.float64)) for x in xs], axis=0)
        ok = np.all(np.abs(got.astype(np.float64) - exact) <= _gamma(max(size - 1, 1), 2.0 ** -24) * mag + 1e-45)
        out["allreduce"] = (rc, bool(ok))
    del xs, got
    # ---- config 5: MPI_Reduce_scatter_block fp16 SUM, 1 GiB sendbuf per rank
    total = 1 << 29
    rcnt = total // size

    def rs_block(j, b):
        return np.random.default_rng((j, b, 5)).uniform(-4, 4, rcnt).astype(np.float16)
    send = torch.from_numpy(np.concatenate([rs_block(rank, b) for b in range(size)])).cuda()
    recv = torch.empty(rcnt, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    rc = mpi.reduce_scatter_block(send.data_ptr(), recv.data_ptr(), rcnt, mpi.MPIX_C_FLOAT16, mpi.MPI_SUM,
                                  comm.value, alg)
    torch.cuda.synchronize()
    got = recv.cpu().numpy()
    del send, recv
    mine = [rs_block(j, rank) for j in range(size)]
    acc = mine[rank].copy()                      # ((x_r + x_{r-1}) + x_{r-2}) + ...
    for i in range(1, size):
        acc = acc + mine[(rank - i) % size]
    if alg == mpi.MPIX_HIP_ALG_REFERENCE_ORDER:
        out["reduce_scatter_block"] = (rc, bool(np.array_equal(got.view(np.uint16), acc.view(np.uint16))))
    else:
        mag = np.sum([np.abs(x.astype(np.float64)) for x in mine], axis=0)
        ok = np.all(np.abs(got.astype(np.float64) - acc.astype(np.float64)) <=
                    2 * _gamma(max(size - 1, 1), 2.0 ** -11) * mag + 2.0 ** -24)
        out["reduce_scatter_block"] = (rc, bool(ok))
    q.put((rank, "ok", 0, out))
    mpi.comm_free(comm.value)


@pytest.mark.parametrize("alg", ["reference_order", "rccl"])
@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_config_size_collectives_over_rccl(mpi, cuda, size, alg):
    """BASELINE configs 4 and 5 at full size: MPI_Allreduce fp32 SUM of 256 MiB
    per rank and MPI_Reduce_scatter_block fp16 SUM of a 1 GiB sendbuf per rank
    (recvcount 2^29 / N), one rank per GPU, both algorithms."""
    if _ngpus() < size:
        pytest.skip(f"needs {size} GPUs, {_ngpus()} visible")
    import ctypes
    a = mpi.MPIX_HIP_ALG_REFERENCE_ORDER if alg == "reference_order" else mpi.MPIX_HIP_ALG_RCCL
    uid = ctypes.create_string_buffer(128)
    assert mpi.load().MPIX_Hip_comm_get_unique_id(uid) == 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_config_rank_main, args=(r, size, uid.raw, q, a)) for r in range(size)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(size):
        r = q.get(timeout=600)
        res[r[0]] = r
    for p in procs:
        p.join(60)
    for r in range(size):
        assert res[r][1] == "ok", res[r]
        for name, (rc, ok) in res[r][3].items():
            assert rc == 0 and ok, (name, alg, r)


# ---------------------------------------------------------------------------
# On a caller's stream (a non-NULL hip_stream): nothing synchronises with the
# host, so two calls in a row overlap, and over RCCL -- unlike the loopback
# transport, which synchronises inside every exchange -- a missing wait between
# them would show.  tests/test_coll_order_cpu.py proves the ordering from the
# logged call sequence; this runs it.
# ---------------------------------------------------------------------------
STREAM_N = (1 << 19) + 7


def _stream_rank_main(rank, size, uid, q, algs):
    """One rank: on one stream of its own, behind slow work and the copy that
    brings the input, an Allreduce fp32 SUM of STREAM_N and, with nothing in
    between, a Reduce_scatter_block whose sendbuf is the Allreduce's recvbuf
    (recvcount STREAM_N // size); a stream-ordered copy out; that stream alone
    is synchronised.  Once per algorithm of `algs`."""
    os.environ["MPIR_CVAR_DEVICE_COLL_PIPELINE_KB"] = "64"
    import sys
    sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    import mpich_pip_amd as mpi
    torch.cuda.set_device(rank)
    lib = mpi.load()
    lib.MPIX_Reduce_local_set_errhandler(mpi.MPI_ERRORS_RETURN)
    comm = ctypes.c_void_p()
    rc = lib.MPIX_Hip_comm_create(ctypes.c_char_p(uid), size, rank, ctypes.byref(comm))
    if rc:
        q.put((rank, "create", rc, mpi.error_string(rc)))
        return
    n, rcnt = STREAM_N, STREAM_N // size
    x = np.random.default_rng(2000 + rank).uniform(-1, 1, n).astype(np.float32)
    hin = torch.from_numpy(x).pin_memory()
    big = torch.ones(64 << 20, device="cuda")
    out = []
    for alg in algs:
        send = torch.full((n,), float("nan"), device="cuda")
        mid = torch.full((n,), float("nan"), device="cuda")
        recv = torch.full((rcnt + 16,), float("nan"), device="cuda")
        hmid = torch.zeros(n).pin_memory()
        hout = torch.zeros(rcnt + 16).pin_memory()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for _ in range(20):
                big.mul_(1.0000001)
            send.copy_(hin, non_blocking=True)
            rc1 = mpi.allreduce(send.data_ptr(), mid.data_ptr(), n, mpi.MPI_FLOAT, mpi.MPI_SUM, comm.value, alg,
                                st.cuda_stream)
            rc2 = mpi.reduce_scatter_block(mid.data_ptr(), recv.data_ptr(), rcnt, mpi.MPI_FLOAT, mpi.MPI_SUM,
                                           comm.value, alg, st.cuda_stream)
            hmid.copy_(mid, non_blocking=True)
            hout.copy_(recv, non_blocking=True)
        st.synchronize()
        out.append((rc1, rc2, x.view(np.uint8), hmid.numpy().view(np.uint8).copy(), hout.numpy().view(np.uint8).copy()))
    q.put((rank, "ok", 0, out))
    torch.cuda.synchronize()
    mpi.comm_free(comm.value)


def _run_stream(size, algs):
    import ctypes
    import mpich_pip_amd as mpi
    uid = ctypes.create_string_buffer(128)
    assert mpi.load().MPIX_Hip_comm_get_unique_id(uid) == 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stream_rank_main, args=(r, size, uid.raw, q, algs)) for r in range(size)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(size):
        r = q.get(timeout=300)
        res[r[0]] = r
    for p in procs:
        p.join(60)
    for r in range(size):
        assert res[r][1] == "ok", res[r]
    return res


@pytest.mark.parametrize("size", [2, 8])
def test_back_to_back_on_a_callers_stream_over_rccl(mpi, orc, cuda, size):
    """Two pipelined reference-order collectives in a row on one caller's
    stream per rank, the second reading what the first wrote, over the RCCL
    transport: bit-exact against the oracle's schedules composed."""
    from oracle import schedules as S
    if _ngpus() < size:
        pytest.skip(f"needs {size} GPUs, {_ngpus()} visible")
    res = _run_stream(size, [mpi.MPIX_HIP_ALG_REFERENCE_ORDER])
    n, rcnt = STREAM_N, STREAM_N // size
    xs = [res[r][3][0][2] for r in range(size)]
    mid = S.allreduce_smp_auto(xs, n, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    want = S.reduce_scatter_block_auto([mid[:size * rcnt * 4].copy() for _ in range(size)], rcnt, 4, mpi.MPI_FLOAT,
                                       mpi.MPI_SUM)
    for r in range(size):
        rc1, rc2, _, gmid, gout = res[r][3][0]
        assert rc1 == 0 and rc2 == 0, (r, rc1, rc2)
        assert np.array_equal(gmid, mid), f"rank {r}: allreduce: {np.count_nonzero(gmid != mid)} bytes differ"
        assert np.array_equal(gout[:rcnt * 4], want[r]), f"rank {r}: {np.count_nonzero(gout[:rcnt * 4] != want[r])}"
        assert np.isnan(gout[rcnt * 4:].view(np.float32)).all(), f"rank {r}: wrote behind recvbuf"


def test_one_rank_rccl_on_a_callers_stream(mpi, cuda):
    """A 1-rank RCCL communicator (always runs): ncclAllReduce and
    ncclReduceScatter on the caller's stream, MPIX_HIP_ALG_RCCL and AUTO, behind
    slow work and the input's copy on that stream; the result is the input."""
    res = _run_stream(1, [mpi.MPIX_HIP_ALG_RCCL, mpi.MPIX_HIP_ALG_AUTO])
    for k, (rc1, rc2, x, gmid, gout) in enumerate(res[0][3]):
        assert rc1 == 0 and rc2 == 0, (k, rc1, rc2)
        assert np.array_equal(gmid, x), f"alg {k}: allreduce: {np.count_nonzero(gmid != x)} bytes differ"
        assert np.array_equal(gout[:STREAM_N * 4], x), f"alg {k}: reduce_scatter_block differs"
        assert np.isnan(gout[STREAM_N * 4:].view(np.float32)).all(), f"alg {k}: wrote behind recvbuf"
