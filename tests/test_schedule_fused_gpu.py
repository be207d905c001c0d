"""Fused schedule combines (MPIX_Reduce_local_multi) vs the reference schedules, on one GPU.

The reference's Allreduce on one node (allreduce_intra_smp.c -> MPIR_Reduce via
reduce_intra_reduce_scatter_gather.c) and its Reduce_scatter_block
(reduce_scatter_block_intra_pairwise.c) call MPIR_Reduce_local log2(p) resp.
p-1 times per element.  The MI355X design gathers every rank's copy of a block
in HBM (all-to-all) and folds them in ONE pass with the schedule's exact
association and operand order.  Here p ranks' buffers live on one GPU; the
expected bytes come from oracle/schedules.py, which runs the reference
schedules step by step through the C oracle.  Bit-exact (complex NaN payloads
excepted, see test_parity_gpu.same).
"""
import numpy as np
import pytest

import _types as T
from test_parity_gpu import same

pytestmark = pytest.mark.gpu


def _pof2(p):
    q = 1
    while q * 2 <= p:
        q *= 2
    return q


def _cnts_disps(count, pof2):
    cnts = [count // pof2 + (1 if i < count % pof2 else 0) for i in range(pof2)]
    disps = [sum(cnts[:i]) for i in range(pof2)]
    return cnts, disps


def _bitrev(n, bits):
    return int(format(n, f"0{bits}b")[::-1], 2) if bits else 0


def fused_allreduce(mpi, torch, xs_dev, count, esz, dt, op):
    """The MI355X reference-order Allreduce on p virtual ranks (one GPU):
    pre-fold (p not a power of two), then per block b the owner newrank
    k = bitrev(b) folds y_j = x_{k ^ j}[b] with MPIX_ORDER_TREE."""
    p = len(xs_dev)
    pof2 = _pof2(p)
    rem = p - pof2
    leaves = []
    for r in range(p):                     # reduce_intra_reduce_scatter_gather.c:138-170
        if r < 2 * rem:
            if r % 2 == 0:
                acc = xs_dev[r].clone()
                torch.cuda.synchronize()
                assert mpi.reduce_local(xs_dev[r + 1].data_ptr(), acc.data_ptr(), count, dt, op) == 0
                leaves.append(acc)
        else:
            leaves.append(xs_dev[r])
    assert len(leaves) == pof2
    cnts, disps = _cnts_disps(count, pof2)
    out = torch.empty(count * esz, dtype=torch.uint8, device="cuda")
    bits = pof2.bit_length() - 1
    for b in range(pof2):
        k = _bitrev(b, bits)
        ys = [leaves[k ^ j].data_ptr() + disps[b] * esz for j in range(pof2)]
        rc = mpi.reduce_local_multi(ys, out.data_ptr() + disps[b] * esz, cnts[b], dt, op, mpi.MPIX_ORDER_TREE)
        assert rc == 0, mpi.error_string(rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


CASES = [("MPI_FLOAT", "MPI_SUM"), ("MPI_DOUBLE", "MPI_SUM"), ("MPIX_C_FLOAT16", "MPI_SUM"),
         ("MPI_INT", "MPI_SUM"), ("MPI_INT64_T", "MPI_PROD"), ("MPI_FLOAT", "MPI_MAX"),
         ("MPI_DOUBLE", "MPI_MIN"), ("MPI_C_FLOAT_COMPLEX", "MPI_SUM"), ("MPI_FLOAT", "MPI_PROD"),
         ("MPI_UNSIGNED_CHAR", "MPI_BXOR"), ("MPI_INT", "MPI_LAND")]


@pytest.mark.parametrize("t,op", CASES, ids=[f"{t}-{o}" for t, o in CASES])
@pytest.mark.parametrize("p", [2, 3, 4, 6, 8])
def test_fused_allreduce_matches_reference_schedule(mpi, orc, cuda, t, op, p):
    from oracle import schedules as S
    torch = cuda
    esz = T.elem_size(t)
    for count, seed in ((1003, p), ((1 << 18) + 5, 7 * p)):
        rng = np.random.default_rng(seed)
        xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(p)]
        want = S.allreduce_smp(xs, count, esz, mpi.DATATYPES[t], mpi.OPS[op])
        xs_dev = [torch.from_numpy(x.copy()).cuda() for x in xs]
        got = fused_allreduce(mpi, torch, xs_dev, count, esz, mpi.DATATYPES[t], mpi.OPS[op])
        assert same(got, want, t), f"p={p} count={count}: {np.count_nonzero(got != want)} bytes differ"


@pytest.mark.parametrize("t,op", [("MPIX_C_FLOAT16", "MPI_SUM"), ("MPI_FLOAT", "MPI_SUM"), ("MPI_INT", "MPI_SUM"),
                                  ("MPI_DOUBLE", "MPI_MAX"), ("MPI_UNSIGNED", "MPI_BOR")])
@pytest.mark.parametrize("p", [2, 3, 5, 8, 11])
def test_fused_reduce_scatter_block_matches_pairwise(mpi, orc, cuda, t, op, p):
    """Config 5's schedule: rank r's block = ((x_r + x_{r-1}) + x_{r-2}) + ... (fp16: per-step rounding)."""
    from oracle import schedules as S
    torch = cuda
    esz = T.elem_size(t)
    recvcount = 4099
    rng = np.random.default_rng(p)
    xs = [T.to_bytes(T.gen(t, recvcount * p, rng, op)) for _ in range(p)]
    want = S.reduce_scatter_block_pairwise(xs, recvcount, esz, mpi.DATATYPES[t], mpi.OPS[op])
    xs_dev = [torch.from_numpy(x.copy()).cuda() for x in xs]
    nb = recvcount * esz
    for r in range(p):
        out = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ys = [xs_dev[(r - i) % p].data_ptr() + r * nb for i in range(p)]
        rc = mpi.reduce_local_multi(ys, out.data_ptr(), recvcount, mpi.DATATYPES[t], mpi.OPS[op],
                                    mpi.MPIX_ORDER_CHAIN)
        assert rc == 0, mpi.error_string(rc)
        got = out.cpu().numpy()
        assert same(got, want[r], t), f"rank {r}"


def test_multi_validation(mpi, cuda):
    torch = cuda
    a = torch.zeros(64, device="cuda")
    b = torch.zeros(64, device="cuda")
    ptrs = [a.data_ptr(), b.data_ptr(), a.data_ptr()]
    # tree needs a power of two
    ec = mpi.error_class
    assert ec(mpi.reduce_local_multi(ptrs, b.data_ptr(), 64, mpi.MPI_FLOAT, mpi.MPI_SUM,
                                     mpi.MPIX_ORDER_TREE)) == mpi.MPI_ERR_ARG
    # op/type check like MPI_Reduce_local
    assert ec(mpi.reduce_local_multi(ptrs[:2], b.data_ptr(), 64, mpi.MPI_FLOAT, mpi.MPI_BAND,
                                     mpi.MPIX_ORDER_CHAIN)) == mpi.MPI_ERR_OP
    h = np.zeros(64, np.float32)
    assert ec(mpi.reduce_local_multi([h.ctypes.data, a.data_ptr()], b.data_ptr(), 64, mpi.MPI_FLOAT, mpi.MPI_SUM,
                                     mpi.MPIX_ORDER_CHAIN)) == mpi.MPI_ERR_BUFFER


def test_multi_overlap_refused(mpi, cuda):
    """outbuf may be inbufs[0] exactly; any other overlap is MPI_ERR_BUFFER,
    whatever MPIR_CVAR_COLL_ALIAS_CHECK says (the CHAIN path for n > 8 writes
    outbuf between passes)."""
    torch = cuda
    ec = mpi.error_class
    bufs = [torch.full((4096,), float(j + 1), device="cuda") for j in range(12)]
    p = [b.data_ptr() for b in bufs]
    F, S, C, T = mpi.MPI_FLOAT, mpi.MPI_SUM, mpi.MPIX_ORDER_CHAIN, mpi.MPIX_ORDER_TREE
    # exactly a later operand, on the multi-pass CHAIN shape and on a fused TREE
    assert ec(mpi.reduce_local_multi(p, p[9], 4096, F, S, C)) == mpi.MPI_ERR_BUFFER
    assert ec(mpi.reduce_local_multi(p[:4], p[2], 4096, F, S, T)) == mpi.MPI_ERR_BUFFER
    # partial overlaps: with operand 0, and a later operand's tail
    assert ec(mpi.reduce_local_multi(p[:4], p[0] + 16, 4096, F, S, T)) == mpi.MPI_ERR_BUFFER
    assert ec(mpi.reduce_local_multi(p[:3], p[2] - 64, 4096, F, S, C)) == mpi.MPI_ERR_BUFFER
    assert "overlaps outbuf" in mpi.error_string(mpi.reduce_local_multi(p[:3], p[1] + 4, 4096, F, S, C))
    # adjacent (touching, not overlapping) and exactly operand 0 are fine
    big = torch.ones(2 * 4096, device="cuda")
    assert mpi.reduce_local_multi([big.data_ptr(), p[1]], big.data_ptr() + 4 * 4096, 4096, F, S, C) == 0
    assert mpi.reduce_local_multi(p, p[0], 4096, F, S, C) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], torch.full((4096,), float(sum(range(1, 13))), device="cuda"))
    assert torch.equal(big[4096:], torch.full((4096,), 3.0, device="cuda"))


ANY = [("MPI_DOUBLE_INT", "MPI_MINLOC"), ("MPI_2INT", "MPI_MAXLOC"), ("MPI_INT", "MPI_LAND"),
       ("MPI_UNSIGNED_SHORT", "MPI_BOR"), ("MPI_C_DOUBLE_COMPLEX", "MPI_PROD"), ("MPI_LONG_DOUBLE", "MPI_SUM"),
       ("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC"), ("MPI_FLOAT", "MPI_SUM"), ("MPIX_C_FLOAT16", "MPI_MAX")]


@pytest.mark.parametrize("t,op", ANY, ids=[f"{t}-{o}" for t, o in ANY])
@pytest.mark.parametrize("n,order", [(2, "TREE"), (4, "TREE"), (16, "TREE"), (64, "TREE"), (3, "CHAIN"),
                                     (13, "CHAIN")])
def test_one_pass_combine_matches_stepwise_fold(mpi, orc, cuda, t, op, n, order):
    """MPIR_Hip_combine's general one-pass path (k_combine_any: any op/type, any n,
    no device temporaries) and the fused kernels agree bit for bit with the
    same fold done one MPIR_Reduce_local step at a time by the oracle.  The
    output aliases operand 0 on the CHAIN cases."""
    torch = cuda
    esz = T.elem_size(t)
    count = 1000 + n
    rng = np.random.default_rng(n)
    xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    acc = [x.copy() for x in xs]
    if order == "TREE":
        step = 1
        while step < n:
            for j in range(0, n, 2 * step):
                assert orc.reduce_local(acc[j + step], acc[j], count, dt, o, check=False) == 0
            step *= 2
    else:
        for j in range(1, n):
            assert orc.reduce_local(acc[j], acc[0], count, dt, o, check=False) == 0
    want = acc[0]
    dev = [torch.from_numpy(x.copy()).cuda() for x in xs]
    out = dev[0] if order == "CHAIN" else torch.zeros(count * esz, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = mpi.reduce_local_multi([d.data_ptr() for d in dev], out.data_ptr(), count, dt, o,
                                mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN)
    assert rc == 0, mpi.error_string(rc)
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), want, t)


def test_concurrent_threads_minloc_tree16_regression(mpi, orc, cuda):
    """Regression for the corruption removed in e7b5d60: several host threads
    folding MPI_MINLOC (no fused kernel: the general path) at once, each on its
    own library stream.  The removed path took its temporaries with
    hipMallocAsync / hipFreeAsync, and the default memory pool handed a block
    freed on one stream to another stream while the first stream's kernels
    still read it (tools/mempool_race.hip: 3 of 1200 results corrupted at 4
    threads, 14 of 2400 at 8; profiles/archive/r02/mempool_race.log).  The product takes
    no stream-ordered allocations (tests/test_no_stream_ordered_alloc_cpu.py);
    this checks the concurrent folds stay bit-exact."""
    import threading
    torch = cuda
    t, op, n, count, iters, nthreads = "MPI_DOUBLE_INT", "MPI_MINLOC", 16, 1 << 16, 12, 4
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    cases = []
    for k in range(nthreads):
        rng = np.random.default_rng(100 + k)
        xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
        acc = [x.copy() for x in xs]
        step = 1
        while step < n:
            for j in range(0, n, 2 * step):
                assert orc.reduce_local(acc[j + step], acc[j], count, dt, o, check=False) == 0
            step *= 2
        dev = [torch.from_numpy(x).cuda() for x in xs]
        outs = [torch.zeros(count * esz, dtype=torch.uint8, device="cuda") for _ in range(iters)]
        cases.append((acc[0], dev, outs))
    torch.cuda.synchronize()
    errors = []

    def run(k):
        want, dev, outs = cases[k]
        for out in outs:
            rc = mpi.reduce_local_multi([d.data_ptr() for d in dev], out.data_ptr(), count, dt, o,
                                        mpi.MPIX_ORDER_TREE)
            if rc:
                errors.append(mpi.error_string(rc))
    th = [threading.Thread(target=run, args=(k,)) for k in range(nthreads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for k, (want, _, outs) in enumerate(cases):
        for i, out in enumerate(outs):
            assert same(out.cpu().numpy(), want, t), (k, i)


EVERY = [(op, t) for op in T.OPS for t in T.ALL_TYPES if T.compute_ok(op, t)]


@pytest.mark.parametrize("op,t", EVERY, ids=[f"{o}-{t}" for o, t in EVERY])
def test_every_pair_fused_matches_stepwise_fold(mpi, orc, cuda, op, t):
    """Every (op, type) the reference computes, through MPIX_Reduce_local_multi:
    TREE of 8 (one fused pass), CHAIN of 3, 5, 6, 7 and 8 (one pass each: the
    pairwise chain of every rank count up to 8) and CHAIN of 11 (a pass of 8,
    then one of 4 reading the first's output) against the same fold done one
    oracle MPIR_Reduce_local step at a time.  Operands with
    specials (NaN, +-0, inf, denormals, extremes); the second round starts
    every buffer one element past 256 B alignment so the fused kernel's head
    and tail elements run too."""
    torch = cuda
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    for k, (n, order) in enumerate(((8, "TREE"), (8, "CHAIN"), (5, "CHAIN"), (3, "CHAIN"), (6, "CHAIN"),
                                    (7, "CHAIN"), (11, "CHAIN"))):
        for off in (0, esz):
            count = 3000 + 7 * n + k
            rng = np.random.default_rng(1000 * n + k + off)
            xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
            acc = [x.copy() for x in xs]
            if order == "TREE":
                step = 1
                while step < n:
                    for j in range(0, n, 2 * step):
                        assert orc.reduce_local(acc[j + step], acc[j], count, dt, o, check=False) == 0
                    step *= 2
            else:
                for j in range(1, n):
                    assert orc.reduce_local(acc[j], acc[0], count, dt, o, check=False) == 0
            nb = count * esz
            dev = []
            for x in xs:
                d = torch.zeros(nb + off + 64, dtype=torch.uint8, device="cuda")
                d[off:off + nb].copy_(torch.from_numpy(x))
                dev.append(d)
            out = torch.zeros(nb + off + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = mpi.reduce_local_multi([d.data_ptr() + off for d in dev], out.data_ptr() + off, count, dt, o,
                                        mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN)
            assert rc == 0, mpi.error_string(rc)
            torch.cuda.synchronize()
            got = out[off:off + nb].cpu().numpy()
            assert same(got, acc[0], t), f"n={n} {order} off={off}: {np.count_nonzero(got != acc[0])} bytes differ"
            assert not out[:off].any() and not out[off + nb:].any(), "wrote outside the output"


@pytest.mark.parametrize("t,order,block_mib", [("MPI_FLOAT", "TREE", 32), ("MPIX_C_FLOAT16", "CHAIN", 128)],
                         ids=["config4-tree8-fp32-32MiB", "config5-chain8-fp16-128MiB"])
def test_fused_full_size_blocks(mpi, orc, cuda, t, order, block_mib):
    """The fused combines at the block sizes of BASELINE configs 4-5 at N = 8
    (Allreduce 256 MiB -> 8 x 32 MiB blocks, TREE; Reduce_scatter_block 1 GiB
    fp16 -> 8 x 128 MiB blocks, CHAIN), bit-exact against the oracle's
    step-by-step fold over the whole block."""
    torch = cuda
    esz = T.elem_size(t)
    n = (block_mib << 20) // esz
    dt, o = mpi.DATATYPES[t], mpi.OPS["MPI_SUM"]
    g = torch.Generator(device="cuda").manual_seed(block_mib)
    if t == "MPI_FLOAT":
        dev = [torch.rand(n, device="cuda", generator=g) * 2 - 1 for _ in range(8)]
    else:
        dev = [(torch.rand(n, device="cuda", generator=g) * 8 - 4).half() for _ in range(8)]
    out = torch.empty_like(dev[0])
    torch.cuda.synchronize()
    rc = mpi.reduce_local_multi([d.data_ptr() for d in dev], out.data_ptr(), n, dt, o,
                                mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN)
    assert rc == 0, mpi.error_string(rc)
    torch.cuda.synchronize()
    acc = [d.cpu().numpy().view(np.uint8).copy() for d in dev]
    del dev
    if order == "TREE":
        step = 1
        while step < 8:
            for j in range(0, 8, 2 * step):
                assert orc.reduce_local(acc[j + step], acc[j], n, dt, o, check=False) == 0
            step *= 2
    else:
        for j in range(1, 8):
            assert orc.reduce_local(acc[j], acc[0], n, dt, o, check=False) == 0
    got = out.cpu().numpy().view(np.uint8)
    assert np.array_equal(got, acc[0]), f"{np.count_nonzero(got != acc[0])} bytes differ"


@pytest.mark.parametrize("t,order,nbytes", [("MPI_FLOAT", "TREE", (256 << 20) + 20), ("MPIX_C_FLOAT16", "CHAIN", (512 << 20) + 6)],
                         ids=["tree2-fp32-256MiB", "chain2-fp16-512MiB"])
def test_two_operand_fold_large_blocks(mpi, orc, cuda, t, order, nbytes):
    """Two-operand folds over blocks of 256 MiB and more run on the 1024 x 1
    shape (launch_combine_p; config 5's 2 x 512 MiB at 2 ranks), with the
    operands one element past 16 B alignment so the head and tail run too;
    bit-exact against the oracle's MPIR_Reduce_local step."""
    torch = cuda
    esz = T.elem_size(t)
    n = nbytes // esz
    dt, o = mpi.DATATYPES[t], mpi.OPS["MPI_SUM"]
    g = torch.Generator(device="cuda").manual_seed(n)
    if t == "MPI_FLOAT":
        dev = [torch.rand(n + 1, device="cuda", generator=g) * 2 - 1 for _ in range(2)]
    else:
        dev = [(torch.rand(n + 1, device="cuda", generator=g) * 8 - 4).half() for _ in range(2)]
    out = torch.zeros_like(dev[0])
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() + esz for d in dev]
    rc = mpi.reduce_local_multi(ptrs, out.data_ptr() + esz, n, dt, o,
                                mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN)
    assert rc == 0, mpi.error_string(rc)
    torch.cuda.synchronize()
    acc = [d.cpu().numpy().view(np.uint8)[esz:].copy() for d in dev]
    del dev
    assert orc.reduce_local(acc[1], acc[0], n, dt, o, check=False) == 0
    got = out.cpu().numpy().view(np.uint8)
    assert not got[:esz].any(), "wrote before the output"
    assert np.array_equal(got[esz:], acc[0]), f"{np.count_nonzero(got[esz:] != acc[0])} bytes differ"


# ---------------------------------------------------------------------------
# The fused fold's launch-plan edges.  Every case asserts the path
# MPIR_Hip_combine_plan_info reports (the launch's own split) before it runs, so
# a case aimed at k_combine_multi_elems cannot pass on k_combine_multi.  Data,
# reference and comparison as in test_every_pair_fused_matches_stepwise_fold: the
# oracle folds one MPIR_Reduce_local step at a time, compared with same(); every
# allocation is zero around its payload and checked after the call.
# ---------------------------------------------------------------------------
ELEMS_STRIDE = 2 * 1048576 + 4099       # k_combine_multi_elems: 4096 workgroups, 1,048,576 elements per stride
ANY_STRIDE = 2 * 2097152 + 4099         # k_combine_any: 8192 workgroups, 2,097,152 elements per stride


def _align_of(t):
    """Alignment of the device type of MPI type t (reduce_ops.hpp)."""
    if t in ("MPI_LONG_DOUBLE", "MPI_C_LONG_DOUBLE_COMPLEX", "MPI_LONG_DOUBLE_INT"):
        return 16
    if t in T.CPLX:
        return T.elem_size(t) // 2
    if t in T.PAIRS:
        return {"MPI_2INT": 4, "MPI_FLOAT_INT": 4, "MPI_LONG_INT": 8, "MPI_SHORT_INT": 4, "MPI_DOUBLE_INT": 8}[t]
    return T.elem_size(t)


def _fold(orc, xs, count, dt, o, order):
    acc = [x.copy() for x in xs]
    n = len(xs)
    if order == "TREE":
        step = 1
        while step < n:
            for j in range(0, n, 2 * step):
                assert orc.reduce_local(acc[j + step], acc[j], count, dt, o, check=False) == 0
            step *= 2
    else:
        for j in range(1, n):
            assert orc.reduce_local(acc[j], acc[0], count, dt, o, check=False) == 0
    return acc[0]


def _has_fused(mpi, t, op):
    """Whether (op, t) has a fused fold: the path of an aligned fold of two (made-up addresses)."""
    a = 1 << 32
    return mpi.combine_plan_info([a, a + 4096], a + 8192, 16, mpi.DATATYPES[t], mpi.OPS[op],
                                 mpi.MPIX_ORDER_CHAIN)["path"] == mpi.COMBINE_FUSED_VECTOR


def _run_fold(mpi, torch, xs, want, t, op, order, offs, off_out, path, alias=False):
    """Operand j at byte offset offs[j] of its own zeroed allocation, the output
    at off_out of another (or operand 0 itself: alias); returns the plan info."""
    esz = T.elem_size(t)
    nb = xs[0].size
    count = nb // esz
    dev = []
    for x, off in zip(xs, offs):
        d = torch.zeros(nb + off + 64, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0
        d[off:off + nb].copy_(torch.from_numpy(x))
        dev.append(d)
    if alias:
        out, off_out = dev[0], offs[0]
    else:
        out = torch.zeros(nb + off_out + 64, dtype=torch.uint8, device="cuda")
    ptrs = [d.data_ptr() + off for d, off in zip(dev, offs)]
    ordv = mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN
    what = f"{op} {t} {order}{len(xs)} count={count} in=+{list(offs)} out=+{off_out}{' (= in[0])' if alias else ''}"
    info = mpi.combine_plan_info(ptrs, out.data_ptr() + off_out, count, mpi.DATATYPES[t], mpi.OPS[op], ordv)
    assert info["path"] == path, f"{what}: aimed at path {path}, the planner says {info}"
    torch.cuda.synchronize()
    rc = mpi.reduce_local_multi(ptrs, out.data_ptr() + off_out, count, mpi.DATATYPES[t], mpi.OPS[op], ordv)
    assert rc == 0, f"{what}: {mpi.error_string(rc)}"
    torch.cuda.synchronize()
    whole = out.cpu().numpy()
    got = whole[off_out:off_out + nb]
    assert same(got, want, t), f"{what}: {np.count_nonzero(got != want)} bytes differ"
    assert not whole[:off_out].any() and not whole[off_out + nb:].any(), f"{what}: wrote outside the output"
    for j in range(1 if alias else 0, len(xs)):
        w = dev[j].cpu().numpy()
        assert np.array_equal(w[offs[j]:offs[j] + nb], xs[j]) and not w[:offs[j]].any() and \
            not w[offs[j] + nb:].any(), f"{what}: operand {j} or its surroundings written"
    return info


@pytest.mark.parametrize("op,t", EVERY, ids=[f"{o}-{t}" for o, t in EVERY])
def test_every_pair_misaligned_operands_element_fold(mpi, orc, cuda, op, t):
    """Operands that do not share the output's alignment mod 16, or are not
    naturally aligned, take the fused fold's element kernel
    (k_combine_multi_elems): every pair with a fused fold, TREE of 2, 4, 8 and
    CHAIN of 2, 3, 5, 8 at count 3001, with all operands off the output, one
    operand off, every operand at another offset, every pointer one byte off its
    natural alignment, and CHAIN into its own first operand.  (The 32-byte
    classes have no fused fold: the same operands go through k_combine_any.)"""
    torch = cuda
    esz, align = T.elem_size(t), _align_of(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    path = mpi.COMBINE_FUSED_ELEMENTS if _has_fused(mpi, t, op) else mpi.COMBINE_ANY
    # the offsets mod 16 a naturally aligned operand can have; a 16 B-aligned type
    # has only 0, and is misaligned by 8 instead
    offs = [k * align for k in range(16 // align)] if align < 16 else [0, 8]
    count = 3001
    for k, (n, order) in enumerate(((2, "TREE"), (4, "TREE"), (8, "TREE"), (2, "CHAIN"), (3, "CHAIN"), (5, "CHAIN"),
                                    (8, "CHAIN"))):
        rng = np.random.default_rng(77 * n + k)
        xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
        want = _fold(orc, xs, count, dt, o, order)
        variants = [([offs[1]] * n, offs[0], False),                                     # all operands off the output
                    ([offs[-1] if j == n // 2 else 0 for j in range(n)], 0, False),      # one operand off
                    ([offs[(j + 1) % len(offs)] for j in range(n)], offs[0], False)]     # each at another offset
        if esz >= 2:
            variants.append(([1] * n, 1, False))                                         # unnatural, all alike
        if order == "CHAIN":
            variants.append(([offs[-1] if j == n - 1 else 0 for j in range(n)], 0, True))   # out == in[0]
        for ins, off_out, alias in variants:
            _run_fold(mpi, torch, xs, want, t, op, order, ins, off_out, path, alias)


# one pair per element size (16 B: the class of 8 B alignment, which may sit at offset 8 too)
VEC_PAIRS = [("MPI_BXOR", "MPI_UNSIGNED_CHAR"), ("MPI_SUM", "MPIX_C_FLOAT16"), ("MPI_SUM", "MPI_FLOAT"),
             ("MPI_MAX", "MPI_DOUBLE"), ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX")]


class _keep_min:
    """MPIR_Hip_set_keep_min_bytes(0) for the "sc1" runs: every result up to 64 MiB
    is then stored sc1 instead of nt."""

    def __init__(self, mpi, store):
        self.lib, self.on = mpi.load(), store == "sc1"

    def __enter__(self):
        self.prev = self.lib.MPIR_Hip_set_keep_min_bytes(0) if self.on else None

    def __exit__(self, *exc):
        if self.on:
            self.lib.MPIR_Hip_set_keep_min_bytes(self.prev)
        return False


@pytest.mark.parametrize("store", ["nt", "sc1"])
@pytest.mark.parametrize("op,t", VEC_PAIRS, ids=[f"{o}-{t}" for o, t in VEC_PAIRS])
def test_fused_vector_path_every_head_and_tail(mpi, orc, cuda, op, t, store):
    """The fused vector kernel (k_combine_multi) with every head size the type
    allows (operands and output alike at esz, 2 esz, ... < 16, and at 0) and
    every tail size, over one full tile and a ragged second one, on both kernel
    shapes (256 x 4 vectors: TREE4; 1024 x 1: CHAIN5); again with sc1 stores."""
    torch = cuda
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    per = 16 // esz
    base = (16384 + 5 * 16) // esz
    with _keep_min(mpi, store):
        for n, order in ((4, "TREE"), (5, "CHAIN")):
            rng = np.random.default_rng(n)
            full = [T.to_bytes(T.gen(t, base + per, rng, op)) for _ in range(n)]
            for extra in range(per):
                count = base + extra
                xs = [x[:count * esz] for x in full]
                want = _fold(orc, xs, count, dt, o, order)
                for off in range(0, 16, esz):
                    info = _run_fold(mpi, torch, xs, want, t, op, order, [off] * n, off, mpi.COMBINE_FUSED_VECTOR)
                    head = -off % 16 // esz
                    assert (info["nhead"], info["ntail"]) == (head, (count - head) % per), (off, count, info)


@pytest.mark.parametrize("store", ["nt", "sc1"])
@pytest.mark.parametrize("op,t", VEC_PAIRS, ids=[f"{o}-{t}" for o, t in VEC_PAIRS])
def test_fused_vector_path_tiny_counts(mpi, orc, cuda, op, t, store):
    """Counts smaller than the head (the head is clamped to the payload and the
    vector region is empty: a grid of one workgroup that only combines head
    elements), and exactly one vector with and without a head."""
    torch = cuda
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    per = 16 // esz
    with _keep_min(mpi, store):
        for n, order in ((2, "TREE"), (8, "TREE"), (3, "CHAIN"), (8, "CHAIN")):
            for count, off in sorted({(c, esz % 16) for c in (1, 2, per - 1) if c >= 1} | {(per, 0), (per, esz % 16)}):
                rng = np.random.default_rng([n, count, off])
                xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
                want = _fold(orc, xs, count, dt, o, order)
                info = _run_fold(mpi, torch, xs, want, t, op, order, [off] * n, off, mpi.COMBINE_FUSED_VECTOR)
                head = min(-off % 16 // esz, count)
                assert info["nhead"] == head and info["ntail"] == (count - head) % per, (count, off, info)


STRIDE_FOLDS = [("MPI_SUM", "MPI_FLOAT", "TREE", 4, ELEMS_STRIDE, 4, "elements"),
                ("MPI_SUM", "MPI_FLOAT", "CHAIN", 5, ELEMS_STRIDE, 4, "elements"),
                ("MPI_LAND", "MPI_INT", "CHAIN", 3, ANY_STRIDE, 0, "vector"),
                ("MPI_MINLOC", "MPI_2INT", "TREE", 16, ANY_STRIDE, 0, "any"),
                ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT", "CHAIN", 2, 2097152 + 4099, 0, "any")]


@pytest.mark.parametrize("op,t,order,n,count,off,path", STRIDE_FOLDS,
                         ids=[f"{o}-{t}-{r}{n}-{p}" for o, t, r, n, _, _, p in STRIDE_FOLDS])
def test_fold_grid_stride_loops_take_another_stride(mpi, orc, cuda, op, t, order, n, count, off, path):
    """The element-granular folds cap their grids (k_combine_multi_elems at 4096
    workgroups, k_combine_any at 8192): counts past two strides, operand 0 `off`
    bytes off the output for the fused fold's element kernel.  MPI_LAND over
    MPI_INT has a fused fold (reg_multi_logic.hip), so its CHAIN of 3 at this
    count runs the vector kernel, as the planner says; the CHAIN branch of
    k_combine_any is reached with a class that has no fused fold
    (MPI_LONG_DOUBLE_INT, one stride and a ragged second)."""
    torch = cuda
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    rng = np.random.default_rng(count + n)
    xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
    want = _fold(orc, xs, count, dt, o, order)
    want_path = {"elements": mpi.COMBINE_FUSED_ELEMENTS, "vector": mpi.COMBINE_FUSED_VECTOR, "any": mpi.COMBINE_ANY}[path]
    _run_fold(mpi, torch, xs, want, t, op, order, [off] + [0] * (n - 1), 0, want_path)


# ---------------------------------------------------------------------------
# MPIX_Reduce_local_multi on a caller's stream (stream=): the fold is enqueued
# and not waited for, so its operands may still be arriving on that stream and
# its result is complete only in that stream's order.  The device collectives
# launch every fold this way (csrc/host/coll_hip.c fold_combine).
# ---------------------------------------------------------------------------
STREAM_FOLDS = [("MPI_SUM", "MPI_FLOAT", "TREE", 4, [4, 4, 4, 4], 4, False, "vector"),       # one element past 16 B
                ("MPI_SUM", "MPI_FLOAT", "TREE", 4, [0, 0, 4, 0], 0, False, "elements"),     # one operand 4 B off
                ("MPI_MINLOC", "MPI_2INT", "TREE", 16, [0] * 16, 0, False, "any"),
                ("MPI_SUM", "MPIX_C_FLOAT16", "CHAIN", 11, [0] * 11, 0, True, "vector")]     # two passes, out == in[0]


def _fold_on_stream(mpi, torch, big, xs, t, op, order, offs, off_out, alias):
    """The fold with every operand's payload 0xA5 until a copy queued on the
    caller's stream -- behind slow work -- brings the data; the fold and the
    copy of the whole output allocation to pinned memory follow on that stream,
    which alone is synchronised.  Returns the output allocation's bytes."""
    esz = T.elem_size(t)
    nb = xs[0].size
    dev, pinned = [], [torch.from_numpy(x.copy()).pin_memory() for x in xs]
    for off in offs:
        d = torch.zeros(nb + off + 64, dtype=torch.uint8, device="cuda")
        d[off:off + nb] = 0xA5
        dev.append(d)
    out = dev[0] if alias else torch.zeros(nb + off_out + 64, dtype=torch.uint8, device="cuda")
    host = torch.zeros(out.numel(), dtype=torch.uint8).pin_memory()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(20):                 # as test_pinned_host_operand_ordered_after_null_stream
            big.mul_(1.0000001)
        for d, off, h in zip(dev, offs, pinned):
            d[off:off + nb].copy_(h, non_blocking=True)
        rc = mpi.reduce_local_multi([d.data_ptr() + off for d, off in zip(dev, offs)], out.data_ptr() + off_out,
                                    nb // esz, mpi.DATATYPES[t], mpi.OPS[op],
                                    mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN,
                                    stream=st.cuda_stream)
        assert rc == 0, mpi.error_string(rc)
        host.copy_(out, non_blocking=True)
    st.synchronize()
    return host.numpy().copy()


@pytest.mark.parametrize("op,t,order,n,offs,off_out,alias,path", STREAM_FOLDS,
                         ids=[f"{o}-{t}-{r}{n}-{p}" for o, t, r, n, _, _, _, p in STREAM_FOLDS])
def test_fold_on_a_callers_stream(mpi, orc, cuda, op, t, order, n, offs, off_out, alias, path):
    """The fused vector kernel, the fused element kernel, k_combine_any and a
    two-pass CHAIN into its own first operand with stream=: the operands are
    poison until the caller's stream delivers them, the result is read in that
    stream's order only (no null-stream operation in between).  Then the same
    under MPIR_Hip_combine_set_flags(MPIR_HIP_COMBINE_UNCAPPED): the same bytes,
    and the call returns the flags it replaced."""
    torch = cuda
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    count = 4099 + 3
    nb = count * esz
    rng = np.random.default_rng(n + count)
    xs = [T.to_bytes(T.gen(t, count, rng, op)) for _ in range(n)]
    want = _fold(orc, xs, count, dt, o, order)
    want_path = {"elements": mpi.COMBINE_FUSED_ELEMENTS, "vector": mpi.COMBINE_FUSED_VECTOR, "any": mpi.COMBINE_ANY}[path]
    a = 1 << 32                                     # (made-up 16 B-aligned addresses: never dereferenced)
    info = mpi.combine_plan_info([a + (j << 24) + off for j, off in enumerate(offs)],
                                 a + off_out + (0 if alias else 64 << 24), count, dt, o,
                                 mpi.MPIX_ORDER_TREE if order == "TREE" else mpi.MPIX_ORDER_CHAIN)
    assert info["path"] == want_path and info["passes"] == (2 if n == 11 else 1), info
    big = torch.ones(64 << 20, device="cuda")
    lib = mpi.load()
    UNCAPPED = 1                                    # MPIR_HIP_COMBINE_UNCAPPED (include/mpir_hip_reduce.h)
    runs = {}
    for flags in (0, UNCAPPED):
        prev = lib.MPIR_Hip_combine_set_flags(flags)
        try:
            assert prev == 0, "the thread's combine flags were left set"
            whole = _fold_on_stream(mpi, torch, big, xs, t, op, order, offs, off_out, alias)
        finally:
            assert lib.MPIR_Hip_combine_set_flags(prev) == flags        # round trip: what was set comes back
        assert lib.MPIR_Hip_combine_set_flags(0) == prev
        got = whole[off_out:off_out + nb]
        assert same(got, want, t), f"flags={flags}: {np.count_nonzero(got != want)} bytes differ"
        assert not whole[:off_out].any() and not whole[off_out + nb:].any(), f"flags={flags}: wrote outside the output"
        runs[flags] = whole
    assert np.array_equal(runs[0], runs[UNCAPPED]), "uncapped fold differs from the capped one"
