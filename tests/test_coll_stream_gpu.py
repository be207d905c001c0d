"""The device collectives on a caller's stream (a non-NULL hip_stream), on one GPU.

With a caller's stream a collective never synchronises with the host
(coll_hip.c coll_end): its input may still be in flight on that stream when the
call is made, its result is complete only in that stream's order, and the next
call on the stream starts while this one runs.  Every case here, per rank (a
loopback communicator: one host thread and one torch.cuda.Stream per rank):
  1. the send buffer starts as 0xA5 poison;
  2. slow work is queued on the rank's stream (as much as
     test_pinned_host_operand_ordered_after_null_stream queues; not asserted on);
  3. the real input is copied into the send buffer on that stream;
  4. the collective is called with that stream's handle;
  5. the result is copied to pinned host memory on the same stream;
  6. that stream alone is synchronised.
Nothing between 4 and the comparison touches the null stream (no
torch.cuda.synchronize(), no .cpu()): the communicator's own streams are
blocking streams, and a null-stream operation would wait for them and hide a
missing join.  A step that ran on another stream than the caller's reads the
poison; a missing join of the fold stream leaves stale bytes in the result.
Expected bytes: oracle/schedules.py, as in test_coll_loopback_gpu.py; reference
order; bit-exact.

What this does not prove: the loopback transport synchronises the call's
stream inside every exchange (coll_hip.c group_exchange), so a missing wait
between an exchange and a fold, or between two calls, cannot show on one GPU.
These cases prove the stream plumbing (every step on the caller's stream or
joined to it) and the reuse of the scratch and the events from call to call;
tests/test_coll_order_cpu.py proves the ordering itself from the logged call
sequence, and test_coll_rccl_gpu.py runs a back-to-back pair over RCCL where
more than one GPU is visible.
"""
import numpy as np
import pytest

import _types as T
from test_coll_loopback_gpu import _pipe_counts, run_ranks
from test_parity_gpu import same

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 64
LONG = (1 << 16) + 5
TYPES = [("MPI_FLOAT", "MPI_SUM"), ("MPIX_C_FLOAT16", "MPI_SUM")]
KINDS = ["allreduce", "reduce", "reduce_scatter_block", "reduce_scatter", "scan", "exscan"]


@pytest.fixture(scope="module")
def slow(cuda):
    """What the slow work runs over: 64 Mi floats."""
    big = cuda.ones(64 << 20, device="cuda")
    cuda.cuda.synchronize()
    yield big
    del big


def queue_slow_work(big):
    for _ in range(20):
        big.mul_(1.0000001)


class Bufs:
    """One rank's buffers of one call: the input in pinned memory, the poisoned
    device buffers, and the pinned copy of everything behind recvbuf."""

    def __init__(self, torch, x, recv_bytes, inplace, has_recv=True):
        self.inplace = inplace
        self.hin = torch.from_numpy(x.copy()).pin_memory()
        self.send = torch.full((x.size,), POISON, dtype=torch.uint8, device="cuda")
        # in place the input goes into recvbuf; out of place recvbuf is poison with a guard behind it
        self.recv = None
        if has_recv:
            self.recv = self.send if inplace else torch.full((recv_bytes + GUARD,), POISON, dtype=torch.uint8,
                                                             device="cuda")
            self.hout = torch.zeros(self.recv.numel(), dtype=torch.uint8).pin_memory()

    def stage_input(self):
        self.send.copy_(self.hin, non_blocking=True)

    def sendbuf(self, mpi):
        return mpi.MPI_IN_PLACE if self.inplace else self.send.data_ptr()

    def copy_out(self):
        if self.recv is not None:
            self.hout.copy_(self.recv, non_blocking=True)

    def result(self, nbytes):
        """The first nbytes of recvbuf; out of place, the guard behind them is checked."""
        got = self.hout.numpy()
        if not self.inplace:
            assert (got[nbytes:] == POISON).all(), "wrote behind recvbuf"
        return got[:nbytes]


def run_on_streams(torch, big, p, bufs, call):
    """Steps 2-6 of the module docstring on every rank; call(r, stream handle)
    issues rank r's collective(s) and returns nothing."""
    streams = [torch.cuda.Stream() for _ in range(p)]
    torch.cuda.synchronize()                # the poison is in place before any rank starts

    def rank(r):
        st = streams[r]
        with torch.cuda.stream(st):
            queue_slow_work(big)
            for b in bufs[r]:
                b.stage_input()
            call(r, st.cuda_stream)
            for b in bufs[r]:
                b.copy_out()
        st.synchronize()

    run_ranks(rank, p)


def ok(mpi, rc):
    assert rc == 0, mpi.error_string(rc)


def one_collective(mpi, torch, big, comms, kind, t, op, count, inplace, root=0, counts=None):
    """One call of `kind` on every rank's stream, compared with the oracle."""
    from oracle import schedules as S
    p = len(comms)
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    REF = mpi.MPIX_HIP_ALG_REFERENCE_ORDER
    rng = np.random.default_rng([p, count, len(kind), esz])
    if kind == "reduce_scatter_block":
        counts = [count] * p
    n = sum(counts) if counts else count
    xs = [T.to_bytes(T.gen(t, n, rng, op)) for _ in range(p)]
    if kind == "allreduce":
        want = [S.allreduce_smp_auto(xs, count, esz, dt, o) if p > 1 else xs[0]] * p
    elif kind == "reduce":
        want = {root: S.reduce_auto(xs, count, esz, dt, o, root) if p > 1 else xs[0]}
    elif kind == "reduce_scatter_block":
        want = S.reduce_scatter_block_auto(xs, count, esz, dt, o)
    elif kind == "reduce_scatter":
        want = S.reduce_scatter_auto(xs, counts, esz, dt, o)
    elif kind == "scan":
        want = S.scan_recursive_doubling(xs, count, esz, dt, o)
    else:
        want = S.exscan_recursive_doubling(xs, count, esz, dt, o)
    out_bytes = [(counts[r] if counts else count) * esz for r in range(p)]
    bufs = []
    for r in range(p):
        if kind == "reduce":        # MPI_IN_PLACE at the root only; no recvbuf elsewhere
            bufs.append([Bufs(torch, xs[r], out_bytes[r], inplace and r == root, has_recv=r == root)])
        else:
            bufs.append([Bufs(torch, xs[r], out_bytes[r], inplace)])

    def call(r, stream):
        b = bufs[r][0]
        sb, rb = b.sendbuf(mpi), b.recv.data_ptr() if b.recv is not None else 0
        if kind == "allreduce":
            ok(mpi, mpi.allreduce(sb, rb, count, dt, o, comms[r], REF, stream))
        elif kind == "reduce":
            ok(mpi, mpi.reduce(sb, rb, count, dt, o, root, comms[r], REF, stream))
        elif kind == "reduce_scatter_block":
            ok(mpi, mpi.reduce_scatter_block(sb, rb, count, dt, o, comms[r], REF, stream))
        elif kind == "reduce_scatter":
            ok(mpi, mpi.reduce_scatter(sb, rb, counts, dt, o, comms[r], REF, stream))
        else:
            ok(mpi, (mpi.scan if kind == "scan" else mpi.exscan)(sb, rb, count, dt, o, comms[r], REF, stream))

    run_on_streams(torch, big, p, bufs, call)
    what = f"{kind} {t} p={p} count={counts or count} inplace={inplace} root={root}"
    for r in range(p):
        b = bufs[r][0]
        if kind == "reduce" and r != root:
            continue
        if kind == "exscan" and r == 0:         # rank 0's recvbuf stays as it was
            before = xs[0] if inplace else np.full(out_bytes[0], POISON, np.uint8)
            assert np.array_equal(b.result(out_bytes[0]), before), f"{what}: exscan wrote rank 0's recvbuf"
            continue
        got = b.result(out_bytes[r])
        assert same(got, want[r], t), f"{what} rank {r}: {np.count_nonzero(got != want[r])} bytes differ"
    for r in range(p):                          # (after every comparison) the sendbuf is read-only
        b = bufs[r][0]
        if not b.inplace:
            assert torch.equal(b.send.cpu(), b.hin), f"{what} rank {r}: sendbuf modified"


@pytest.mark.parametrize("t,op", TYPES, ids=[t for t, _ in TYPES])
@pytest.mark.parametrize("p", [2, 3, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_collective_on_a_callers_stream(mpi, orc, cuda, slow, kind, p, t, op):
    """All six entry points, short (count 3: one exchange and a fold) and long
    ((1 << 16) + 5, per rank for the reduce-scatters), out of place and in
    place, Reduce at roots 0 and p - 1.  (The long count first: a call that
    finds the scratch too small frees it behind a hipDeviceSynchronize, which
    would deliver the input before anything of the call is queued.)"""
    comms = mpi.comm_create_loopback(p)
    try:
        for count in (LONG, 3):
            # Reduce_scatter: counts around `count`, not all alike
            counts = [count + (q % 3) for q in range(p)] if kind == "reduce_scatter" else None
            for inplace in (False, True):
                for root in ((0, p - 1) if kind == "reduce" else (0,)):
                    one_collective(mpi, cuda, slow, comms, kind, t, op, count, inplace, root, counts)
    finally:
        for c in comms:
            mpi.comm_free(c)


@pytest.mark.parametrize("t,op", TYPES, ids=[t for t, _ in TYPES])
@pytest.mark.parametrize("p", [2, 3, 8])
@pytest.mark.parametrize("kind", ["allreduce", "reduce", "reduce_scatter_block", "reduce_scatter"])
def test_pipelined_collective_on_a_callers_stream(mpi, orc, cuda, slow, kind, p, t, op, monkeypatch):
    """The schedules that fold on the communicator's second stream
    (MPIR_CVAR_DEVICE_COLL_PIPELINE_KB=64: several chunks at these sizes), whose
    last fold the caller's stream has to join before the copy out."""
    monkeypatch.setenv("MPIR_CVAR_DEVICE_COLL_PIPELINE_KB", "64")
    esz = T.elem_size(t)
    comms = mpi.comm_create_loopback(p)
    try:
        count = (1 << 17) + 5 if kind == "reduce_scatter_block" else (1 << 19) + 7
        # (_pipe_counts is defined for 3 and 8 ranks; at 2: a short block and a long one)
        counts = None if kind != "reduce_scatter" else \
            [5000 * (4 // esz), 160003 * (4 // esz)] if p == 2 else _pipe_counts(p, esz)
        for inplace in (False, True):
            for root in ((0, p - 1) if kind == "reduce" else (0,)):
                one_collective(mpi, cuda, slow, comms, kind, t, op, count, inplace, root, counts)
    finally:
        for c in comms:
            mpi.comm_free(c)


@pytest.mark.parametrize("kb", ["0", "64"], ids=["unpipelined", "pipelined"])
@pytest.mark.parametrize("p", [3, 8])
def test_chain_of_collectives_on_one_stream(mpi, orc, cuda, slow, p, kb, monkeypatch):
    """Four collectives in a row on each rank's stream with no host
    synchronisation between them, each reading what the one before wrote:
    Allreduce x -> a; Exscan of a in place; Reduce_scatter_block from a into b;
    Reduce of b to root p - 1.  Only a and the root's result come back.  The
    calls share the communicator's scratch and (pipelined) its fold stream and
    events.  Expected: the oracle's schedules composed on the CPU."""
    from oracle import schedules as S
    monkeypatch.setenv("MPIR_CVAR_DEVICE_COLL_PIPELINE_KB", kb)
    torch = cuda
    t, op, esz = "MPI_FLOAT", "MPI_SUM", 4
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    REF = mpi.MPIX_HIP_ALG_REFERENCE_ORDER
    n = (1 << 19) + 7
    rc_ = n // p                   # the Reduce_scatter_block's recvcount: p blocks fit in a
    root = p - 1
    rng = np.random.default_rng(1000 + p)
    xs = [T.to_bytes(T.gen(t, n, rng, op)) for _ in range(p)]
    a_all = S.allreduce_smp_auto(xs, n, esz, dt, o)
    ex = S.exscan_recursive_doubling([a_all.copy() for _ in range(p)], n, esz, dt, o)
    a_want = [a_all if r == 0 else ex[r] for r in range(p)]
    b_want = S.reduce_scatter_block_auto([a[:p * rc_ * esz].copy() for a in a_want], rc_, esz, dt, o)
    c_want = S.reduce_auto([b.copy() for b in b_want], rc_, esz, dt, o, root)

    comms = mpi.comm_create_loopback(p)
    try:
        hin = [torch.from_numpy(x.copy()).pin_memory() for x in xs]
        x_dev = [torch.full((n * esz,), POISON, dtype=torch.uint8, device="cuda") for _ in range(p)]
        a_dev = [torch.full((n * esz + GUARD,), POISON, dtype=torch.uint8, device="cuda") for _ in range(p)]
        b_dev = [torch.full((rc_ * esz + GUARD,), POISON, dtype=torch.uint8, device="cuda") for _ in range(p)]
        c_dev = torch.full((rc_ * esz + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        a_out = [torch.zeros(n * esz + GUARD, dtype=torch.uint8).pin_memory() for _ in range(p)]
        c_out = torch.zeros(rc_ * esz + GUARD, dtype=torch.uint8).pin_memory()
        streams = [torch.cuda.Stream() for _ in range(p)]

        def chain(r, s):
            ok(mpi, mpi.allreduce(x_dev[r].data_ptr(), a_dev[r].data_ptr(), n, dt, o, comms[r], REF, s))
            ok(mpi, mpi.exscan(mpi.MPI_IN_PLACE, a_dev[r].data_ptr(), n, dt, o, comms[r], REF, s))
            ok(mpi, mpi.reduce_scatter_block(a_dev[r].data_ptr(), b_dev[r].data_ptr(), rc_, dt, o, comms[r], REF, s))
            ok(mpi, mpi.reduce(b_dev[r].data_ptr(), c_dev.data_ptr() if r == root else 0, rc_, dt, o, root,
                               comms[r], REF, s))

        # once on the communicator's own stream, over the poison: the scratch is
        # grown to what the chain needs, so that no call of the chain proper
        # frees it (behind a hipDeviceSynchronize, which would order everything)
        run_ranks(lambda r: chain(r, 0), p)
        for d in x_dev + a_dev + b_dev + [c_dev]:
            d.fill_(POISON)
        torch.cuda.synchronize()

        def rank(r):
            st = streams[r]
            with torch.cuda.stream(st):
                queue_slow_work(slow)
                x_dev[r].copy_(hin[r], non_blocking=True)
                chain(r, st.cuda_stream)
                a_out[r].copy_(a_dev[r], non_blocking=True)
                if r == root:
                    c_out.copy_(c_dev, non_blocking=True)
            st.synchronize()

        run_ranks(rank, p)
        for r in range(p):
            got = a_out[r].numpy()
            assert same(got[:n * esz], a_want[r], t), f"a on rank {r}: {np.count_nonzero(got[:n * esz] != a_want[r])}"
            assert (got[n * esz:] == POISON).all(), f"rank {r}: wrote behind a"
        got = c_out.numpy()
        assert same(got[:rc_ * esz], c_want, t), f"root: {np.count_nonzero(got[:rc_ * esz] != c_want)} bytes differ"
        assert (got[rc_ * esz:] == POISON).all(), "wrote behind the root's recvbuf"
    finally:
        for c in comms:
            mpi.comm_free(c)
