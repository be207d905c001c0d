"""MPIX_Reduce_local_batch on the GPU: one launch, many segments, each result
the oracle's MPI_Reduce_local on that segment (bit-exact, test_parity_gpu.same's
complex-NaN rule).

Every operand of every segment sits in an arena of its own, filled with 0xA5,
at a chosen byte phase of the 16 KiB grid the tile path lays over inoutbuf's
address (test_plan_edges_gpu.Arena).  After each call every payload must equal
the oracle's and every other byte of every arena must still be 0xA5: a
workgroup that found the wrong segment, a tile cut at the wrong byte or a head
or tail lane off by one all show there.  Before a batch runs,
MPIR_Hip_batch_plan_info -- the launch's own planner -- must report for each
segment the path it was built for.  Every batch runs twice: synchronously on
the library stream, and enqueued on a torch stream that is then synchronised.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import CASES, CASE_IDS, TILE, Arena

pytestmark = pytest.mark.gpu

EMPTY, TILEPATH, ELEMS, SINGLE = range(4)
WILD = 0x10                  # an empty segment's pointers: never looked at


class Seg:
    """One segment: its two arenas, its data and the oracle's result."""

    def __init__(self, mpi, orc, torch, op, t, n, phase_in, phase_io, kind, seed, ain=None):
        self.n, self.kind, self.t = n, kind, t
        self.what = f"{op} {t} n={n} in=+{phase_in} io=+{phase_io}"
        esz = T.elem_size(t)
        rng = np.random.default_rng(seed)
        self.a = T.to_bytes(T.gen(t, n, rng, op))                                    # inout
        self.b = ain.b[:n * esz] if ain else T.to_bytes(T.gen(t, n, rng, op))        # in
        self.want = self.a.copy()
        self.rc_oracle = orc.reduce_local(self.b.copy(), self.want, n, mpi.DATATYPES[t], mpi.OPS[op])
        self.aio = Arena(torch, n * esz + 4 * TILE)
        self.pio = self.aio.place(TILE + phase_io, self.a)
        if ain:                                     # a shared inbuf: the first reader's arena
            self.ain, self.pin = None, ain.pin
        else:
            self.ain = Arena(torch, n * esz + 4 * TILE)
            self.pin = self.ain.place(TILE + phase_in, self.b)

    def args(self):
        return (self.pin, self.pio, self.n)

    def check(self, way, want=None):
        want = self.want if want is None else want
        got = self.aio.check(f"{self.what} {way} inoutbuf")
        if self.ain:
            assert np.array_equal(self.ain.check(f"{self.what} {way} inbuf"), self.b), f"{self.what} {way}: inbuf modified"
        if not same(got, want, self.t):
            pytest.fail(f"{self.what} {way}:\n" + explain(got, want, self.a, self.b, T.elem_size(self.t)))


def run_batch(mpi, torch, op, t, segs, stream, expect_rc=0):
    """segs: Seg objects and None (an empty segment).  Asserts the planner's
    paths, then runs the batch both ways and checks every arena."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    args = [s.args() if s else (WILD, WILD + 4, 0) for s in segs]
    info = None
    if not expect_rc:                   # (a refused pair has no kernel, so no plan)
        info = mpi.batch_plan_info(args, dt, o)
        for s, kind, groups in zip(segs, info["seg_kind"], info["seg_groups"]):
            assert kind == (s.kind if s else EMPTY), \
                f"{s.what if s else 'empty'}: aimed at {s.kind if s else EMPTY}, the planner says {kind}"
            assert (groups >= 1) == bool(s)
    for way in ("sync", "stream"):
        if way == "stream":
            for s in segs:
                if s:
                    s.aio.restore(s.a)
        torch.cuda.synchronize()
        if way == "sync":
            rc = mpi.reduce_local_batch(args, dt, o)
        else:
            rc = mpi.reduce_local_batch(args, dt, o, stream.cuda_stream)
            stream.synchronize()
        assert mpi.error_class(rc) == expect_rc, f"{op} {t} {way}: {mpi.error_string(rc)}"
        for s in segs:
            if s:
                s.check(way, s.a if expect_rc else None)
    return info


def edge_specs(t, align):
    """(count, phase of inbuf, phase of inoutbuf, path) for the segments of the
    edge batch; phases are byte offsets from a 16 KiB boundary."""
    esz = T.elem_size(t)
    per = TILE // esz                       # the element path's run per workgroup
    out = []
    delta = esz % 16 or 8                   # inbuf at another offset mod 16
    if esz <= 16:
        maxtail = 16 - esz
        shifts = (0, 4096, TILE - 16)       # inbuf: the same phase mod 16, another mod 16 KiB
        k = 0
        for pio in sorted({0, 16, esz, TILE - 16, TILE - 16 + esz}):
            if pio % align:
                continue
            head = -pio % 16
            if head % esz:
                continue
            s = (pio + head) % TILE                          # the vector region's phase on the grid
            to_edge = TILE - s
            lens = [(to_edge, 0),                            # ends exactly on a grid boundary
                    (to_edge - 16 if to_edge > 16 else to_edge + TILE - 16, 0),     # 16 B before one
                    (to_edge + 16, 0),                       # 16 B after one
                    (to_edge + TILE, maxtail)]               # exactly two grid tiles and the largest tail
            if to_edge > 48:
                lens.append((48, 0))                         # wholly inside tile 0
            if esz < 16:
                lens += [(0, esz), (0, maxtail)]             # no vector region: head and tail only
            for v, tail in lens:
                n = (head + v + tail) // esz
                if n >= 1:
                    out.append((n, pio + shifts[k % 3], pio, TILEPATH))
                    k += 1
            out.append((1, pio + shifts[k % 3], pio, TILEPATH))                     # count 1
    else:
        for pin, pio in ((0, 0), (16, 16), (0, 16)):         # 16 B-aligned: still the element path
            for n in (1, per - 1, per, per + 1):
                out.append((n, pin, pio, ELEMS))
    # ---- element path: another offset mod 16; off natural alignment
    for pin, pio in ((delta, 0), (0, delta)):
        for n in (1, 5, 257, per - 1, per + 1):
            out.append((n, pin, pio, ELEMS))
    if align > 1:
        for pin, pio in ((1, 1), (3, 1)):
            for n in (1, 5, per + 1):
                out.append((n, pin, pio, ELEMS))
    return out


def placement(specs, t):
    """The edge batch's order: a five-tile segment between one-tile segments up
    front, empty segments at the first, a middle and the last position."""
    esz = T.elem_size(t)
    path = TILEPATH if esz <= 16 else ELEMS
    one, five = TILE // esz, 5 * TILE // esz
    front = [(one, 0, 0, path), (five, 4096, 0, path), (one, 0, 0, path)]
    mid = len(specs) // 2
    return [None] + front + specs[:mid] + [None] + specs[mid:] + [None]


@pytest.mark.parametrize("op,t,align", CASES, ids=CASE_IDS)
def test_batch_edges(mpi, orc, cuda, op, t, align):
    torch = cuda
    order = placement(edge_specs(t, align), t)
    segs = [Seg(mpi, orc, torch, op, t, *spec, seed=[i, spec[0]]) if spec else None for i, spec in enumerate(order)]
    info = run_batch(mpi, torch, op, t, segs, torch.cuda.Stream())
    assert info["empty"] == 3 and info["elems"] >= 10
    assert info["tile"] >= (20 if T.elem_size(t) < 16 else 3 if T.elem_size(t) == 16 else 0)
    assert info["launches"] == -(-(len(segs) - 3) // info["max_segs"])


@pytest.mark.parametrize("which", ["K-1", "K", "K+1", "2K+1"])
def test_launch_boundary(mpi, orc, cuda, which):
    """The argument table holds K segments: K - 1, K, K + 1 and 2K + 1 of them,
    with distinct data and mixed counts and paths, across one, two and three launches."""
    torch = cuda
    op, t = "MPI_SUM", "MPI_FLOAT"
    K = mpi.batch_plan_info([], mpi.DATATYPES[t], mpi.OPS[op])["max_segs"]
    n = {"K-1": K - 1, "K": K, "K+1": K + 1, "2K+1": 2 * K + 1}[which]
    counts = np.random.default_rng(n).integers(1, 701, n).tolist()
    counts[0], counts[-1], counts[n // 2] = 1, 700, 700
    segs = []
    for i, c in enumerate(counts):
        pio = (0, 4, 16, TILE - 16, TILE - 8)[i % 5]
        tile = i % 4 != 3                               # every fourth segment: inbuf 4 B off, the element path
        segs.append(Seg(mpi, orc, torch, op, t, c, pio + (2048 if tile else 4), pio, TILEPATH if tile else ELEMS,
                        seed=[n, i]))
    info = run_batch(mpi, torch, op, t, segs, torch.cuda.Stream())
    assert info["launches"] == -(-n // K) and info["max_segs"] == K


@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_batch_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, through a
    three-segment batch: the tile path with head and tail, the element path,
    and count 1.  What the reference's compute switch refuses (LAND / LOR on
    floating types) the batch refuses with the same class, writing nothing."""
    torch = cuda
    esz = T.elem_size(t)
    vec = max(16 // esz, 1)
    pio = esz if esz < 16 else 0            # head elements where the type has any
    path = TILEPATH if esz <= 16 else ELEMS
    delta = esz % 16 or 8
    # below 16 B: vec - 1 head elements, one tile and a vector of whole vectors, one tail element
    specs = [((vec - 1) + TILE // esz + vec + 1 if esz < 16 else TILE // esz + 3, pio + 4096, pio, path),
             (1000, delta, 0, ELEMS),
             (1, 32, 32, path)]
    segs = [Seg(mpi, orc, torch, op, t, *spec, seed=[7, i]) for i, spec in enumerate(specs)]
    if esz < 16:
        single = mpi.plan_info(*segs[0].args(), mpi.DATATYPES[t], mpi.OPS[op]) if T.compute_ok(op, t) else None
        assert single is None or (single["nhead"] >= 1 and single["ntail"] >= 1), single
    rcs = {s.rc_oracle for s in segs}
    assert len(rcs) == 1
    run_batch(mpi, torch, op, t, segs, torch.cuda.Stream(), expect_rc=rcs.pop())


def test_shared_input(mpi, orc, cuda):
    """16 segments reading one inbuf (segments may share or overlap inputs)."""
    torch = cuda
    op, t = "MPI_SUM", "MPI_FLOAT"
    first = Seg(mpi, orc, torch, op, t, 6000, 0, 0, TILEPATH, seed=[16, 0])
    segs = [first]
    for i in range(1, 16):
        pio = (0, 16, 4, TILE - 16)[i % 4]              # 4: inoutbuf at another offset mod 16 than the shared inbuf
        segs.append(Seg(mpi, orc, torch, op, t, 6000 - 37 * i, 0, pio, ELEMS if pio == 4 else TILEPATH, seed=[16, i],
                        ain=first))
    run_batch(mpi, torch, op, t, segs, torch.cuda.Stream())


@pytest.mark.parametrize("phase_in,n", [(0, 100000), (4, 100000), (4, 3)], ids=["tile", "shift", "elems"])
def test_one_segment_is_the_single_call(mpi, orc, cuda, phase_in, n):
    """A batch with exactly one non-empty segment goes through MPIR_Hip_reduce:
    the same result, and synchronously the direct AQL dispatch where it is up."""
    torch = cuda
    lib = mpi.load()
    lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
    op, t = "MPI_SUM", "MPI_FLOAT"
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    state = lib.MPIR_Hip_direct_prepare(torch.cuda.current_device())
    s = Seg(mpi, orc, torch, op, t, n, phase_in, 0, SINGLE, seed=[1, n])
    args = [(WILD, WILD, 0), s.args(), (WILD, WILD, 0)]
    assert mpi.batch_plan_info(args, dt, o)["seg_kind"] == [EMPTY, SINGLE, EMPTY]
    torch.cuda.synchronize()
    assert mpi.reduce_local(*s.args(), dt, o) == 0
    s.check("MPI_Reduce_local")
    single = s.aio.check("single")
    stream = torch.cuda.Stream()
    for way in ("sync", "stream"):
        s.aio.restore(s.a)
        torch.cuda.synchronize()
        d0 = lib.MPIR_Hip_direct_dispatches()
        rc = mpi.reduce_local_batch(args, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert rc == 0, mpi.error_string(rc)
        d1 = lib.MPIR_Hip_direct_dispatches()
        assert np.array_equal(s.aio.check(way), single), f"{way}: differs from MPI_Reduce_local"
        s.check(way)
        if state == 1:
            assert d1 - d0 == (1 if way == "sync" else 0), f"{way}: direct dispatches {d1 - d0}"


def test_no_partial_work(mpi, orc, cuda):
    """Everything is classified before the first launch: a host inbuf in the last
    segment of three launches' worth fails the call with nothing written."""
    torch = cuda
    op, t = "MPI_SUM", "MPI_FLOAT"
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    K = mpi.batch_plan_info([], dt, o)["max_segs"]
    segs = [Seg(mpi, orc, torch, op, t, 100 + i, 0, 0, TILEPATH, seed=[3, i]) for i in range(2 * K + 2)]
    host_in = np.ones(64, dtype=np.float32)
    last = Seg(mpi, orc, torch, op, t, 64, 0, 0, TILEPATH, seed=[3, 9999])
    args = [s.args() for s in segs] + [(host_in.ctypes.data, last.pio, 64)]
    stream = torch.cuda.Stream()
    for way in ("sync", "stream"):
        torch.cuda.synchronize()
        rc = mpi.reduce_local_batch(args, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
        assert "device-resident" in mpi.error_string(rc)
        for s in segs + [last]:
            s.check(way, s.a)
    # the same batch without the host pointer runs
    assert mpi.reduce_local_batch(args[:-1] + [last.args()], dt, o) == 0
    for s in segs + [last]:
        s.check("all device")
