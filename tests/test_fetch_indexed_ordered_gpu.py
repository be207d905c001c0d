"""MPIX_Reduce_local_fetch_indexed_ordered on the GPU: the ordered indexed
reduction that also hands out, in block k of a packed fetchbuf, what block k's
target held just before contribution k.

Expected values come from the oracle: per distinct target, k in table order, the
row copied into fetch_want[k], then MPI_Reduce_local of input block k into the
row (MPI_NO_OP and MPI_REPLACE in numpy).  The arenas are test_indexed_gpu's,
fetchbuf a third one: prefilled with the complement of what it should receive,
0xA5 around it.  After each call every distinct target must equal the oracle's
row, every block of fetchbuf the oracle's bytes -- the first block of every run
byte-equal to the old target, later ones under test_parity_gpu.same's complex-NaN
rule -- every guard byte of all three arenas must still be 0xA5, and the input
arena and the tables must be unchanged.  Before a shape runs the call's own
planner must report the form the shape aims at.  Every shape runs three ways:
synchronously with device tables, on a torch stream with device tables, and
synchronously with host tables.

Every address a kernel forms here stays inside its arena.
"""
import numpy as np
import pytest

import _types as T
from test_indexed_gpu import Arena, slots, threshold
from test_indexed_ordered_gpu import TYPES, build_orders, repeated, shape1
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import TILE

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
FORMS = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
WAYS = ("sync", "stream", "host-tables")
BYTE_OPS = ("MPI_NO_OP", "MPI_REPLACE")


def oracle_fetch(orc, a, b, src, dst, nb, bl, dt, op, o):
    """a's rows (one per distinct target) after blocks 0 .. nb - 1 in that order,
    what each block's target held just before it, and the class returned"""
    want = a.copy()
    fetch = np.empty((nb, a.shape[1]), np.uint8)
    rcs = set()
    for k in range(nb):
        fetch[k] = want[dst[k]]
        if op == "MPI_REPLACE":
            want[dst[k]] = b[src[k]]
        elif op != "MPI_NO_OP":
            rcs.add(orc.reduce_local(b[src[k]].copy(), want[dst[k]], bl, dt, o))
    assert len(rcs) <= 1
    return want, fetch, (rcs.pop() if rcs else 0)


def heads(dst):
    """is block k the first of its target's run?"""
    seen = set()
    return np.array([not (d in seen or seen.add(d)) for d in dst.tolist()])


class Case:
    """Operands of one shape: arenas, tables, expected rows and fetched blocks."""

    def __init__(self, mpi, orc, torch, stream, op, t, nb, bl, unit, tin, tio, pin, pio, pfe, seed, order=True):
        self.mpi, self.torch, self.stream, self.op, self.t = mpi, torch, stream, op, t
        self.dt, self.o = mpi.DATATYPES[t], getattr(mpi, op)
        self.nb, self.bl, self.unit = nb, bl, unit
        self.esz = T.elem_size(t)
        rb = self.rb = bl * self.esz
        rng = np.random.default_rng([seed, nb, bl])
        self.tio = tio = np.ascontiguousarray(tio, dtype=np.int64)
        off_in = np.arange(nb, dtype=np.int64) * rb if tin is None else np.asarray(tin, np.int64) * unit
        uin, self.src = np.unique(off_in, return_inverse=True)
        self.uio, self.dst = np.unique(tio * unit, return_inverse=True)
        gop = "MPI_SUM" if op in BYTE_OPS else op
        self.a = T.to_bytes(T.gen(t, len(self.uio) * bl, rng, gop)).reshape(len(self.uio), rb)
        self.b = T.to_bytes(T.gen(t, len(uin) * bl, rng, gop)).reshape(len(uin), rb)
        self.want, self.fwant, self.rc_want = oracle_fetch(orc, self.a, self.b, self.src, self.dst, nb, bl, self.dt, op, self.o)
        self.what = f"{op} {t} {nb} x {bl} onto {len(self.uio)} unit {unit} in=+{pin} io=+{pio} fetch=+{pfe}"
        self.ain, self.aio = Arena(torch, self.b, uin, pin), Arena(torch, self.a, self.uio, pio)
        self.afe = Arena(torch, ~self.fwant, np.arange(nb, dtype=np.int64) * rb, pfe)
        self.host = [None if tin is None else np.ascontiguousarray(tin, dtype=np.int64), tio]
        self.devt = [None if x is None else torch.from_numpy(x).cuda() for x in self.host]
        self.dptr = [0 if x is None else x.data_ptr() for x in self.devt]
        self.dorder = self.horder = None
        if order:
            self.dorder, self.horder = build_orders(mpi, torch, stream, tio, self.devt[1], self.what)
        no_op = op == "MPI_NO_OP"
        self.pin = 0 if no_op else self.ain.ptr         # MPI_NO_OP: inbuf is passed as 0

    def tables(self, way):
        if way == "host-tables":
            return self.host + [self.horder]
        return self.dptr + [None if self.dorder is None else self.dorder.data_ptr()]

    def plan(self, form, expect=None):
        m = self.mpi
        if self.rc_want:
            return None
        info = m.fetch_indexed_ordered_plan_info(self.pin, self.dptr[0], self.aio.ptr, self.dptr[1], self.afe.ptr,
                                                 None if self.dorder is None else self.dorder.data_ptr(), self.unit, self.nb,
                                                 self.bl, self.dt, self.o)
        assert info["form"] == form, f"{self.what}: aimed at {FORMS[form]}, the planner says {info}"
        if expect:
            expect(info, self.tio if self.horder is None else self.tio[self.horder])
        return info

    def call(self, way):
        tabs = self.tables(way)
        self.torch.cuda.synchronize()
        rc = self.mpi.reduce_local_fetch_indexed_ordered(self.pin, tabs[0], self.aio.ptr, tabs[1], self.afe.ptr, tabs[2],
                                                         self.unit, self.nb, self.bl, self.dt, self.o,
                                                         self.stream.cuda_stream if way == "stream" else 0)
        self.stream.synchronize()
        return rc

    def reset(self):
        self.aio.upload()
        self.afe.upload()

    def check(self, way, want=None, fwant=None):
        """both outputs against the oracle; returns (rows, fetched blocks)"""
        want = self.want if want is None else want
        fwant = self.fwant if fwant is None else fwant
        what = f"{self.what} {way}"
        got = self.aio.check(f"{what} inoutbuf")
        fgot = self.afe.check(f"{what} fetchbuf")
        assert np.array_equal(self.ain.check(f"{what} inbuf"), self.b), f"{what}: inbuf modified"
        if self.rc_want:
            assert np.array_equal(got, self.a) and np.array_equal(fgot, ~self.fwant), f"{what}: a refused call wrote"
            return got, fgot
        # the first block of a run is a byte copy of the old target; later ones follow same()'s rule
        first = heads(self.dst)
        for k in range(0 if not np.array_equal(fgot, fwant) else self.nb, self.nb):
            if not (np.array_equal(fgot[k], fwant[k]) if first[k] else same(fgot[k], fwant[k], self.t)):
                ks = np.nonzero(self.dst == self.dst[k])[0]
                pytest.fail(f"{what} fetchbuf block {k} (its target's blocks: {ks.tolist()[:20]}):\n" +
                            explain(fgot[k], fwant[k], self.a[self.dst[k]], self.b[self.src[k]], self.esz))
        for j in range(0 if not np.array_equal(got, want) else len(self.uio), len(self.uio)):
            if not same(got[j], want[j], self.t):
                ks = np.nonzero(self.dst == j)[0]
                pytest.fail(f"{what} target {j}, blocks {ks.tolist()[:20]}:\n" +
                            explain(got[j], want[j], self.a[j], self.b[self.src[ks[-1]]], self.esz))
        return got, fgot

    def tables_unchanged(self):
        for x, h in zip(self.devt + [self.dorder], self.host + [self.horder]):
            if x is not None:
                assert np.array_equal(x.cpu().numpy(), h), f"{self.what}: a table was written"


def run(mpi, orc, torch, stream, op, t, nb, bl, unit, tin, tio, pin, pio, pfe, form, seed=0, expect=None, ways=WAYS,
        tell_apart=False):
    """One shape every way.  Returns the case (its last outputs still in the arenas)."""
    c = Case(mpi, orc, torch, stream, op, t, nb, bl, unit, tin, tio, pin, pio, pfe, seed)
    if tell_apart:
        # in every run of two or more, consecutive fetched blocks differ: a fetch that stored
        # the head's value throughout, or stored after the combine, shows in this data
        for j in range(len(c.uio)):
            ks = np.nonzero(c.dst == j)[0]
            for k0, k1 in zip(ks[:-1], ks[1:]):
                assert not np.array_equal(c.fwant[k0], c.fwant[k1]), f"{c.what}: blocks {k0} and {k1} fetch the same bytes"
            assert not np.array_equal(c.fwant[ks[-1]], c.want[j]), f"{c.what}: the last fetch of target {j} is its end value"
        # ... and the order of application: descending k gives other target bits
        back = c.a.copy()
        for k in range(nb - 1, -1, -1):
            orc.reduce_local(c.b[c.src[k]].copy(), back[c.dst[k]], bl, c.dt, c.o)
        assert not np.array_equal(back, c.want), f"{c.what}: the order of application does not show in this data"
    c.plan(form, expect)
    for n, way in enumerate(ways):
        if n:
            c.reset()
        rc = c.call(way)
        assert mpi.error_class(rc) == c.rc_want, f"{c.what} {way}: {mpi.error_string(rc)}"
        c.check(way)
    c.tables_unchanged()
    return c


# ---------------------------------------------------------------- 1. narrow vectors
@pytest.mark.parametrize("t", ["MPI_FLOAT", "MPIX_C_FLOAT16"])
def test_narrow_vectors_runs_across_a_workgroup_boundary(mpi, orc, cuda, t):
    """400 blocks of 48 bytes onto 37 slots: two workgroups, the run at sorted
    position 341 in both."""
    bl = 48 // T.elem_size(t)
    assert 48 < threshold(mpi, t)

    def two(info, sorted_displs):
        assert info["groups"] == 2 and info["launches"] == 1, info
        assert sorted_displs[340] == sorted_displs[341] or sorted_displs[341] == sorted_displs[342]
        assert len(np.unique(sorted_displs)) == 37

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", t, 400, bl, 16, None, shape1(16), 16, 32, 48, NARROW_VEC, seed=1,
        expect=two, tell_apart=True)


# ---------------------------------------------------------------- 2. element forms
def test_narrow_elements(mpi, orc, cuda):
    """disp_unit 4 and the base 4 bytes off: 4800 elements, 4096 a workgroup, the
    boundary inside a block and inside a run."""

    def two(info, sorted_displs):
        assert info["groups"] == 2 and 4096 % 12, info
        assert sorted_displs[340] == sorted_displs[341] or sorted_displs[341] == sorted_displs[342]

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 400, 12, 4, None, shape1(4), 16, 36, 16, NARROW_ELEMS,
        seed=2, expect=two, tell_apart=True)


def test_fetchbuf_alignment_alone_decides_the_form(mpi, orc, cuda):
    """Everything 16-aligned but fetchbuf 4 bytes off: the element form; the same
    operands with fetchbuf aligned: vectors."""
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 400, 12, 16, None, shape1(16, seed=3), 16, 32, 4, NARROW_ELEMS, seed=3)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 400, 12, 16, None, shape1(16, seed=3), 16, 32, 0, NARROW_VEC, seed=3)


# ---------------------------------------------------------------- 3. wide blocks
def wide_shape(mpi, unit):
    bl = threshold(mpi) // 4 + TILE // 4 + 3
    assert bl * 4 >= threshold(mpi) and (bl * 4) % 16
    far = (bl + 5) * 4 // unit + (1 if unit == 1 else 0)
    return bl, far, np.array([0, far, 0, far, 0], dtype=np.int64)


@pytest.mark.parametrize("unit,pio,pfe", [(4, 4, 4), (4, 4, 8), (1, 1, 3)],
                         ids=["fetch-at-target-phase", "fetch-4-off", "target-off-alignment"])
def test_wide_runs_of_three_and_two(mpi, orc, cuda, unit, pio, pfe):
    """5 blocks of several tiles with a ragged end onto 2 targets (k = 0, 2, 4 and
    k = 1, 3), bases off the tile grid.  Packed fetch blocks of this length sit
    at varying phases mod 16, so one run takes the descriptor stores for some
    blocks and the element stores for others; with byte displacements and an odd
    base the targets are off their alignment: the element form."""
    bl, far, tio = wide_shape(mpi, unit)
    if unit == 4:
        # does block k of fetch share its target's phase mod 16?  Block 0 as the case says, and both answers occur
        shares = [(pfe + k * bl * 4) % 16 == (pio + int(tio[k]) * 4) % 16 for k in range(5)]
        assert shares[0] == (pfe == pio) and len(set(shares)) == 2, shares

    def runs(info, sorted_displs):
        assert info["groups"] == 5 * info["per"] and info["per"] >= -(-bl * 4 // TILE), info
        assert sorted_displs.tolist() == [0, 0, 0, far, far]

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 5, bl, unit, None, tio, 4, pio, pfe, WIDE, seed=4,
        expect=runs, tell_apart=True)


# ---------------------------------------------------------------- 4. edges of the run loop
@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_run_loop_edges(mpi, orc, cuda, unit, form):
    """One run from position 0 to the table's end (fetchbuf an exclusive prefix
    scan); no repeats at all (byte-equal to the fetching ragged call with uniform
    starts); runs of one between runs of five; one block; and order NULL on a
    table whose equal entries are adjacent (equal to the call with the built order)."""
    stream = cuda.cuda.Stream()
    pio = 32 if unit == 16 else 36
    k = 64 // unit
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 300, 12, unit, None, np.full(300, 5 * k, np.int64), 16, pio, 16, form,
        seed=5, tell_apart=True)
    # no repeats
    c = run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 400, 12, unit, None, slots(400, 6, gap=0) * k, 16, pio, 16, form,
            seed=6)
    got, fgot = c.check("no repeats")
    c.reset()
    cuda.cuda.synchronize()
    starts = np.arange(401, dtype=np.int64) * 12
    assert mpi.reduce_local_fetch_ragged(c.ain.ptr, c.aio.ptr, c.tio, c.afe.ptr, starts, unit, 400, 4800, c.dt, c.o) == 0
    assert np.array_equal(c.aio.check("fetch_ragged inoutbuf"), got), f"{c.what}: target differs from MPIX_Reduce_local_fetch_ragged"
    assert np.array_equal(c.afe.check("fetch_ragged fetchbuf"), fgot), f"{c.what}: fetchbuf differs from MPIX_Reduce_local_fetch_ragged"
    # targets 0, 2, 4, ... once; 1, 3, 5, ... five times; in a shuffled table
    rng = np.random.default_rng(7)
    mixed = rng.permutation(np.concatenate([np.arange(0, 40, 2), np.repeat(np.arange(1, 40, 2), 5)])).astype(np.int64)

    def singles(info, sorted_displs):
        _, counts = np.unique(sorted_displs, return_counts=True)
        assert counts.tolist() == [1, 5] * 20

    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", len(mixed), 12, unit, None, mixed * k, 16, pio, 16, form, seed=7,
        expect=singles)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 1, 12, unit, None, np.array([3 * k], np.int64), 16, pio, 16, form, seed=8)
    # order NULL: runs of 1 and 3, equal entries adjacent, the runs themselves in no order
    adj = np.concatenate([[s] * (1 if s % 2 else 3) for s in slots(60, 9, gap=0).tolist()]).astype(np.int64) * k
    c = Case(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", len(adj), 12, unit, None, adj, 16, pio, 16, seed=9)
    _, counts = np.unique(adj, return_counts=True)
    assert sorted(set(counts.tolist())) == [1, 3] and not (np.diff(adj) >= 0).all()
    c.plan(form)
    assert mpi.error_class(c.call("sync")) == 0
    built = c.check("built order")
    c.dorder = c.horder = None
    c.plan(form)
    for way in WAYS:
        c.reset()
        rc = c.call(way)
        assert rc == 0, f"{c.what} order NULL {way}: {mpi.error_string(rc)}"
        nul = c.check(f"order NULL {way}")
        assert np.array_equal(nul[0], built[0]) and np.array_equal(nul[1], built[1]), f"{c.what}: order NULL differs, {way}"
    c.tables_unchanged()


# ---------------------------------------------------------------- 5. types
@pytest.mark.parametrize("op,t", TYPES, ids=[f"{o}-{t}" for o, t in TYPES])
def test_types_where_order_or_representation_matters(mpi, orc, cuda, op, t):
    assert (op, t) in MATRIX
    esz = T.elem_size(t)
    assert 48 % esz == 0 and esz <= 16
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, 400, 48 // esz, 16, None, shape1(16, seed=10), 16, 32, 16, NARROW_VEC,
        seed=10)


@pytest.mark.parametrize("t", ["MPI_FLOAT", "MPI_LONG_DOUBLE", "MPI_C_LONG_DOUBLE_COMPLEX"])
@pytest.mark.parametrize("op", BYTE_OPS)
def test_no_op_and_replace(mpi, orc, cuda, op, t):
    """MPI_NO_OP: inbuf passed as 0, target and input arena unchanged, every block
    of a run the old target.  MPI_REPLACE: fetchbuf[k] the previous contribution,
    the target the run's last input block."""
    esz = T.elem_size(t)
    rb = 48 if esz <= 16 else 64            # the 32-byte class takes the element form and its own block size
    form = NARROW_VEC if esz <= 16 else NARROW_ELEMS
    c = run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, 400, rb // esz, 16, None, shape1(16, seed=11) * (2 if rb == 64 else 1),
            16, 32, 16, form, seed=11)
    got, fgot = c.check("last way")
    if op == "MPI_NO_OP":
        assert c.pin == 0
        assert np.array_equal(got, c.a) and np.array_equal(fgot, c.a[c.dst])
    else:
        for j in range(len(c.uio)):
            ks = np.nonzero(c.dst == j)[0]
            assert np.array_equal(got[j], c.b[c.src[ks[-1]]])
            assert np.array_equal(fgot[ks[0]], c.a[j]) and np.array_equal(fgot[ks[1:]], c.b[c.src[ks[:-1]]])


def test_a_pair_the_library_refuses(mpi, orc, cuda):
    """MPI_LAND on MPI_FLOAT: the oracle's class, nothing written (check does both)."""
    assert not T.compute_ok("MPI_LAND", "MPI_FLOAT")
    c = run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_LAND", "MPI_FLOAT", 400, 12, 16, None, shape1(16, seed=12), 16, 32, 16,
            NARROW_VEC, seed=12)
    assert c.rc_want == mpi.MPI_ERR_OP


# ---------------------------------------------------------------- 6. launches
def test_lowered_cap_runs_cross_launch_boundaries(mpi, orc, cuda):
    """The per-launch workgroup cap lowered to 3: 2731 blocks onto 211 targets make
    three launches of 1024 sorted positions with a run across a boundary; the
    wide shape becomes several launches too."""
    lib = mpi.load()
    stream = cuda.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        def crossing(info, sorted_displs):
            rpl = info["rows_per_launch"]
            assert info["launches"] == 3 and rpl == 1024, info
            assert any(sorted_displs[p - 1] == sorted_displs[p] for p in range(rpl, len(sorted_displs), rpl))

        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 16, None, shape1(16, 2731, 211, seed=13), 16, 32, 16,
            NARROW_VEC, seed=13, expect=crossing, tell_apart=True)
        bl, far, tio = wide_shape(mpi, 4)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 5, bl, 4, None, tio, 4, 4, 4, WIDE, seed=14,
            expect=lambda i, s: i["launches"] == -(-5 // max(1, 3 // i["per"])) > 1 or pytest.fail(str(i)), tell_apart=True)
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3


# ---------------------------------------------------------------- 7. graph
def test_captured_in_a_graph(mpi, orc, cuda):
    """Captured on one stream and replayed twice: the target is the oracle applied
    twice, fetchbuf the second pass's fetch values."""
    torch = cuda
    s = torch.cuda.Stream()
    c = Case(mpi, orc, torch, s, "MPI_SUM", "MPI_FLOAT", 400, 12, 16, None, shape1(16, seed=15), 0, 16, 16, seed=15)
    twice, fsecond, rc = oracle_fetch(orc, c.want, c.b, c.src, c.dst, c.nb, c.bl, c.dt, c.op, c.o)
    assert rc == 0 and not np.array_equal(fsecond, c.fwant)
    assert c.plan(NARROW_VEC)["launches"] == 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_fetch_indexed_ordered(c.ain.ptr, None, c.aio.ptr, c.dptr[1], c.afe.ptr, c.dorder.data_ptr(),
                                                          16, c.nb, c.bl, c.dt, c.o, cs) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.aio.check("captured inoutbuf"), c.a)      # capture records, it does not run
    assert np.array_equal(c.afe.check("captured fetchbuf"), ~c.fwant)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    c.check("replayed twice", want=twice, fwant=fsecond)
    c.tables_unchanged()


# ---------------------------------------------------------------- 8. routes and refusals
def test_routes_and_refusals(mpi, orc, cuda):
    torch = cuda
    stream = torch.cuda.Stream()
    nb, bl = 400, 12
    c = Case(mpi, orc, torch, stream, "MPI_SUM", "MPI_FLOAT", nb, bl, 16, None, shape1(16, seed=16), 0, 16, 16, seed=16)
    dt, o = c.dt, c.o
    call = mpi.reduce_local_fetch_indexed_ordered
    tio, horder, dorder, dtio = c.tio, c.horder, c.dorder.data_ptr(), c.dptr[1]

    def refused(rc, cls, what):
        stream.synchronize()
        assert mpi.error_class(rc) == cls, f"{what}: {mpi.error_string(rc)}"
        assert np.array_equal(c.aio.check(what), c.a), f"{what}: inoutbuf written by a refused call"
        assert np.array_equal(c.afe.check(what), ~c.fwant), f"{what}: fetchbuf written by a refused call"
        assert np.array_equal(c.ain.check(what), c.b), what

    # both tables NULL: MPIX_Reduce_local_fetch on nblocks x blocklen elements
    flat = Arena(torch, c.a[:1].repeat(8, 0).reshape(1, -1), np.array([0]), 16)
    fin = Arena(torch, c.b[:8].reshape(1, -1), np.array([0]), 0)
    ffe = Arena(torch, np.zeros((1, 8 * bl * 4), np.uint8), np.array([0]), 16)
    assert call(fin.ptr, None, flat.ptr, None, ffe.ptr, None, 16, 8, bl, dt, o) == 0
    r1, f1 = flat.check("no tables"), ffe.check("no tables fetchbuf")
    flat.upload()
    ffe.upload()
    assert mpi.reduce_local_fetch(fin.ptr, flat.ptr, ffe.ptr, 8 * bl, dt, o) == 0
    assert np.array_equal(flat.check("fetch"), r1) and np.array_equal(ffe.check("fetch fetchbuf"), f1)
    assert np.array_equal(f1, c.a[:1].repeat(8, 0).reshape(1, -1))
    # MPI_ERR_ARG
    refused(call(c.ain.ptr, None, c.aio.ptr, None, c.afe.ptr, horder, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG, "order without inout_displs")
    refused(call(c.ain.ptr, None, c.aio.ptr, None, c.afe.ptr, dorder, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG,
            "device order without inout_displs")
    refused(call(c.ain.ptr, np.arange(nb, dtype=np.int64) * 3, c.aio.ptr, None, c.afe.ptr, None, 16, nb, bl, dt, o),
            mpi.MPI_ERR_ARG, "in_displs without inout_displs")
    twice = horder.copy()
    twice[7] = twice[8]
    wild = horder.copy()
    wild[3] = nb
    neg = horder.copy()
    neg[3] = -1
    p = int(np.nonzero(tio[horder][1:] != tio[horder][:-1])[0][0])     # positions p, p + 1: two different targets
    desc = horder.copy()
    desc[[p, p + 1]] = desc[[p + 1, p]]
    q = int(np.nonzero(tio[horder][1:] == tio[horder][:-1])[0][0])     # positions q, q + 1: one target
    tie = horder.copy()
    tie[[q, q + 1]] = tie[[q + 1, q]]
    for bad, why in ((twice, "a repeated entry"), (wild, "an entry == nblocks"), (neg, "a negative entry"),
                     (desc, "a descending pair"), (tie, "a tie out of table order")):
        refused(call(c.ain.ptr, None, c.aio.ptr, tio, c.afe.ptr, bad, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG, f"host order with {why}")
    # order NULL promises that equal entries are adjacent: one entry equal to a non-adjacent earlier one
    apart = slots(nb, 16, gap=0) * 4
    apart[nb - 1] = apart[3]
    refused(call(c.ain.ptr, None, c.aio.ptr, apart, c.afe.ptr, None, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG,
            "order NULL with a non-adjacent repeat in a host table")
    # MPI_ERR_BUFFER
    cs = stream.cuda_stream
    refused(call(c.ain.ptr, None, c.aio.ptr, dtio, c.afe.ptr, horder, 16, nb, bl, dt, o, cs), mpi.MPI_ERR_BUFFER, "host order on a stream")
    refused(call(c.ain.ptr, None, c.aio.ptr, tio, c.afe.ptr, dorder, 16, nb, bl, dt, o, cs), mpi.MPI_ERR_BUFFER,
            "host inout_displs on a stream")
    refused(call(c.ain.ptr, None, c.aio.ptr, dtio, 0, dorder, 16, nb, bl, dt, o), mpi.MPI_ERR_BUFFER, "fetchbuf NULL")
    for d in (0, 16, nb * bl * 4 - 16):
        refused(call(c.ain.ptr, None, c.aio.ptr, dtio, c.ain.ptr + d, dorder, 16, nb, bl, dt, o), mpi.MPI_ERR_BUFFER,
                f"fetchbuf over the packed inbuf at +{d}")
    # ... which MPI_NO_OP accepts: it never looks at inbuf (the input arena serves as fetchbuf, then is put back)
    rc = call(c.ain.ptr, None, c.aio.ptr, dtio, c.ain.ptr, dorder, 16, nb, bl, dt, mpi.MPI_NO_OP)
    assert rc == 0, mpi.error_string(rc)
    assert np.array_equal(c.ain.check("NO_OP into the input arena"), c.a[c.dst])
    assert np.array_equal(c.aio.check("NO_OP"), c.a)
    c.ain.upload()
    # fetchbuf inside the target's span, which only a host table shows
    lo, hi = int(c.uio.min()), int(c.uio.max()) + bl * 4
    for d in (lo, lo - 64, hi - 1, (lo + hi) // 2 // 16 * 16):
        refused(call(c.ain.ptr, None, c.aio.ptr, tio, c.aio.ptr + d, horder, 16, nb, bl, dt, o), mpi.MPI_ERR_BUFFER,
                f"fetchbuf in the target's span at {d}")
    # a device order with out-of-range values: undefined result, but the call returns
    # and writes no guard byte of the target arena or the fetchbuf arena
    broken = horder.copy()
    broken[5], broken[9], broken[nb - 1] = nb + 1000, -3, 2 ** 31 - 1
    dbroken = torch.from_numpy(broken).cuda()
    torch.cuda.synchronize()
    rc = call(c.ain.ptr, None, c.aio.ptr, dtio, c.afe.ptr, dbroken.data_ptr(), 16, nb, bl, dt, o)
    assert rc == 0, mpi.error_string(rc)
    c.aio.check("device order out of range: inoutbuf guards")
    c.afe.check("device order out of range: fetchbuf guards")
    assert np.array_equal(c.ain.check("device order out of range: inbuf"), c.b)
    # and the valid order on the same operands still gives the oracle's
    c.reset()
    assert c.call("sync") == 0
    c.check("valid order")
    c.tables_unchanged()
