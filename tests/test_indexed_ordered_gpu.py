"""MPIX_Reduce_local_indexed_ordered on the GPU: an indexed reduction whose
output table names the same block many times, the result the oracle's
MPI_Reduce_local applied block by block in ascending k into one row per distinct
target (bit-exact, test_parity_gpu.same's complex-NaN rule).

The arenas are test_indexed_gpu's: 0xA5 around and between the blocks, the base
at a chosen byte phase.  After each call every distinct target must equal the
oracle's, every guard byte must still be 0xA5, and the input arena and all three
tables must be unchanged: a run folded in another order, a head that missed its
run's end, a run lost at a workgroup or launch boundary, a sort that treated the
displacements as unsigned all show there.  Before a shape runs the call's own
planner must report the form the shape aims at.  Every shape runs three ways:
synchronously with device tables, on a torch stream with device tables, and
synchronously with host tables.  The order table comes from
MPIX_Reduce_local_order in the first two (the library's scratch, then the
caller's, whose bytes past the reported size must stay untouched) and from
numpy's stable argsort in the third; all three must be equal.

Every address a kernel forms here stays inside its arena.
"""
import numpy as np
import pytest

import _types as T
from test_indexed_gpu import Arena, slots, threshold
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import FILL, TILE

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
FORMS = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
WAYS = ("sync", "stream", "host-tables")
TAIL = 4096                     # bytes of a caller's work allocation past the reported size


def oracle_rows(orc, a, b, src, dst, ks, bl, dt, o):
    """a's rows (one per distinct target) after blocks ks, in that order; the classes returned"""
    want = a.copy()
    rcs = {orc.reduce_local(b[src[k]].copy(), want[dst[k]], bl, dt, o) for k in ks}
    assert len(rcs) == 1
    return want, rcs.pop()


def repeated(nb, distinct, seed):
    """nb target numbers in [0, distinct): every one at least once, the rest drawn at random"""
    rng = np.random.default_rng([seed, nb, distinct])
    return rng.permutation(np.concatenate([np.arange(distinct), rng.integers(0, distinct, nb - distinct)])).astype(np.int64)


def build_orders(mpi, torch, stream, tio, dtio, what):
    """The order of tio three ways: the library's scratch, the caller's (on the
    stream), numpy.  Returns (device order tensor, host order)."""
    nb = len(tio)
    host = np.argsort(tio, kind="stable").astype(np.int32)
    ws = mpi.reduce_local_order_worksize(nb)
    d1 = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    d2 = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    work = torch.full((ws + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = mpi.reduce_local_order(dtio.data_ptr(), nb, d1.data_ptr())
    assert rc == 0, f"{what}: order, library scratch: {mpi.error_string(rc)}"
    rc = mpi.reduce_local_order(dtio.data_ptr(), nb, d2.data_ptr(), work.data_ptr(), ws, stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, f"{what}: order, caller's work on a stream: {mpi.error_string(rc)}"
    assert np.array_equal(d1.cpu().numpy(), host), f"{what}: MPIX_Reduce_local_order differs from numpy's stable argsort"
    assert np.array_equal(d2.cpu().numpy(), host), f"{what}: the stream build differs from numpy's stable argsort"
    assert (work[ws:].cpu().numpy() == FILL).all(), f"{what}: work written past the reported {ws} bytes"
    assert np.array_equal(dtio.cpu().numpy(), tio), f"{what}: the build wrote its input table"
    return d1, host


def run(mpi, orc, torch, stream, op, t, nb, bl, unit, tin, tio, pin, pio, form, seed=0, expect=None, ways=WAYS,
        order_matters=False, against_indexed=False):
    """nb blocks of bl elements; tio (int64, units of `unit` bytes) may repeat, tin
    (or None: packed) too.  Asserts the planner's form, runs the call every way
    and checks both arenas and the tables.  Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    rb = bl * esz
    rng = np.random.default_rng([seed, nb, bl])
    tio = np.ascontiguousarray(tio, dtype=np.int64)
    off_in = np.arange(nb, dtype=np.int64) * rb if tin is None else np.asarray(tin, np.int64) * unit
    uin, src = np.unique(off_in, return_inverse=True)
    uio, dst = np.unique(tio * unit, return_inverse=True)
    a = T.to_bytes(T.gen(t, len(uio) * bl, rng, op)).reshape(len(uio), rb)      # one row per distinct target
    b = T.to_bytes(T.gen(t, len(uin) * bl, rng, op)).reshape(len(uin), rb)      # one per input placement
    want, rc_want = oracle_rows(orc, a, b, src, dst, range(nb), bl, dt, o)
    what = f"{op} {t} {nb} x {bl} onto {len(uio)} unit {unit} in=+{pin}{'' if tin is None else '/table'} io=+{pio}"
    if order_matters:
        # the case can tell a wrong order only if another order gives other bits
        back, _ = oracle_rows(orc, a, b, src, dst, range(nb - 1, -1, -1), bl, dt, o)
        differ = int((want.reshape(-1, esz) != back.reshape(-1, esz)).any(axis=1).sum())
        print(f"{what}: descending k differs from ascending in {differ} of {len(uio) * bl} elements")
        assert differ >= 1, f"{what}: the order of application does not show in this data"
    ain, aio = Arena(torch, b, uin, pin), Arena(torch, a, uio, pio)
    host = [None if tin is None else np.ascontiguousarray(tin, dtype=np.int64), tio]
    devt = [None if x is None else torch.from_numpy(x).cuda() for x in host]
    dptr = [0 if x is None else x.data_ptr() for x in devt]
    dorder, horder = build_orders(mpi, torch, stream, tio, devt[1], what)
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.indexed_ordered_plan_info(ain.ptr, dptr[0], aio.ptr, dptr[1], dorder.data_ptr(), unit, nb, bl, dt, o)
        assert info["form"] == form, f"{what}: aimed at {FORMS[form]}, the planner says {info}"
        assert info == mpi.indexed_ordered_plan_info(ain.ptr, host[0], aio.ptr, host[1], horder, unit, nb, bl, dt, o)
        if expect:
            expect(info, tio[horder])
    for n, way in enumerate(ways):
        if n:
            aio.upload()
        torch.cuda.synchronize()
        tabs = host + [horder] if way == "host-tables" else dptr + [dorder.data_ptr()]
        rc = mpi.reduce_local_indexed_ordered(ain.ptr, tabs[0], aio.ptr, tabs[1], tabs[2], unit, nb, bl, dt, o,
                                              stream.cuda_stream if way == "stream" else 0)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        assert np.array_equal(ain.check(f"{what} {way} inbuf"), b), f"{what} {way}: inbuf modified"
        for j in range(0 if not np.array_equal(got, want) else len(uio), len(uio)):
            if not same(got[j], want[j], t):
                ks = np.nonzero(dst == j)[0]
                pytest.fail(f"{what} {way} ({FORMS[form]}) target {j}, blocks {ks.tolist()[:20]}:\n" +
                            explain(got[j], want[j], a[j], b[src[ks[-1]]], esz))
    if against_indexed:
        # all targets distinct: byte-equal to the indexed call on the same operands
        aio.upload()
        torch.cuda.synchronize()
        assert mpi.reduce_local_indexed(ain.ptr, dptr[0], aio.ptr, dptr[1], unit, nb, bl, dt, o) == 0
        plain = aio.check(f"{what} indexed")
        assert np.array_equal(plain, got), f"{what}: differs from MPIX_Reduce_local_indexed"
    for x, h in zip(devt + [dorder], host + [horder]):
        if x is not None:
            assert np.array_equal(x.cpu().numpy(), h), f"{what}: a table was written"
    return info


def shape1(unit, nb=400, distinct=37, seed=1):
    """nb blocks of 48 bytes onto `distinct` slots 64 bytes apart, in units of `unit`"""
    return slots(distinct, seed, gap=0)[repeated(nb, distinct, seed)] * (64 // unit)


# ---------------------------------------------------------------- narrow blocks
@pytest.mark.parametrize("t", ["MPI_FLOAT", "MPIX_C_FLOAT16"])
def test_narrow_vectors_runs_across_a_workgroup_boundary(mpi, orc, cuda, t):
    """400 blocks of 48 bytes (12 floats, 24 halves) onto 37 slots: 1200 vectors,
    two workgroups, the boundary inside the block at sorted position 341, whose
    run is longer than one block and so lies in both workgroups.  The data must
    be able to tell a wrong order: descending k gives other bits."""
    bl = 48 // T.elem_size(t)
    assert 48 < threshold(mpi, t)

    def two(info, sorted_displs):
        assert info["groups"] == 2 and info["launches"] == 1, info
        assert 1024 // 3 == 341 and 1024 % 3
        assert sorted_displs[340] == sorted_displs[341] or sorted_displs[341] == sorted_displs[342]
        assert len(np.unique(sorted_displs)) == 37

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", t, 400, bl, 16, None, shape1(16), 16, 32, NARROW_VEC, seed=1,
        expect=two, order_matters=True)


def test_narrow_elements(mpi, orc, cuda):
    """The same shape with disp_unit 4 and the base 4 bytes off: 4800 elements,
    4096 a workgroup, the boundary inside a block and inside a run."""

    def two(info, sorted_displs):
        assert info["groups"] == 2 and 4096 % 12, info
        assert sorted_displs[340] == sorted_displs[341] or sorted_displs[341] == sorted_displs[342]

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 400, 12, 4, None, shape1(4), 16, 36, NARROW_ELEMS,
        seed=2, expect=two, order_matters=True)


# ---------------------------------------------------------------- wide blocks
@pytest.mark.parametrize("unit,pio", [(4, 4), (1, 1)], ids=["tile-grid", "target-off-alignment"])
def test_wide_runs_of_three_and_two(mpi, orc, cuda, unit, pio):
    """5 blocks onto 2 targets, k = 0, 2, 4 and k = 1, 3: blocks of several tiles
    with a ragged end, the bases off the 16 KiB grid.  The packed input blocks
    fall at different residues mod 16, so within one run some are read through
    the descriptor and some element by element.  With byte displacements and an
    odd base the targets themselves are off their alignment: the element form."""
    bl = threshold(mpi) // 4 + TILE // 4 + 3
    assert bl * 4 >= threshold(mpi) and (bl * 4) % 16
    far = (bl + 5) * 4 // unit + (1 if unit == 1 else 0)
    tio = np.array([0, far, 0, far, 0], dtype=np.int64)

    def runs(info, sorted_displs):
        assert info["groups"] == 5 * info["per"] and info["per"] >= -(-bl * 4 // TILE), info
        assert sorted_displs.tolist() == [0, 0, 0, far, far]

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 5, bl, unit, None, tio, 4, pio, WIDE, seed=3,
        expect=runs, order_matters=True)


# ---------------------------------------------------------------- edges of the run loop
@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_run_loop_edges(mpi, orc, cuda, unit, form):
    """One run from position 0 to the table's end; no repeats at all (also
    byte-equal to the indexed call); runs of one between longer runs; one block."""
    stream = cuda.cuda.Stream()
    pio = 32 if unit == 16 else 36
    k = 64 // unit
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 300, 12, unit, None, np.full(300, 5 * k, np.int64), 16, pio, form,
        seed=4, order_matters=True)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 400, 12, unit, None, slots(400, 5, gap=0) * k, 16, pio, form,
        seed=5, against_indexed=True)
    # targets 0, 2, 4, ... once; 1, 3, 5, ... five times; in a shuffled table
    rng = np.random.default_rng(6)
    mixed = rng.permutation(np.concatenate([np.arange(0, 40, 2), np.repeat(np.arange(1, 40, 2), 5)])).astype(np.int64)

    def singles(info, sorted_displs):
        _, counts = np.unique(sorted_displs, return_counts=True)
        assert counts.tolist() == [1, 5] * 20

    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", len(mixed), 12, unit, None, mixed * k, 16, pio, form, seed=6,
        expect=singles)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 1, 12, unit, None, np.array([3 * k], np.int64), 16, pio, form, seed=7)


@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_both_tables_with_repeats(mpi, orc, cuda, unit, form):
    """in_displs repeats input blocks and inout_displs repeats targets."""
    rng = np.random.default_rng(8)
    tin = rng.integers(0, 50, 400).astype(np.int64) * (48 // unit)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 400, 12, unit, tin, shape1(unit, seed=8), 0,
        16 if unit == 16 else 20, form, seed=8, order_matters=True)


@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_signed_displacements_widely_spread(mpi, orc, cuda, unit, form):
    """37 targets around a base in the middle of the arena, 64 KiB + 64 bytes
    apart: negative displacements (all high bits set) sort below zero and the
    positive ones, which a sort on unsigned keys would put first."""
    step = (65536 + 64) // unit
    tio = (slots(37, 9, gap=0, lo=-18) * step)[repeated(300, 37, 9)]
    assert (tio < 0).any() and (tio > 0).any() and (tio == 0).any()

    def signed(info, sorted_displs):
        assert sorted_displs[0] == -18 * step and sorted_displs[-1] == 18 * step

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 300, 12, unit, None, tio, 0,
        0 if unit == 16 else 4, form, seed=9, expect=signed, order_matters=True)


# ---------------------------------------------------------------- types
TYPES = [("MPI_SUM", "MPI_LONG_DOUBLE"), ("MPI_PROD", "MPI_C_FLOAT_COMPLEX"), ("MPI_MAXLOC", "MPI_DOUBLE_INT"),
         ("MPI_MINLOC", "MPI_DOUBLE_INT"), ("MPI_SUM", "MPI_INT"), ("MPI_BXOR", "MPI_UNSIGNED_CHAR"),
         ("MPI_LAND", "MPI_C_BOOL")]


@pytest.mark.parametrize("op,t", TYPES, ids=[f"{o}-{t}" for o, t in TYPES])
def test_types_where_order_or_representation_matters(mpi, orc, cuda, op, t):
    """x87 sums, complex products, MAXLOC / MINLOC ties, integer wraparound, bytes
    and bools on shape 1's layout: 400 blocks of 48 bytes onto 37 slots."""
    assert (op, t) in MATRIX
    esz = T.elem_size(t)
    assert 48 % esz == 0 and esz <= 16
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, 400, 48 // esz, 16, None, shape1(16, seed=10), 16, 32, NARROW_VEC,
        seed=10)


def test_a_pair_the_library_refuses(mpi, orc, cuda):
    """MPI_LAND on MPI_FLOAT: the oracle's class, nothing written (run checks both)."""
    assert not T.compute_ok("MPI_LAND", "MPI_FLOAT")
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_LAND", "MPI_FLOAT", 400, 12, 16, None, shape1(16, seed=11), 16, 32,
        NARROW_VEC, seed=11)


# ---------------------------------------------------------------- launches
def test_lowered_cap_runs_cross_launch_boundaries(mpi, orc, cuda):
    """The per-launch workgroup cap lowered to 3: 2731 blocks onto 211 targets
    make three launches of 1024 sorted positions, and a run lies across a
    boundary between two of them (asserted from the planner's rows_per_launch);
    the wide shape becomes one launch per block, its runs of 3 and 2 across
    them."""
    lib = mpi.load()
    stream = cuda.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        def crossing(info, sorted_displs):
            rpl = info["rows_per_launch"]
            assert info["launches"] == 3 and rpl == 1024, info
            assert any(sorted_displs[p - 1] == sorted_displs[p] for p in range(rpl, len(sorted_displs), rpl))

        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 16, None, shape1(16, 2731, 211, seed=12), 16, 32,
            NARROW_VEC, seed=12, expect=crossing, order_matters=True)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 4, None, shape1(4, 2731, 211, seed=12), 16, 36,
            NARROW_ELEMS, seed=13, expect=lambda i, s: i["launches"] > 1 or pytest.fail(str(i)))
        bl = threshold(mpi) // 4 + TILE // 4 + 3
        far = bl + 5
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 5, bl, 4, None, np.array([0, far, 0, far, 0], np.int64), 4, 4,
            WIDE, seed=14, expect=lambda i, s: i["launches"] == -(-5 // max(1, 3 // i["per"])) > 1 or pytest.fail(str(i)),
            order_matters=True)
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3


def test_captured_in_a_graph(mpi, orc, cuda):
    """With device tables and an order built beforehand the combine is captured
    on one stream (no parallel branches) and replayed twice: the oracle applied
    twice."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb, bl = 400, 12
    rng = np.random.default_rng(15)
    tio = shape1(16, seed=15)
    uio, dst = np.unique(tio * 16, return_inverse=True)
    a = T.to_bytes(T.gen("MPI_FLOAT", len(uio) * bl, rng, specials=False)).reshape(len(uio), bl * 4)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng, specials=False)).reshape(nb, bl * 4)
    src = np.arange(nb)
    once, rc = oracle_rows(orc, a, b, src, dst, range(nb), bl, dt, o)
    assert rc == 0
    twice, _ = oracle_rows(orc, once, b, src, dst, range(nb), bl, dt, o)
    ain, aio = Arena(torch, b, np.arange(nb) * bl * 4, 0), Arena(torch, a, uio, 16)
    dtio = torch.from_numpy(tio).cuda()
    s = torch.cuda.Stream()
    dorder, _ = build_orders(mpi, torch, s, tio, dtio, "graph")
    assert mpi.indexed_ordered_plan_info(ain.ptr, 0, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), 16, nb, bl, dt, o)["form"] == NARROW_VEC
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_indexed_ordered(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), 16, nb, bl,
                                                    dt, o, cs) == 0
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("captured inoutbuf"), a)        # capture records, it does not run
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("replayed twice"), twice)
    assert np.array_equal(ain.check("replayed twice inbuf"), b)


# ---------------------------------------------------------------- routes and failures
def test_routes_and_failures(mpi, orc, cuda):
    """order NULL is the indexed call; an order without inout_displs, a host order
    that is no stable sort of a host inout_displs, a host table on a stream and a
    short work_bytes are refused with nothing written; a device order holding
    out-of-range values returns, and writes no guard byte (the kernel clamps what
    it reads from the table)."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb, bl = 400, 12
    rng = np.random.default_rng(16)
    tio = shape1(16, seed=16)
    uio, dst = np.unique(tio * 16, return_inverse=True)
    a = T.to_bytes(T.gen("MPI_FLOAT", len(uio) * bl, rng)).reshape(len(uio), bl * 4)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng)).reshape(nb, bl * 4)
    ain, aio = Arena(torch, b, np.arange(nb) * bl * 4, 0), Arena(torch, a, uio, 16)
    dtio = torch.from_numpy(tio).cuda()
    stream = torch.cuda.Stream()
    dorder, horder = build_orders(mpi, torch, stream, tio, dtio, "routes")

    def refused(rc, cls, what):
        stream.synchronize()
        assert mpi.error_class(rc) == cls, f"{what}: {mpi.error_string(rc)}"
        assert np.array_equal(aio.check(what), a), f"{what}: inoutbuf written by a refused call"
        assert np.array_equal(ain.check(what), b), what

    call = mpi.reduce_local_indexed_ordered
    # order NULL: the indexed call, here on a table without repeats
    tdist = slots(len(uio), 16, gap=0) * 4
    adist = Arena(torch, a, tdist * 16, 16)
    bdist = Arena(torch, b[:len(uio)], np.arange(len(uio)) * bl * 4, 0)
    assert call(bdist.ptr, None, adist.ptr, tdist, None, 16, len(uio), bl, dt, o) == 0
    first = adist.check("order NULL")
    adist.upload()
    assert mpi.reduce_local_indexed(bdist.ptr, None, adist.ptr, tdist, 16, len(uio), bl, dt, o) == 0
    assert np.array_equal(adist.check("indexed"), first)
    # an order table and a packed target
    refused(call(ain.ptr, None, aio.ptr, None, horder, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG, "order without inout_displs")
    refused(call(ain.ptr, None, aio.ptr, None, dorder.data_ptr(), 16, nb, bl, dt, o), mpi.MPI_ERR_ARG,
            "device order without inout_displs")
    # host orders that break a condition
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
        refused(call(ain.ptr, None, aio.ptr, tio, bad, 16, nb, bl, dt, o), mpi.MPI_ERR_ARG, f"host order with {why}")
    # a host table with a stream, whichever it is
    cs = stream.cuda_stream
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), horder, 16, nb, bl, dt, o, cs), mpi.MPI_ERR_BUFFER,
            "host order on a stream")
    refused(call(ain.ptr, None, aio.ptr, tio, dorder.data_ptr(), 16, nb, bl, dt, o, cs), mpi.MPI_ERR_BUFFER,
            "host inout_displs on a stream")
    # the build: short work, no work on a stream, a host table on a stream
    ws = mpi.reduce_local_order_worksize(nb)
    work = torch.full((ws,), FILL, dtype=torch.uint8, device="cuda")
    d3 = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in (0, cs):
        rc = mpi.reduce_local_order(dtio.data_ptr(), nb, d3.data_ptr(), work.data_ptr(), ws - 1, s)
        stream.synchronize()
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG, mpi.error_string(rc)
    rc = mpi.reduce_local_order(dtio.data_ptr(), nb, d3.data_ptr(), 0, 0, cs)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
    rc = mpi.reduce_local_order(tio, nb, d3.data_ptr(), work.data_ptr(), ws, cs)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
    stream.synchronize()
    assert (d3.cpu().numpy() == -1).all() and (work.cpu().numpy() == FILL).all(), "a refused build wrote"
    # mixed placement in the synchronous build
    mixed = np.full(nb, -1, np.int32)
    assert mpi.reduce_local_order(dtio.data_ptr(), nb, mixed) == 0 and np.array_equal(mixed, horder)
    assert mpi.reduce_local_order(tio, nb, d3.data_ptr()) == 0 and np.array_equal(d3.cpu().numpy(), horder)
    # a device order with out-of-range values: undefined result, but the call
    # returns and every address stays inside the blocks
    broken = horder.copy()
    broken[5], broken[9], broken[nb - 1] = nb + 1000, -3, 2 ** 31 - 1
    dbroken = torch.from_numpy(broken).cuda()
    torch.cuda.synchronize()
    rc = call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dbroken.data_ptr(), 16, nb, bl, dt, o)
    assert rc == 0, mpi.error_string(rc)
    aio.check("device order out of range: inoutbuf guards")
    assert np.array_equal(ain.check("device order out of range: inbuf"), b)
    # and the valid order on the same operands still gives the oracle's rows
    aio.upload()
    want, _ = oracle_rows(orc, a, b, np.arange(nb), dst, range(nb), bl, dt, o)
    assert call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), 16, nb, bl, dt, o) == 0
    assert np.array_equal(aio.check("valid order"), want)
