"""MPIX_Reduce_local_indexed on the GPU: equal blocks at the places a
displacement table names, in one launch, every block the oracle's
MPI_Reduce_local on it (bit-exact, test_parity_gpu.same's complex-NaN rule).

Each operand sits in an arena of its own, filled with 0xA5, its base pointer at
a chosen byte phase of the 16 KiB grid (in the middle of the arena where the
table holds negative displacements).  After each call every block of inoutbuf
must equal the oracle's, every other byte of the arena -- the gaps between
blocks included -- must still be 0xA5, and the input arena must be unchanged:
a workgroup that read the wrong table entry, a flattened unit mapped one block
off, a table pointer not advanced for a later launch all show there.  Every
output table is a permutation of slots with gaps, so no two output blocks
overlap.  Before a shape runs, MPIR_Hip_indexed_plan_info -- the launch's own
planner -- must report the form the shape was built for; sizes hang on the
threshold it reports.  Every shape runs three ways: synchronously with device
tables, enqueued on a torch stream with device tables, and synchronously with
host (numpy) tables.

Every address a kernel forms here stays inside its arena.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import FILL, TILE

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
FORMS = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
WAYS = ("sync", "stream", "host-tables")


class Arena:
    """A device allocation filled with 0xA5 around `rows` (m x block bytes), row j
    at byte offset offs[j] (signed) from a base pointer that sits `phase` bytes
    past a 16 KiB boundary."""

    def __init__(self, torch, rows, offs, phase):
        m, rb = rows.shape
        offs = np.asarray(offs, dtype=np.int64)
        assert offs.shape == (m,)
        lo, hi = int(offs.min()), int(offs.max()) + rb
        below = -(-max(-lo, 0) // TILE) * TILE              # room for negative displacements
        self.torch = torch
        self.t = torch.empty(below + max(hi, 0) + phase + 4 * TILE, dtype=torch.uint8, device="cuda")
        off = -self.t.data_ptr() % TILE + TILE + below + phase
        self.ptr = self.t.data_ptr() + off
        self.idx = off + offs[:, None] + np.arange(rb)[None, :]
        assert self.idx.min() >= TILE // 2 and self.idx.max() < self.t.numel() - TILE // 2
        self.host = np.full(self.t.numel(), FILL, np.uint8)
        self.host[self.idx] = rows
        self.guard = np.ones(self.t.numel(), bool)
        self.guard[self.idx] = False
        assert (~self.guard).sum() == m * rb, "blocks overlap"
        self.upload()

    def upload(self):
        self.t.copy_(self.torch.from_numpy(self.host))

    def check(self, what):
        """The blocks' bytes, after asserting that nothing around or between them was written."""
        self.torch.cuda.synchronize()
        whole = self.t.cpu().numpy()
        bad = np.nonzero(self.guard & (whole != FILL))[0]
        assert not bad.size, f"{what}: guard bytes written at arena offsets {(bad[:8] - (self.ptr - self.t.data_ptr())).tolist()} from the base"
        return whole[self.idx]


def threshold(mpi, t="MPI_FLOAT", op="MPI_SUM"):
    return mpi.indexed_plan_info(1 << 32, 0, 1 << 40, 0, 1, 1, 1, mpi.DATATYPES[t], mpi.OPS[op])["threshold"]


def slots(nb, seed, gap=1, lo=0):
    """nb distinct slot numbers with gaps between them, in a random order"""
    rng = np.random.default_rng([seed, nb, 77])
    return (rng.permutation(nb).astype(np.int64) + lo) * (1 + gap)


def run(mpi, orc, torch, stream, op, t, nb, bl, unit, tin, tio, pin, pio, form, seed=0, expect=None, ways=WAYS):
    """nb blocks of bl elements.  tin / tio: the displacement tables (int64, in
    units of `unit` bytes) or None for a packed side; pin / pio: the bases' byte
    phases.  A repeated tin entry reads the same input block again.  Asserts the
    planner's form, runs the call every way and checks both arenas.
    expect(info): further plan checks.  Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    rb = bl * esz
    rng = np.random.default_rng([seed, nb, bl])
    off_in = np.arange(nb, dtype=np.int64) * rb if tin is None else np.asarray(tin, np.int64) * unit
    off_io = np.arange(nb, dtype=np.int64) * rb if tio is None else np.asarray(tio, np.int64) * unit
    uniq, src = np.unique(off_in, return_inverse=True)      # input placements, and each block's
    a = T.to_bytes(T.gen(t, nb * bl, rng, op)).reshape(nb, rb)              # inout blocks
    b = T.to_bytes(T.gen(t, len(uniq) * bl, rng, op)).reshape(len(uniq), rb)  # in blocks, one per placement
    want = a.copy()
    rcs = {orc.reduce_local(b[src[k]].copy(), want[k], bl, dt, o) for k in range(nb)}       # block by block
    assert len(rcs) == 1
    rc_want = rcs.pop()
    ain, aio = Arena(torch, b, uniq, pin), Arena(torch, a, off_io, pio)
    host = [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (tin, tio)]
    devt = [None if x is None else torch.from_numpy(x).cuda() for x in host]
    dptr = [0 if x is None else x.data_ptr() for x in devt]
    what = f"{op} {t} {nb} x {bl} unit {unit} in=+{pin}{'' if tin is None else '/table'} io=+{pio}{'' if tio is None else '/table'}"
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.indexed_plan_info(ain.ptr, dptr[0], aio.ptr, dptr[1], unit, nb, bl, dt, o)
        assert info["form"] == form, f"{what}: aimed at {FORMS[form]}, the planner says {info}"
        assert info == mpi.indexed_plan_info(ain.ptr, host[0], aio.ptr, host[1], unit, nb, bl, dt, o)
        if expect:
            expect(info)
    for n, way in enumerate(ways):
        if n:
            aio.upload()
        torch.cuda.synchronize()
        tabs = host if way == "host-tables" else dptr
        rc = mpi.reduce_local_indexed(ain.ptr, tabs[0], aio.ptr, tabs[1], unit, nb, bl, dt, o,
                                      stream.cuda_stream if way == "stream" else 0)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        assert np.array_equal(ain.check(f"{what} {way} inbuf"), b), f"{what} {way}: inbuf modified"
        for k in range(0 if not np.array_equal(got, want) else nb, nb):
            if not same(got[k], want[k], t):
                pytest.fail(f"{what} {way} ({FORMS[form]}) block {k}:\n" + explain(got[k], want[k], a[k], b[src[k]], esz))
    for x, h in zip(devt, host):
        if x is not None:
            assert np.array_equal(x.cpu().numpy(), h), f"{what}: a table was written"
    return info


# ---------------------------------------------------------------- narrow blocks
@pytest.mark.parametrize("unit,off,form", [(16, 0, NARROW_VEC), (4, 4, NARROW_ELEMS)], ids=["vec", "base-4-off"])
def test_scatter_blocks_of_three_vectors(mpi, orc, cuda, unit, off, form):
    """400 blocks of 12 floats scattered to permuted slots 64 bytes apart: 1200
    vectors, two workgroups, their boundary inside a block.  With disp_unit 4
    and a base 4 bytes off the same blocks go element by element: 4800
    elements, 4096 a workgroup, the boundary again inside a block."""
    assert 48 < threshold(mpi)

    def two(info):
        assert info["groups"] == 2 and info["launches"] == 1 and (400 * 3) % 1024 and 4096 % 12, info

    tio = slots(400, unit, gap=0) * (64 // unit)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 400, 12, unit, None, tio, 16, 32 + off, form,
        seed=unit, expect=two)


def test_bytes_at_odd_displacements(mpi, orc, cuda):
    """6000 blocks of 3 bytes at odd byte displacements (hindexed_block, disp_unit
    1): 16384 is no multiple of 3, so the first workgroup's span ends inside a
    block, and no element is aligned."""
    assert 3 < threshold(mpi, "MPI_UNSIGNED_CHAR", "MPI_BXOR")

    def two(info):
        assert info["groups"] == 2 and info["per"] % 3, info

    tio = slots(6000, 1, gap=0) * 8 + 1             # 1, 9, 17, ...: every displacement odd
    assert (tio % 2 == 1).all()
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", 6000, 3, 1, None, tio, 1, 0, NARROW_ELEMS,
        expect=two)


def test_column_of_doubles(mpi, orc, cuda):
    """blocklen 1: 3000 doubles at permuted places (disp_unit 8), two workgroups."""
    assert 8 < threshold(mpi, "MPI_DOUBLE")

    def two(info):
        assert info["groups"] == 2 and info["per"] == TILE // 8, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_DOUBLE", 3000, 1, 8, None, slots(3000, 2, gap=2), 0, 0,
        NARROW_ELEMS, expect=two)


@pytest.mark.parametrize("unit,bl,form", [(16, 8, NARROW_VEC), (4, 7, NARROW_ELEMS)], ids=["vec", "elems"])
def test_negative_displacements(mpi, orc, cuda, unit, bl, form):
    """37 blocks around a base in the middle of the arena: half the table is negative."""
    tio = slots(37, unit, gap=1, lo=-18) * (32 // unit)
    assert (tio < 0).sum() == 18 and (tio > 0).sum() == 18
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_FLOAT", 37, bl, unit, None, tio, 0, 0, form, seed=bl)
    # both sides indexed, both with negative entries
    tin = slots(37, unit + 1, gap=2, lo=-30) * (32 // unit)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_FLOAT", 37, bl, unit, tin, tio, 16, 0, form, seed=bl + 1)


@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_gather_and_both_tables(mpi, orc, cuda, unit, form):
    """The gather direction (in_displs given, the output packed), and both sides
    indexed with two different permutations; 400 blocks of 12 floats."""
    stream = cuda.cuda.Stream()
    tin = slots(400, 3, gap=1) * (48 // unit)
    tio = slots(400, 4, gap=0) * (64 // unit)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 400, 12, unit, tin, None, 0, 16, form, seed=1)
    run(mpi, orc, cuda, stream, "MPI_PROD", "MPI_FLOAT", 400, 12, unit, tin, tio, 32, 16, form, seed=2)


def test_broadcast_one_input_block(mpi, orc, cuda):
    """in_displs all zero: one input block of 8 floats combined into each of 700
    output blocks (a repeated input entry is fine)."""
    tio = slots(700, 5, gap=0) * 3
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 700, 8, 16, np.zeros(700, np.int64), tio, 0, 16,
        NARROW_VEC)


# ---------------------------------------------------------------- wide blocks
def test_wide_blocks_on_both_paths(mpi, orc, cuda):
    """5 blocks of 3 x 4096 + 7 floats, the input packed, disp_unit 4 and the
    output displacements at different residues mod 16: some blocks share their
    pointers' offset mod 16 (the tile path, with head and tail elements) and
    some do not (the element path), which the batch's planner confirms for the
    very addresses."""
    bl = 3 * 4096 + 7
    assert bl * 4 >= threshold(mpi)
    res = np.array([0, 3, 1, 1, 2], dtype=np.int64)
    tio = slots(5, 6, gap=0) * (bl + 9) + res
    probe = {}

    def both(info):
        assert info["groups"] == 5 * info["per"] and info["launches"] == 1, info
        probe.update(info)

    # (the arenas' addresses are only known inside run: the paths are asserted on phases here)
    in_phase = (4 + np.arange(5) * bl * 4) % 16
    io_phase = (4 + tio * 4) % 16
    tile = in_phase == io_phase
    assert tile.any() and (~tile).any(), (in_phase, io_phase)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 5, bl, 4, None, tio, 4, 4, WIDE, expect=both)
    assert probe["per"] >= -(-bl * 4 // TILE)


def test_wide_blocks_of_the_32_byte_class(mpi, orc, cuda):
    """MPI_LONG_DOUBLE_INT MAXLOC: every block the element form, 512 elements a workgroup."""
    thr = threshold(mpi, "MPI_LONG_DOUBLE_INT", "MPI_MAXLOC")
    bl = max(thr // 32, 512) + 513

    def elems(info):
        assert info["per"] == -(-bl // 512) and info["groups"] == 4 * info["per"], info

    tio = slots(4, 7, gap=0) * (bl * 2 + 3)         # disp_unit 16: the type's alignment
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAXLOC", "MPI_LONG_DOUBLE_INT", 4, bl, 16, None, tio, 16, 0, WIDE,
        expect=elems)


def test_threshold_and_one_element_below(mpi, orc, cuda):
    """Block bytes at the reported threshold take the wide form, one element less
    the narrow one; both exact."""
    thr = threshold(mpi)
    stream = cuda.cuda.Stream()
    tio = slots(7, 8, gap=0) * (thr // 16 + 4)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4, 16, None, tio, 16, 32, WIDE, seed=1)
    below = run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4 - 1, 16, None, tio, 16, 32, NARROW_ELEMS, seed=3)
    assert below["threshold"] == thr
    if thr >= 32:
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4 - 4, 16, None, tio, 16, 32, NARROW_VEC, seed=4)


# ---------------------------------------------------------------- the matrix
@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_indexed_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, on one
    wide shape (blocks with head and tail elements, the displacements another
    residue mod 16 from block to block so that blocks change path where the
    type can) and one narrow one, sized from the reported threshold.  What the
    reference's compute switch refuses (LAND / LOR on floating types) the call
    refuses with the same class, writing nothing."""
    esz = T.elem_size(t)
    thr = threshold(mpi) if not T.compute_ok(op, t) else threshold(mpi, t, op)
    stream = cuda.cuda.Stream()
    vec = max(16 // esz, 1)
    bl = -(-thr // esz) + TILE // esz + vec + 1
    pio = esz if esz < 16 else 0            # head elements where the type has any
    unit = min(esz, 16)
    tio = slots(3, 9, gap=0) * (bl * esz // unit + 16 // unit + 1)
    run(mpi, orc, cuda, stream, op, t, 3, bl, unit, None, tio, pio + 4096, pio, WIDE, seed=1)
    if 3 * esz < thr:                       # (a 16-byte element 8 bytes off: no vectors)
        tio = slots(37, 10, gap=0) * (5 * esz // unit)
        run(mpi, orc, cuda, stream, op, t, 37, 3, unit, None, tio, 0, esz if esz < 16 else 8, NARROW_ELEMS, seed=2)
    if esz <= 16 and 48 < thr:
        run(mpi, orc, cuda, stream, op, t, 37, 48 // esz, 16, slots(37, 11, gap=0) * 4, slots(37, 12, gap=0) * 5, 16, 0,
            NARROW_VEC, seed=3)


# ---------------------------------------------------------------- launches, routes, failures
def test_lowered_cap_forces_several_launches(mpi, orc, cuda):
    """The per-launch workgroup cap lowered to 3 (the strided call's hook): the
    narrow shapes split into block ranges with the table pointers and the packed
    base advanced, the wide one into single blocks; all exact."""
    lib = mpi.load()
    thr = threshold(mpi)
    stream = cuda.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        tio = slots(2731, 13, gap=0) * 4
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 16, None, tio, 0, 16, NARROW_VEC, seed=1,
            expect=lambda i: (i["launches"], i["rows_per_launch"], i["groups"]) == (3, 1024, 9) or pytest.fail(str(i)))
        tin = slots(2731, 14, gap=1) * 3
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 16, tin, tio, 0, 16, NARROW_VEC, seed=2,
            expect=lambda i: i["launches"] == 3 or pytest.fail(str(i)))
        t8 = slots(40000, 15, gap=0) * 7 + 2
        run(mpi, orc, cuda, stream, "MPI_BXOR", "MPI_UNSIGNED_CHAR", 40000, 3, 1, t8, None, 1, 2, NARROW_ELEMS, seed=3,
            expect=lambda i: (i["launches"], i["rows_per_launch"]) == (3, TILE) or pytest.fail(str(i)))
        bl = thr // 4 + TILE // 4 + 3
        tw = slots(5, 16, gap=0) * (bl + 5)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 5, bl, 4, None, tw, 0, 4, WIDE, seed=4,
            expect=lambda i: i["launches"] == -(-5 // max(1, 3 // i["per"])) > 1 or pytest.fail(str(i)))
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3


def test_single_call_rule(mpi, orc, cuda):
    """Both tables NULL goes through MPIR_Hip_reduce on nblocks x blocklen
    elements: the same result, and synchronously the direct AQL dispatch where
    it is up."""
    torch = cuda
    lib = mpi.load()
    lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
    state = lib.MPIR_Hip_direct_prepare(torch.cuda.current_device())
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb, bl = 37, 2703
    rng = np.random.default_rng(nb)
    a = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng)).reshape(1, -1)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng)).reshape(1, -1)
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, nb * bl, dt, o) == 0
    ain, aio = Arena(torch, b, [0], 0), Arena(torch, a, [0], 0)
    assert mpi.indexed_plan_info(ain.ptr, 0, aio.ptr, 0, 4, nb, bl, dt, o)["form"] == SINGLE
    stream = torch.cuda.Stream()
    for way in ("sync", "stream"):
        aio.upload()
        torch.cuda.synchronize()
        d0 = lib.MPIR_Hip_direct_dispatches()
        rc = mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, None, 4, nb, bl, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert rc == 0, mpi.error_string(rc)
        d1 = lib.MPIR_Hip_direct_dispatches()
        assert np.array_equal(aio.check(way), want), f"{way}: differs from the oracle"
        if state == 1:
            assert d1 - d0 == (1 if way == "sync" else 0), f"{way}: direct dispatches {d1 - d0}"


def test_no_partial_work(mpi, orc, cuda):
    """Residency is settled before the first launch: a host inbuf or inoutbuf, a
    host table whose highest block ends in host memory, and a host table on a
    stream all fail the call with MPI_ERR_BUFFER and nothing written, however
    many launches it would have made."""
    torch = cuda
    lib = mpi.load()
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb = 3000
    rng = np.random.default_rng(5)
    a = T.to_bytes(T.gen("MPI_FLOAT", nb * 12, rng)).reshape(nb, 48)
    tio = slots(nb, 17, gap=0) * 4
    aio = Arena(torch, a, tio * 16, 0)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * 12, rng)).reshape(nb, 48)
    ain = Arena(torch, b, np.arange(nb) * 48, 0)
    dtio = torch.from_numpy(tio).cuda()
    host_in = np.ones(nb * 12, dtype=np.float32)
    # one block displaced into this process's host memory: the highest block of the
    # table or the lowest, as the addresses fall -- the library classifies both ends
    far = tio.copy()
    far[np.argmax(tio)] = (host_in.ctypes.data - aio.ptr) // 16
    end = "highest" if host_in.ctypes.data > aio.ptr else "lowest"
    # the highest block 2^40 bytes past the arena, where no allocation is (the
    # library looks the address up; nothing dereferences it)
    beyond = tio.copy()
    beyond[np.argmax(tio)] += 1 << 36
    stream = torch.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(1) == 0          # several launches, had any been made
    try:
        def refused(rc, what):
            stream.synchronize()
            assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, f"{what}: {mpi.error_string(rc)}"
            assert "device-resident" in mpi.error_string(rc), what
            assert np.array_equal(aio.check(what), a), f"{what}: inoutbuf written by a refused call"
            assert np.array_equal(ain.check(what), b) and (host_in == 1).all(), what

        assert mpi.indexed_plan_info(ain.ptr, 0, aio.ptr, dtio.data_ptr(), 16, nb, 12, dt, o)["launches"] > 1
        for way, s in (("sync", 0), ("stream", stream.cuda_stream)):
            torch.cuda.synchronize()
            refused(mpi.reduce_local_indexed(host_in.ctypes.data, None, aio.ptr, dtio.data_ptr(), 16, nb, 12, dt, o, s),
                    f"{way}: host inbuf")
            refused(mpi.reduce_local_indexed(aio.ptr, dtio.data_ptr(), host_in.ctypes.data, None, 16, nb, 12, dt, o, s),
                    f"{way}: host inoutbuf")
            # a host table on a stream, though every block it names is device memory
            if s:
                refused(mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, tio, 16, nb, 12, dt, o, s), "host table on a stream")
                refused(mpi.reduce_local_indexed(aio.ptr, tio, ain.ptr, None, 16, nb, 12, dt, o, s),
                        "host input table on a stream")
        refused(mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, far, 16, nb, 12, dt, o), f"{end} block in host memory")
        refused(mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, beyond, 16, nb, 12, dt, o), "highest block past the arena")
        # a displacement whose byte offset overflows: MPI_ERR_ARG, nothing written
        big = tio.copy()
        big[7] = 1 << 60
        rc = mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, big, 16, nb, 12, dt, o)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG, mpi.error_string(rc)
        assert np.array_equal(aio.check("overflow"), a)
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 1
    # the same call with device operands and the host table runs
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, nb * 12, dt, o) == 0
    assert mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, tio, 16, nb, 12, dt, o) == 0
    assert np.array_equal(aio.check("all device"), want)


def test_host_tables_of_growing_size_reuse_the_table_buffer(mpi, orc, cuda):
    """The library's table buffer grows on demand: a small host table, one past
    its first size, and the small one again, both sides from the host."""
    stream = cuda.cuda.Stream()
    for nb in (100, 9000, 100):
        tin = slots(nb, nb, gap=0)
        tio = slots(nb, nb + 1, gap=1)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", nb, 2, 16, tin, tio, 0, 16, NARROW_VEC, seed=nb,
            ways=("host-tables",))


def test_captured_in_a_graph(mpi, orc, cuda):
    """With device tables the stream call carries everything else in its kernel
    arguments: captured into a graph (one stream, no parallel branches) and
    replayed twice it equals the oracle applied twice."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb, bl = 400, 12
    rng = np.random.default_rng(9)
    a = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng, specials=False)).reshape(nb, bl * 4)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng, specials=False)).reshape(nb, bl * 4)
    once = a.copy()
    assert orc.reduce_local(b.copy(), once, nb * bl, dt, o) == 0
    twice = once.copy()
    assert orc.reduce_local(b.copy(), twice, nb * bl, dt, o) == 0
    tio = slots(nb, 18, gap=0) * 4
    ain, aio = Arena(torch, b, np.arange(nb) * bl * 4, 0), Arena(torch, a, tio * 16, 16)
    dtio = torch.from_numpy(tio).cuda()
    assert mpi.indexed_plan_info(ain.ptr, 0, aio.ptr, dtio.data_ptr(), 16, nb, bl, dt, o)["form"] == NARROW_VEC
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_indexed(ain.ptr, None, aio.ptr, dtio.data_ptr(), 16, nb, bl, dt, o, cs) == 0
    torch.cuda.synchronize()
    # capture records, it does not run
    assert np.array_equal(aio.check("captured inoutbuf"), a)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("replayed twice"), twice)
    assert np.array_equal(ain.check("replayed twice inbuf"), b)
