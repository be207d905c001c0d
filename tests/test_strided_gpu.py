"""MPIX_Reduce_local_strided on the GPU: the rows of a vector-shaped operand in
one launch, every row the oracle's MPI_Reduce_local on it (bit-exact,
test_parity_gpu.same's complex-NaN rule).

Each operand sits in an arena of its own, filled with 0xA5, its row 0 at a
chosen byte phase of the 16 KiB grid.  After each call every row of inoutbuf
must equal the oracle's, every other byte of the arena -- the gaps between rows
included -- must still be 0xA5, and the input arena must be unchanged: a
workgroup that took the wrong row, a flattened unit mapped one row off, a tile
cut at the wrong byte all show there.  Before a shape runs,
MPIR_Hip_strided_plan_info -- the launch's own planner -- must report the form
the shape was built for; sizes hang on the threshold it reports, never on a
number written here.  Every shape runs twice: synchronously on the library
stream, and enqueued on a torch stream that is then synchronised.
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


class Image:
    """A device allocation filled with 0xA5 around `rows` (n x row bytes), row r
    at `phase` bytes past a 16 KiB boundary plus r x stride."""

    def __init__(self, torch, rows, stride, phase):
        n, rb = rows.shape
        assert n == 1 or stride >= rb
        self.torch = torch
        self.t = torch.empty((n - 1) * stride + rb + 4 * TILE, dtype=torch.uint8, device="cuda")
        off = -self.t.data_ptr() % TILE + TILE + phase
        self.ptr = self.t.data_ptr() + off
        self.idx = off + np.arange(n)[:, None] * stride + np.arange(rb)[None, :]
        self.host = np.full(self.t.numel(), FILL, np.uint8)
        self.host[self.idx] = rows
        self.guard = np.ones(self.t.numel(), bool)
        self.guard[self.idx] = False
        self.upload()

    def upload(self):
        self.t.copy_(self.torch.from_numpy(self.host))

    def check(self, what):
        """The rows' bytes, after asserting that nothing around or between them was written."""
        self.torch.cuda.synchronize()
        whole = self.t.cpu().numpy()
        bad = np.nonzero(self.guard & (whole != FILL))[0]
        assert not bad.size, f"{what}: guard bytes written at arena offsets {(bad[:8] - self.idx[0, 0]).tolist()} from row 0"
        return whole[self.idx]


def threshold(mpi, t="MPI_FLOAT", op="MPI_SUM"):
    return mpi.strided_plan_info(1 << 32, 0, 1 << 40, 0, 1, 1, mpi.DATATYPES[t], mpi.OPS[op])["threshold"]


def run(mpi, orc, torch, stream, op, t, nb, bl, si, so, pin, pio, form, seed=0, expect=None):
    """nb rows of bl elements, inbuf at phase pin and stride si (0: one row),
    inoutbuf at phase pio and stride so.  Asserts the planner's form, runs the
    call both ways and checks both arenas.  expect(info): further plan checks.
    Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    rb = bl * esz
    rng = np.random.default_rng([seed, nb, bl])
    nin = nb if si else 1
    a = T.to_bytes(T.gen(t, nb * bl, rng, op)).reshape(nb, rb)          # inout rows
    b = T.to_bytes(T.gen(t, nin * bl, rng, op)).reshape(nin, rb)        # in rows
    want = a.copy()
    rcs = {orc.reduce_local(b[r if si else 0].copy(), want[r], bl, dt, o) for r in range(nb)}   # row by row
    assert len(rcs) == 1
    rc_want = rcs.pop()
    ain, aio = Image(torch, b, si, pin), Image(torch, a, so, pio)
    what = f"{op} {t} {nb} x {bl} in=+{pin}/{si} io=+{pio}/{so}"
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.strided_plan_info(ain.ptr, si, aio.ptr, so, nb, bl, dt, o)
        assert info["form"] == form, f"{what}: aimed at {FORMS[form]}, the planner says {info}"
        if expect:
            expect(info)
    for way in ("sync", "stream"):
        if way == "stream":
            aio.upload()
        torch.cuda.synchronize()
        rc = mpi.reduce_local_strided(ain.ptr, si, aio.ptr, so, nb, bl, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        assert np.array_equal(ain.check(f"{what} {way} inbuf"), b), f"{what} {way}: inbuf modified"
        for r in range(nb):
            if not same(got[r], want[r], t):
                pytest.fail(f"{what} {way} ({FORMS[form]}) row {r}:\n" + explain(got[r], want[r], a[r], b[r if si else 0], esz))
    return info


# ---------------------------------------------------------------- wide rows
def test_wide_rows_on_both_paths(mpi, orc, cuda):
    """5 rows of 3 x 4096 + 7 floats, the input packed, the output 36 bytes
    further apart per row, the bases 4 bytes apart: the rows' pointers share
    their offset mod 16 in some rows and not in others."""
    bl = 3 * 4096 + 7
    assert bl * 4 >= threshold(mpi)

    def both(info):
        assert info["tile_rows"] >= 1 and info["elem_rows"] >= 1 and info["tile_rows"] + info["elem_rows"] == 5, info
        assert info["groups"] == 5 * info["per"] and info["launches"] == 1, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 5, bl, bl * 4, bl * 4 + 36, 0, 4, WIDE, expect=both)


@pytest.mark.parametrize("off", [0, 8192], ids=["on-grid", "8KiB-off"])
def test_wide_rows_of_two_tiles(mpi, orc, cuda, off):
    """Rows of exactly two tiles, bases and strides on the 16 KiB grid: two
    workgroups a row, none idle.  8 KiB off the grid tile 0 is cut and every row
    takes three; G covers them."""
    bl = 2 * TILE // 4
    assert bl * 4 >= threshold(mpi)

    def grid(info):
        assert info["per"] == (2 if off == 0 else 3) and info["tile_rows"] == 6 and info["groups"] == 6 * info["per"], info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 6, bl, 3 * TILE, 4 * TILE, off, off, WIDE, seed=off,
        expect=grid)
    # rows that need one workgroup fewer than G: the trailing one of each row idles
    def idle(info):
        assert info["per"] == 3 and info["groups"] == 18, info
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 6, bl, 3 * TILE, 4 * TILE + 16, off, off, WIDE,
        seed=off + 1, expect=idle if off == 0 else None)


def test_threshold_and_one_element_below(mpi, orc, cuda):
    """Row bytes at the reported threshold take the wide form, one element less
    the narrow one; both exact."""
    thr = threshold(mpi)
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4, thr, thr + 64, 16, 32, WIDE, seed=1)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4, thr, thr + 68, 16, 32, WIDE, seed=2)
    below = run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4 - 1, thr, thr + 64, 16, 32, NARROW_ELEMS, seed=3)
    assert below["threshold"] == thr
    if thr >= 32:
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 7, thr // 4 - 4, thr, thr + 64, 16, 32, NARROW_VEC, seed=4)


def test_in_stride_zero(mpi, orc, cuda):
    """One input row combined into every output row, wide and narrow."""
    thr = threshold(mpi)
    stream = cuda.cuda.Stream()
    bl = thr // 4 + TILE // 4 + 5
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 6, bl, 0, bl * 4 + 12, 0, 0, WIDE, seed=1)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 700, 8, 0, 48, 0, 16, NARROW_VEC, seed=2)
    run(mpi, orc, cuda, stream, "MPI_MAX", "MPI_DOUBLE", 700, 3, 0, 40, 8, 0, NARROW_ELEMS, seed=3)


def test_wide_rows_of_the_32_byte_class(mpi, orc, cuda):
    """MPI_LONG_DOUBLE_INT MAXLOC: every row the element form, 512 elements a workgroup."""
    thr = threshold(mpi, "MPI_LONG_DOUBLE_INT", "MPI_MAXLOC")
    bl = max(thr // 32, 512) + 513

    def elems(info):
        assert info["tile_rows"] == 0 and info["elem_rows"] == 4 and info["per"] == -(-bl // 512), info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAXLOC", "MPI_LONG_DOUBLE_INT", 4, bl, bl * 32 + 16, bl * 32 + 48, 16, 0,
        WIDE, expect=elems)


# ---------------------------------------------------------------- narrow rows
def test_column_of_doubles(mpi, orc, cuda):
    """blocklen 1: 3000 doubles 24 bytes apart, two workgroups."""
    assert 8 < threshold(mpi, "MPI_DOUBLE")

    def two(info):
        assert info["groups"] == 2 and info["per"] == TILE // 8, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_DOUBLE", 3000, 1, 8, 24, 0, 0, NARROW_ELEMS, expect=two)


def test_bytes_at_an_odd_stride(mpi, orc, cuda):
    """3 bytes at stride 7, 6000 rows: 16384 is no multiple of 3, so the first
    workgroup's span ends inside a row, and no element is aligned."""
    assert 3 < threshold(mpi, "MPI_UNSIGNED_CHAR", "MPI_BXOR")

    def two(info):
        assert info["groups"] == 2 and info["per"] % 3, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", 6000, 3, 5, 7, 1, 3, NARROW_ELEMS, expect=two)


@pytest.mark.parametrize("off,form", [(0, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "base-4-off"])
def test_rows_of_three_vectors(mpi, orc, cuda, off, form):
    """12 floats at strides 64 (inout) and 48 (in) on 16-byte bases, 400 rows:
    1200 vectors, the workgroups' boundary inside a row.  A base 4 bytes off
    takes the element form: 4800 elements, 4096 a workgroup, the boundary again
    inside a row."""
    assert 48 < threshold(mpi)

    def two(info):
        assert info["groups"] == 2 and (400 * 3) % 1024 and 4096 % 12, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 400, 12, 48, 64, 16, 32 + off, form, seed=off, expect=two)


# ---------------------------------------------------------------- the matrix
@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_strided_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, on one
    wide shape (rows with head and tail elements, the strides another residue
    mod 16 so that rows change path where the type can) and one narrow one.
    What the reference's compute switch refuses (LAND / LOR on floating types)
    the call refuses with the same class, writing nothing."""
    esz = T.elem_size(t)
    thr = threshold(mpi) if not T.compute_ok(op, t) else threshold(mpi, t, op)
    stream = cuda.cuda.Stream()
    vec = max(16 // esz, 1)
    bl = -(-thr // esz) + TILE // esz + vec + 1
    pio = esz if esz < 16 else 0            # head elements where the type has any
    run(mpi, orc, cuda, stream, op, t, 3, bl, bl * esz + 5 * esz, bl * esz + 16 + esz, pio + 4096, pio, WIDE, seed=1)
    if 3 * esz < thr:                       # (a 16-byte element 8 bytes off: no vectors)
        run(mpi, orc, cuda, stream, op, t, 37, 3, 4 * esz, 5 * esz, 0, esz if esz < 16 else 8, NARROW_ELEMS, seed=2)
    if esz <= 16 and 48 < thr:
        run(mpi, orc, cuda, stream, op, t, 37, 48 // esz, 64, 80, 16, 0, NARROW_VEC, seed=3)


# ---------------------------------------------------------------- launches, routes, failures
def test_lowered_cap_forces_several_launches(mpi, orc, cuda):
    """The per-launch workgroup cap lowered to 3: the narrow shapes split into row
    ranges with the bases advanced, the wide one into single rows; all exact."""
    lib = mpi.load()
    thr = threshold(mpi)
    stream = cuda.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 2731, 12, 48, 64, 0, 16, NARROW_VEC, seed=1,
            expect=lambda i: (i["launches"], i["rows_per_launch"], i["groups"]) == (3, 1024, 9) or pytest.fail(str(i)))
        run(mpi, orc, cuda, stream, "MPI_BXOR", "MPI_UNSIGNED_CHAR", 40000, 3, 3, 7, 1, 2, NARROW_ELEMS, seed=2,
            expect=lambda i: (i["launches"], i["rows_per_launch"]) == (3, TILE) or pytest.fail(str(i)))
        bl = thr // 4 + TILE // 4 + 3
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 5, bl, bl * 4, bl * 4 + 20, 0, 4, WIDE, seed=3,
            expect=lambda i: i["launches"] == -(-5 // max(1, 3 // i["per"])) > 1 or pytest.fail(str(i)))
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3


@pytest.mark.parametrize("shape", ["one-row", "contiguous"])
def test_single_call_rule(mpi, orc, cuda, shape):
    """One row, or contiguous rows, goes through MPIR_Hip_reduce: the same
    result, and synchronously the direct AQL dispatch where it is up."""
    torch = cuda
    lib = mpi.load()
    lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
    state = lib.MPIR_Hip_direct_prepare(torch.cuda.current_device())
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    nb, bl, si, so = (1, 100003, 12, 0) if shape == "one-row" else (37, 2703, 2703 * 4, 2703 * 4)
    rng = np.random.default_rng(nb)
    a = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng)).reshape(1, -1)
    b = T.to_bytes(T.gen("MPI_FLOAT", nb * bl, rng)).reshape(1, -1)
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, nb * bl, dt, o) == 0
    ain, aio = Image(torch, b, 0, 0), Image(torch, a, 0, 0)
    assert mpi.strided_plan_info(ain.ptr, si, aio.ptr, so, nb, bl, dt, o)["form"] == SINGLE
    stream = torch.cuda.Stream()
    for way in ("sync", "stream"):
        aio.upload()
        torch.cuda.synchronize()
        d0 = lib.MPIR_Hip_direct_dispatches()
        rc = mpi.reduce_local_strided(ain.ptr, si, aio.ptr, so, nb, bl, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert rc == 0, mpi.error_string(rc)
        d1 = lib.MPIR_Hip_direct_dispatches()
        assert np.array_equal(aio.check(way), want), f"{way}: differs from the oracle"
        if state == 1:
            assert d1 - d0 == (1 if way == "sync" else 0), f"{way}: direct dispatches {d1 - d0}"


def test_no_partial_work(mpi, orc, cuda):
    """Residency is settled before the first launch: a host inbuf (or inoutbuf)
    fails the call with nothing written, however many launches it would have made."""
    torch = cuda
    lib = mpi.load()
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    rng = np.random.default_rng(5)
    a = T.to_bytes(T.gen("MPI_FLOAT", 3000 * 12, rng)).reshape(3000, 48)
    aio = Image(torch, a, 64, 0)
    host_in = np.ones(3000 * 12, dtype=np.float32)
    stream = torch.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(1) == 0          # several launches, had any been made
    try:
        for way in ("sync", "stream"):
            torch.cuda.synchronize()
            rc = mpi.reduce_local_strided(host_in.ctypes.data, 48, aio.ptr, 64, 3000, 12, dt, o,
                                          0 if way == "sync" else stream.cuda_stream)
            stream.synchronize()
            assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
            assert "device-resident" in mpi.error_string(rc)
            assert np.array_equal(aio.check(way), a), f"{way}: inoutbuf written by a refused call"
            # a host inoutbuf under a device inbuf
            rc = mpi.reduce_local_strided(aio.ptr, 64, host_in.ctypes.data, 48, 3000, 12, dt, o,
                                          0 if way == "sync" else stream.cuda_stream)
            assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
            assert (host_in == 1).all()
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 1
    # the same call with a device inbuf runs
    b = T.to_bytes(T.gen("MPI_FLOAT", 3000 * 12, rng)).reshape(3000, 48)
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, 3000 * 12, dt, o) == 0
    ain = Image(torch, b, 48, 0)
    assert mpi.reduce_local_strided(ain.ptr, 48, aio.ptr, 64, 3000, 12, dt, o) == 0
    assert np.array_equal(aio.check("all device"), want)
