"""MPIX_Reduce_local_strided without a GPU: its argument checks through the C
ABI, and its launch planner (MPIR_Hip_strided_plan_info: the planner the launch
itself runs, host arithmetic on the pointer values) on made-up addresses.

What the planner must get right is what the kernel relies on.  A wide row's
workgroup finds its row and tile by dividing by G, so G may never be below what
any row needs and the grid must be nblocks x G; each row's path and workgroups
are the batch's for the same pointers.  A narrow launch's workgroups must cover
its rows' units exactly, 16-byte units only where every address the kernel
forms is a multiple of 16.  A launch may hold no more workgroups than the cap.
Forms and the threshold are read from the planner, never assumed.
"""
import ctypes

import numpy as np
import pytest

import _types as T

TILE = 16384
BASE = 1 << 32
FAR = 1 << 40                # inoutbuf's arena, far from inbuf's
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
BATCH_TILE, BATCH_ELEMS = 1, 2
ENOKERNEL, EARG = 3, 5


def _host(n=64):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _plan(mpi, ai, si, ao, so, nb, bl, t="MPI_FLOAT", op="MPI_SUM"):
    return mpi.strided_plan_info(ai, si, ao, so, nb, bl, mpi.DATATYPES[t], mpi.OPS[op])


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_strided", "MPIR_Hip_reduce_strided", "MPIR_Hip_strided_plan_info",
                 "MPIR_Hip_set_strided_wide_bytes", "MPIR_Hip_strided_test_max_groups"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name


def test_negative_counts(mpi):
    a, b = _host()
    for nb, bl in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        rc = mpi.reduce_local_strided(b.ctypes.data, 16, a.ctypes.data, 32, nb, bl, mpi.MPI_FLOAT, mpi.MPI_SUM)
        assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT, (nb, bl, mpi.error_string(rc))
    assert not a.any()


def test_zero_counts_succeed_without_touching_a_pointer(mpi):
    for nb, bl in ((0, 4), (4, 0), (0, 0)):
        for pin, pio in ((WILD, WILD + 4), (WILD, WILD), (0, 0), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
            assert mpi.reduce_local_strided(pin, 16, pio, 32, nb, bl, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0, (nb, bl, pin)
        # an output stride that would overlap rows is not looked at either: there are no rows
        assert mpi.reduce_local_strided(WILD, 0, WILD + 4, 0, nb, bl, mpi.MPI_DOUBLE, mpi.MPI_MAX) == 0
        # ... but the op still is
        rc = mpi.reduce_local_strided(WILD, 16, WILD + 4, 32, nb, bl, mpi.MPI_FLOAT, mpi.MPI_OP_NULL)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP


@pytest.mark.parametrize("op", ["MPI_REPLACE", "MPI_NO_OP", "MPI_OP_NULL", "BAD_HANDLE"])
def test_ops_refused_as_in_reduce_local(mpi, op):
    handle = {"MPI_REPLACE": mpi.MPI_REPLACE, "MPI_NO_OP": mpi.MPI_NO_OP, "MPI_OP_NULL": mpi.MPI_OP_NULL,
              "BAD_HANDLE": 0x44000003}[op]
    a, b = _host()
    rc = mpi.reduce_local_strided(b.ctypes.data, 16, a.ctypes.data, 32, 4, 4, mpi.MPI_FLOAT, handle)
    single = mpi.reduce_local(b.ctypes.data, a.ctypes.data, 4, mpi.MPI_FLOAT, handle)
    assert mpi.error_class(rc) == mpi.error_class(single) == mpi.MPI_ERR_OP
    assert not a.any()


def test_user_op_refused_with_the_batchs_text(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    try:
        a, b = _host()
        rc = mpi.reduce_local_strided(b.ctypes.data, 16, a.ctypes.data, 32, 4, 4, mpi.MPI_FLOAT, op.value)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        assert "user MPI_Op functions run on the host" in mpi.error_string(rc)
        assert not a.any()
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0


def test_land_and_lor_on_floats_are_err_op(mpi):
    a, b = _host()
    for op in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            rc = mpi.reduce_local_strided(b.ctypes.data, 32, a.ctypes.data, 64, 2, 2, dt, op)
            assert mpi.error_class(rc) == mpi.MPI_ERR_OP
            assert "not defined for this datatype" in mpi.error_string(rc)
    # an op the type's check_dtype refuses outright
    rc = mpi.reduce_local_strided(b.ctypes.data, 32, a.ctypes.data, 64, 2, 2, mpi.MPI_FLOAT, mpi.MPI_BAND)
    assert mpi.error_class(rc) == mpi.MPI_ERR_OP
    assert not a.any()


def test_aliased_and_in_place(mpi):
    a, b = _host()
    rc = mpi.reduce_local_strided(a.ctypes.data, 32, a.ctypes.data, 32, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc)
    for pin, pio in ((mpi.MPI_IN_PLACE, a.ctypes.data), (b.ctypes.data, mpi.MPI_IN_PLACE)):
        rc = mpi.reduce_local_strided(pin, 32, pio, 32, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "MPI_IN_PLACE" in mpi.error_string(rc)
    assert not a.any()


def test_strides(mpi):
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    for si, so in ((-4, 32), (16, -32), (-1, -1)):
        rc = mpi.reduce_local_strided(pb, si, pa, so, 4, 4, f, s)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "negative" in mpi.error_string(rc)
    # output rows would overlap: one byte short of the row, and 0
    for so in (15, 12, 0):
        rc = mpi.reduce_local_strided(pb, 16, pa, so, 2, 4, f, s)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "overlap" in mpi.error_string(rc), so
    # a single row has no stride to check; in_stride may be anything >= 0.  All of
    # these pass the argument checks and are then refused as host memory
    for si, so, nb in ((16, 0, 1), (0, 16, 4), (4, 16, 4), (1000, 16, 4), (3, 17, 4)):
        rc = mpi.reduce_local_strided(pb, si, pa, so, nb, 4, f, s)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc), (si, so, nb)
    assert not a.any()


@pytest.mark.parametrize("nb,si,so", [(1, 16, 16), (4, 16, 16), (4, 16, 32), (300, 0, 16)],
                         ids=["one-row", "contiguous", "strided", "shared-row"])
def test_host_pointers_refused_as_non_device(mpi, nb, si, so):
    """The single-call shapes are no exception: the strided call never takes
    MPI_Reduce_local's host paths."""
    a, b = _host(2048)
    rc = mpi.reduce_local_strided(b.ctypes.data, si, a.ctypes.data, so, nb, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER
    assert "device-resident" in mpi.error_string(rc) and "aliased" not in mpi.error_string(rc)
    assert not a.any()


def test_shim_refuses_replace_unknown_pairs_and_bad_strides(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 8)()
    f32 = mpi.ELEM["F32"]

    def info(op, elem, so=64, nb=4, bl=4):
        return lib.MPIR_Hip_strided_plan_info(BASE, 16, FAR, so, nb, bl, op, elem, out)

    assert info(mpi.MPI_REPLACE & 0xF, f32) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_strided(BASE, 16, FAR, 64, 4, 4, mpi.MPI_REPLACE & 0xF, f32, None, 1) == ENOKERNEL
    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL            # no BAND on floats
    assert info(mpi.MPI_MAXLOC & 0xF, f32) == ENOKERNEL
    assert info(0, f32) == ENOKERNEL and info(mpi.MPI_SUM & 0xF, 99) == ENOKERNEL
    assert info(mpi.MPI_SUM & 0xF, f32) == 0
    assert info(mpi.MPI_SUM & 0xF, f32, so=15) == EARG           # output rows would overlap
    assert info(mpi.MPI_SUM & 0xF, f32, so=15, nb=1) == 0        # one row: no stride to check
    assert info(mpi.MPI_SUM & 0xF, f32, so=1 << 63, nb=3) == EARG      # a span past the address space
    assert lib.MPIR_Hip_reduce_strided(BASE, 16, FAR, 15, 4, 4, mpi.MPI_SUM & 0xF, f32, None, 1) == EARG
    with pytest.raises(ValueError):
        _plan(mpi, BASE, 16, FAR, 15, 4, 4)
    with pytest.raises(LookupError):
        _plan(mpi, BASE, 16, FAR, 64, 4, 4, op="MPI_BAND")


# ---------------------------------------------------------------- the planner
def test_empty_and_single(mpi):
    for nb, bl in ((0, 100), (100, 0)):
        info = _plan(mpi, WILD, 16, WILD, 16, nb, bl)
        assert (info["form"], info["launches"], info["groups"]) == (EMPTY, 0, 0)
    dt, o = mpi.DATATYPES["MPI_FLOAT"], mpi.OPS["MPI_SUM"]
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1)["threshold"]
    wide = thr // 4 + 7
    # one row, whatever the strides say; contiguous rows, narrow and wide, at any phase
    for ai, si, ao, so, nb, bl in ((BASE, 0, FAR, 0, 1, 100000), (BASE + 4, 12345, FAR, 1, 1, 100000),
                                   (BASE, 12, FAR + 8, 12, 3000, 3), (BASE + 4, 4 * wide, FAR, 4 * wide, 9, wide),
                                   (BASE + 4, 8, FAR + 8, 8, 3, 2)):
        info = _plan(mpi, ai, si, ao, so, nb, bl)
        single = mpi.plan_info(ai, ao, nb * bl, dt, o)
        assert info["form"] == SINGLE, info
        assert (info["launches"], info["groups"], info["rows_per_launch"]) == (1, single["groups"], nb), (info, single)
    # one stride off the row's bytes is not contiguous
    assert _plan(mpi, BASE, 12, FAR, 16, 3000, 3)["form"] != SINGLE
    assert _plan(mpi, BASE, 16, FAR, 12, 3000, 3)["form"] != SINGLE
    assert _plan(mpi, BASE, 0, FAR, 12, 3000, 3)["form"] != SINGLE


@pytest.mark.parametrize("op,t", [("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_UNSIGNED_CHAR"),
                                  ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX"), ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT")],
                         ids=["f32", "u8", "cf64", "ldi"])
def test_wide_rows_are_the_batchs_segments(mpi, op, t):
    """Base phases 0..15 and strides of every residue the type allows mod 16, so
    that rows change path within a call: each row's path and workgroups are
    MPIR_Hip_batch_plan_info's for that row's (in, io, blocklen); G is never
    below any row's count, and at most one above the least; the grid is nblocks x G."""
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, t, op)["threshold"]
    nb = 9
    both = 0
    for row_bytes in sorted({thr, thr + esz, -(-thr // TILE) * TILE, -(-thr // TILE) * TILE + TILE,
                             2 * TILE + 16 + esz, 3 * TILE - esz}):
        row_bytes = max(row_bytes, thr) // esz * esz
        bl = row_bytes // esz
        for phase in range(16):
            for res_o in (0, 4, 8, 12):
                for res_i, pin in ((0, 0), (4, 0), (res_o, phase), (8, 3)):
                    ai, ao = BASE + pin, FAR + TILE - 32 + phase
                    si, so = row_bytes + 16 * 5 + res_i, row_bytes + 16 * 3 + res_o
                    info = _plan(mpi, ai, si, ao, so, nb, bl, t, op)
                    segs = [(ai + r * si, ao + r * so, bl) for r in range(nb)]
                    batch = mpi.batch_plan_info(segs, dt, o)
                    what = f"{t} rows of {row_bytes} B, in +{pin}/{si}, io +{phase}/{so}: {info}, batch {batch}"
                    assert info["form"] == WIDE, what
                    assert info["tile_rows"] == batch["tile"] and info["elem_rows"] == batch["elems"], what
                    G = info["per"]
                    assert G >= max(batch["seg_groups"]) and G <= min(batch["seg_groups"]) + 1, what
                    assert (info["launches"], info["groups"], info["rows_per_launch"]) == (1, nb * G, nb), what
                    both += bool(batch["tile"] and batch["elems"])
    assert both or esz == 32


def test_wide_rows_on_the_grid_leave_no_idle_workgroup(mpi):
    """inoutbuf's base and stride both multiples of 16 KiB: every row starts a tile,
    and G is exactly every row's count; 8 KiB off, tile 0 is cut and G is one more."""
    t, op = "MPI_FLOAT", "MPI_SUM"
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1)["threshold"]
    bl = max(2 * TILE, -(-thr // TILE) * TILE) // 4
    tiles = bl * 4 // TILE
    for off, want in ((0, tiles), (8192, tiles + 1)):
        info = _plan(mpi, BASE, bl * 4, FAR + off, 4 * TILE + bl * 4, 6, bl)
        batch = mpi.batch_plan_info([(BASE + r * bl * 4, FAR + off + r * (4 * TILE + bl * 4), bl) for r in range(6)], dt, o)
        assert info["form"] == WIDE and info["per"] == want, info
        assert batch["seg_groups"] == [want] * 6 and info["groups"] == 6 * want
        assert info["tile_rows"] == 6
    # on the grid but the input another phase mod 16: element rows, the same G
    info = _plan(mpi, BASE + 4, bl * 4, FAR, 4 * TILE + bl * 4, 6, bl)
    assert info["per"] == tiles and info["elem_rows"] == 6


def test_form_flips_exactly_at_the_reported_threshold(mpi):
    lib = mpi.load()
    for t, op in (("MPI_FLOAT", "MPI_SUM"), ("MPI_UNSIGNED_CHAR", "MPI_BXOR"), ("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC")):
        esz = T.elem_size(t)
        thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, t, op)["threshold"]
        assert thr >= esz and thr % esz == 0
        so = 2 * thr
        at = _plan(mpi, BASE, 0, FAR, so, 7, thr // esz, t, op)
        below = _plan(mpi, BASE, 0, FAR, so, 7, thr // esz - 1, t, op)
        assert at["form"] == WIDE and at["threshold"] == thr, at
        assert below["form"] in (NARROW_VEC, NARROW_ELEMS) and below["threshold"] == thr, below
    # the run-time setter moves it; 0 makes every row wide
    prev = lib.MPIR_Hip_set_strided_wide_bytes(256)
    try:
        assert _plan(mpi, BASE, 0, FAR, 512, 7, 64)["form"] == WIDE
        assert _plan(mpi, BASE, 0, FAR, 512, 7, 63)["form"] == NARROW_ELEMS
        assert _plan(mpi, BASE, 0, FAR, 512, 7, 64)["threshold"] == 256
        assert lib.MPIR_Hip_set_strided_wide_bytes(0) == 256
        assert _plan(mpi, BASE, 0, FAR, 24, 7, 1)["form"] == WIDE
        lib.MPIR_Hip_set_strided_wide_bytes(1 << 40)
        assert _plan(mpi, BASE, 0, FAR, 24, 7, 1)["threshold"] == 1 << 30       # clamped: a row's units fit 32 bits
    finally:
        lib.MPIR_Hip_set_strided_wide_bytes(prev)
    assert _plan(mpi, BASE, 0, FAR, 0, 1, 1)["threshold"] == prev


def test_narrow_vec_needs_all_five_alignments(mpi):
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1)["threshold"]
    assert thr > 48
    good = dict(ai=BASE, si=48, ao=FAR, so=64, bl=12)

    def form(t="MPI_FLOAT", op="MPI_SUM", nb=400, **kw):
        a = dict(good, **kw)
        return _plan(mpi, a["ai"], a["si"], a["ao"], a["so"], nb, a["bl"], t, op)

    info = form()
    assert info["form"] == NARROW_VEC and info["per"] == TILE // 16, info
    assert info["groups"] == -(-400 * 3 // info["per"]) == 2            # 1200 vectors: the boundary falls inside a row
    assert form(si=0)["form"] == NARROW_VEC                             # one input row for every output row
    for broken in (dict(ai=BASE + 4), dict(ao=FAR + 8), dict(si=52), dict(so=72), dict(bl=13), dict(bl=11),
                   dict(ai=BASE + 16 + 1), dict(so=64 + 2)):
        info = form(**broken)
        assert info["form"] == NARROW_ELEMS and info["per"] == TILE // 4, (broken, info)
    # every 16-byte-or-smaller class takes vectors; the 32-byte classes never do
    assert form("MPI_UNSIGNED_CHAR", "MPI_BXOR", bl=48)["form"] == NARROW_VEC
    assert form("MPI_C_DOUBLE_COMPLEX", "MPI_SUM", bl=3)["form"] == NARROW_VEC
    wide = form("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC", si=64, so=96, bl=2)
    assert wide["form"] == NARROW_ELEMS and wide["per"] == TILE // 32


def test_narrow_workgroups_cover_the_units(mpi):
    # a column of doubles: one element per row, 2048 per workgroup
    col = _plan(mpi, BASE, 8, FAR, 24, 3000, 1, "MPI_DOUBLE", "MPI_SUM")
    assert (col["form"], col["per"], col["groups"], col["launches"]) == (NARROW_ELEMS, 2048, 2, 1)
    # 3 bytes at stride 7: 18000 byte units, the first workgroup's span ends inside row 5461
    u8 = _plan(mpi, BASE, 3, FAR, 7, 6000, 3, "MPI_UNSIGNED_CHAR", "MPI_BXOR")
    assert (u8["form"], u8["per"], u8["groups"]) == (NARROW_ELEMS, TILE, 2) and TILE % 3
    for nb in (1365, 1366, 2 * 1365 + 1, 2731):
        assert _plan(mpi, BASE, 48, FAR, 64, nb, 12)["groups"] == -(-nb * 3 // 1024), nb


def test_launches_split_at_the_cap_and_at_a_lowered_cap(mpi):
    lib = mpi.load()
    cap = mpi.BATCH_MAX_GROUPS
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1)["threshold"]
    # wide rows at the real cap: G workgroups a row, whole rows per launch
    bl = max(thr, 3 * TILE) // 4 + 1
    nb = 2 ** 23
    info = _plan(mpi, BASE, 0, FAR + 4, bl * 4 + 4, nb, bl)
    G = info["per"]
    assert info["form"] == WIDE and G >= 2
    assert info["rows_per_launch"] == cap // G
    assert info["launches"] == -(-nb // (cap // G)) and info["groups"] == nb * G
    assert info["rows_per_launch"] * G <= cap
    # narrow rows at the real cap: INT_MAX rows of one 16-byte vector below it, rows of 255 vectors above it
    one = _plan(mpi, BASE, 0, FAR, 16, 2 ** 31 - 1, 4)
    assert (one["form"], one["launches"], one["groups"]) == (NARROW_VEC, 1, -(-(2 ** 31 - 1) // 1024))
    assert one["groups"] <= cap
    if thr >= 4096:
        nb = 100_000_000
        big = _plan(mpi, BASE, 0, FAR, 4096, nb, 1020)
        rpl = cap * 1024 // 255
        assert big["form"] == NARROW_VEC and big["rows_per_launch"] == rpl < 2 ** 32
        assert big["launches"] == -(-nb // rpl)
        assert big["groups"] == (nb // rpl) * -(-rpl * 255 // 1024) + -(-(nb % rpl) * 255 // 1024)
        assert -(-rpl * 255 // 1024) <= cap
    # a lowered cap (the calling thread's): the same arithmetic at a small size
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        narrow = _plan(mpi, BASE, 48, FAR, 64, 2731, 12)                # 8193 vectors, 1024 per workgroup
        assert narrow["rows_per_launch"] == 3 * 1024 // 3 == 1024
        assert (narrow["launches"], narrow["groups"]) == (3, 3 + 3 + 3)
        wide = _plan(mpi, BASE, 0, FAR + 4, bl * 4 + 4, 7, bl)
        assert wide["form"] == WIDE and wide["rows_per_launch"] == max(1, 3 // G)       # a row is never split
        assert wide["launches"] == -(-7 // wide["rows_per_launch"]) and wide["groups"] == 7 * G
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3
        assert _plan(mpi, BASE, 48, FAR, 64, 2731, 12)["launches"] == 1
    finally:
        lib.MPIR_Hip_strided_test_max_groups(0)
