"""MPIX_Reduce_local_indexed without a GPU: its argument checks through the C
ABI, and its launch planner (MPIR_Hip_indexed_plan_info: the planner the launch
itself runs, host arithmetic on the pointer values; a table is only compared
with NULL) on made-up addresses.

What the planner must get right is what the kernel relies on.  A wide block's
workgroup finds its block and tile by dividing by G, and the host cannot see
where a device table puts a block, so G may never be below what a block of that
length needs at ANY address.  A narrow launch's workgroups must cover its
blocks' units exactly, 16-byte units only where every address the kernel forms
is provably a multiple of 16 whatever the table holds.  A launch may hold no
more workgroups than the cap, and the launches partition the blocks.  Forms and
the threshold are read from the planner, never assumed.

(A host table with a stream is MPI_ERR_BUFFER, but on a machine without a GPU
every call with made-up bases is MPI_ERR_BUFFER already: that check is in
test_indexed_gpu.py.)
"""
import ctypes

import numpy as np
import pytest

import _types as T

TILE = 16384
BASE = 1 << 32
FAR = 1 << 40                # inoutbuf's arena, far from inbuf's
TAB_I, TAB_O = 1 << 44, (1 << 44) + (1 << 30)       # where device tables would be
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
ENOKERNEL, EARG = 3, 5


def _host(n=64):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _plan(mpi, ai, ti, ao, to, unit, nb, bl, t="MPI_FLOAT", op="MPI_SUM"):
    return mpi.indexed_plan_info(ai, ti, ao, to, unit, nb, bl, mpi.DATATYPES[t], mpi.OPS[op])


def _call(mpi, b, a, nb=4, bl=4, unit=16, dt=None, op=None, tab=None):
    tab = np.arange(nb if nb > 0 else 1, dtype=np.int64) if tab is None else tab
    return mpi.reduce_local_indexed(b, None, a, tab, unit, nb, bl, mpi.MPI_FLOAT if dt is None else dt,
                                    mpi.MPI_SUM if op is None else op)


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_indexed", "MPIR_Hip_reduce_indexed", "MPIR_Hip_indexed_plan_info"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    assert mpi.INDEXED_NAMES == ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
    assert (mpi.INDEXED_EMPTY, mpi.INDEXED_SINGLE, mpi.INDEXED_WIDE, mpi.INDEXED_NARROW_VEC,
            mpi.INDEXED_NARROW_ELEMS) == (EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS)


def test_negative_counts(mpi):
    a, b = _host()
    for nb, bl in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, nb, bl)
        assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT, (nb, bl, mpi.error_string(rc))
    assert not a.any()


def test_zero_counts_succeed_without_touching_a_pointer_or_a_table(mpi):
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    for nb, bl in ((0, 4), (4, 0), (0, 0)):
        for pin, pio in ((WILD, WILD + 4), (WILD, WILD), (0, 0), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
            for ti, to in ((WILD, WILD), (0, WILD), (WILD, 0), (0, 0)):
                assert mpi.reduce_local_indexed(pin, ti, pio, to, 4, nb, bl, f, s) == 0, (nb, bl, pin, ti, to)
                # ... on a stream too: a wild (host) table is not looked at either
                assert mpi.reduce_local_indexed(pin, ti, pio, to, 4, nb, bl, f, s, stream=WILD) == 0
        # ... but the op still is
        rc = mpi.reduce_local_indexed(WILD, 0, WILD + 4, WILD, 4, nb, bl, f, mpi.MPI_OP_NULL)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP


@pytest.mark.parametrize("op", ["MPI_REPLACE", "MPI_NO_OP", "MPI_OP_NULL", "BAD_HANDLE"])
def test_ops_refused_as_in_reduce_local(mpi, op):
    handle = {"MPI_REPLACE": mpi.MPI_REPLACE, "MPI_NO_OP": mpi.MPI_NO_OP, "MPI_OP_NULL": mpi.MPI_OP_NULL,
              "BAD_HANDLE": 0x44000003}[op]
    a, b = _host()
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, op=handle)
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
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, op=op.value)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        assert "user MPI_Op functions run on the host" in mpi.error_string(rc)
        assert not a.any()
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0


def test_land_and_lor_on_floats_are_err_op(mpi):
    a, b = _host()
    for op in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            rc = _call(mpi, b.ctypes.data, a.ctypes.data, 2, 2, dt=dt, op=op)
            single = mpi.reduce_local(b.ctypes.data, a.ctypes.data, 2, dt, op)
            assert mpi.error_class(rc) == mpi.error_class(single) == mpi.MPI_ERR_OP
            assert "not defined for this datatype" in mpi.error_string(rc)
    # an op the type's check_dtype refuses outright
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, 2, 2, op=mpi.MPI_BAND)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local(b.ctypes.data, a.ctypes.data, 2, mpi.MPI_FLOAT,
                                                                   mpi.MPI_BAND)) == mpi.MPI_ERR_OP
    assert not a.any()


def test_aliased_and_in_place(mpi):
    a, b = _host()
    rc = _call(mpi, a.ctypes.data, a.ctypes.data)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc)
    for pin, pio in ((mpi.MPI_IN_PLACE, a.ctypes.data), (b.ctypes.data, mpi.MPI_IN_PLACE)):
        rc = _call(mpi, pin, pio)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "MPI_IN_PLACE" in mpi.error_string(rc)
    assert not a.any()


def test_disp_unit_must_be_positive(mpi):
    a, b = _host()
    for unit in (0, -1, -16):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, unit=unit)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc), unit
    # an empty call is no exception (the strided call checks the sign of its strides
    # before it returns for an empty one too), and both layers say so: the MPIX
    # entry MPI_ERR_ARG with no pointer looked at, the planner ValueError
    for nb, bl in ((0, 4), (4, 0), (0, 0)):
        for unit in (0, -1):
            rc = mpi.reduce_local_indexed(WILD, None, WILD + 4, WILD, unit, nb, bl, mpi.MPI_FLOAT, mpi.MPI_SUM)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc), (nb, bl, unit)
        with pytest.raises(ValueError):
            _plan(mpi, WILD, 0, WILD, WILD, 0, nb, bl)
        assert mpi.reduce_local_indexed(WILD, None, WILD + 4, WILD, 1, nb, bl, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    # the op is looked at first, as the strided call looks at it before its strides
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, unit=0, op=mpi.MPI_REPLACE)
    assert mpi.error_class(rc) == mpi.MPI_ERR_OP
    # every positive unit passes the argument checks; the operands are then refused as host memory
    for unit in (1, 3, 4, 16, 1 << 40):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, unit=unit)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc), unit
    assert not a.any()


@pytest.mark.parametrize("ti,to", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["single", "scatter", "gather", "both"])
def test_host_pointers_refused_as_non_device(mpi, ti, to):
    """The single-call shape is no exception: the indexed call never takes
    MPI_Reduce_local's host paths."""
    a, b = _host(2048)
    tab = np.arange(300, dtype=np.int64)
    rc = mpi.reduce_local_indexed(b.ctypes.data, tab if ti else None, a.ctypes.data, tab if to else None, 16, 300, 4,
                                  mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER
    assert "device-resident" in mpi.error_string(rc) and "aliased" not in mpi.error_string(rc)
    assert not a.any()


def test_shim_refuses_replace_unknown_pairs_and_bad_units(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 6)()
    f32 = mpi.ELEM["F32"]

    def info(op, elem, unit=16, nb=4, bl=4):
        return lib.MPIR_Hip_indexed_plan_info(BASE, None, FAR, TAB_O, unit, nb, bl, op, elem, out)

    assert info(mpi.MPI_REPLACE & 0xF, f32) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_indexed(BASE, None, FAR, TAB_O, 16, 4, 4, mpi.MPI_REPLACE & 0xF, f32, None, 1) == ENOKERNEL
    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL            # no BAND on floats
    assert info(mpi.MPI_MAXLOC & 0xF, f32) == ENOKERNEL
    assert info(0, f32) == ENOKERNEL and info(mpi.MPI_SUM & 0xF, 99) == ENOKERNEL
    assert info(mpi.MPI_SUM & 0xF, f32) == 0
    assert info(mpi.MPI_SUM & 0xF, f32, unit=0) == EARG
    assert info(mpi.MPI_SUM & 0xF, f32, unit=1 << 63) == EARG     # no MPI_Aint holds it
    # ... whatever the counts, as the MPIX entry answers (test_disp_unit_must_be_positive)
    assert info(mpi.MPI_SUM & 0xF, f32, unit=0, nb=0) == EARG and info(mpi.MPI_SUM & 0xF, f32, unit=0, bl=0) == EARG
    assert lib.MPIR_Hip_reduce_indexed(WILD, None, WILD, WILD, 0, 0, 4, mpi.MPI_SUM & 0xF, f32, None, 1) == EARG
    assert info(mpi.MPI_SUM & 0xF, f32, unit=1, nb=0) == 0        # no blocks: no pointer is looked at
    assert info(mpi.MPI_SUM & 0xF, f32, nb=1 << 40, bl=1 << 40) == EARG      # a packed side past the address space
    assert lib.MPIR_Hip_reduce_indexed(BASE, None, FAR, TAB_O, 0, 4, 4, mpi.MPI_SUM & 0xF, f32, None, 1) == EARG
    with pytest.raises(ValueError):
        _plan(mpi, BASE, 0, FAR, TAB_O, 0, 4, 4)
    with pytest.raises(LookupError):
        _plan(mpi, BASE, 0, FAR, TAB_O, 16, 4, 4, op="MPI_BAND")
    with pytest.raises(TypeError):
        _plan(mpi, BASE, 0, FAR, np.arange(4, dtype=np.int32), 16, 4, 4)


# ---------------------------------------------------------------- the planner
def test_empty_and_single(mpi):
    for nb, bl in ((0, 100), (100, 0)):
        info = _plan(mpi, WILD, WILD, WILD, WILD, 4, nb, bl)
        assert (info["form"], info["launches"], info["groups"]) == (EMPTY, 0, 0)
    dt, o = mpi.DATATYPES["MPI_FLOAT"], mpi.OPS["MPI_SUM"]
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1)["threshold"]
    wide = thr // 4 + 7
    # both tables NULL: the single call on nblocks x blocklen elements, narrow and wide blocks, at any phase
    for ai, ao, nb, bl in ((BASE, FAR, 1, 100000), (BASE + 4, FAR, 1, 100000), (BASE, FAR + 8, 3000, 3),
                           (BASE + 4, FAR, 9, wide), (BASE + 4, FAR + 8, 3, 2)):
        for unit in (1, 16, 12345):
            info = _plan(mpi, ai, 0, ao, 0, unit, nb, bl)
            single = mpi.plan_info(ai, ao, nb * bl, dt, o)
            assert info["form"] == SINGLE, info
            assert (info["launches"], info["groups"], info["rows_per_launch"]) == (1, single["groups"], nb), (info, single)
    # one table, either side, is not the single call -- not even for one block
    assert _plan(mpi, BASE, TAB_I, FAR, 0, 4, 3000, 3)["form"] != SINGLE
    assert _plan(mpi, BASE, 0, FAR, TAB_O, 4, 3000, 3)["form"] != SINGLE
    assert _plan(mpi, BASE, 0, FAR, TAB_O, 4, 1, 3)["form"] != SINGLE


@pytest.mark.parametrize("op,t", [("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_UNSIGNED_CHAR"),
                                  ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX"), ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT")],
                         ids=["f32", "u8", "cf64", "ldi"])
def test_wide_G_covers_a_block_at_every_phase(mpi, op, t):
    """The grid is nblocks x G, and G is at least MPIR_Hip_batch_plan_info's
    workgroups for a segment of the block's length wherever a table may put it:
    inoutbuf phases mod 16 KiB in steps of the element around the tile and the
    16-byte boundaries, the input at the same phase mod 16 (tile path) and at
    another (element path).  G is also no more than one above the least."""
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1, t, op)["threshold"]
    nb = 9
    step = min(esz, 16)
    phases = sorted({p % TILE for c in (0, 16, 8192, TILE - 16, TILE) for p in range(c - 2 * 16, c + 2 * 16 + 1, step)})
    paths = set()
    for row_bytes in sorted({thr, thr + esz, -(-thr // TILE) * TILE, -(-thr // TILE) * TILE + TILE,
                             -(-thr // TILE) * TILE + 16, 2 * TILE + 16 + esz, 3 * TILE - esz, 3 * TILE + 15}):
        row_bytes = max(row_bytes, thr) // esz * esz
        bl = row_bytes // esz
        plans = [_plan(mpi, BASE, ti, FAR + 4 * (ti == 0), to, unit, nb, bl, t, op)
                 for ti, to, unit in ((0, TAB_O, 1), (TAB_I, 0, 16), (TAB_I, TAB_O, esz))]
        info = plans[0]
        assert all(p == info for p in plans), plans         # G depends on the length alone
        G = info["per"]
        assert info["form"] == WIDE
        assert (info["launches"], info["groups"], info["rows_per_launch"]) == (1, nb * G, nb), info
        segs = [(BASE + (pi if same else pi + min(esz, 8)), FAR + po, bl) for po in phases for pi in (po % 16, po % 16 + 4 * TILE)
                for same in (True, False)]
        need = []
        for k in range(0, len(segs), 100):
            batch = mpi.batch_plan_info(segs[k:k + 100], dt, o)
            need += batch["seg_groups"]
            paths |= {"tile"} if batch["tile"] else set()
            paths |= {"elems"} if batch["elems"] else set()
        assert G >= max(need), (t, row_bytes, G, max(need))
        assert G <= min(need) + 1, (t, row_bytes, G, min(need))
    assert paths == ({"elems"} if esz == 32 else {"tile", "elems"})


def test_form_flips_exactly_at_the_reported_threshold(mpi):
    lib = mpi.load()
    for t, op in (("MPI_FLOAT", "MPI_SUM"), ("MPI_UNSIGNED_CHAR", "MPI_BXOR"), ("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC")):
        esz = T.elem_size(t)
        thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1, t, op)["threshold"]
        assert thr >= esz and thr % esz == 0
        assert thr == mpi.strided_plan_info(BASE, 0, FAR, 0, 1, 1, mpi.DATATYPES[t], mpi.OPS[op])["threshold"]
        at = _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, thr // esz, t, op)
        below = _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, thr // esz - 1, t, op)
        assert at["form"] == WIDE and at["threshold"] == thr, at
        assert below["form"] in (NARROW_VEC, NARROW_ELEMS) and below["threshold"] == thr, below
    # the strided call's run-time setter moves it; 0 makes every block wide
    prev = lib.MPIR_Hip_set_strided_wide_bytes(256)
    try:
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, 64)["form"] == WIDE
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, 63)["form"] == NARROW_ELEMS
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, 60)["form"] == NARROW_VEC
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, 64)["threshold"] == 256
        assert lib.MPIR_Hip_set_strided_wide_bytes(0) == 256
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 7, 1)["form"] == WIDE
    finally:
        lib.MPIR_Hip_set_strided_wide_bytes(prev)
    assert _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1)["threshold"] == prev


def test_narrow_vec_exactly_when_all_four_conditions_hold(mpi):
    """Element at most 16 bytes; block bytes a multiple of 16; both bases
    multiples of 16; disp_unit a multiple of 16 for each side with a table (one
    disp_unit serves both, so: whenever there is a table)."""
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1)["threshold"]
    assert thr > 48
    good = dict(ai=BASE, ti=0, ao=FAR, to=TAB_O, unit=16, bl=12)

    def form(t="MPI_FLOAT", op="MPI_SUM", nb=400, **kw):
        a = dict(good, **kw)
        return _plan(mpi, a["ai"], a["ti"], a["ao"], a["to"], a["unit"], nb, a["bl"], t, op)

    info = form()
    assert info["form"] == NARROW_VEC and info["per"] == TILE // 16, info
    assert info["groups"] == -(-400 * 3 // info["per"]) == 2            # 1200 vectors: the boundary falls inside a block
    for fine in (dict(unit=32), dict(unit=48), dict(unit=64 * 1024), dict(ti=TAB_I, to=0), dict(ti=TAB_I),
                 dict(to=TAB_O + 8), dict(ai=BASE + 16), dict(bl=4)):
        assert form(**fine)["form"] == NARROW_VEC, fine
    for broken in (dict(ai=BASE + 4), dict(ao=FAR + 8), dict(ai=BASE + 16 + 1), dict(bl=13), dict(bl=11), dict(bl=1),
                   dict(unit=4), dict(unit=1), dict(unit=8), dict(unit=24), dict(unit=17),
                   dict(unit=4, ti=TAB_I, to=0), dict(unit=8, ti=TAB_I)):
        info = form(**broken)
        assert info["form"] == NARROW_ELEMS and info["per"] == TILE // 4, (broken, info)
    # every 16-byte-or-smaller class takes vectors; the 32-byte classes never do
    assert form("MPI_UNSIGNED_CHAR", "MPI_BXOR", bl=48)["form"] == NARROW_VEC
    assert form("MPI_UNSIGNED_CHAR", "MPI_BXOR", bl=47)["form"] == NARROW_ELEMS
    assert form("MPI_C_DOUBLE_COMPLEX", "MPI_SUM", bl=3)["form"] == NARROW_VEC
    wide = form("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC", unit=32, bl=2)
    assert wide["form"] == NARROW_ELEMS and wide["per"] == TILE // 32


def test_narrow_workgroups_cover_the_units(mpi):
    # a column of doubles: one element per block, 2048 per workgroup
    col = _plan(mpi, BASE, 0, FAR, TAB_O, 8, 3000, 1, "MPI_DOUBLE", "MPI_SUM")
    assert (col["form"], col["per"], col["groups"], col["launches"]) == (NARROW_ELEMS, 2048, 2, 1)
    # 3 bytes a block: 18000 byte units, the first workgroup's span ends inside block 5461
    u8 = _plan(mpi, BASE, 0, FAR, TAB_O, 1, 6000, 3, "MPI_UNSIGNED_CHAR", "MPI_BXOR")
    assert (u8["form"], u8["per"], u8["groups"]) == (NARROW_ELEMS, TILE, 2) and TILE % 3
    for nb in (1, 1365, 1366, 2 * 1365 + 1, 2731, 65536):
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, nb, 12)["groups"] == -(-nb * 3 // 1024), nb
        assert _plan(mpi, BASE, TAB_I, FAR, 0, 4, nb, 12)["groups"] == -(-nb * 12 // 4096), nb
    # any block count below the cap is one launch
    assert _plan(mpi, BASE, 0, FAR, TAB_O, 8, 65536, 1, "MPI_DOUBLE", "MPI_SUM")["launches"] == 1
    assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 65536, 64)["launches"] == 1


def _partition(info, nb):
    """the launches' block counts, from launches and rows_per_launch"""
    rpl = info["rows_per_launch"]
    sizes = [rpl] * (nb // rpl) + ([nb % rpl] if nb % rpl else [])
    assert len(sizes) == info["launches"] and sum(sizes) == nb, (info, sizes)
    return sizes


def test_launches_split_at_the_cap_and_at_a_lowered_cap(mpi):
    lib = mpi.load()
    cap = mpi.BATCH_MAX_GROUPS
    thr = _plan(mpi, BASE, 0, FAR, 0, 1, 1, 1)["threshold"]
    # wide blocks at the real cap: G workgroups a block, whole blocks per launch
    bl = max(thr, 3 * TILE) // 4 + 1
    nb = 2 ** 23
    info = _plan(mpi, BASE, 0, FAR + 4, TAB_O, 4, nb, bl)
    G = info["per"]
    assert info["form"] == WIDE and G >= 2
    assert info["rows_per_launch"] == cap // G and info["groups"] == nb * G
    assert all(n * G <= cap for n in _partition(info, nb))
    # narrow blocks at the real cap: INT_MAX blocks of one 16-byte vector stay below it
    one = _plan(mpi, BASE, 0, FAR, TAB_O, 16, 2 ** 31 - 1, 4)
    assert (one["form"], one["launches"], one["groups"]) == (NARROW_VEC, 1, -(-(2 ** 31 - 1) // 1024))
    assert one["groups"] <= cap
    if thr >= 4096:
        nb = 100_000_000
        big = _plan(mpi, BASE, 0, FAR, TAB_O, 16, nb, 1020)
        assert big["form"] == NARROW_VEC and big["rows_per_launch"] == cap * 1024 // 255 < 2 ** 32
        sizes = _partition(big, nb)
        assert all(-(-n * 255 // 1024) <= cap for n in sizes)
        assert big["groups"] == sum(-(-n * 255 // 1024) for n in sizes)
    # a lowered cap (the calling thread's, the strided call's hook): the same arithmetic at a small size
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        narrow = _plan(mpi, BASE, 0, FAR, TAB_O, 16, 2731, 12)          # 8193 vectors, 1024 per workgroup
        assert narrow["rows_per_launch"] == 3 * 1024 // 3 == 1024
        sizes = _partition(narrow, 2731)
        assert sizes == [1024, 1024, 683] and narrow["groups"] == 3 + 3 + 3
        assert all(-(-n * 3 // 1024) <= 3 for n in sizes)
        elems = _partition(_plan(mpi, BASE, TAB_I, FAR, 0, 1, 6000, 3, "MPI_UNSIGNED_CHAR", "MPI_BXOR"), 6000)
        assert all(-(-n * 3 // TILE) <= 3 for n in elems) and len(elems) == 1
        wbl = max(thr, TILE) // 4                                        # a block of G <= 3: whole blocks per launch
        wide = _plan(mpi, BASE, 0, FAR, TAB_O, 4, 7, wbl)
        Gw = wide["per"]
        assert wide["form"] == WIDE and wide["rows_per_launch"] == max(1, 3 // Gw)
        if Gw <= 3:
            assert all(n * Gw <= 3 for n in _partition(wide, 7))
        assert wide["groups"] == 7 * Gw
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3
        assert _plan(mpi, BASE, 0, FAR, TAB_O, 16, 2731, 12)["launches"] == 1
    finally:
        lib.MPIR_Hip_strided_test_max_groups(0)
