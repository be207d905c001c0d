"""MPIX_Reduce_local_ragged without a GPU: its argument checks through the C ABI,
held against MPIX_Reduce_local_indexed's answers where the two calls share an
argument, and its launch planner (MPIR_Hip_ragged_plan_info: the planner the
launch itself runs, host arithmetic on the counts; a table is only compared
with NULL) on made-up addresses.

What the planner must get right is what the kernel relies on: the grid is the
packed elements' 16 KiB spans, one launch whatever the pieces are, the rounds
of the wave-wide search are ceil(log64(npieces + 1)), and the boundaries a
workgroup keeps in LDS fit 16 KiB.

A host table's contents are checked before the operands' residency, so the
refusals of an unsound starts and of an overflowing displacement show here,
on host buffers that a sound call would then refuse as non-device memory.
(A host table with a stream, and a piece outside device memory, need device
operands to get that far: test_ragged_gpu.py.)
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX

TILE = 16384
BASE = 1 << 32
FAR = 1 << 40                # inoutbuf's arena, far from inbuf's
TAB_I, TAB_O, TAB_S = 1 << 44, (1 << 44) + (1 << 30), (1 << 44) + (1 << 31)     # where device tables would be
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, RAGGED = range(3)
ENOKERNEL, EARG = 3, 5
INT_MAX = (1 << 31) - 1
MAX_GROUPS = 1 << 23         # MPIR_HIP_BATCH_MAX_GROUPS


def _host(n=64):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _plan(mpi, ti, to, ts, unit, n, count, t="MPI_FLOAT", op="MPI_SUM", ai=BASE, ao=FAR):
    return mpi.ragged_plan_info(ai, ti, ao, to, ts, unit, n, count, mpi.DATATYPES[t], mpi.OPS[op])


def _call(mpi, b, a, n=4, count=16, unit=16, dt=None, op=None, tab="default", starts="default"):
    tab = np.arange(max(n, 1), dtype=np.int64) if isinstance(tab, str) else tab
    starts = np.linspace(0, max(count, 0), max(n, 0) + 1).astype(np.int64) if isinstance(starts, str) else starts
    return mpi.reduce_local_ragged(b, None, a, tab, starts, unit, n, count, mpi.MPI_FLOAT if dt is None else dt,
                                   mpi.MPI_SUM if op is None else op)


def _indexed(mpi, b, a, nb=4, bl=4, unit=16, dt=None, op=None):
    return mpi.reduce_local_indexed(b, None, a, np.arange(max(nb, 1), dtype=np.int64), unit, nb, bl,
                                    mpi.MPI_FLOAT if dt is None else dt, mpi.MPI_SUM if op is None else op)


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_ragged", "MPIR_Hip_reduce_ragged", "MPIR_Hip_ragged_plan_info"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    assert mpi.RAGGED_NAMES == ["empty", "single", "ragged"]
    assert (mpi.RAGGED_EMPTY, mpi.RAGGED_SINGLE, mpi.RAGGED_RAGGED) == (EMPTY, SINGLE, RAGGED)


def test_negative_counts(mpi):
    a, b = _host()
    for n, count in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, n, count)
        assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT, (n, count, mpi.error_string(rc))
        assert mpi.error_class(rc) == mpi.error_class(_indexed(mpi, b.ctypes.data, a.ctypes.data, n, count))
    assert not a.any()


def test_zero_count_succeeds_without_touching_a_pointer_or_a_table(mpi):
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    for n in (0, 4):
        for pin, pio in ((WILD, WILD + 4), (WILD, WILD), (0, 0), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
            for ti, to, ts in ((WILD, WILD, WILD), (0, WILD, WILD), (WILD, 0, 0), (0, 0, 0), (0, 0, WILD)):
                assert mpi.reduce_local_ragged(pin, ti, pio, to, ts, 4, n, 0, f, s) == 0, (n, pin, ti, to, ts)
                # ... on a stream too: a wild (host) table is not looked at either
                assert mpi.reduce_local_ragged(pin, ti, pio, to, ts, 4, n, 0, f, s, stream=WILD) == 0
        # ... but the op and disp_unit still are
        rc = mpi.reduce_local_ragged(WILD, 0, WILD + 4, WILD, WILD, 4, n, 0, f, mpi.MPI_OP_NULL)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        for unit in (0, -1):
            rc = mpi.reduce_local_ragged(WILD, 0, WILD + 4, WILD, WILD, unit, n, 0, f, s)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc)
            with pytest.raises(ValueError):
                _plan(mpi, 0, WILD, WILD, 0, n, 0)


@pytest.mark.parametrize("op", ["MPI_REPLACE", "MPI_NO_OP", "MPI_OP_NULL", "BAD_HANDLE"])
def test_ops_refused_as_the_indexed_call_refuses_them(mpi, op):
    handle = {"MPI_REPLACE": mpi.MPI_REPLACE, "MPI_NO_OP": mpi.MPI_NO_OP, "MPI_OP_NULL": mpi.MPI_OP_NULL,
              "BAD_HANDLE": 0x44000003}[op]
    a, b = _host()
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, op=handle)
    other = _indexed(mpi, b.ctypes.data, a.ctypes.data, op=handle)
    assert mpi.error_class(rc) == mpi.error_class(other) == mpi.MPI_ERR_OP
    # the op comes before the buffers and before disp_unit
    rc = _call(mpi, a.ctypes.data, a.ctypes.data, op=handle, unit=0)
    assert mpi.error_class(rc) == mpi.error_class(_indexed(mpi, a.ctypes.data, a.ctypes.data, op=handle, unit=0)) == mpi.MPI_ERR_OP
    assert not a.any()


def test_user_op_and_undefined_pairs(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    a, b = _host()
    try:
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, op=op.value)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        assert "user MPI_Op functions run on the host" in mpi.error_string(rc)
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0
    for o in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            rc = _call(mpi, b.ctypes.data, a.ctypes.data, 2, 4, dt=dt, op=o)
            assert mpi.error_class(rc) == mpi.error_class(_indexed(mpi, b.ctypes.data, a.ctypes.data, 2, 2, dt=dt, op=o)) == mpi.MPI_ERR_OP
            assert "not defined for this datatype" in mpi.error_string(rc)
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, 2, 4, op=mpi.MPI_BAND)
    assert mpi.error_class(rc) == mpi.MPI_ERR_OP
    assert not a.any()


def test_in_place_aliased_then_disp_unit(mpi):
    a, b = _host()
    for pin, pio in ((mpi.MPI_IN_PLACE, a.ctypes.data), (b.ctypes.data, mpi.MPI_IN_PLACE)):
        rc = _call(mpi, pin, pio)
        assert mpi.error_class(rc) == mpi.error_class(_indexed(mpi, pin, pio)) == mpi.MPI_ERR_BUFFER
        assert "MPI_IN_PLACE" in mpi.error_string(rc)
        # ... before disp_unit
        assert mpi.error_class(_call(mpi, pin, pio, unit=0)) == mpi.MPI_ERR_BUFFER
    rc = _call(mpi, a.ctypes.data, a.ctypes.data)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc)
    assert mpi.error_class(_call(mpi, a.ctypes.data, a.ctypes.data, unit=0)) == mpi.MPI_ERR_BUFFER
    for unit in (0, -1, -16):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, unit=unit)
        assert mpi.error_class(rc) == mpi.error_class(_indexed(mpi, b.ctypes.data, a.ctypes.data, unit=unit)) == mpi.MPI_ERR_ARG
        assert "disp_unit" in mpi.error_string(rc), unit
    # every positive unit passes the argument checks; the operands are then refused as host memory
    for unit in (1, 3, 4, 16, 1 << 40):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, unit=unit)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc), unit
    assert not a.any()


def test_no_pieces_and_no_starts(mpi):
    a, b = _host()
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, n=0, count=16)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "no pieces" in mpi.error_string(rc)
    # ... with no table either
    rc = mpi.reduce_local_ragged(b.ctypes.data, None, a.ctypes.data, None, None, 4, 0, 16, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG
    tab = np.arange(4, dtype=np.int64)
    for ti, to in ((tab, None), (None, tab), (tab, tab)):
        rc = mpi.reduce_local_ragged(b.ctypes.data, ti, a.ctypes.data, to, None, 4, 4, 16, mpi.MPI_FLOAT, mpi.MPI_SUM)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "starts" in mpi.error_string(rc)
    # both after disp_unit
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, n=0, count=16, unit=0)
    assert "disp_unit" in mpi.error_string(rc)
    assert not a.any()


def test_host_tables_are_read_and_refused(mpi):
    """starts must begin at 0, never decrease and end at count; every
    displacement times disp_unit must fit an MPI_Aint: MPI_ERR_ARG, before the
    operands are looked at (host memory here, which a sound call is refused for)."""
    a, b = _host(2048)
    n, count = 300, 1200
    good = np.arange(n + 1, dtype=np.int64) * 4
    tab = np.arange(n, dtype=np.int64)
    f, sm = mpi.MPI_FLOAT, mpi.MPI_SUM

    def call(ti, to, starts, unit=16):
        return mpi.reduce_local_ragged(b.ctypes.data, ti, a.ctypes.data, to, starts, unit, n, count, f, sm)

    first = good.copy()
    first[0] = 1
    down = good.copy()
    down[100] = down[99] - 1
    short, long_ = good.copy(), good.copy()
    short[-1] -= 1
    long_[-1] += 1
    for what, starts in (("starts[0] != 0", first), ("a decreasing entry", down), ("ends short of count", short),
                         ("ends past count", long_)):
        for ti, to in ((None, tab), (tab, None), (tab, tab)):
            rc = call(ti, to, starts)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "starts" in mpi.error_string(rc), (what, mpi.error_string(rc))
    # empty pieces are sound: equal neighbours, at either end too
    flat = good.copy()
    flat[1], flat[-2], flat[150] = 0, count, flat[149]
    rc = call(None, tab, flat)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc)
    big = tab.copy()
    big[7] = 1 << 60
    neg = tab.copy()
    neg[299] = -(1 << 60)
    for t in (big, neg):
        for ti, to in ((None, t), (t, None), (tab, t)):
            rc = call(ti, to, good)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG, mpi.error_string(rc)
        # ... with disp_unit 1 the same entries fit: the operands are then refused
        assert mpi.error_class(call(None, t, good, unit=1)) == mpi.MPI_ERR_BUFFER
    assert not a.any() and (b == 1).all()
    assert (good == np.arange(n + 1) * 4).all() and (tab == np.arange(n)).all()


@pytest.mark.parametrize("ti,to", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["single", "scatter", "gather", "both"])
def test_host_pointers_refused_as_non_device(mpi, ti, to):
    """The single-call shape is no exception: the ragged call never takes
    MPI_Reduce_local's host paths."""
    a, b = _host(2048)
    tab = np.arange(300, dtype=np.int64)
    starts = np.arange(301, dtype=np.int64) * 4
    rc = mpi.reduce_local_ragged(b.ctypes.data, tab if ti else None, a.ctypes.data, tab if to else None, starts, 16,
                                 300, 1200, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER
    assert "device-resident" in mpi.error_string(rc) and "aliased" not in mpi.error_string(rc)
    assert not a.any()


def test_shim_refuses_replace_unknown_pairs_and_bad_arguments(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 6)()
    f32 = mpi.ELEM["F32"]
    sum_ = mpi.MPI_SUM & 0xF

    def info(op, elem, unit=16, n=4, count=16, ts=TAB_S, to=TAB_O):
        return lib.MPIR_Hip_ragged_plan_info(BASE, None, FAR, to, ts, unit, n, count, op, elem, out)

    assert info(mpi.MPI_REPLACE & 0xF, f32) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_ragged(BASE, None, FAR, TAB_O, TAB_S, 16, 4, 16, mpi.MPI_REPLACE & 0xF, f32, None, 1) == ENOKERNEL
    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL            # no BAND on floats
    assert info(mpi.MPI_MAXLOC & 0xF, f32) == ENOKERNEL
    assert info(0, f32) == ENOKERNEL and info(sum_, 99) == ENOKERNEL
    assert info(sum_, f32) == 0
    assert info(sum_, f32, unit=0) == EARG and info(sum_, f32, unit=1 << 63) == EARG
    assert info(sum_, f32, unit=0, count=0) == EARG                # whatever the counts
    assert lib.MPIR_Hip_reduce_ragged(WILD, None, WILD, WILD, WILD, 0, 0, 0, sum_, f32, None, 1) == EARG
    assert info(sum_, f32, n=0, count=0) == 0 and info(sum_, f32, n=4, count=0) == 0    # nothing to do
    assert lib.MPIR_Hip_reduce_ragged(WILD, WILD, WILD, WILD, WILD, 1, 4, 0, sum_, f32, None, 1) == 0
    assert info(sum_, f32, n=0) == EARG                             # elements and no pieces
    assert info(sum_, f32, n=0, to=None) == EARG
    assert info(sum_, f32, ts=None) == EARG                         # a table and no starts
    assert lib.MPIR_Hip_reduce_ragged(WILD, None, WILD, WILD, None, 4, 4, 16, sum_, f32, None, 1) == EARG
    assert info(sum_, f32, ts=None, to=None) == 0                   # the single call needs none
    assert info(sum_, f32, count=INT_MAX) == 0 and info(sum_, f32, count=INT_MAX + 1) == EARG
    assert info(sum_, f32, n=INT_MAX, count=INT_MAX) == 0 and info(sum_, f32, n=INT_MAX + 1, count=INT_MAX) == EARG
    with pytest.raises(ValueError):
        _plan(mpi, 0, TAB_O, TAB_S, 0, 4, 16)
    with pytest.raises(LookupError):
        _plan(mpi, 0, TAB_O, TAB_S, 16, 4, 16, op="MPI_BAND")
    with pytest.raises(TypeError):
        _plan(mpi, 0, TAB_O, np.arange(5, dtype=np.int32), 16, 4, 16)


def test_every_pair_of_the_indexed_call_has_a_ragged_kernel(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 6)()
    both = 0
    for op in range(16):
        for elem in range(64):
            ind = lib.MPIR_Hip_indexed_plan_info(BASE, None, FAR, TAB_O, 16, 4, 4, op, elem, out)
            rag = lib.MPIR_Hip_ragged_plan_info(BASE, None, FAR, TAB_O, TAB_S, 16, 4, 16, op, elem, out)
            assert (ind == ENOKERNEL) == (rag == ENOKERNEL), (op, elem, ind, rag)
            both += rag == 0
    assert both >= len([1 for o, t in MATRIX if T.compute_ok(o, t)]) // 4 > 0


# ---------------------------------------------------------------- the planner
def test_empty_and_single(mpi):
    for n in (0, 100):
        info = _plan(mpi, WILD, WILD, WILD, 4, n, 0, ai=WILD, ao=WILD)
        assert (info["form"], info["launches"], info["groups"]) == (EMPTY, 0, 0)
    dt, o = mpi.DATATYPES["MPI_FLOAT"], mpi.OPS["MPI_SUM"]
    # both tables NULL: the single call on count elements at any phase, starts given or not
    for ai, ao, n, count in ((BASE, FAR, 1, 100000), (BASE + 4, FAR, 7, 100000), (BASE, FAR + 8, 3000, 9000),
                             (BASE + 4, FAR + 8, 3, 6)):
        for unit in (1, 16, 12345):
            for ts in (0, TAB_S, WILD):
                info = _plan(mpi, 0, 0, ts, unit, n, count, ai=ai, ao=ao)
                single = mpi.plan_info(ai, ao, count, dt, o)
                assert (info["form"], info["launches"], info["groups"]) == (SINGLE, 1, single["groups"]), (info, single)
    # one table, either side, is not the single call -- not even for one piece
    assert _plan(mpi, TAB_I, 0, TAB_S, 4, 3000, 9000)["form"] == RAGGED
    assert _plan(mpi, 0, TAB_O, TAB_S, 4, 3000, 9000)["form"] == RAGGED
    assert _plan(mpi, 0, TAB_O, TAB_S, 4, 1, 3)["form"] == RAGGED


def test_one_launch_of_the_packed_spans_for_every_size(mpi):
    """ceil(count x size / 16 KiB) workgroups of 16 KiB / size elements, one
    launch, for every element size of the parity matrix with count around
    multiples of the span -- and whatever the tables, the phases or npieces."""
    seen = set()
    for op, t in MATRIX:
        esz = T.elem_size(t)
        if esz in seen or not T.compute_ok(op, t):
            continue
        seen.add(esz)
        per = TILE // esz
        for k in (1, 2, 5, 1000):
            for count in (k * per - 1, k * per, k * per + 1):
                for n, ti, to, ai in ((1, 0, TAB_O, BASE), (count, TAB_I, 0, BASE + esz), (70000, TAB_I, TAB_O, BASE + 4)):
                    info = _plan(mpi, ti, to, TAB_S, 1, n, count, t=t, op=op, ai=ai)
                    assert (info["form"], info["launches"], info["per"]) == (RAGGED, 1, per), (t, count, info)
                    assert info["groups"] == -(-count * esz // TILE) == -(-count // per), (t, count, info)
    assert seen >= {1, 2, 4, 8, 16, 32}, seen


def test_search_rounds_and_lds(mpi):
    for n, rounds in ((1, 1), (2, 1), (63, 1), (64, 2), (65, 2), (4095, 2), (4096, 3), (4097, 3), (262143, 3),
                      (262144, 4), (INT_MAX, 6)):
        info = _plan(mpi, 0, TAB_O, TAB_S, 4, n, max(n, 5000))
        assert info["rounds"] == rounds, (n, info)
        assert 64 ** rounds >= n + 1 > 64 ** (rounds - 1)
        assert info["lds_entries"] % 256 == 0 and 256 <= info["lds_entries"] and info["lds_entries"] * 4 <= 16 << 10, info


def test_int_max_elements_of_the_32_byte_class_fit_one_launch(mpi):
    info = _plan(mpi, 0, TAB_O, TAB_S, 16, 1000, INT_MAX, t="MPI_LONG_DOUBLE_INT", op="MPI_MAXLOC")
    assert info["launches"] == 1 and info["groups"] == -(-INT_MAX * 32 // TILE) < MAX_GROUPS, info
    info = _plan(mpi, 0, TAB_O, TAB_S, 1, INT_MAX, INT_MAX, t="MPI_UNSIGNED_CHAR", op="MPI_BXOR")
    assert info["launches"] == 1 and info["groups"] == -(-INT_MAX // TILE), info
