"""MPIX_Reduce_local_indexed_chunked, MPIX_Reduce_local_chunked_worksize and
MPIX_Reduce_local_runs without a GPU: the argument checks through the C ABI in
the ordered call's order with the NULL combinations of the two tables, the work
size, the runstart build on host tables against the numpy statement of its
definition, what a host runstart is checked for, the planner
(MPIR_Hip_indexed_chunked_plan_info) against the ordered call's on made-up
addresses, and the family's (op, class) matrix.

(A host order or runstart is read and checked before the operands' residency,
so a wrong one is MPI_ERR_ARG here too; with sound tables every call with host
bases ends at residency with MPI_ERR_BUFFER on a machine without a GPU.)
"""
import ctypes

import numpy as np
import pytest

from test_kernel_tables_cpu import MATRIX, OP

TILE = 16384
BASE = 1 << 32
FAR = 1 << 40
TAB_I, TAB_O, TAB_ORD, TAB_RUN = 1 << 44, (1 << 44) + (1 << 30), (1 << 44) + (1 << 31), (1 << 44) + (1 << 29)
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
ENOKERNEL, EARG = 3, 5
C = 64


def runs_of(displs, order):
    """The numpy statement of runstart's definition: the smallest sorted position with the same displacement"""
    d = np.asarray(displs)[order]
    heads = np.concatenate([[True], d[1:] != d[:-1]])
    return np.maximum.accumulate(np.where(heads, np.arange(len(d)), 0)).astype(np.int32)


def _host(n=64):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _call(mpi, b, a, nb=4, bl=4, unit=16, dt=None, op=None, tab=None, order=None, runs=None, **kw):
    n = nb if nb > 0 else 1
    tab = np.arange(n, dtype=np.int64) if tab is None else tab
    order = np.arange(n, dtype=np.int32) if order is None else order
    runs = np.arange(n, dtype=np.int32) if runs is None else runs
    return mpi.reduce_local_indexed_chunked(b, None, a, tab, order, runs, unit, nb, bl,
                                            mpi.MPI_FLOAT if dt is None else dt, mpi.MPI_SUM if op is None else op, **kw)


# ---------------------------------------------------------------- argument checks
def test_exported_declared_and_the_constant(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_indexed_chunked", "MPIX_Reduce_local_chunked_worksize", "MPIX_Reduce_local_runs",
                 "MPIR_Hip_reduce_indexed_chunked", "MPIR_Hip_indexed_chunked_plan_info", "MPIR_Hip_chunked_worksize",
                 "MPIR_Hip_runs_build"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    assert mpi.REDUCE_LOCAL_CHUNK == C
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert "#define MPIX_REDUCE_LOCAL_CHUNK 64" in open(os.path.join(inc, "mpi_reduce_local.h")).read()
    assert "#define MPIR_HIP_REDUCE_CHUNK 64" in open(os.path.join(inc, "mpir_hip_reduce.h")).read()


def test_negative_counts(mpi):
    a, b = _host()
    for nb, bl in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, nb, bl)
        assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT, (nb, bl, mpi.error_string(rc))
        assert "MPIX_Reduce_local_indexed_chunked" in mpi.error_string(rc)
    assert not a.any()


def test_zero_counts_succeed_without_touching_a_pointer_or_a_table(mpi):
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    call = mpi.reduce_local_indexed_chunked
    for nb, bl in ((0, 4), (4, 0), (0, 0)):
        for pin, pio in ((WILD, WILD + 4), (WILD, WILD), (0, 0), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
            for ti, to in ((WILD, WILD), (0, WILD), (WILD, 0), (0, 0)):
                for order, runs in ((WILD, WILD), (WILD, 0), (0, WILD)):
                    assert call(pin, ti, pio, to, order, runs, 4, nb, bl, f, s) == 0, (nb, bl, pin, ti, to, order, runs)
                    assert call(pin, ti, pio, to, order, runs, 4, nb, bl, f, s, work=WILD, work_bytes=0, stream=WILD) == 0
        # ... but the op and disp_unit still are
        rc = call(WILD, 0, WILD + 4, WILD, WILD, WILD, 4, nb, bl, f, mpi.MPI_OP_NULL)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        rc = call(WILD, 0, WILD + 4, WILD, WILD, WILD, 0, nb, bl, f, s)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc)


@pytest.mark.parametrize("op", ["MPI_REPLACE", "MPI_NO_OP", "MPI_OP_NULL", "BAD_HANDLE"])
def test_ops_refused_as_in_the_indexed_call(mpi, op):
    handle = {"MPI_REPLACE": mpi.MPI_REPLACE, "MPI_NO_OP": mpi.MPI_NO_OP, "MPI_OP_NULL": mpi.MPI_OP_NULL,
              "BAD_HANDLE": 0x44000003}[op]
    a, b = _host()
    rc = _call(mpi, b.ctypes.data, a.ctypes.data, op=handle)
    plain = mpi.reduce_local_indexed(b.ctypes.data, None, a.ctypes.data, np.arange(4, dtype=np.int64), 16, 4, 4,
                                     mpi.MPI_FLOAT, handle)
    assert mpi.error_class(rc) == mpi.error_class(plain) == mpi.MPI_ERR_OP
    assert not a.any()


def test_the_ordered_calls_order_of_checks_and_the_null_combinations(mpi):
    """ops, counts, MPI_IN_PLACE, the alias check, disp_unit, then the two tables'
    own rules, work_bytes, then the host tables, then residency."""
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    call = mpi.reduce_local_indexed_chunked
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    # a negative count beats a refused op; a refused op beats MPI_IN_PLACE, aliasing and a bad unit
    assert mpi.error_class(_call(mpi, pb, pa, nb=-1, op=mpi.MPI_REPLACE)) == mpi.MPI_ERR_COUNT
    assert mpi.error_class(_call(mpi, mpi.MPI_IN_PLACE, pa, unit=0, op=mpi.MPI_REPLACE)) == mpi.MPI_ERR_OP
    assert mpi.error_class(_call(mpi, pa, pa, unit=0, op=mpi.MPI_REPLACE)) == mpi.MPI_ERR_OP
    # MPI_IN_PLACE and aliasing beat a bad unit
    for pin, pio in ((mpi.MPI_IN_PLACE, pa), (pb, mpi.MPI_IN_PLACE)):
        rc = _call(mpi, pin, pio, unit=0)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "MPI_IN_PLACE" in mpi.error_string(rc)
    rc = _call(mpi, pa, pa, unit=0)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc)
    # a bad unit beats a missing table
    order = np.arange(4, dtype=np.int32)
    tab = np.arange(4, dtype=np.int64)
    for unit in (0, -1, -16):
        for o, r, t in ((order, None, tab), (None, order, tab), (order, order, None)):
            rc = call(pb, None, pa, t, o, r, unit, 4, 4, f, s)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc), unit
    # exactly one of the two tables
    for o, r, missing in ((order, None, "runstart is NULL"), (None, order, "order is NULL")):
        for t in (tab, None):
            rc = call(pb, None, pa, t, o, r, 16, 4, 4, f, s)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and missing in mpi.error_string(rc), mpi.error_string(rc)
    # either one given with a packed target
    for ti in (None, tab):
        rc = call(pb, ti, pa, None, order, order, 16, 4, 4, f, s)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "packed target" in mpi.error_string(rc)
    # work_bytes: negative, and less than the reported size (before any residency)
    ws = mpi.reduce_local_chunked_worksize(4, 4, f)
    for wb in (-1, 0, ws - 1):
        rc = _call(mpi, pb, pa, work=WILD, work_bytes=wb)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "work_bytes" in mpi.error_string(rc), wb
    # all arguments good: host bases are refused as the ordered call refuses them
    for kw in ({}, {"work": WILD, "work_bytes": ws}):
        rc = _call(mpi, pb, pa, **kw)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc)
        assert "MPIX_Reduce_local_indexed_chunked" in mpi.error_string(rc)
    # host tables with a stream
    assert mpi.error_class(_call(mpi, pb, pa, work=WILD, work_bytes=ws, stream=WILD)) == mpi.MPI_ERR_BUFFER
    assert not a.any()


def test_both_tables_null_is_the_indexed_call(mpi):
    """Neither table: MPIX_Reduce_local_indexed's answers, its name on the error stack."""
    a, b = _host()
    tab = np.arange(4, dtype=np.int64)
    for args in ((b.ctypes.data, None, a.ctypes.data, tab, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, None, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 0, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 16, -1, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_REPLACE)):
        rc = mpi.reduce_local_indexed_chunked(*args[:4], None, None, *args[4:], work=WILD, work_bytes=0)
        text = mpi.error_string(rc)
        plain = mpi.reduce_local_indexed(*args)
        assert mpi.error_class(rc) == mpi.error_class(plain) != 0 and text == mpi.error_string(plain), args
        assert "MPIX_Reduce_local_indexed_chunked" not in text
    assert not a.any()


def test_shim_argument_checks(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 8)()
    f32, sum_ = mpi.ELEM["F32"], mpi.MPI_SUM & 0xF

    def info(op=sum_, elem=f32, unit=16, nb=4, bl=4, to=TAB_O, order=TAB_ORD, runs=TAB_RUN):
        return lib.MPIR_Hip_indexed_chunked_plan_info(BASE, None, FAR, to, order, runs, unit, nb, bl, op, elem, out)

    assert info() == 0 and out[6] == 2 * out[1] == 2
    assert info(op=mpi.MPI_REPLACE & 0xF) == ENOKERNEL and info(op=mpi.MPI_BAND & 0xF) == ENOKERNEL
    assert info(op=0) == ENOKERNEL and info(elem=99) == ENOKERNEL
    assert info(unit=0) == EARG and info(unit=0, nb=0) == EARG and info(unit=1 << 63) == EARG
    assert info(nb=0) == 0 and info(bl=0) == 0 and info(nb=0, to=None) == 0
    assert info(to=None) == EARG and info(to=None, runs=None) == EARG and info(to=None, order=None) == EARG
    assert info(order=None) == EARG and info(runs=None) == EARG
    assert info(nb=1 << 31) == EARG and info(nb=(1 << 31) - 1, bl=1) == 0    # the tables hold ints
    assert info(to=None, order=None, runs=None) == 0 and out[0] == SINGLE    # no table: the indexed planner's answer
    call = lib.MPIR_Hip_reduce_indexed_chunked
    assert call(BASE, None, FAR, None, TAB_ORD, TAB_RUN, 16, 4, 4, sum_, f32, None, 0, None, 1) == EARG
    assert call(BASE, None, FAR, TAB_O, None, TAB_RUN, 16, 4, 4, sum_, f32, None, 0, None, 1) == EARG
    assert call(BASE, None, FAR, TAB_O, TAB_ORD, None, 16, 4, 4, sum_, f32, None, 0, None, 1) == EARG
    assert call(WILD, None, WILD, WILD, WILD, WILD, 16, 0, 4, sum_, f32, WILD, 0, None, 1) == 0
    assert call(BASE, None, FAR, TAB_O, TAB_ORD, TAB_RUN, 16, 4, 4, mpi.MPI_REPLACE & 0xF, f32, None, 0, None, 1) == ENOKERNEL
    with pytest.raises(ValueError):
        mpi.indexed_chunked_plan_info(BASE, 0, FAR, 0, TAB_ORD, TAB_RUN, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    with pytest.raises(LookupError):
        mpi.indexed_chunked_plan_info(BASE, 0, FAR, TAB_O, TAB_ORD, TAB_RUN, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_BAND)
    with pytest.raises(TypeError):
        mpi.indexed_chunked_plan_info(BASE, 0, FAR, TAB_O, TAB_ORD, np.arange(4, dtype=np.int64), 16, 4, 4, mpi.MPI_FLOAT,
                                      mpi.MPI_SUM)


# ---------------------------------------------------------------- the work size
def test_worksize(mpi):
    lib = mpi.load()
    f = mpi.MPI_FLOAT
    out = ctypes.c_long(0)
    for nb, bl in ((-1, 4), (4, -1)):
        assert mpi.error_class(lib.MPIX_Reduce_local_chunked_worksize(nb, bl, f, ctypes.byref(out))) == mpi.MPI_ERR_COUNT
    assert mpi.error_class(lib.MPIX_Reduce_local_chunked_worksize(4, 4, f, None)) == mpi.MPI_ERR_ARG
    assert mpi.error_class(lib.MPIX_Reduce_local_chunked_worksize(4, 4, 0x0c000000, ctypes.byref(out))) == mpi.MPI_ERR_TYPE
    with pytest.raises(ValueError):
        mpi.reduce_local_chunked_worksize(-5, 4, f)
    ns = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 4097, 65536, 10 ** 6, (1 << 31) - 1]
    bls = [0, 1, 3, 4, 5, 12, 64, 4096, 4099, 1 << 20]
    for t in ("MPI_FLOAT", "MPI_UNSIGNED_CHAR", "MPI_LONG_DOUBLE_INT"):
        dt = mpi.DATATYPES[t]
        esz = lib.MPIR_Hip_elem_size(mpi._ELEM_BY_HANDLE[dt])
        grid = [[mpi.reduce_local_chunked_worksize(n, bl, dt) for bl in bls] for n in ns]
        # monotone in both arguments, and room for two partials per window of 64 positions
        assert all(row == sorted(row) for row in grid), t
        assert all(col == sorted(col) for col in map(list, zip(*grid))), t
        assert all(grid[i][j] >= 2 * -(-n // C) * bl * esz for i, n in enumerate(ns) for j, bl in enumerate(bls)), t
        # ... from its three arguments alone
        assert grid == [[mpi.reduce_local_chunked_worksize(n, bl, dt) for bl in bls] for n in ns]
    # past an MPI_Aint
    rc = lib.MPIX_Reduce_local_chunked_worksize((1 << 31) - 1, (1 << 31) - 1, mpi.MPI_C_LONG_DOUBLE_COMPLEX, ctypes.byref(out))
    assert rc == 0 or mpi.error_class(rc) == mpi.MPI_ERR_ARG
    u = ctypes.c_uint64(0)
    assert lib.MPIR_Hip_chunked_worksize(1 << 31, 4, mpi.ELEM["F32"], ctypes.byref(u)) == EARG
    assert lib.MPIR_Hip_chunked_worksize(1 << 20, 1 << 62, mpi.ELEM["F32"], ctypes.byref(u)) == EARG
    assert lib.MPIR_Hip_chunked_worksize(4, 4, 0, ctypes.byref(u)) == ENOKERNEL


def test_worksize_and_host_runs_open_no_gpu_runtime(mpi):
    """In a fresh process: the work size asked and a runstart table built with all
    three tables on the host, and the HSA runtime still not initialised
    afterwards (on a machine with a GPU that is the test)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import ctypes, os, sys\nsys.path[:0] = [{root!r}, os.path.join({root!r}, 'mpich-pip_amd')]\n"
            "import numpy as np, mpich_pip_amd as m\n"
            "assert m.reduce_local_chunked_worksize(65536, 64, m.MPI_FLOAT) >= 2 * 1024 * 256\n"
            "d = np.array([3, -1, 3, 0, -1], dtype=np.int64); o = np.zeros(5, dtype=np.int32); r = np.zeros(5, dtype=np.int32)\n"
            "assert m.reduce_local_order(d, 5, o) == 0 and o.tolist() == [1, 4, 3, 0, 2], o\n"
            "assert m.reduce_local_runs(d, o, 5, r) == 0 and r.tolist() == [0, 0, 2, 3, 3], r\n"
            "hsa = ctypes.CDLL('libhsa-runtime64.so.1'); v = ctypes.c_uint16(0)\n"
            "print('hsa', hex(hsa.hsa_system_get_info(0, ctypes.byref(v))))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["hsa", "0x100b"], r.stdout        # HSA_STATUS_ERROR_NOT_INITIALIZED


# ---------------------------------------------------------------- the runstart build on the host
def _tables():
    rng = np.random.default_rng(3)
    yield "signed with repeats", rng.integers(-50, 50, 1000)
    yield "one", np.array([-5])
    yield "all equal", np.full(257, 7)
    yield "all distinct", rng.permutation(4099) - 2000
    yield "signed extremes", np.array([0, -1, 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0,
                                       np.iinfo(np.int64).max, -(1 << 32), 1 << 32, -(1 << 32) - 1, 1 << 63 - 1])


@pytest.mark.parametrize("name,displs", list(_tables()), ids=[n for n, _ in _tables()])
def test_host_runs_are_the_definition(mpi, name, displs):
    displs = np.ascontiguousarray(displs, dtype=np.int64)
    order = np.argsort(displs, kind="stable").astype(np.int32)
    before = displs.copy(), order.copy()
    runs = np.full(len(displs) + 2, -7, dtype=np.int32)
    body = runs[1:-1]
    assert mpi.load().MPIX_Reduce_local_runs(displs.ctypes.data, order.ctypes.data, len(displs), body.ctypes.data, None) == 0
    assert np.array_equal(body, runs_of(displs, order)), name
    assert runs[0] == runs[-1] == -7 and np.array_equal(displs, before[0]) and np.array_equal(order, before[1])
    # the definition, word for word
    d = displs[order]
    assert all(body[p] == min(q for q in range(len(d)) if d[q] == d[p]) for p in range(0, len(d), max(1, len(d) // 50)))


def test_runs_arguments(mpi):
    d = np.array([2, 1, 2], dtype=np.int64)
    o = np.array([1, 0, 2], dtype=np.int32)
    r = np.full(3, -1, dtype=np.int32)
    rc = mpi.reduce_local_runs(d, o, -1, r)
    assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT and "MPIX_Reduce_local_runs" in mpi.error_string(rc)
    assert mpi.reduce_local_runs(WILD, WILD, 0, WILD) == 0 and mpi.reduce_local_runs(0, 0, 0, 0) == 0
    for args in ((0, o, 3, r), (d, 0, 3, r), (d, o, 3, 0)):
        assert mpi.error_class(mpi.reduce_local_runs(*args)) == mpi.MPI_ERR_ARG
    assert mpi.error_class(mpi.reduce_local_runs(d, o, 3, r, stream=WILD)) == mpi.MPI_ERR_BUFFER
    for bad in (3, -1):
        wild = o.copy()
        wild[1] = bad
        assert mpi.error_class(mpi.reduce_local_runs(d, wild, 3, r)) == mpi.MPI_ERR_ARG
    assert (r == -1).all()
    assert mpi.reduce_local_runs(d, o, 3, r) == 0 and r.tolist() == [0, 1, 1]
    assert mpi.load().MPIR_Hip_runs_build(d.ctypes.data, o.ctypes.data, 1 << 31, r.ctypes.data, None, 1) == EARG


def test_a_host_runstart_off_by_one_anywhere_is_refused(mpi):
    """Host tables throughout: every single entry of runstart moved by one, up or
    down, is MPI_ERR_ARG before the operands are looked at, and nothing is
    written; so is an entry outside 0 <= runstart[p] <= p through the shim."""
    rng = np.random.default_rng(5)
    tio = rng.integers(0, 9, 150).astype(np.int64) * 3
    order = np.argsort(tio, kind="stable").astype(np.int32)
    good = runs_of(tio, order)
    a, b = np.zeros(150 * 4 * 4, np.float32), np.ones(150 * 4, np.float32)
    call = mpi.reduce_local_indexed_chunked
    args = (16, 150, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    for p in range(150):
        for step in (-1, 1):
            bad = good.copy()
            bad[p] += step
            rc = call(b.ctypes.data, None, a.ctypes.data, tio, order, bad, *args)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "runstart" in mpi.error_string(rc), (p, step, mpi.error_string(rc))
    # the sound table gets as far as residency
    rc = call(b.ctypes.data, None, a.ctypes.data, tio, order, good, *args)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
    assert not a.any() and (b == 1).all()
    lib = mpi.load()
    f32, sum_ = mpi.ELEM["F32"], mpi.MPI_SUM & 0xF
    shim = lambda runs: lib.MPIR_Hip_reduce_indexed_chunked(b.ctypes.data, None, a.ctypes.data, tio.ctypes.data, order.ctypes.data,
                                                            runs.ctypes.data, 16, 150, 4, sum_, f32, None, 0, None, 1)
    for p, v in ((0, 1), (0, -1), (7, 8), (149, 150), (30, -2)):
        bad = good.copy()
        bad[p] = v
        assert shim(bad) == EARG, (p, v)
    assert not a.any()


# ---------------------------------------------------------------- the planner
SHAPES = [(400, 12, 16, 16, 32), (400, 12, 4, 16, 36), (400, 12, 16, 16, 36), (5, 8195, 4, 4, 4), (5, 8195, 1, 4, 1),
          (2731, 12, 16, 0, 16), (1, 12, 16, 0, 0), (300, 4096, 16, 0, 0), (70000, 3, 1, 1, 2)]


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("ti", [0, TAB_I], ids=["packed-in", "in-table"])
def test_plan_is_the_ordered_calls_twice(mpi, cap, ti):
    """Form, launches, workgroups, per, threshold and rows per launch of either
    kernel are the ordered planner's for the same arguments, under the per-launch
    cap too (which gives several launches of each); the call makes twice the
    launches, and the work bytes are MPIX_Reduce_local_chunked_worksize's."""
    lib = mpi.load()
    assert lib.MPIR_Hip_strided_test_max_groups(cap) == 0
    try:
        seen, several = set(), 0
        for t, op in (("MPI_FLOAT", "MPI_SUM"), ("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC"), ("MPI_UNSIGNED_CHAR", "MPI_BXOR")):
            for nb, bl, unit, pin, pio in SHAPES:
                args = (BASE + pin, ti, FAR + pio, TAB_O)
                rest = (unit, nb, bl, mpi.DATATYPES[t], mpi.OPS[op])
                got = mpi.indexed_chunked_plan_info(*args, TAB_ORD, TAB_RUN, *rest)
                assert got.pop("total_launches") == 2 * got["launches"]
                assert got.pop("work_bytes") == mpi.reduce_local_chunked_worksize(nb, bl, mpi.DATATYPES[t])
                assert got == mpi.indexed_ordered_plan_info(*args, TAB_ORD, *rest), (t, nb, bl, unit)
                assert got["form"] in (WIDE, NARROW_VEC, NARROW_ELEMS)
                seen.add(got["form"])
                several += got["launches"] > 1
                if cap:
                    assert got["groups"] <= cap * got["launches"] or got["form"] == WIDE
        assert seen == {WIDE, NARROW_VEC, NARROW_ELEMS}
        assert several if cap else not several
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == cap


def test_each_form_at_its_boundary(mpi):
    """A block of the threshold's bytes is WIDE, 16 less NARROW_VEC; one element
    off 16, a base off 16 or a unit off 16 is NARROW_ELEMS."""
    f, s = mpi.MPI_FLOAT, mpi.MPI_SUM
    thr = mpi.indexed_chunked_plan_info(BASE, 0, FAR, TAB_O, TAB_ORD, TAB_RUN, 16, 8, 4, f, s)["threshold"]

    def form(bl, unit=16, pin=0, pio=0):
        return mpi.indexed_chunked_plan_info(BASE + pin, 0, FAR + pio, TAB_O, TAB_ORD, TAB_RUN, unit, 200, bl, f, s)["form"]

    assert form(thr // 4) == WIDE and form(thr // 4 - 4) == NARROW_VEC and form(thr // 4 - 1) == NARROW_ELEMS
    assert form(4) == NARROW_VEC and form(3) == NARROW_ELEMS and form(4, unit=4) == NARROW_ELEMS
    assert form(4, pio=4) == NARROW_ELEMS and form(4, pin=8) == NARROW_ELEMS and form(thr // 4 + 3, unit=1, pio=1) == WIDE


# ---------------------------------------------------------------- the family's matrix
def test_the_family_holds_the_matrix_and_no_replace(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 8)()
    expected = {(OP[o], mpi.ELEM[e]) for o, es in MATRIX.items() for e in es}
    assert len(expected) == 118
    nelems = len(mpi.ELEM) + 1
    grid = [(o, e) for o in range(16) for e in range(nelems + 1)]
    # (the arguments of test_kernel_tables_cpu.py's ordered family, runstart beside order)
    rcs = {p: lib.MPIR_Hip_indexed_chunked_plan_info(BASE, None, FAR, (1 << 44) + (1 << 30), (1 << 44) + (1 << 29), TAB_RUN,
                                                     16, 4, 4, *p, out) for p in grid}
    none = {p for p in grid if rcs[p] == ENOKERNEL}
    assert none == set(grid) - expected, sorted(none ^ (set(grid) - expected))
    assert all(rcs[(OP["REPLACE"], e)] == ENOKERNEL for e in mpi.ELEM.values())
    assert all(rcs[p] == 0 for p in expected), [(p, rcs[p]) for p in expected if rcs[p]][:5]
