"""MPIX_Reduce_local_indexed_ordered and MPIX_Reduce_local_order without a GPU:
the argument checks through the C ABI in the indexed call's order, the order
build with both tables on the host (a host stable sort: the GPU runtime is not
opened) against numpy's stable argsort, the work size, and the planner
(MPIR_Hip_indexed_ordered_plan_info) against the indexed call's on made-up
addresses.

(Residency comes after the argument checks, and on a machine without a GPU
every call with made-up or host bases ends there with MPI_ERR_BUFFER; what a
host order table is checked for, and a host table with a stream, are in
test_indexed_ordered_gpu.py.)
"""
import ctypes

import numpy as np
import pytest

TILE = 16384
BASE = 1 << 32
FAR = 1 << 40
TAB_I, TAB_O, TAB_ORD = 1 << 44, (1 << 44) + (1 << 30), (1 << 44) + (1 << 31)   # where device tables would be
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
ENOKERNEL, EARG = 3, 5


def _host(n=64):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _call(mpi, b, a, nb=4, bl=4, unit=16, dt=None, op=None, tab=None, order=None):
    n = nb if nb > 0 else 1
    tab = np.arange(n, dtype=np.int64) if tab is None else tab
    order = np.arange(n, dtype=np.int32) if order is None else order
    return mpi.reduce_local_indexed_ordered(b, None, a, tab, order, unit, nb, bl, mpi.MPI_FLOAT if dt is None else dt,
                                            mpi.MPI_SUM if op is None else op)


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_indexed_ordered", "MPIX_Reduce_local_order", "MPIX_Reduce_local_order_worksize",
                 "MPIR_Hip_reduce_indexed_ordered", "MPIR_Hip_indexed_ordered_plan_info", "MPIR_Hip_order_build",
                 "MPIR_Hip_order_worksize"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name


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
                # (an order table with no inout_displs too: nothing is looked at)
                assert mpi.reduce_local_indexed_ordered(pin, ti, pio, to, WILD, 4, nb, bl, f, s) == 0, (nb, bl, pin, ti, to)
                assert mpi.reduce_local_indexed_ordered(pin, ti, pio, to, WILD, 4, nb, bl, f, s, stream=WILD) == 0
        # ... but the op and disp_unit still are
        rc = mpi.reduce_local_indexed_ordered(WILD, 0, WILD + 4, WILD, WILD, 4, nb, bl, f, mpi.MPI_OP_NULL)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        rc = mpi.reduce_local_indexed_ordered(WILD, 0, WILD + 4, WILD, WILD, 0, nb, bl, f, s)
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


def test_user_op_and_logical_ops_on_floats(mpi):
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
        rc = _call(mpi, b.ctypes.data, a.ctypes.data, 2, 2, op=o)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP and "not defined for this datatype" in mpi.error_string(rc)
    assert not a.any()


def test_the_indexed_calls_order_of_checks(mpi):
    """ops, counts, MPI_IN_PLACE, the alias check, disp_unit, then the order
    table's own rule, then residency."""
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
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
    # a bad unit beats the missing inout_displs
    order = np.arange(4, dtype=np.int32)
    for unit in (0, -1, -16):
        rc = mpi.reduce_local_indexed_ordered(pb, None, pa, None, order, unit, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
        assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "disp_unit" in mpi.error_string(rc), unit
    # an order table with a packed target, before residency is looked at
    rc = mpi.reduce_local_indexed_ordered(pb, None, pa, None, order, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "packed target" in mpi.error_string(rc)
    rc = mpi.reduce_local_indexed_ordered(pb, np.arange(4, dtype=np.int64), pa, None, order, 16, 4, 4, mpi.MPI_FLOAT,
                                          mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "packed target" in mpi.error_string(rc)
    # all arguments good: host bases are refused as the indexed call refuses them
    rc = _call(mpi, pb, pa)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc)
    assert "MPIX_Reduce_local_indexed_ordered" in mpi.error_string(rc)
    assert not a.any()


def test_order_null_is_the_indexed_call(mpi):
    """No order table: MPIX_Reduce_local_indexed's answers, its name on the error stack."""
    a, b = _host()
    tab = np.arange(4, dtype=np.int64)
    for args in ((b.ctypes.data, None, a.ctypes.data, tab, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, None, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 0, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 16, -1, 4, mpi.MPI_FLOAT, mpi.MPI_SUM),
                 (b.ctypes.data, None, a.ctypes.data, tab, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_REPLACE)):
        rc = mpi.reduce_local_indexed_ordered(*args[:4], None, *args[4:])
        text = mpi.error_string(rc)
        plain = mpi.reduce_local_indexed(*args)
        assert mpi.error_class(rc) == mpi.error_class(plain) != 0 and text == mpi.error_string(plain), args
        assert "MPIX_Reduce_local_indexed_ordered" not in text
    assert not a.any()


def test_shim_argument_checks(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 6)()
    f32, sum_ = mpi.ELEM["F32"], mpi.MPI_SUM & 0xF

    def info(op=sum_, elem=f32, unit=16, nb=4, bl=4, to=TAB_O, order=TAB_ORD):
        return lib.MPIR_Hip_indexed_ordered_plan_info(BASE, None, FAR, to, order, unit, nb, bl, op, elem, out)

    assert info() == 0
    assert info(op=mpi.MPI_REPLACE & 0xF) == ENOKERNEL and info(op=mpi.MPI_BAND & 0xF) == ENOKERNEL
    assert info(op=0) == ENOKERNEL and info(elem=99) == ENOKERNEL
    assert info(unit=0) == EARG and info(unit=0, nb=0) == EARG and info(unit=1 << 63) == EARG
    assert info(nb=0) == 0 and info(bl=0) == 0 and info(nb=0, to=None) == 0
    assert info(to=None) == EARG                                    # an order table, a packed target
    assert info(nb=1 << 31) == EARG and info(nb=(1 << 31) - 1, bl=1) == 0    # the order table holds ints
    assert info(to=None, order=None) == 0 and out[0] == SINGLE       # no order: the indexed planner's answer
    assert lib.MPIR_Hip_reduce_indexed_ordered(BASE, None, FAR, None, TAB_ORD, 16, 4, 4, sum_, f32, None, 1) == EARG
    assert lib.MPIR_Hip_reduce_indexed_ordered(WILD, None, WILD, WILD, WILD, 16, 0, 4, sum_, f32, None, 1) == 0
    assert lib.MPIR_Hip_reduce_indexed_ordered(BASE, None, FAR, TAB_O, TAB_ORD, 16, 4, 4, mpi.MPI_REPLACE & 0xF, f32, None,
                                               1) == ENOKERNEL
    with pytest.raises(ValueError):
        mpi.indexed_ordered_plan_info(BASE, 0, FAR, 0, TAB_ORD, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)
    with pytest.raises(LookupError):
        mpi.indexed_ordered_plan_info(BASE, 0, FAR, TAB_O, TAB_ORD, 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_BAND)
    with pytest.raises(TypeError):
        mpi.indexed_ordered_plan_info(BASE, 0, FAR, TAB_O, np.arange(4, dtype=np.int64), 16, 4, 4, mpi.MPI_FLOAT, mpi.MPI_SUM)


# ---------------------------------------------------------------- the planner
SHAPES = [(400, 12, 16, 16, 32), (400, 12, 4, 16, 36), (400, 12, 16, 16, 36), (5, 8195, 4, 4, 4), (5, 8195, 1, 4, 1),
          (2731, 12, 16, 0, 16), (1, 12, 16, 0, 0), (300, 4096, 16, 0, 0), (70000, 3, 1, 1, 2)]


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("ti", [0, TAB_I], ids=["packed-in", "in-table"])
def test_plan_is_the_indexed_calls(mpi, cap, ti):
    """Form, launches, workgroups, per, threshold and rows per launch are the
    indexed planner's for the same arguments, under the per-launch cap too."""
    lib = mpi.load()
    assert lib.MPIR_Hip_strided_test_max_groups(cap) == 0
    try:
        seen = set()
        for t, op in (("MPI_FLOAT", "MPI_SUM"), ("MPI_LONG_DOUBLE_INT", "MPI_MAXLOC"), ("MPI_UNSIGNED_CHAR", "MPI_BXOR")):
            for nb, bl, unit, pin, pio in SHAPES:
                args = (BASE + pin, ti, FAR + pio, TAB_O)
                rest = (unit, nb, bl, mpi.DATATYPES[t], mpi.OPS[op])
                got = mpi.indexed_ordered_plan_info(*args, TAB_ORD, *rest)
                assert got == mpi.indexed_plan_info(*args, *rest), (t, nb, bl, unit)
                assert got["form"] in (WIDE, NARROW_VEC, NARROW_ELEMS)
                seen.add(got["form"])
                if cap:
                    assert got["groups"] <= cap * got["launches"] or got["form"] == WIDE
        assert seen == {WIDE, NARROW_VEC, NARROW_ELEMS}
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == cap


# ---------------------------------------------------------------- the order build on the host
def _tables():
    rng = np.random.default_rng(3)
    yield "random with repeats", rng.integers(-50, 50, 1000)
    yield "all equal", np.full(257, 7)
    yield "all distinct", rng.permutation(4099) - 2000
    yield "descending", np.arange(300, 0, -1)
    yield "ascending", np.arange(300)
    yield "signed extremes", np.array([0, -1, 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0,
                                       np.iinfo(np.int64).max, -(1 << 32), 1 << 32, -(1 << 32) - 1, 1 << 63 - 1])
    yield "signed spread", rng.integers(-(1 << 62), 1 << 62, 5000) >> rng.integers(0, 62, 5000)
    yield "one", np.array([-5])


@pytest.mark.parametrize("name,displs", list(_tables()), ids=[n for n, _ in _tables()])
def test_host_build_is_numpys_stable_argsort(mpi, name, displs):
    displs = np.ascontiguousarray(displs, dtype=np.int64)
    before = displs.copy()
    order = np.full(len(displs) + 2, -7, dtype=np.int32)
    body = order[1:-1]
    assert mpi.load().MPIX_Reduce_local_order(displs.ctypes.data, len(displs), body.ctypes.data, None, 0, None) == 0
    assert np.array_equal(body, np.argsort(displs, kind="stable").astype(np.int32)), name
    assert order[0] == order[-1] == -7 and np.array_equal(displs, before)
    # the format the combine documents: a permutation, displacements non-decreasing, ties ascending
    assert np.array_equal(np.sort(body), np.arange(len(displs)))
    d = displs[body]
    assert (d[1:] >= d[:-1]).all() and (body[1:][d[1:] == d[:-1]] > body[:-1][d[1:] == d[:-1]]).all()


def test_host_build_opens_no_gpu_runtime(mpi):
    """Both tables on the host, in a fresh process: sorted, and the HSA runtime
    still not initialised afterwards (on a machine with a GPU that is the test)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import ctypes, os, sys\nsys.path[:0] = [{root!r}, os.path.join({root!r}, 'mpich-pip_amd')]\n"
            "import numpy as np, mpich_pip_amd as m\n"
            "d = np.array([3, -1, 3, 0, -1], dtype=np.int64); o = np.zeros(5, dtype=np.int32)\n"
            "assert m.reduce_local_order(d, 5, o) == 0 and o.tolist() == [1, 4, 3, 0, 2], o\n"
            "hsa = ctypes.CDLL('libhsa-runtime64.so.1'); v = ctypes.c_uint16(0)\n"
            "print('hsa', hex(hsa.hsa_system_get_info(0, ctypes.byref(v))))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["hsa", "0x100b"], r.stdout        # HSA_STATUS_ERROR_NOT_INITIALIZED


def test_build_arguments(mpi):
    lib = mpi.load()
    d = np.array([2, 1, 2], dtype=np.int64)
    o = np.full(3, -1, dtype=np.int32)
    rc = mpi.reduce_local_order(d, -1, o)
    assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT and "MPIX_Reduce_local_order" in mpi.error_string(rc)
    assert mpi.reduce_local_order(WILD, 0, WILD, WILD, 0) == 0 and mpi.reduce_local_order(0, 0, 0) == 0
    assert mpi.error_class(mpi.reduce_local_order(0, 3, o)) == mpi.MPI_ERR_ARG
    assert mpi.error_class(mpi.reduce_local_order(d, 3, 0)) == mpi.MPI_ERR_ARG
    # host tables with a stream; work too small (looked at before any residency)
    assert mpi.error_class(mpi.reduce_local_order(d, 3, o, stream=WILD)) == mpi.MPI_ERR_BUFFER
    ws = mpi.reduce_local_order_worksize(3)
    rc = mpi.reduce_local_order(d, 3, o, work=WILD, work_bytes=ws - 1)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "work_bytes" in mpi.error_string(rc)
    assert mpi.error_class(mpi.reduce_local_order(d, 3, o, work=WILD, work_bytes=-1)) == mpi.MPI_ERR_ARG
    assert (o == -1).all()
    # work is ignored by the host sort
    assert mpi.reduce_local_order(d, 3, o, work=WILD, work_bytes=ws) == 0 and o.tolist() == [1, 0, 2]
    out = ctypes.c_uint64(0)
    assert lib.MPIR_Hip_order_worksize(1 << 31, ctypes.byref(out)) == EARG
    assert lib.MPIR_Hip_order_build(d.ctypes.data, 1 << 31, o.ctypes.data, None, 0, None, 1) == EARG


def test_worksize(mpi):
    lib = mpi.load()
    rc = lib.MPIX_Reduce_local_order_worksize(-1, ctypes.byref(ctypes.c_long(0)))
    assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT
    assert mpi.error_class(lib.MPIX_Reduce_local_order_worksize(4, None)) == mpi.MPI_ERR_ARG
    with pytest.raises(ValueError):
        mpi.reduce_local_order_worksize(-5)
    ns = [0, 1, 2, 3, 31, 32, 33, 255, 256, 257, 1000, 4095, 4096, 4097, 65536, 10 ** 6, 10 ** 6 + 1, 1 << 24, (1 << 31) - 1]
    sizes = [mpi.reduce_local_order_worksize(n) for n in ns]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    # never less than the sorted keys and a double buffer of the pairs
    assert all(s >= n * (8 + 8 + 4) for n, s in zip(ns, sizes))
