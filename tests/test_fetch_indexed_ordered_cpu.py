"""MPIX_Reduce_local_fetch_indexed_ordered without a GPU: its argument checks
through the C ABI on host buffers (which a sound call is then refused for as
non-device memory, so a check that comes earlier shows by its class and text),
and its launch planner (MPIR_Hip_fetch_indexed_ordered_plan_info: the ordered
call's plan with fetchbuf joining the alignment test) on made-up addresses.

The argument rules are MPIX_Reduce_local_indexed_ordered's in that call's order,
with MPIX_Reduce_local_fetch's validation of the op (MPI_NO_OP and MPI_REPLACE
pass) and its rules for fetchbuf on top.  (Host tables, a fetchbuf inside the
target's span and the order-less promise need device operands to get that far:
test_fetch_indexed_ordered_gpu.py.)
"""
import ctypes
import os

import numpy as np
import pytest

BASE = 1 << 32               # inbuf's arena
FAR = 1 << 40                # inoutbuf's
FETCH = 1 << 41              # fetchbuf's
TAB_I, TAB_O, TAB_ORD = (1 << 44) + (1 << 29), (1 << 44) + (1 << 30), (1 << 44) + (1 << 31)
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
EBUFFER, ENOKERNEL, EARG = 1, 3, 5
NAMES = ("MPIX_Reduce_local_fetch_indexed_ordered", "MPIR_Hip_reduce_fetch_indexed_ordered",
         "MPIR_Hip_fetch_indexed_ordered_plan_info")


class Host:
    """Three host arrays (in = 1, inout = 2, fetch = 3, floats), a host output
    table with repeats and its order, and a check that a refused call left all
    of them alone."""

    def __init__(self, n=256, nb=8, bl=4):
        self.b = np.full(n, 1, np.float32)
        self.a = np.full(n, 2, np.float32)
        self.f = np.full(n, 3, np.float32)
        self.pb, self.pa, self.pf = self.b.ctypes.data, self.a.ctypes.data, self.f.ctypes.data
        self.nb, self.bl = nb, bl
        self.tab = (np.arange(nb, dtype=np.int64) % 3)
        self.order = np.argsort(self.tab, kind="stable").astype(np.int32)
        self.tab0, self.order0 = self.tab.copy(), self.order.copy()

    def untouched(self):
        return ((self.b == 1).all() and (self.a == 2).all() and (self.f == 3).all() and
                np.array_equal(self.tab, self.tab0) and np.array_equal(self.order, self.order0))


def _call(mpi, h, pb="b", pa="a", pf="f", nb=None, bl=None, unit=16, dt=None, op=None, tin=None, tio="t", order="o",
          stream=0):
    return mpi.reduce_local_fetch_indexed_ordered(
        h.pb if pb == "b" else pb, tin, h.pa if pa == "a" else pa, h.tab if isinstance(tio, str) else tio,
        h.pf if pf == "f" else pf, h.order if isinstance(order, str) else order, unit, h.nb if nb is None else nb,
        h.bl if bl is None else bl, mpi.MPI_FLOAT if dt is None else dt, mpi.MPI_SUM if op is None else op, stream)


def _refused(mpi, rc, cls, text=None):
    assert mpi.error_class(rc) == cls, mpi.error_string(rc)
    if text:
        assert text in mpi.error_string(rc), mpi.error_string(rc)


def _validated(mpi, rc):
    """The call passed every argument check and was then refused as host memory."""
    _refused(mpi, rc, mpi.MPI_ERR_BUFFER, "device-resident")


def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    assert callable(mpi.reduce_local_fetch_indexed_ordered) and callable(mpi.fetch_indexed_ordered_plan_info)
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    assert "MPIX_Reduce_local_fetch_indexed_ordered(" in open(os.path.join(inc, "mpi_reduce_local.h")).read()
    shim = open(os.path.join(inc, "mpir_hip_reduce.h")).read()
    assert "MPIR_Hip_reduce_fetch_indexed_ordered(" in shim and "MPIR_Hip_fetch_indexed_ordered_plan_info(" in shim


def test_negative_counts(mpi):
    h = Host()
    for nb, bl in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, nb=nb, bl=bl, op=op), mpi.MPI_ERR_COUNT, "negative")
    _refused(mpi, _call(mpi, h, nb=-1, op=mpi.MPI_OP_NULL), mpi.MPI_ERR_COUNT)       # ... before the op
    assert h.untouched()


def test_zero_counts_succeed_without_touching_a_pointer_or_a_table(mpi):
    f = mpi.MPI_FLOAT
    ip = mpi.MPI_IN_PLACE
    call = mpi.reduce_local_fetch_indexed_ordered
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        for nb, bl in ((0, 4), (4, 0), (0, 0)):
            for pin, pio, pf in ((WILD, WILD + 4, WILD + 8), (WILD, WILD, WILD), (0, 0, 0), (ip, ip, ip)):
                for ti, to, od in ((WILD, WILD, WILD), (0, WILD, WILD), (WILD, 0, WILD), (0, 0, WILD), (0, WILD, 0), (0, 0, 0)):
                    assert call(pin, ti, pio, to, pf, od, 4, nb, bl, f, op) == 0, (op, nb, bl, pin, ti, to, od)
                    # ... on a stream too: a wild (host) table is not looked at either
                    assert call(pin, ti, pio, to, pf, od, 4, nb, bl, f, op, stream=WILD) == 0
    # ... but the op and disp_unit still are
    for nb, bl in ((0, 4), (4, 0)):
        _refused(mpi, call(WILD, WILD, WILD + 4, WILD, WILD + 8, WILD, 4, nb, bl, f, mpi.MPI_OP_NULL), mpi.MPI_ERR_OP)
        _refused(mpi, call(WILD, WILD, WILD + 4, WILD, WILD + 8, WILD, 4, nb, bl, f, mpi.MPI_LAND), mpi.MPI_ERR_OP)
        for unit in (0, -1):
            for op in (mpi.MPI_SUM, mpi.MPI_NO_OP):
                _refused(mpi, call(WILD, WILD, WILD + 4, WILD, WILD + 8, WILD, unit, nb, bl, f, op), mpi.MPI_ERR_ARG,
                         "disp_unit")
        with pytest.raises(ValueError):
            mpi.fetch_indexed_ordered_plan_info(WILD, WILD, WILD, WILD, WILD, WILD, 0, nb, bl, f, mpi.MPI_SUM)
        info = mpi.fetch_indexed_ordered_plan_info(WILD, WILD, WILD, WILD, WILD, WILD, 4, nb, bl, f, mpi.MPI_SUM)
        assert info["form"] == EMPTY and info["launches"] == 0, info


@pytest.mark.parametrize("op", ["MPI_NO_OP", "MPI_REPLACE"])
def test_copy_ops_pass_the_op_check_and_end_at_residency(mpi, op):
    o = getattr(mpi, op)
    h = Host()
    # the ordered call refuses them as ops ...
    rc = mpi.reduce_local_indexed_ordered(h.pb, None, h.pa, h.tab, h.order, 16, h.nb, h.bl, mpi.MPI_FLOAT, o)
    _refused(mpi, rc, mpi.MPI_ERR_OP)
    # ... this one takes them on every basic type, and refuses the host memory
    for t in ("MPI_FLOAT", "MPI_UNSIGNED_CHAR", "MPI_SHORT", "MPI_DOUBLE", "MPI_LONG_DOUBLE", "MPI_LONG_DOUBLE_INT",
              "MPI_C_LONG_DOUBLE_COMPLEX", "MPI_SHORT_INT", "MPI_WCHAR"):
        _validated(mpi, _call(mpi, h, nb=2, bl=1, dt=mpi.DATATYPES[t], op=o))
    for dt in (0x8C010005, 0xCC000000, mpi.MPI_DATATYPE_NULL):
        _refused(mpi, _call(mpi, h, dt=dt, op=o), mpi.MPI_ERR_TYPE, "derived")
    assert h.untouched()


def test_user_null_and_undefined_ops(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    h = Host()
    try:
        _refused(mpi, _call(mpi, h, op=op.value), mpi.MPI_ERR_OP, "predefined")
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0
    _refused(mpi, _call(mpi, h, op=op.value), mpi.MPI_ERR_OP)      # the freed handle is invalid
    for handle in (mpi.MPI_OP_NULL, 0x18000003, 0x44000003, 0x58000000, 0x5800000F):
        _refused(mpi, _call(mpi, h, op=handle), mpi.MPI_ERR_OP)
        _refused(mpi, _call(mpi, h, pb=h.pa, op=handle, unit=0), mpi.MPI_ERR_OP)     # before the buffers and disp_unit
    for o in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            _refused(mpi, _call(mpi, h, dt=dt, op=o), mpi.MPI_ERR_OP, "not defined for this datatype")
    _refused(mpi, _call(mpi, h, op=mpi.MPI_BAND), mpi.MPI_ERR_OP)
    assert h.untouched()


def test_in_place_in_each_position_alias_and_disp_unit(mpi):
    h = Host()
    ip = mpi.MPI_IN_PLACE
    for kw, name in ((dict(pb=ip), "inbuf"), (dict(pa=ip), "inoutbuf"), (dict(pf=ip), "fetchbuf")):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, op=op, **kw), mpi.MPI_ERR_BUFFER, f"'{name}' cannot be MPI_IN_PLACE")
            _refused(mpi, _call(mpi, h, op=op, unit=0, **kw), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")    # before disp_unit
    # MPI_NO_OP never looks at inbuf; the other two positions are refused
    _validated(mpi, _call(mpi, h, pb=ip, op=mpi.MPI_NO_OP))
    _validated(mpi, _call(mpi, h, pb=0, tin=WILD, op=mpi.MPI_NO_OP))
    _refused(mpi, _call(mpi, h, pa=ip, op=mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    _refused(mpi, _call(mpi, h, pf=ip, op=mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    assert os.environ.get("MPIR_CVAR_COLL_ALIAS_CHECK", "1") != "0"
    for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, pb=h.pa, op=op), mpi.MPI_ERR_BUFFER, "aliased")
    _validated(mpi, _call(mpi, h, pb=h.pa, op=mpi.MPI_NO_OP))
    for unit in (0, -1, -16):
        _refused(mpi, _call(mpi, h, unit=unit), mpi.MPI_ERR_ARG, "disp_unit")
    _validated(mpi, _call(mpi, h))
    assert h.untouched()


def test_tables_fetchbuf_and_packed_overlap(mpi):
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, tio=None, op=op), mpi.MPI_ERR_ARG, "order table with no inout_displs")
        _refused(mpi, _call(mpi, h, pf=0, op=op), mpi.MPI_ERR_BUFFER, "fetchbuf")
        _refused(mpi, _call(mpi, h, pf=0, op=op, tio=None, order=None), mpi.MPI_ERR_BUFFER, "fetchbuf")
    for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, tin=h.tab, tio=None, order=None, op=op), mpi.MPI_ERR_ARG, "in_displs with no inout_displs")
    # both after disp_unit
    _refused(mpi, _call(mpi, h, tio=None, unit=0), mpi.MPI_ERR_ARG, "disp_unit")
    # no table at all is the fetch call; order NULL with a table passes the argument checks
    _validated(mpi, _call(mpi, h, tio=None, order=None))
    _validated(mpi, _call(mpi, h, order=None))
    # fetchbuf over a packed inbuf's nblocks x blocklen x size bytes
    buf = np.full(4096, 7, np.uint8)
    p = buf.ctypes.data + 256
    nbytes = h.nb * h.bl * 4
    for pf in (p + 1024 + nbytes - 1, p + 1024 - nbytes + 1, p + 1024):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, pb=p + 1024, pa=p, pf=pf, op=op), mpi.MPI_ERR_BUFFER, "fetchbuf overlaps inbuf")
        _validated(mpi, _call(mpi, h, pb=p + 1024, pa=p, pf=pf, op=mpi.MPI_NO_OP))
        # an input with a table is no range the library can see
        _validated(mpi, _call(mpi, h, pb=p + 1024, pa=p, pf=pf, tin=h.tab))
    for pf in (p + 1024 + nbytes, p + 1024 - nbytes):
        _validated(mpi, _call(mpi, h, pb=p + 1024, pa=p, pf=pf))       # touching is not overlapping
    _refused(mpi, _call(mpi, h, pb=p + 2048, pa=p, pf=p + 8, tio=None, order=None), mpi.MPI_ERR_BUFFER,
             "fetchbuf overlaps inoutbuf")
    assert (buf == 7).all() and h.untouched()


def test_shim_answers_alike(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 6)()
    f32 = mpi.ELEM["F32"]
    sum_ = mpi.MPI_SUM & 0xF

    def info(op, elem, unit=16, nb=4, bl=4, ti=None, to=TAB_O, od=TAB_ORD):
        return lib.MPIR_Hip_fetch_indexed_ordered_plan_info(BASE, ti, FAR, to, FETCH, od, unit, nb, bl, op, elem, out)

    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL and info(0, f32) == ENOKERNEL and info(sum_, 99) == ENOKERNEL
    assert info(mpi.MPI_NO_OP & 0xF, 99) == ENOKERNEL
    assert info(sum_, f32) == 0 and info(mpi.MPI_NO_OP & 0xF, f32) == 0 and info(mpi.MPI_REPLACE & 0xF, f32) == 0
    assert info(sum_, f32, unit=0) == EARG and info(sum_, f32, unit=0, nb=0) == EARG
    assert info(sum_, f32, to=None) == EARG                         # an order and a packed target
    assert info(sum_, f32, to=None, od=None, ti=TAB_I) == EARG      # a gather onto a packed target
    assert info(mpi.MPI_NO_OP & 0xF, f32, to=None, od=None, ti=TAB_I) == 0      # NO_OP never looks at in_displs
    assert info(sum_, f32, to=None, od=None) == 0 and out[0] == SINGLE
    assert info(sum_, f32, od=None) == 0 and out[0] == NARROW_VEC   # order NULL: the identity, the same plan
    assert info(sum_, f32, nb=(1 << 31)) == EARG and info(sum_, f32, nb=(1 << 31) - 1) == 0
    h = Host()
    assert lib.MPIR_Hip_reduce_fetch_indexed_ordered(h.pb, None, h.pa, h.tab.ctypes.data, h.pf, h.order.ctypes.data, 16,
                                                     h.nb, h.bl, sum_, f32, None, 1) == EBUFFER
    assert lib.MPIR_Hip_reduce_fetch_indexed_ordered(WILD, WILD, WILD, WILD, WILD, WILD, 1, 4, 0, sum_, f32, None, 1) == 0
    assert h.untouched()
    # every pair of the ordered call has a kernel here, and the byte ops every element class
    for op in range(16):
        for elem in range(64):
            od = lib.MPIR_Hip_indexed_ordered_plan_info(BASE, None, FAR, TAB_O, TAB_ORD, 16, 4, 4, op, elem, out)
            fo = info(op, elem)
            if op in (mpi.MPI_NO_OP & 0xF, mpi.MPI_REPLACE & 0xF):
                assert (fo == 0) == bool(lib.MPIR_Hip_elem_size(elem)) and fo in (0, ENOKERNEL), (op, elem, fo)
            else:
                assert (od == ENOKERNEL) == (fo == ENOKERNEL) and fo in (0, ENOKERNEL), (op, elem, od, fo)


def test_plan_is_the_ordered_calls_where_fetchbuf_is_aligned(mpi):
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    thr = mpi.indexed_plan_info(BASE, 0, FAR, TAB_O, 1, 1, 1, dt, o)["threshold"]
    seen = set()
    for nb, bl, unit, di, do in ((400, 12, 16, 0, 0), (400, 12, 16, 16, 32), (400, 12, 4, 0, 0), (400, 12, 16, 4, 0),
                                 (400, 12, 16, 0, 8), (70000, 3, 4, 0, 0), (5, thr // 4 + 4099, 4, 4, 4), (1, 12, 16, 0, 0)):
        for ti in (None, TAB_I):
            want = mpi.indexed_ordered_plan_info(BASE + di, ti, FAR + do, TAB_O, TAB_ORD, unit, nb, bl, dt, o)
            for df in (0, 16, 48):
                for od in (TAB_ORD, None):
                    got = mpi.fetch_indexed_ordered_plan_info(BASE + di, ti, FAR + do, TAB_O, FETCH + df, od, unit, nb, bl, dt, o)
                    assert got == want, (nb, bl, unit, di, do, df, got, want)
            seen.add(want["form"])
            for df in (4, 8, 12, 20):
                got = mpi.fetch_indexed_ordered_plan_info(BASE + di, ti, FAR + do, TAB_O, FETCH + df, TAB_ORD, unit, nb, bl, dt, o)
                if want["form"] == NARROW_VEC:
                    assert got["form"] == NARROW_ELEMS and got["launches"] >= 1, (df, got)
                    elems = mpi.indexed_ordered_plan_info(BASE + di + 4, ti, FAR + do, TAB_O, TAB_ORD, unit, nb, bl, dt, o)
                    assert got == elems, (got, elems)
                else:
                    assert got == want, (df, got, want)
    assert seen == {WIDE, NARROW_VEC, NARROW_ELEMS}, seen
    # MPI_NO_OP never looks at inbuf or in_displs: their alignment does not count
    got = mpi.fetch_indexed_ordered_plan_info(BASE + 4, TAB_I, FAR, TAB_O, FETCH, TAB_ORD, 16, 400, 12, dt, mpi.MPI_NO_OP)
    assert got["form"] == NARROW_VEC, got
    got = mpi.fetch_indexed_ordered_plan_info(0, 0, FAR, TAB_O, FETCH + 4, TAB_ORD, 16, 400, 12, dt, mpi.MPI_NO_OP)
    assert got["form"] == NARROW_ELEMS, got
    # no table at all: the fetch call's plan
    single = mpi.fetch_plan_info(BASE, FAR, FETCH, 4800, dt, o)
    got = mpi.fetch_indexed_ordered_plan_info(BASE, None, FAR, None, FETCH, None, 16, 400, 12, dt, o)
    assert (got["form"], got["launches"], got["groups"]) == (SINGLE, 1, single["groups"]), (got, single)
