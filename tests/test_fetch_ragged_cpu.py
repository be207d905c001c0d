"""MPIX_Reduce_local_fetch_ragged without a GPU: its argument checks through the
C ABI on host buffers (which a sound call is then refused for as non-device
memory, so a check that comes earlier shows by its class and text), and its
launch planner (MPIR_Hip_fetch_ragged_plan_info: the planner the launch itself
runs, host arithmetic on the addresses and counts) on made-up addresses.

The argument rules are MPIX_Reduce_local_ragged's in that call's order, with
MPIX_Reduce_local_fetch's validation of the op (MPI_NO_OP and MPI_REPLACE pass)
and its rules for fetchbuf on top.  Host tables are read before the operands'
residency is looked at, so an unsound starts and an overflowing displacement
show here too.  (A host table with a stream, a piece outside device memory and
fetchbuf inside the pieces' extent need device operands to get that far:
test_fetch_ragged_gpu.py.)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX

TILE = 16384
BASE = 1 << 32               # inbuf's arena
FAR = 1 << 40                # inoutbuf's
FETCH = 1 << 41              # fetchbuf's
TAB_O, TAB_S = (1 << 44) + (1 << 30), (1 << 44) + (1 << 31)     # where device tables would be
WILD = 0x10                  # an address that would fault if touched
EMPTY, SINGLE, RAGGED = range(3)
EBUFFER, ENOKERNEL, EARG = 1, 3, 5
INT_MAX = (1 << 31) - 1
MAX_GROUPS = 1 << 23         # MPIR_HIP_BATCH_MAX_GROUPS
NAMES = ("MPIX_Reduce_local_fetch_ragged", "MPIR_Hip_reduce_fetch_ragged", "MPIR_Hip_fetch_ragged_plan_info")
# one type of each element size, for the two byte ops
BY_SIZE = {1: "MPI_UNSIGNED_CHAR", 2: "MPI_SHORT", 4: "MPI_FLOAT", 8: "MPI_DOUBLE", 16: "MPI_LONG_DOUBLE",
           32: "MPI_LONG_DOUBLE_INT"}


class Host:
    """Three host arrays (in = 1, inout = 2, fetch = 3, floats), two sound host
    tables, and a check that a refused call left all of them alone."""

    def __init__(self, n=64, pieces=4):
        self.b = np.full(n, 1, np.float32)
        self.a = np.full(n, 2, np.float32)
        self.f = np.full(n, 3, np.float32)
        self.pb, self.pa, self.pf = self.b.ctypes.data, self.a.ctypes.data, self.f.ctypes.data
        self.n = pieces
        self.count = 4 * pieces
        self.tab = np.arange(pieces, dtype=np.int64)
        self.starts = np.arange(pieces + 1, dtype=np.int64) * 4

    def untouched(self):
        return ((self.b == 1).all() and (self.a == 2).all() and (self.f == 3).all() and
                (self.tab == np.arange(self.n)).all() and (self.starts == np.arange(self.n + 1) * 4).all())


def _call(mpi, h, pb="b", pa="a", pf="f", n=None, count=None, unit=16, dt=None, op=None, tab="t", starts="s", stream=0):
    return mpi.reduce_local_fetch_ragged(h.pb if pb == "b" else pb, h.pa if pa == "a" else pa,
                                         h.tab if isinstance(tab, str) else tab, h.pf if pf == "f" else pf,
                                         h.starts if isinstance(starts, str) else starts, unit,
                                         h.n if n is None else n, h.count if count is None else count,
                                         mpi.MPI_FLOAT if dt is None else dt, mpi.MPI_SUM if op is None else op, stream)


def _refused(mpi, rc, cls, text=None):
    assert mpi.error_class(rc) == cls, mpi.error_string(rc)
    if text:
        assert text in mpi.error_string(rc), mpi.error_string(rc)


def _validated(mpi, rc):
    """The call passed every argument check and was then refused as host memory."""
    _refused(mpi, rc, mpi.MPI_ERR_BUFFER, "device-resident")


def _plan(mpi, to, ts, unit, n, count, t="MPI_FLOAT", op="MPI_SUM", ai=BASE, ao=FAR, af=FETCH):
    return mpi.fetch_ragged_plan_info(ai, ao, to, af, ts, unit, n, count, mpi.DATATYPES[t], getattr(mpi, op))


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    assert "MPIX_Reduce_local_fetch_ragged(" in open(os.path.join(inc, "mpi_reduce_local.h")).read()
    shim = open(os.path.join(inc, "mpir_hip_reduce.h")).read()
    assert "MPIR_Hip_reduce_fetch_ragged(" in shim and "MPIR_Hip_fetch_ragged_plan_info(" in shim


def test_negative_counts(mpi):
    h = Host()
    for n, count in ((-1, 4), (4, -1), (-3, -3), (-1, 0), (0, -1)):
        for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, n=n, count=count, op=op), mpi.MPI_ERR_COUNT, "negative")
    # ... before the op
    _refused(mpi, _call(mpi, h, n=-1, op=mpi.MPI_OP_NULL), mpi.MPI_ERR_COUNT)
    assert h.untouched()


def test_zero_count_succeeds_without_touching_a_pointer_or_a_table(mpi):
    f = mpi.MPI_FLOAT
    ip = mpi.MPI_IN_PLACE
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        for n in (0, 4):
            for pin, pio, pf in ((WILD, WILD + 4, WILD + 8), (WILD, WILD, WILD), (0, 0, 0), (ip, ip, ip)):
                for to, ts in ((WILD, WILD), (0, WILD), (WILD, 0), (0, 0)):
                    assert mpi.reduce_local_fetch_ragged(pin, pio, to, pf, ts, 4, n, 0, f, op) == 0, (op, n, pin, to, ts)
                    # ... on a stream too: a wild (host) table is not looked at either
                    assert mpi.reduce_local_fetch_ragged(pin, pio, to, pf, ts, 4, n, 0, f, op, stream=WILD) == 0
    # ... but the op and disp_unit still are
    for n in (0, 4):
        _refused(mpi, mpi.reduce_local_fetch_ragged(WILD, WILD + 4, WILD, WILD + 8, WILD, 4, n, 0, f, mpi.MPI_OP_NULL),
                 mpi.MPI_ERR_OP)
        _refused(mpi, mpi.reduce_local_fetch_ragged(WILD, WILD + 4, WILD, WILD + 8, WILD, 4, n, 0, f, mpi.MPI_LAND),
                 mpi.MPI_ERR_OP)
        for unit in (0, -1):
            for op in (mpi.MPI_SUM, mpi.MPI_NO_OP):
                _refused(mpi, mpi.reduce_local_fetch_ragged(WILD, WILD + 4, WILD, WILD + 8, WILD, unit, n, 0, f, op),
                         mpi.MPI_ERR_ARG, "disp_unit")
        with pytest.raises(ValueError):
            _plan(mpi, WILD, WILD, 0, n, 0)


@pytest.mark.parametrize("op", ["MPI_OP_NULL", "BAD_KIND", "BAD_MPI_KIND", "INDEX_0", "INDEX_15"])
def test_null_and_invalid_ops(mpi, op):
    """MPIR_ERRTEST_OP_GACC, as MPIX_Reduce_local_fetch answers"""
    handle = {"MPI_OP_NULL": mpi.MPI_OP_NULL, "BAD_KIND": 0x18000003, "BAD_MPI_KIND": 0x44000003,
              "INDEX_0": 0x58000000, "INDEX_15": 0x5800000F}[op]
    h = Host()
    rc = _call(mpi, h, op=handle)
    _refused(mpi, rc, mpi.MPI_ERR_OP)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 4, mpi.MPI_FLOAT, handle))
    # the op comes before the buffers and before disp_unit
    _refused(mpi, _call(mpi, h, pb=h.pa, op=handle, unit=0), mpi.MPI_ERR_OP)
    assert h.untouched()


@pytest.mark.parametrize("op", ["MPI_NO_OP", "MPI_REPLACE"])
def test_copy_ops_pass_validation_and_are_refused_only_as_host_memory(mpi, op):
    o = getattr(mpi, op)
    h = Host()
    # refused by the ragged call, accepted here
    rc = mpi.reduce_local_ragged(h.pb, None, h.pa, h.tab, h.starts, 16, h.n, h.count, mpi.MPI_FLOAT, o)
    _refused(mpi, rc, mpi.MPI_ERR_OP)
    # every basic type of the table, and a builtin one outside it (MPI_WCHAR, by its handle's size)
    for t in ("MPI_FLOAT", "MPI_UNSIGNED_CHAR", "MPI_SHORT", "MPI_DOUBLE", "MPI_LONG_DOUBLE", "MPI_LONG_DOUBLE_INT",
              "MPI_C_LONG_DOUBLE_COMPLEX", "MPI_SHORT_INT", "MPI_WCHAR"):
        _validated(mpi, _call(mpi, h, n=2, count=2, starts=np.arange(3, dtype=np.int64), dt=mpi.DATATYPES[t], op=o))
    # derived handles (direct and indirect kind), a builtin-kind handle of another object class, the null handle
    for dt in (0x8C010005, 0xCC000000, 0x48000406, mpi.MPI_DATATYPE_NULL):
        _refused(mpi, _call(mpi, h, dt=dt, op=o), mpi.MPI_ERR_TYPE, "derived")
    assert h.untouched()


def test_user_op_and_undefined_pairs(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    h = Host()
    try:
        _refused(mpi, _call(mpi, h, op=op.value), mpi.MPI_ERR_OP, "predefined")
        assert h.untouched()
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0
    _refused(mpi, _call(mpi, h, op=op.value), mpi.MPI_ERR_OP)      # the freed handle is invalid
    for o in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            _refused(mpi, _call(mpi, h, dt=dt, op=o), mpi.MPI_ERR_OP, "not defined for this datatype")
    # MPI_Reduce_local's datatype check: the same class as the single call's
    rc = _call(mpi, h, op=mpi.MPI_BAND)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local(h.pb, h.pa, 2, mpi.MPI_FLOAT, mpi.MPI_BAND)) == mpi.MPI_ERR_OP
    rc = _call(mpi, h, dt=mpi.MPI_DATATYPE_NULL)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local(h.pb, h.pa, 2, mpi.MPI_DATATYPE_NULL, mpi.MPI_SUM))
    assert h.untouched()


def test_in_place_in_each_position_then_disp_unit(mpi):
    h = Host()
    ip = mpi.MPI_IN_PLACE
    for kw, name in ((dict(pb=ip), "inbuf"), (dict(pa=ip), "inoutbuf"), (dict(pf=ip), "fetchbuf")):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, op=op, **kw), mpi.MPI_ERR_BUFFER, f"'{name}' cannot be MPI_IN_PLACE")
            # ... before disp_unit, as in the ragged call
            _refused(mpi, _call(mpi, h, op=op, unit=0, **kw), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    # MPI_NO_OP never looks at inbuf; the other two positions are refused
    _validated(mpi, _call(mpi, h, pb=ip, op=mpi.MPI_NO_OP))
    _refused(mpi, _call(mpi, h, pa=ip, op=mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    _refused(mpi, _call(mpi, h, pf=ip, op=mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    for unit in (0, -1, -16):
        _refused(mpi, _call(mpi, h, unit=unit), mpi.MPI_ERR_ARG, "disp_unit")
    # every positive unit passes the argument checks (a host table's products fit)
    for unit in (1, 3, 4, 16, 1 << 40):
        _validated(mpi, _call(mpi, h, unit=unit))
    assert h.untouched()


def test_null_fetchbuf(mpi):
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, pf=0, op=op), mpi.MPI_ERR_BUFFER, "fetchbuf")
        # ... with a contiguous target too
        _refused(mpi, _call(mpi, h, pf=0, op=op, tab=None), mpi.MPI_ERR_BUFFER, "fetchbuf")
    _validated(mpi, _call(mpi, h, pb=0, op=mpi.MPI_NO_OP))         # MPI_NO_OP with a NULL inbuf passes validation
    assert h.untouched()


def test_aliased_operands_with_the_check_on(mpi):
    assert os.environ.get("MPIR_CVAR_COLL_ALIAS_CHECK", "1") != "0"
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, pb=h.pa, op=op), mpi.MPI_ERR_BUFFER, "aliased")
        _refused(mpi, _call(mpi, h, pb=h.pa, op=op, unit=0), mpi.MPI_ERR_BUFFER, "aliased")      # before disp_unit
    _validated(mpi, _call(mpi, h, pb=h.pa, op=mpi.MPI_NO_OP))      # MPI_NO_OP never looks at inbuf
    assert h.untouched()


_ALIAS_OFF = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import mpich_pip_amd as m
lib = m.load()
assert lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN) == 0
a = np.full(256, 2, np.float32)
f = np.full(64, 3, np.float32)
tab = np.arange(4, dtype=np.int64)
starts = np.arange(5, dtype=np.int64) * 4
def call(pb, pa, pf, op=m.MPI_SUM, t=tab):
    return m.reduce_local_fetch_ragged(pb, pa, t, pf, starts, 16, 4, 16, m.MPI_FLOAT, op)
rc = call(a.ctypes.data, a.ctypes.data, f.ctypes.data)
assert m.error_class(rc) == m.MPI_ERR_BUFFER, m.error_string(rc)
assert "device-resident" in m.error_string(rc) and "aliased" not in m.error_string(rc), m.error_string(rc)
# the overlap of fetchbuf with inbuf is checked whatever the alias check says
for pf in (a.ctypes.data + 512 + 63, a.ctypes.data + 512 - 63, a.ctypes.data + 512):
    for op in (m.MPI_SUM, m.MPI_REPLACE):
        rc = call(a.ctypes.data + 512, a.ctypes.data, pf, op)
        assert m.error_class(rc) == m.MPI_ERR_BUFFER and "fetchbuf overlaps inbuf" in m.error_string(rc), m.error_string(rc)
    rc = call(a.ctypes.data + 512, a.ctypes.data, pf, m.MPI_NO_OP)
    assert m.error_class(rc) == m.MPI_ERR_BUFFER and "device-resident" in m.error_string(rc), m.error_string(rc)
# ... and with a contiguous target's range
rc = call(a.ctypes.data + 512, a.ctypes.data, a.ctypes.data + 8, t=None)
assert m.error_class(rc) == m.MPI_ERR_BUFFER and "fetchbuf overlaps inoutbuf" in m.error_string(rc), m.error_string(rc)
assert (a == 2).all() and (f == 3).all()
print("alias-off ok")
"""


def test_fetchbuf_overlapping_inbuf_with_the_alias_check_off():
    """MPIR_CVAR_COLL_ALIAS_CHECK=0 is read once per process: a fresh one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPIR_CVAR_COLL_ALIAS_CHECK="0")
    r = subprocess.run([sys.executable, "-c", _ALIAS_OFF.format(paths=[os.path.join(root, "mpich-pip_amd"), root])],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "alias-off ok" in r.stdout, r.stdout + r.stderr


def test_fetchbuf_overlapping_inbuf(mpi):
    """the two packed ranges, count x size bytes each"""
    buf = np.full(2048, 7, np.uint8)
    p = buf.ctypes.data + 256
    h = Host()
    nb = h.count * 4                                # 16 floats
    for pf in (p + 512 + nb - 1, p + 512 - nb + 1, p + 512, p + 512 + 4):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            _refused(mpi, _call(mpi, h, pb=p + 512, pa=p, pf=pf, op=op), mpi.MPI_ERR_BUFFER, "fetchbuf overlaps inbuf")
        _validated(mpi, _call(mpi, h, pb=p + 512, pa=p, pf=pf, op=mpi.MPI_NO_OP))
    # touching is not overlapping
    for pf in (p + 512 + nb, p + 512 - nb):
        _validated(mpi, _call(mpi, h, pb=p + 512, pa=p, pf=pf))
    # the ranges are the datatype's: 16 doubles reach twice as far
    _refused(mpi, _call(mpi, h, pb=p + 512, pa=p, pf=p + 512 + 2 * nb - 1, dt=mpi.MPI_DOUBLE), mpi.MPI_ERR_BUFFER, "overlaps")
    assert (buf == 7).all() and h.untouched()


def test_no_pieces_and_no_starts(mpi):
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        _refused(mpi, _call(mpi, h, n=0, op=op), mpi.MPI_ERR_ARG, "no pieces")
        _refused(mpi, _call(mpi, h, n=0, op=op, tab=None, starts=None), mpi.MPI_ERR_ARG)       # with no table either
        _refused(mpi, _call(mpi, h, op=op, starts=None), mpi.MPI_ERR_ARG, "starts")
    # both after disp_unit
    _refused(mpi, _call(mpi, h, n=0, unit=0), mpi.MPI_ERR_ARG, "disp_unit")
    _refused(mpi, _call(mpi, h, starts=None, unit=0), mpi.MPI_ERR_ARG, "disp_unit")
    # a contiguous target needs no starts
    _validated(mpi, _call(mpi, h, tab=None, starts=None))
    _validated(mpi, _call(mpi, h, tab=None, starts=WILD))
    assert h.untouched()


def test_host_tables_are_read_and_refused(mpi):
    """starts must begin at 0, never decrease and end at count; every
    displacement times disp_unit must fit an MPI_Aint: MPI_ERR_ARG, before the
    operands are looked at (host memory here, which a sound call is refused for)."""
    n, count = 300, 1200
    h = Host(2048, n)
    good, tab = h.starts, h.tab
    first = good.copy()
    first[0] = 1
    down = good.copy()
    down[100] = down[99] - 1
    short, long_ = good.copy(), good.copy()
    short[-1] -= 1
    long_[-1] += 1
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        for what, starts in (("starts[0] != 0", first), ("a decreasing entry", down), ("ends short of count", short),
                             ("ends past count", long_)):
            rc = _call(mpi, h, op=op, starts=starts)
            assert mpi.error_class(rc) == mpi.MPI_ERR_ARG and "starts" in mpi.error_string(rc), (what, mpi.error_string(rc))
    # empty pieces are sound: equal neighbours, at either end too
    flat = good.copy()
    flat[1], flat[-2], flat[150] = 0, count, flat[149]
    _validated(mpi, _call(mpi, h, starts=flat))
    big = tab.copy()
    big[7] = 1 << 60
    neg = tab.copy()
    neg[299] = -(1 << 60)
    for t in (big, neg):
        _refused(mpi, _call(mpi, h, tab=t), mpi.MPI_ERR_ARG, "address space")
        # ... with disp_unit 1 the same entries fit: the operands are then refused
        _validated(mpi, _call(mpi, h, tab=t, unit=1))
    assert h.untouched()


@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_NO_OP", "MPI_REPLACE"])
@pytest.mark.parametrize("table", [False, True], ids=["contiguous", "ragged"])
def test_host_pointers_refused_as_non_device(mpi, op, table):
    h = Host(2048, 300)
    o = getattr(mpi, op)
    rc = _call(mpi, h, op=o, tab="t" if table else None)
    _validated(mpi, rc)
    assert "aliased" not in mpi.error_string(rc)
    # the shim answers the same on its own
    lib = mpi.load()
    assert lib.MPIR_Hip_reduce_fetch_ragged(h.pb, h.pa, h.tab.ctypes.data if table else None, h.pf, h.starts.ctypes.data,
                                            16, h.n, h.count, o & 0xF, mpi.ELEM["F32"], None, 1) == EBUFFER
    assert h.untouched()


def test_shim_refuses_unknown_pairs_and_bad_arguments(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 7)()
    f32 = mpi.ELEM["F32"]
    sum_ = mpi.MPI_SUM & 0xF

    def info(op, elem, unit=16, n=4, count=16, ts=TAB_S, to=TAB_O):
        return lib.MPIR_Hip_fetch_ragged_plan_info(BASE, FAR, to, FETCH, ts, unit, n, count, op, elem, out)

    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL            # no BAND on floats
    assert info(mpi.MPI_MAXLOC & 0xF, f32) == ENOKERNEL
    assert info(0, f32) == ENOKERNEL and info(15, f32) == ENOKERNEL and info(sum_, 99) == ENOKERNEL
    assert info(mpi.MPI_NO_OP & 0xF, 99) == ENOKERNEL and info(mpi.MPI_REPLACE & 0xF, 0) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_fetch_ragged(BASE, FAR, TAB_O, FETCH, TAB_S, 16, 4, 16, mpi.MPI_BAND & 0xF, f32, None, 1) == ENOKERNEL
    assert info(sum_, f32) == 0 and info(mpi.MPI_NO_OP & 0xF, f32) == 0 and info(mpi.MPI_REPLACE & 0xF, f32) == 0
    assert info(sum_, f32, unit=0) == EARG and info(sum_, f32, unit=1 << 63) == EARG
    assert info(sum_, f32, unit=0, count=0) == EARG                # whatever the counts
    assert lib.MPIR_Hip_reduce_fetch_ragged(WILD, WILD, WILD, WILD, WILD, 0, 0, 0, sum_, f32, None, 1) == EARG
    assert info(sum_, f32, n=0, count=0) == 0 and info(sum_, f32, n=4, count=0) == 0    # nothing to do
    assert lib.MPIR_Hip_reduce_fetch_ragged(WILD, WILD, WILD, WILD, WILD, 1, 4, 0, sum_, f32, None, 1) == 0
    assert info(sum_, f32, n=0) == EARG                             # elements and no pieces
    assert info(sum_, f32, n=0, to=None) == EARG
    assert info(sum_, f32, ts=None) == EARG                         # a table and no starts
    assert lib.MPIR_Hip_reduce_fetch_ragged(WILD, WILD, WILD, WILD, None, 4, 4, 16, sum_, f32, None, 1) == EARG
    assert info(sum_, f32, ts=None, to=None) == 0                   # the contiguous target needs none
    assert info(sum_, f32, count=INT_MAX) == 0 and info(sum_, f32, count=INT_MAX + 1) == EARG
    assert info(sum_, f32, n=INT_MAX, count=INT_MAX) == 0 and info(sum_, f32, n=INT_MAX + 1, count=INT_MAX) == EARG
    with pytest.raises(ValueError):
        _plan(mpi, TAB_O, TAB_S, 0, 4, 16)
    with pytest.raises(LookupError):
        _plan(mpi, TAB_O, TAB_S, 16, 4, 16, op="MPI_BAND")
    with pytest.raises(TypeError):
        _plan(mpi, TAB_O, np.arange(5, dtype=np.int32), 16, 4, 16)


def test_every_pair_of_the_ragged_call_has_a_kernel_and_the_byte_ops_every_size(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 7)()
    both = 0
    sizes = {}
    for elem in range(64):
        size = lib.MPIR_Hip_elem_size(elem)
        if size:
            sizes.setdefault(size, []).append(elem)
    assert sorted(sizes) == [1, 2, 4, 8, 16, 32], sizes
    for op in range(16):
        for elem in range(64):
            rag = lib.MPIR_Hip_ragged_plan_info(BASE, None, FAR, TAB_O, TAB_S, 16, 4, 16, op, elem, out)
            fr = lib.MPIR_Hip_fetch_ragged_plan_info(BASE, FAR, TAB_O, FETCH, TAB_S, 16, 4, 16, op, elem, out)
            if op in (mpi.MPI_NO_OP & 0xF, mpi.MPI_REPLACE & 0xF):
                # every element class, whatever the ragged call has for it
                assert (fr == 0) == bool(lib.MPIR_Hip_elem_size(elem)) and fr in (0, ENOKERNEL), (op, elem, fr)
            else:
                assert (rag == ENOKERNEL) == (fr == ENOKERNEL) and fr in (0, ENOKERNEL), (op, elem, rag, fr)
                both += fr == 0
    assert both >= len([1 for o, t in MATRIX if T.compute_ok(o, t)]) // 4 > 0
    for size, t in BY_SIZE.items():
        assert T.elem_size(t) == size
        for op in ("MPI_NO_OP", "MPI_REPLACE"):
            info = mpi.fetch_ragged_plan_info(BASE, FAR, TAB_O, FETCH, TAB_S, 16, 4, 16, mpi.DATATYPES[t], getattr(mpi, op))
            assert (info["form"], info["launches"], info["per"]) == (RAGGED, 1, TILE // size), (t, op, info)


# ---------------------------------------------------------------- the planner
def test_empty_and_single(mpi):
    for n in (0, 100):
        for op in ("MPI_SUM", "MPI_NO_OP", "MPI_REPLACE"):
            info = mpi.fetch_ragged_plan_info(WILD, WILD, WILD, WILD, WILD, 4, n, 0, mpi.MPI_FLOAT, getattr(mpi, op))
            assert info == dict(form=EMPTY, launches=0, groups=0, per=0, rounds=0, lds_entries=0, packed_sides_aligned=0)
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    # no table: the fetch call on count elements at any phase, starts given or not
    for ai, ao, af, n, count in ((BASE, FAR, FETCH, 1, 100000), (BASE + 4, FAR, FETCH, 7, 100000),
                                 (BASE, FAR + 8, FETCH + 8, 3000, 9000), (BASE + 4, FAR + 8, FETCH, 3, 6)):
        for unit in (1, 16, 12345):
            for ts in (0, TAB_S, WILD):
                info = mpi.fetch_ragged_plan_info(ai, ao, None, af, ts, unit, n, count, dt, o)
                single = mpi.fetch_plan_info(ai, ao, af, count, dt, o)
                assert (info["form"], info["launches"], info["groups"]) == (SINGLE, 1, single["groups"]), (info, single)
    # ... whose copy ops are device copies: one for MPI_NO_OP, two for MPI_REPLACE
    assert mpi.fetch_ragged_plan_info(BASE, FAR, None, FETCH, 0, 4, 3, 9, dt, mpi.MPI_NO_OP)["launches"] == 1
    assert mpi.fetch_ragged_plan_info(BASE, FAR, None, FETCH, 0, 4, 3, 9, dt, mpi.MPI_REPLACE)["launches"] == 2
    # a table is not the fetch call -- not even for one piece
    assert _plan(mpi, TAB_O, TAB_S, 4, 3000, 9000)["form"] == RAGGED
    assert _plan(mpi, TAB_O, TAB_S, 4, 1, 3)["form"] == RAGGED
    for op in ("MPI_NO_OP", "MPI_REPLACE"):
        assert _plan(mpi, TAB_O, TAB_S, 4, 1, 3, op=op)["launches"] == 1


def test_one_launch_of_the_packed_spans_for_every_size(mpi):
    """ceil(count x size / 16 KiB) workgroups of 16 KiB / size elements, one
    launch, for every element size from 1 to 32 bytes with count around
    multiples of the span -- whatever the phases or npieces, and for the byte
    ops as for a combine."""
    seen = set()
    for op, t in MATRIX:
        esz = T.elem_size(t)
        if esz in seen or not T.compute_ok(op, t):
            continue
        seen.add(esz)
        per = TILE // esz
        for k in (1, 2, 5, 1000):
            for count in (k * per - 1, k * per, k * per + 1):
                for n, ai, o in ((1, BASE, op), (count, BASE + esz, op), (70000, BASE + 4, "MPI_NO_OP"),
                                 (7, BASE, "MPI_REPLACE")):
                    info = _plan(mpi, TAB_O, TAB_S, 1, n, count, t=t, op=o, ai=ai)
                    assert (info["form"], info["launches"], info["per"]) == (RAGGED, 1, per), (t, count, info)
                    assert info["groups"] == -(-count * esz // TILE) == -(-count // per), (t, count, info)
    assert seen >= {1, 2, 4, 8, 16, 32}, seen


def test_search_rounds_and_lds(mpi):
    for n, rounds in ((1, 1), (2, 1), (63, 1), (64, 2), (65, 2), (4095, 2), (4096, 3), (4097, 3), (262143, 3),
                      (262144, 4), (INT_MAX, 6)):
        info = _plan(mpi, TAB_O, TAB_S, 4, n, max(n, 5000))
        assert info["rounds"] == rounds, (n, info)
        assert 64 ** rounds >= n + 1 > 64 ** (rounds - 1)
        # the boundaries and one side's offsets (8 bytes each for the first 256 pieces): 13 KiB
        assert info["lds_entries"] % 256 == 0 and info["lds_entries"] * 4 + 256 * 8 == 13 << 10, info


def test_packed_sides_aligned_exactly_when_both_packed_bases_are(mpi):
    for di in range(0, 20, 4):
        for df in range(0, 20, 4):
            for do in (0, 4, 8):        # the target's phase is the device's to look at
                info = _plan(mpi, TAB_O, TAB_S, 4, 100, 5000, ai=BASE + di, ao=FAR + do, af=FETCH + df)
                assert info["packed_sides_aligned"] == int(di % 16 == 0 and df % 16 == 0), (di, df, do, info)
                # MPI_NO_OP never looks at inbuf
                info = _plan(mpi, TAB_O, TAB_S, 4, 100, 5000, op="MPI_NO_OP", ai=BASE + di, ao=FAR + do, af=FETCH + df)
                assert info["packed_sides_aligned"] == int(df % 16 == 0), (di, df, do, info)
    assert _plan(mpi, TAB_O, TAB_S, 1, 100, 5000, t="MPI_UNSIGNED_CHAR", op="MPI_BXOR", ai=BASE + 1)["packed_sides_aligned"] == 0


def test_int_max_elements_of_the_32_byte_class_fit_one_launch(mpi):
    info = _plan(mpi, TAB_O, TAB_S, 16, 1000, INT_MAX, t="MPI_LONG_DOUBLE_INT", op="MPI_MAXLOC")
    assert info["launches"] == 1 and info["groups"] == -(-INT_MAX * 32 // TILE) < MAX_GROUPS, info
    info = _plan(mpi, TAB_O, TAB_S, 16, 1000, INT_MAX, t="MPI_LONG_DOUBLE_INT", op="MPI_REPLACE")
    assert info["launches"] == 1 and info["groups"] == -(-INT_MAX * 32 // TILE), info
    info = _plan(mpi, TAB_O, TAB_S, 1, INT_MAX, INT_MAX, t="MPI_UNSIGNED_CHAR", op="MPI_BXOR")
    assert info["launches"] == 1 and info["groups"] == -(-INT_MAX // TILE), info
