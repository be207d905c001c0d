"""MPIX_Reduce_local_fetch without a GPU: its argument checks through the C ABI,
and its planner (MPIR_Hip_fetch_plan_info: the planner the launch itself runs,
host arithmetic on the pointer values) on made-up addresses.

Every refused call must leave its buffers as they were; where the error
precedes classification the buffers are host arrays, so that shows here.  A
call that passes validation ends, on host arrays, at the residency check
("device-resident"): that is how a case "accepted as far as validation goes" is
told from one validation refused.

What the planner must get right is what the kernel relies on: the tile path
exactly when all three pointers are naturally aligned and congruent mod 16, its
grid the batch's for the segment (in, io, count), tile 0's head and tail
elements the single call's.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _types as T

TILE = 16384
BASE = 1 << 32               # inbuf's arena
FAR = 1 << 40                # inoutbuf's
FETCH = 1 << 41              # fetchbuf's
WILD = 0x10                  # an address that would fault if touched
EMPTY, COPY, TILEP, ELEMS = range(4)
BATCH_TILE = 1
ENOKERNEL = 3


class Host:
    """Three host arrays (in = 1, inout = 2, fetch = 3, floats) and a check that
    a refused call left them alone."""

    def __init__(self, n=64):
        self.b = np.full(n, 1, np.float32)
        self.a = np.full(n, 2, np.float32)
        self.f = np.full(n, 3, np.float32)
        self.pb, self.pa, self.pf = self.b.ctypes.data, self.a.ctypes.data, self.f.ctypes.data

    def untouched(self):
        return (self.b == 1).all() and (self.a == 2).all() and (self.f == 3).all()


def _refused(mpi, rc, cls, text=None):
    assert mpi.error_class(rc) == cls, mpi.error_string(rc)
    if text:
        assert text in mpi.error_string(rc), mpi.error_string(rc)


def _validated(mpi, rc):
    """The call passed every argument check and was then refused as host memory."""
    _refused(mpi, rc, mpi.MPI_ERR_BUFFER, "device-resident")


# ---------------------------------------------------------------- argument checks
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_fetch", "MPIR_Hip_reduce_fetch", "MPIR_Hip_fetch_plan_info"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mpi_reduce_local.h")).read()
    assert "MPIX_Reduce_local_fetch(" in header


@pytest.mark.parametrize("op", ["MPI_OP_NULL", "BAD_KIND", "BAD_MPI_KIND", "INDEX_0", "INDEX_15"])
def test_null_and_invalid_ops(mpi, op):
    handle = {"MPI_OP_NULL": mpi.MPI_OP_NULL, "BAD_KIND": 0x18000003, "BAD_MPI_KIND": 0x44000003,
              "INDEX_0": 0x58000000, "INDEX_15": 0x5800000F}[op]
    h = Host()
    _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 4, mpi.MPI_FLOAT, handle), mpi.MPI_ERR_OP)
    assert h.untouched()


def test_user_op_is_not_predefined(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    try:
        h = Host()
        _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 4, mpi.MPI_FLOAT, op.value), mpi.MPI_ERR_OP, "predefined")
        assert h.untouched()
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0
    # the freed handle is invalid
    _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 4, mpi.MPI_FLOAT, op.value), mpi.MPI_ERR_OP)


def test_land_and_lor_on_floats_and_a_refused_type(mpi):
    h = Host()
    for op in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 2, dt, op), mpi.MPI_ERR_OP, "not defined for this datatype")
    # MPI_Reduce_local's datatype check: the same class as the single call's
    rc = mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 2, mpi.MPI_FLOAT, mpi.MPI_BAND)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local(h.pb, h.pa, 2, mpi.MPI_FLOAT, mpi.MPI_BAND)) == mpi.MPI_ERR_OP
    rc = mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 2, mpi.MPI_DATATYPE_NULL, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.error_class(mpi.reduce_local(h.pb, h.pa, 2, mpi.MPI_DATATYPE_NULL, mpi.MPI_SUM))
    assert h.untouched()


@pytest.mark.parametrize("op", ["MPI_NO_OP", "MPI_REPLACE"])
def test_copy_ops_accepted_on_basic_types_only(mpi, op):
    o = getattr(mpi, op)
    h = Host()
    # refused by every other entry point
    _refused(mpi, mpi.reduce_local(h.pb, h.pa, 4, mpi.MPI_FLOAT, o), mpi.MPI_ERR_OP)
    # every basic type of the table, and a builtin one outside it (MPI_WCHAR, by its handle's size)
    for t in ("MPI_FLOAT", "MPI_UNSIGNED_CHAR", "MPI_LONG_DOUBLE", "MPI_LONG_DOUBLE_INT", "MPI_C_LONG_DOUBLE_COMPLEX",
              "MPI_SHORT_INT", "MPI_WCHAR"):
        _validated(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 2, mpi.DATATYPES[t], o))
    # derived handles (direct and indirect kind), a builtin-kind handle of another object class, the null handle
    for dt in (0x8C010005, 0xCC000000, 0x48000406, mpi.MPI_DATATYPE_NULL):
        _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 2, dt, o), mpi.MPI_ERR_TYPE, "derived")
    assert h.untouched()


def test_negative_count(mpi):
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, h.pf, -1, mpi.MPI_FLOAT, op), mpi.MPI_ERR_COUNT)
    assert h.untouched()


def test_count_zero_succeeds_without_touching_a_pointer(mpi):
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        for pin, pio, pf in ((WILD, WILD + 4, WILD + 8), (WILD, WILD, WILD), (0, 0, 0),
                             (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
            assert mpi.reduce_local_fetch(pin, pio, pf, 0, mpi.MPI_FLOAT, op) == 0, (op, pin)
    # ... but the op and the datatype still are
    _refused(mpi, mpi.reduce_local_fetch(WILD, WILD + 4, WILD + 8, 0, mpi.MPI_FLOAT, mpi.MPI_OP_NULL), mpi.MPI_ERR_OP)
    _refused(mpi, mpi.reduce_local_fetch(WILD, WILD + 4, WILD + 8, 0, mpi.MPI_FLOAT, mpi.MPI_LAND), mpi.MPI_ERR_OP)


def test_in_place_in_each_position(mpi):
    h = Host()
    ip = mpi.MPI_IN_PLACE
    for args, name in (((ip, h.pa, h.pf), "inbuf"), ((h.pb, ip, h.pf), "inoutbuf"), ((h.pb, h.pa, ip), "fetchbuf")):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            rc = mpi.reduce_local_fetch(*args, 4, mpi.MPI_FLOAT, op)
            _refused(mpi, rc, mpi.MPI_ERR_BUFFER, f"'{name}' cannot be MPI_IN_PLACE")
    # MPI_NO_OP never looks at inbuf; the other two positions are refused
    _validated(mpi, mpi.reduce_local_fetch(ip, h.pa, h.pf, 4, mpi.MPI_FLOAT, mpi.MPI_NO_OP))
    _refused(mpi, mpi.reduce_local_fetch(h.pb, ip, h.pf, 4, mpi.MPI_FLOAT, mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, ip, 4, mpi.MPI_FLOAT, mpi.MPI_NO_OP), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    assert h.untouched()


def test_null_fetchbuf(mpi):
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        _refused(mpi, mpi.reduce_local_fetch(h.pb, h.pa, 0, 4, mpi.MPI_FLOAT, op), mpi.MPI_ERR_BUFFER, "fetchbuf")
    assert h.untouched()


def test_aliased_operands_with_the_check_on(mpi):
    assert os.environ.get("MPIR_CVAR_COLL_ALIAS_CHECK", "1") != "0"
    h = Host()
    for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
        _refused(mpi, mpi.reduce_local_fetch(h.pa, h.pa, h.pf, 4, mpi.MPI_FLOAT, op), mpi.MPI_ERR_BUFFER, "aliased")
    # MPI_NO_OP never looks at inbuf
    _validated(mpi, mpi.reduce_local_fetch(h.pa, h.pa, h.pf, 4, mpi.MPI_FLOAT, mpi.MPI_NO_OP))
    assert h.untouched()


_ALIAS_OFF = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import mpich_pip_amd as m
lib = m.load()
assert lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN) == 0
a = np.full(64, 2, np.float32)
f = np.full(64, 3, np.float32)
rc = m.reduce_local_fetch(a.ctypes.data, a.ctypes.data, f.ctypes.data, 4, m.MPI_FLOAT, m.MPI_SUM)
assert m.error_class(rc) == m.MPI_ERR_BUFFER, m.error_string(rc)
assert "device-resident" in m.error_string(rc) and "aliased" not in m.error_string(rc), m.error_string(rc)
# the overlap of fetchbuf is checked whatever the alias check says
rc = m.reduce_local_fetch(a.ctypes.data + 64, a.ctypes.data, a.ctypes.data + 8, 4, m.MPI_FLOAT, m.MPI_SUM)
assert m.error_class(rc) == m.MPI_ERR_BUFFER and "fetchbuf overlaps inoutbuf" in m.error_string(rc), m.error_string(rc)
assert (a == 2).all() and (f == 3).all()
print("alias-off ok")
"""


def test_aliased_operands_with_the_check_off():
    """MPIR_CVAR_COLL_ALIAS_CHECK=0 is read once per process: a fresh one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPIR_CVAR_COLL_ALIAS_CHECK="0")
    r = subprocess.run([sys.executable, "-c", _ALIAS_OFF.format(paths=[os.path.join(root, "mpich-pip_amd"), root])],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "alias-off ok" in r.stdout, r.stdout + r.stderr


def test_fetchbuf_overlap(mpi):
    buf = np.full(1024, 7, np.uint8)
    p = buf.ctypes.data + 256
    n, nb = 16, 64                                  # 16 floats
    F = mpi.MPI_FLOAT
    # inoutbuf at p, inbuf far from it; fetchbuf one byte into inoutbuf at either end
    for pf in (p + nb - 1, p - nb + 1, p, p + 4):
        for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
            _refused(mpi, mpi.reduce_local_fetch(p + 512, p, pf, n, F, op), mpi.MPI_ERR_BUFFER, "fetchbuf overlaps inoutbuf")
    # touching is not overlapping
    for pf in (p + nb, p - nb):
        _validated(mpi, mpi.reduce_local_fetch(p + 512, p, pf, n, F, mpi.MPI_SUM))
    # fetchbuf over inbuf: refused, but under MPI_NO_OP, which never looks at inbuf
    for pf in (p + 512 + nb - 1, p + 512 - nb + 1, p + 512):
        for op in (mpi.MPI_SUM, mpi.MPI_REPLACE):
            _refused(mpi, mpi.reduce_local_fetch(p + 512, p, pf, n, F, op), mpi.MPI_ERR_BUFFER, "fetchbuf overlaps inbuf")
        _validated(mpi, mpi.reduce_local_fetch(p + 512, p, pf, n, F, mpi.MPI_NO_OP))
    # the ranges are the datatype's: 16 doubles reach twice as far
    _refused(mpi, mpi.reduce_local_fetch(p + 512, p, p + 2 * nb - 1, n, mpi.MPI_DOUBLE, mpi.MPI_SUM), mpi.MPI_ERR_BUFFER,
             "overlaps")
    assert (buf == 7).all()


def test_no_op_with_null_inbuf_passes_validation(mpi):
    h = Host()
    _validated(mpi, mpi.reduce_local_fetch(0, h.pa, h.pf, 4, mpi.MPI_FLOAT, mpi.MPI_NO_OP))
    assert h.untouched()


@pytest.mark.parametrize("op", ["MPI_SUM", "MPI_NO_OP", "MPI_REPLACE"])
def test_host_pointers_refused_as_non_device(mpi, op):
    h = Host(4096)
    rc = mpi.reduce_local_fetch(h.pb, h.pa, h.pf, 4096, mpi.MPI_FLOAT, getattr(mpi, op))
    _validated(mpi, rc)
    assert h.untouched()
    # the shim answers the same on its own
    lib = mpi.load()
    assert lib.MPIR_Hip_reduce_fetch(h.pb, h.pa, h.pf, 4096, getattr(mpi, op) & 0xF, mpi.ELEM["F32"], None, 1) == 1
    assert h.untouched()


def test_shim_refuses_unknown_pairs(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 4)()
    f32 = mpi.ELEM["F32"]

    def info(op, elem, count=4):
        return lib.MPIR_Hip_fetch_plan_info(BASE, FAR, FETCH, count, op, elem, out)

    assert info(mpi.MPI_SUM & 0xF, f32) == 0
    assert info(mpi.MPI_BAND & 0xF, f32) == ENOKERNEL            # no BAND on floats
    assert info(mpi.MPI_MAXLOC & 0xF, f32) == ENOKERNEL
    assert info(0, f32) == ENOKERNEL and info(15, f32) == ENOKERNEL and info(mpi.MPI_SUM & 0xF, 99) == ENOKERNEL
    assert info(mpi.MPI_NO_OP & 0xF, 99) == ENOKERNEL and info(mpi.MPI_REPLACE & 0xF, 0) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_fetch(BASE, FAR, FETCH, 4, mpi.MPI_BAND & 0xF, f32, None, 1) == ENOKERNEL
    with pytest.raises(LookupError):
        mpi.fetch_plan_info(BASE, FAR, FETCH, 4, mpi.MPI_FLOAT, mpi.MPI_BAND)


# ---------------------------------------------------------------- the planner
def test_empty_and_copy(mpi):
    for op in (mpi.MPI_SUM, mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        assert mpi.fetch_plan_info(WILD, WILD, WILD, 0, mpi.MPI_FLOAT, op) == dict(path=EMPTY, groups=0, nhead=0, ntail=0)
    for op in (mpi.MPI_NO_OP, mpi.MPI_REPLACE):
        for t in ("MPI_FLOAT", "MPI_UNSIGNED_CHAR", "MPI_LONG_DOUBLE", "MPI_LONG_DOUBLE_INT"):
            for pin, pio, pf in ((BASE, FAR, FETCH), (BASE + 3, FAR + 1, FETCH + 7), (0, FAR, FETCH)):
                info = mpi.fetch_plan_info(pin, pio, pf, 100003, mpi.DATATYPES[t], op)
                assert info == dict(path=COPY, groups=0, nhead=0, ntail=0), (op, t, info)


@pytest.mark.parametrize("op,t", [("MPI_SUM", "MPI_FLOAT"), ("MPI_BXOR", "MPI_UNSIGNED_CHAR"), ("MPI_SUM", "MPIX_C_FLOAT16"),
                                  ("MPI_MAX", "MPI_DOUBLE"), ("MPI_MINLOC", "MPI_SHORT_INT"),
                                  ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX"), ("MPI_SUM", "MPI_LONG_DOUBLE")],
                         ids=["f32", "u8", "f16", "f64", "short_int", "cf64", "x80"])
def test_tile_path_exactly_when_aligned_and_congruent(mpi, op, t):
    """inoutbuf at phases 0..15, the other two pointers at every residue mod 16:
    TILE exactly when all three are naturally aligned (a multiple of the element's
    size off the 16-byte grid) and congruent mod 16.  A TILE plan's grid is the
    batch's for the segment (in, io, count), its head and tail the single call's;
    an ELEMS plan's grid is the count over the elements a workgroup owns."""
    esz = T.elem_size(t)
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    tiles = 0
    for count in (2 * TILE // esz + 7, 3):
        for pio in range(16):
            ao = FAR + TILE - 32 + pio          # tile 0 cut 32 bytes before a grid line
            for rin in range(16):
                for rf in range(16):
                    ai, af = BASE + 4096 + rin, FETCH + 8192 + rf
                    info = mpi.fetch_plan_info(ai, ao, af, count, dt, o)
                    want_tile = pio % esz == 0 and rin == pio and rf == pio
                    what = f"{t} count {count} in +{rin} io +{pio} fetch +{rf}: {info}"
                    assert info["path"] == (TILEP if want_tile else ELEMS), what
                    if not want_tile:
                        assert (info["groups"], info["nhead"], info["ntail"]) == (-(-count * esz // TILE), 0, 0), what
                        continue
                    tiles += 1
                    batch = mpi.batch_plan_info([(ai, ao, count), (ai, ao, count)], dt, o)
                    assert batch["seg_kind"] == [BATCH_TILE, BATCH_TILE], what
                    assert info["groups"] == batch["seg_groups"][0], (what, batch)
                    single = mpi.plan_info(ai, ao, count, dt, o)
                    assert (info["nhead"], info["ntail"]) == (single["nhead"], single["ntail"]), (what, single)
    assert tiles == 2 * 16 // esz


def test_tile_grid_follows_inoutbufs_address(mpi):
    """On the grid one workgroup per 16 KiB; 8 KiB off it tile 0 is cut and there
    is one more, wherever the other two buffers sit on their own grids."""
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    n = 2 * TILE // 4
    for off, want in ((0, 2), (8192, 3), (16, 3), (TILE - 16, 3)):
        for oin, ofe in ((0, 0), (4096, 0), (0, 4096 + 16 * 5)):
            info = mpi.fetch_plan_info(BASE + oin, FAR + off, FETCH + ofe, n, dt, o)
            assert info == dict(path=TILEP, groups=want, nhead=0, ntail=0), (off, oin, ofe, info)
    assert mpi.fetch_plan_info(BASE, FAR, FETCH, n + 4, dt, o)["groups"] == 3
    assert mpi.fetch_plan_info(BASE + 4, FAR + 4, FETCH + 4, 1, dt, o) == dict(path=TILEP, groups=1, nhead=1, ntail=0)
    # the largest count the public entry point takes stays one launch
    big = mpi.fetch_plan_info(BASE + 4, FAR + 4, FETCH + 4, 2 ** 31 - 1, mpi.DATATYPES["MPI_C_DOUBLE_COMPLEX"],
                              mpi.MPI_SUM)
    assert big["path"] == ELEMS and big["groups"] <= mpi.BATCH_MAX_GROUPS
    big = mpi.fetch_plan_info(BASE + 16, FAR + 16, FETCH + 16, 2 ** 31 - 1, mpi.DATATYPES["MPI_C_DOUBLE_COMPLEX"],
                              mpi.MPI_SUM)
    assert big["path"] == TILEP and big["groups"] == 2 ** 21 <= mpi.BATCH_MAX_GROUPS
    big = mpi.fetch_plan_info(BASE + 8192, FAR + 8192, FETCH + 8192, 2 ** 31 - 1, mpi.DATATYPES["MPI_C_DOUBLE_COMPLEX"],
                              mpi.MPI_SUM)
    assert big["path"] == TILEP and big["groups"] == 2 ** 21 + 1 <= mpi.BATCH_MAX_GROUPS


@pytest.mark.parametrize("op,t", [("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT"), ("MPI_SUM", "MPI_C_LONG_DOUBLE_COMPLEX")])
def test_32_byte_classes_are_always_elems(mpi, op, t):
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    for count in (1, 512, 513, 700, 2 ** 31 - 1):
        for pin, pio, pf in ((0, 0, 0), (16, 16, 16), (0, 16, 0), (8, 8, 8), (1, 2, 3)):
            info = mpi.fetch_plan_info(BASE + pin, FAR + pio, FETCH + pf, count, dt, o)
            assert info == dict(path=ELEMS, groups=-(-count // 512), nhead=0, ntail=0), (count, pin, pio, pf, info)
            assert info["groups"] <= mpi.BATCH_MAX_GROUPS
