"""MPIX_Compare_and_swap_indexed_ordered without a GPU: its argument checks
through the C ABI on host buffers (which a sound call is then refused for as
non-device memory, so a check that comes earlier shows by its class and text),
the accepted datatypes against a list written out here from the reference, and
its launch planner (MPIR_Hip_cas_plan_info) on made-up addresses.

(Host tables, a result inside the targets' span and the order-less promise need
device operands to get that far: test_cas_gpu.py.)
"""
import ctypes
import os

import numpy as np
import pytest

ORIGIN = 1 << 32             # made-up arenas, 16 KiB aligned
COMPARE = 1 << 33
TARGET = 1 << 40
RESULT = 1 << 41
TAB, TAB_ORD = (1 << 44) + (1 << 30), (1 << 44) + (1 << 31)
WILD = 0x10                  # an address that would fault if touched
TILE = 16384
EMPTY, CONTIG_TILE, CONTIG_ELEMS, INDEXED = range(4)
EBUFFER, ENOKERNEL, EARG = 1, 3, 5
NAMES = ("MPIX_Compare_and_swap_indexed_ordered", "MPIR_Hip_cas_indexed_ordered", "MPIR_Hip_cas_plan_info")

# MPIR_Type_is_rma_atomic, src/mpi/rma/rmatypeutil.c:23-43, for a build with no
# Fortran and no C++ (MPIR_Compare_equal, :53-76, compares each of them with ==
# on its C type: the element's bytes)
ATOMIC = (
    # MPIR_OP_TYPE_GROUP_C_INTEGER, src/include/mpir_op_util.h:263-281
    "MPI_INT", "MPI_LONG", "MPI_SHORT", "MPI_UNSIGNED_SHORT", "MPI_UNSIGNED", "MPI_UNSIGNED_LONG", "MPI_LONG_LONG",
    "MPI_UNSIGNED_LONG_LONG", "MPI_SIGNED_CHAR", "MPI_UNSIGNED_CHAR", "MPI_INT8_T", "MPI_INT16_T", "MPI_INT32_T",
    "MPI_INT64_T", "MPI_UINT8_T", "MPI_UINT16_T", "MPI_UINT32_T", "MPI_UINT64_T",
    # MPIR_OP_TYPE_GROUP_C_INTEGER_EXTRA, :284-285
    "MPI_CHAR",
    # MPIR_OP_TYPE_GROUP_FORTRAN_INTEGER without Fortran, :288-292
    "MPI_AINT", "MPI_OFFSET", "MPI_COUNT",
    # MPIR_OP_TYPE_GROUP_LOGICAL without Fortran and C++, :323-326
    "MPI_C_BOOL",
    # MPIR_OP_TYPE_GROUP_BYTE, :344-345
    "MPI_BYTE",
)
SIZE = {"MPI_INT": 4, "MPI_LONG": 8, "MPI_SHORT": 2, "MPI_UNSIGNED_SHORT": 2, "MPI_UNSIGNED": 4, "MPI_UNSIGNED_LONG": 8,
        "MPI_LONG_LONG": 8, "MPI_UNSIGNED_LONG_LONG": 8, "MPI_SIGNED_CHAR": 1, "MPI_UNSIGNED_CHAR": 1, "MPI_INT8_T": 1,
        "MPI_INT16_T": 2, "MPI_INT32_T": 4, "MPI_INT64_T": 8, "MPI_UINT8_T": 1, "MPI_UINT16_T": 2, "MPI_UINT32_T": 4,
        "MPI_UINT64_T": 8, "MPI_CHAR": 1, "MPI_AINT": 8, "MPI_OFFSET": 8, "MPI_COUNT": 8, "MPI_C_BOOL": 1, "MPI_BYTE": 1}


class Host:
    """Four host arrays (origin = 1, compare = 2, target = 2, result = 3, ints: every
    compare would succeed), a host table with repeats and its order, and a check
    that a refused call left all of them alone."""

    def __init__(self, n=64, count=8):
        self.o = np.full(n, 1, np.int32)
        self.c = np.full(n, 2, np.int32)
        self.t = np.full(n, 2, np.int32)
        self.r = np.full(n, 3, np.int32)
        self.po, self.pc, self.pt, self.pr = (x.ctypes.data for x in (self.o, self.c, self.t, self.r))
        self.count = count
        self.tab = (np.arange(count, dtype=np.int64) % 3)
        self.order = np.argsort(self.tab, kind="stable").astype(np.int32)
        self.tab0, self.order0 = self.tab.copy(), self.order.copy()

    def untouched(self):
        return ((self.o == 1).all() and (self.c == 2).all() and (self.t == 2).all() and (self.r == 3).all() and
                np.array_equal(self.tab, self.tab0) and np.array_equal(self.order, self.order0))


def _call(mpi, h, po="o", pc="c", pt="t", pr="r", count=None, unit=4, dt=None, tab="t", order="o", stream=0):
    return mpi.compare_and_swap_indexed_ordered(
        h.po if po == "o" else po, h.pc if pc == "c" else pc, h.pt if pt == "t" else pt,
        h.tab if isinstance(tab, str) else tab, h.pr if pr == "r" else pr, h.order if isinstance(order, str) else order,
        unit, h.count if count is None else count, mpi.MPI_INT if dt is None else dt, stream)


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
    assert callable(mpi.compare_and_swap_indexed_ordered) and callable(mpi.cas_plan_info)
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    assert "MPIX_Compare_and_swap_indexed_ordered(" in open(os.path.join(inc, "mpi_reduce_local.h")).read()
    shim = open(os.path.join(inc, "mpir_hip_reduce.h")).read()
    assert "MPIR_Hip_cas_indexed_ordered(" in shim and "MPIR_Hip_cas_plan_info(" in shim


def test_every_datatype_is_accepted_exactly_when_the_reference_calls_it_atomic(mpi):
    assert len(set(ATOMIC)) == len(ATOMIC) == 24 and set(ATOMIC) <= set(mpi.DATATYPES)
    h = Host()
    for name, dt in mpi.DATATYPES.items():
        rc = _call(mpi, h, dt=dt, count=2, unit=8)
        if name in ATOMIC:
            _validated(mpi, rc)
            assert mpi.load().MPIR_Hip_elem_size(mpi.ELEM[mpi.ELEM_OF[name]]) == SIZE[name], name
        else:
            _refused(mpi, rc, mpi.MPI_ERR_TYPE, "not permitted for atomic operations")
    for name in ("MPI_WCHAR", "MPI_FLOAT", "MPI_DOUBLE", "MPI_LONG_DOUBLE", "MPIX_C_FLOAT16", "MPI_C_FLOAT_COMPLEX",
                 "MPI_C_DOUBLE_COMPLEX", "MPI_C_LONG_DOUBLE_COMPLEX", "MPI_2INT", "MPI_LONG_DOUBLE_INT"):
        assert name in mpi.DATATYPES and name not in ATOMIC
    # null and invalid handles, a derived-kind handle
    _refused(mpi, _call(mpi, h, dt=mpi.MPI_DATATYPE_NULL), mpi.MPI_ERR_TYPE, "Null datatype")
    for dt in (0, 0x8C010005, 0xCC000000, 0x4C0004FF, 0x58000003):
        _refused(mpi, _call(mpi, h, dt=dt), mpi.MPI_ERR_TYPE)
    # MPI_PACKED: a valid builtin handle this library has no descriptor for
    _refused(mpi, _call(mpi, h, dt=0x4C00010F), mpi.MPI_ERR_TYPE, "not permitted for atomic operations")
    assert h.untouched()


def test_negative_count_comes_first(mpi):
    h = Host()
    for count in (-1, -300):
        _refused(mpi, _call(mpi, h, count=count), mpi.MPI_ERR_COUNT, "negative count")
        _refused(mpi, _call(mpi, h, count=count, dt=mpi.MPI_FLOAT, unit=0), mpi.MPI_ERR_COUNT)   # before type and unit
    assert h.untouched()


def test_zero_count_succeeds_without_touching_a_pointer_or_a_table(mpi):
    ip = mpi.MPI_IN_PLACE
    call = mpi.compare_and_swap_indexed_ordered
    for name in ATOMIC:
        dt = mpi.DATATYPES[name]
        for ptrs in ((WILD, WILD + 8, WILD + 16, WILD + 24), (WILD,) * 4, (0,) * 4, (ip,) * 4):
            for tab, od in ((WILD, WILD), (0, WILD), (WILD, 0), (0, 0)):
                for stream in (0, WILD):
                    assert call(ptrs[0], ptrs[1], ptrs[2], tab, ptrs[3], od, 4, 0, dt, stream) == 0, (name, ptrs, tab, od)
    # ... but the type and disp_unit still are, in that order
    _refused(mpi, call(WILD, WILD, WILD, WILD, WILD, WILD, 4, 0, mpi.MPI_FLOAT), mpi.MPI_ERR_TYPE, "MPI_FLOAT")
    _refused(mpi, call(WILD, WILD, WILD, WILD, WILD, WILD, 0, 0, mpi.MPI_FLOAT), mpi.MPI_ERR_TYPE, "atomic")
    for unit in (0, -1, -16):
        _refused(mpi, call(WILD, WILD, WILD, WILD, WILD, WILD, unit, 0, mpi.MPI_INT), mpi.MPI_ERR_ARG, "disp_unit")
    with pytest.raises(ValueError):
        mpi.cas_plan_info(WILD, WILD, WILD, WILD, WILD, WILD, 0, 0, mpi.MPI_INT)
    info = mpi.cas_plan_info(WILD, WILD, WILD, WILD, WILD, WILD, 4, 0, mpi.MPI_INT)
    assert info["form"] == EMPTY and info["launches"] == 0 and info["groups"] == 0, info


def test_null_in_place_alias_order_and_overlap_in_that_order(mpi):
    h = Host()
    ip = mpi.MPI_IN_PLACE
    # 3. disp_unit before the pointers
    _refused(mpi, _call(mpi, h, po=0, unit=0), mpi.MPI_ERR_ARG, "disp_unit")
    # 5. NULL origin, compare, result: MPI_ERR_ARG, before MPI_IN_PLACE
    for kw, name in ((dict(po=0), "origin"), (dict(pc=0), "compare"), (dict(pr=0), "result")):
        _refused(mpi, _call(mpi, h, **kw), mpi.MPI_ERR_ARG, f"Null pointer in parameter {name}")
        _refused(mpi, _call(mpi, h, pt=ip, **kw), mpi.MPI_ERR_ARG, "Null pointer")
    # 6. MPI_IN_PLACE in each of the four positions, before the alias check and the order rule
    for kw, name in ((dict(po=ip), "origin"), (dict(pc=ip), "compare"), (dict(pt=ip), "target"), (dict(pr=ip), "result")):
        _refused(mpi, _call(mpi, h, **kw), mpi.MPI_ERR_BUFFER, f"'{name}' cannot be MPI_IN_PLACE")
        _refused(mpi, _call(mpi, h, tab=None, **kw), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    # 7. the alias check, before the order rule
    assert os.environ.get("MPIR_CVAR_COLL_ALIAS_CHECK", "1") != "0"
    _refused(mpi, _call(mpi, h, po=h.pt), mpi.MPI_ERR_BUFFER, "aliased")
    _refused(mpi, _call(mpi, h, pc=h.pt), mpi.MPI_ERR_BUFFER, "aliased")
    _refused(mpi, _call(mpi, h, pc=h.pt, tab=None), mpi.MPI_ERR_BUFFER, "aliased")
    # 8. order without target_displs, before the overlap rule
    _refused(mpi, _call(mpi, h, tab=None), mpi.MPI_ERR_ARG, "order table with no target_displs")
    _refused(mpi, _call(mpi, h, tab=None, pr=h.po), mpi.MPI_ERR_ARG, "order table with no target_displs")
    # 9. result's packed range over origin's, compare's, a contiguous target's
    nbytes = h.count * 4
    for d in (0, 4, nbytes - 1, 1 - nbytes):
        _refused(mpi, _call(mpi, h, pr=h.po + d), mpi.MPI_ERR_BUFFER, "result overlaps origin")
        _refused(mpi, _call(mpi, h, pr=h.pc + d), mpi.MPI_ERR_BUFFER, "result overlaps compare")
        _refused(mpi, _call(mpi, h, pr=h.pt + d, tab=None, order=None), mpi.MPI_ERR_BUFFER, "result overlaps target")
        # ... a target with a table is no range the library can see from here
        _validated(mpi, _call(mpi, h, pr=h.pt + d))
    buf = np.full(4096, 7, np.uint8)
    p = buf.ctypes.data + 256
    for d in (nbytes, -nbytes):
        _validated(mpi, _call(mpi, h, po=p + 1024, pr=p + 1024 + d))        # touching is not overlapping
    # origin and compare are only read: equal or overlapping is fine
    _validated(mpi, _call(mpi, h, pc=h.po))
    _validated(mpi, _call(mpi, h, pc=h.po + 4))
    # a sound call every way
    _validated(mpi, _call(mpi, h))
    _validated(mpi, _call(mpi, h, order=None))
    _validated(mpi, _call(mpi, h, tab=None, order=None))
    _validated(mpi, _call(mpi, h, stream=WILD))
    assert (buf == 7).all() and h.untouched()


def test_shim_answers_alike(mpi):
    lib = mpi.load()
    out = (ctypes.c_uint64 * 8)()
    i32 = mpi.ELEM["I32"]

    def info(elem, unit=4, count=8, tab=TAB, od=TAB_ORD):
        return lib.MPIR_Hip_cas_plan_info(ORIGIN, COMPARE, TARGET, tab, RESULT, od, unit, count, elem, out)

    assert info(0) == ENOKERNEL and info(99) == ENOKERNEL
    assert info(i32) == 0 and out[0] == INDEXED
    assert info(i32, unit=0) == EARG and info(i32, unit=0, count=0) == EARG
    assert info(i32, tab=None) == EARG                          # an order and a contiguous target
    assert info(i32, tab=None, od=None) == 0 and out[0] == CONTIG_TILE
    assert info(i32, od=None) == 0 and out[0] == INDEXED        # order NULL: the identity, the same plan
    assert info(i32, count=(1 << 31)) == EARG and info(i32, count=(1 << 31) - 1) == 0
    # a kernel exactly for the element classes of 1, 2, 4 and 8 bytes
    for elem in range(64):
        size = lib.MPIR_Hip_elem_size(elem)
        assert info(elem) == (0 if size in (1, 2, 4, 8) else ENOKERNEL), (elem, size)
    h = Host()
    assert lib.MPIR_Hip_cas_indexed_ordered(h.po, h.pc, h.pt, h.tab.ctypes.data, h.pr, h.order.ctypes.data, 4, h.count,
                                            i32, None, 1) == EBUFFER
    assert lib.MPIR_Hip_cas_indexed_ordered(WILD, WILD, WILD, WILD, WILD, WILD, 1, 0, i32, None, 1) == 0
    assert h.untouched()


@pytest.mark.parametrize("t", ["MPI_SIGNED_CHAR", "MPI_SHORT", "MPI_INT", "MPI_LONG", "MPI_BYTE", "MPI_C_BOOL"])
def test_contiguous_plan_over_the_four_pointers_phases(mpi, t):
    """The tile form exactly where origin, compare and result share the target's
    offset mod 16 and the target is naturally aligned; its grid is the fetch
    call's for the same target address and byte count."""
    dt, n = mpi.DATATYPES[t], SIZE[t]
    fetch_dt = {1: mpi.MPI_SIGNED_CHAR, 2: mpi.MPI_SHORT, 4: mpi.MPI_INT, 8: mpi.MPI_LONG}[n]
    count = (2 * TILE + 3 * 16) // n + 1
    seen = set()
    phases = sorted({0, n, 8, 16 - n, 16, TILE - 16, 1, 3} if n > 1 else {0, 1, 7, 15, 16, TILE - 1})
    for pt in phases:
        for po in (pt, pt + 16, pt + n, (pt + 8) % 16):
            for pc in (pt, pt + 32, (pt + n) % 16):
                for pr in (pt, pt + 48, (pt + 4) % 16 if n < 16 else pt):
                    info = mpi.cas_plan_info(ORIGIN + po, COMPARE + pc, TARGET + pt, None, RESULT + pr, None, n, count, dt)
                    tile = pt % n == 0 and all((p - pt) % 16 == 0 for p in (po, pc, pr))
                    assert info["form"] == (CONTIG_TILE if tile else CONTIG_ELEMS), (pt, po, pc, pr, info)
                    assert info["launches"] == 1 and info["ahead"] >= 1
                    seen.add(info["form"])
                    if tile:
                        f = mpi.fetch_plan_info(ORIGIN + pt, TARGET + pt, RESULT + pt, count, fetch_dt, mpi.MPI_BXOR)
                        assert f["path"] == mpi.FETCH_NAMES.index("tile")
                        assert (info["groups"], info["nhead"], info["ntail"]) == (f["groups"], f["nhead"], f["ntail"]), (info, f)
                        head = (-pt % 16) // n
                        assert info["nhead"] == head and info["ntail"] == (count - head) * n % 16 // n
                    else:
                        assert info["groups"] == -(-count * n // TILE) and info["per"] == TILE // n, info
                        assert info["nhead"] == info["ntail"] == 0
    assert seen == {CONTIG_TILE, CONTIG_ELEMS}


def test_indexed_plan_groups_and_launches_also_at_a_lowered_cap(mpi):
    lib = mpi.load()
    dt = mpi.MPI_LONG
    a = mpi.cas_plan_info(ORIGIN, COMPARE, TARGET, TAB, RESULT, TAB_ORD, 8, 1, dt)
    per, ahead = a["per"], a["ahead"]
    assert per >= 256 and per % 256 == 0 and ahead >= 1
    for count in (1, per - 1, per, per + 1, 7 * per + 5, 65536, (1 << 31) - 1):
        for od in (TAB_ORD, None):
            info = mpi.cas_plan_info(ORIGIN + 1, COMPARE + 3, TARGET + 5, TAB, RESULT + 7, od, 1, count, dt)
            assert info == dict(form=INDEXED, launches=1, groups=-(-count // per), rows_per_launch=count, per=per,
                                ahead=ahead, nhead=0, ntail=0), info
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        for count in (1, 3 * per, 3 * per + 1, 7 * per + 5, 9 * per):
            info = mpi.cas_plan_info(ORIGIN, COMPARE, TARGET, TAB, RESULT, TAB_ORD, 8, count, dt)
            rpl = min(count, 3 * per)
            assert info["rows_per_launch"] == rpl and info["launches"] == -(-count // rpl), info
            assert info["groups"] == -(-count // per), info        # a full launch is whole workgroups
        # the contiguous form is one launch whatever the cap
        info = mpi.cas_plan_info(ORIGIN, COMPARE, TARGET, None, RESULT, None, 8, 16 * TILE, dt)
        assert info["form"] == CONTIG_TILE and info["launches"] == 1 and info["groups"] == 128, info
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3
