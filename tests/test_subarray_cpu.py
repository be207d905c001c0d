"""MPIX_Reduce_local_subarray without a GPU: its argument checks through the C
ABI in the order the header states them, and its planner
(MPIR_Hip_subarray_plan_info: the normal form and the launches the call itself
computes, host arithmetic on the arguments) on made-up addresses.

What the planner must get right is what the kernel relies on: the box brought to
a row of contiguous elements under k outer dimensions, each a count and one byte
stride per side; a box of no outer dimension handed to the single call and one of
a single outer dimension to the strided call with exactly the five numbers that
describe it; for more, the strided call's forms, threshold, G and launch split.
A Python model of the normal form and of the kernel's row addressing is held to
numpy's own indexing of the box; the GPU tests rely on that arithmetic.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

TILE = 16384
BASE = 1 << 32               # inbuf's arena
FAR = 1 << 40                # inoutbuf's arena, far from inbuf's
ENOKERNEL, EARG = 3, 5
SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS, STRIDED = range(1, 6)
C, F = 56, 57


def _host(n=4096):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def _plan(mpi, sub, isz=None, ist=None, osz=None, ost=None, order=C, t="MPI_FLOAT", op="MPI_SUM", ai=BASE, ao=FAR):
    return mpi.subarray_plan_info(ai, isz, ist, ao, osz, ost, sub, order, mpi.DATATYPES[t], mpi.OPS[op])


def _call(mpi, pin, pio, sub, isz=None, ist=None, osz=None, ost=None, order=C, dt=None, op=None, ndims=None):
    return mpi.reduce_local_subarray(pin, isz, ist, pio, osz, ost, sub, order, mpi.MPI_FLOAT if dt is None else dt,
                                     mpi.MPI_SUM if op is None else op, ndims=ndims)


def _refused(mpi, rc, cls, text=None):
    assert mpi.error_class(rc) == cls, mpi.error_string(rc)
    if text:
        assert text in mpi.error_string(rc), mpi.error_string(rc)


# ---------------------------------------------------------------- exports and header
def test_exported_and_declared(mpi):
    lib = mpi.load()
    for name in ("MPIX_Reduce_local_subarray", "MPIR_Hip_reduce_subarray", "MPIR_Hip_subarray_plan_info"):
        assert hasattr(lib, name) and name in mpi.EXPORTED_SYMBOLS, name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mpi_reduce_local.h")).read()
    assert "MPICH_API_PUBLIC int MPIX_Reduce_local_subarray(" in header
    for name, value in (("MPI_ERR_DIMS", 11), ("MPI_ORDER_C", 56), ("MPI_ORDER_FORTRAN", 57),
                        ("MPIX_REDUCE_LOCAL_SUBARRAY_MAXDIMS", 8)):
        line = [l for l in header.splitlines() if l.startswith(f"#define {name} ")]
        assert len(line) == 1 and int(line[0].split()[2]) == value, name
    assert (mpi.MPI_ERR_DIMS, mpi.MPI_ORDER_C, mpi.MPI_ORDER_FORTRAN, mpi.SUBARRAY_MAXDIMS) == (11, 56, 57, 8)


# ---------------------------------------------------------------- error classes, in order
GOOD = dict(sub=[2, 3], isz=[4, 5], ist=[1, 1], osz=[6, 7], ost=[2, 2])


def test_a_sound_call_reaches_residency(mpi):
    """Host operands pass every argument check and are then refused as not device memory."""
    a, b = _host()
    _refused(mpi, _call(mpi, b.ctypes.data, a.ctypes.data, **GOOD), mpi.MPI_ERR_BUFFER, "device-resident")
    _refused(mpi, _call(mpi, b.ctypes.data, a.ctypes.data, [2, 3]), mpi.MPI_ERR_BUFFER, "device-resident")   # both packed
    assert not a.any()


def test_ops_and_types_come_first(mpi):
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    for handle in (mpi.MPI_REPLACE, mpi.MPI_NO_OP, mpi.MPI_OP_NULL, 0x44000003):
        # ... ahead of a bad ndims, a null array, a bad dimension, MPI_IN_PLACE
        _refused(mpi, _call(mpi, pb, pa, op=handle, **GOOD), mpi.MPI_ERR_OP)
        _refused(mpi, _call(mpi, pb, pa, [2, 3], op=handle, ndims=0), mpi.MPI_ERR_OP)
        _refused(mpi, _call(mpi, mpi.MPI_IN_PLACE, pa, [0, 3], op=handle), mpi.MPI_ERR_OP)
    for op in (mpi.MPI_LAND, mpi.MPI_LOR):
        for dt in (mpi.MPI_FLOAT, mpi.MPI_DOUBLE):
            _refused(mpi, _call(mpi, pb, pa, [2, 3], dt=dt, op=op, ndims=99), mpi.MPI_ERR_OP, "not defined for this datatype")
    _refused(mpi, _call(mpi, pb, pa, [2, 3], op=mpi.MPI_BAND), mpi.MPI_ERR_OP)
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(x, y, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    try:
        _refused(mpi, _call(mpi, pb, pa, [2, 3], op=op.value, ndims=-1), mpi.MPI_ERR_OP, "user MPI_Op functions run on the host")
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0
    assert not a.any()


def test_ndims_null_arrays_and_order(mpi):
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    for nd in (0, -1, 9, 1 << 20):
        _refused(mpi, _call(mpi, pb, pa, [1] * 9, ndims=nd), mpi.MPI_ERR_DIMS)
        # ... ahead of a null array, a bad order and a bad dimension
        _refused(mpi, _call(mpi, pb, pa, None, ndims=nd), mpi.MPI_ERR_DIMS)
        _refused(mpi, _call(mpi, pb, pa, [0] * 9, order=3, ndims=nd), mpi.MPI_ERR_DIMS)
    assert mpi.error_class(_call(mpi, pb, pa, [1] * 8)) == mpi.MPI_ERR_BUFFER      # 8 dimensions pass
    _refused(mpi, _call(mpi, pb, pa, None, ndims=2), mpi.MPI_ERR_ARG, "subsizes")
    _refused(mpi, _call(mpi, pb, pa, [2, 3], isz=[4, 5]), mpi.MPI_ERR_ARG, "in_starts")
    _refused(mpi, _call(mpi, pb, pa, [2, 3], osz=[4, 5]), mpi.MPI_ERR_ARG, "inout_starts")
    # starts without sizes are not looked at: the side is packed
    assert mpi.error_class(_call(mpi, pb, pa, [2, 3], ist=[-7, -7], ost=[99, 99])) == mpi.MPI_ERR_BUFFER
    for order in (0, 1, 55, 58, -1):
        _refused(mpi, _call(mpi, pb, pa, order=order, **GOOD), mpi.MPI_ERR_ARG, "order")
        # ... ahead of a bad dimension and of MPI_IN_PLACE
        _refused(mpi, _call(mpi, mpi.MPI_IN_PLACE, pa, [0, 3], order=order), mpi.MPI_ERR_ARG, "order")
    # a null array ahead of the order
    _refused(mpi, _call(mpi, pb, pa, None, order=3, ndims=2), mpi.MPI_ERR_ARG, "subsizes")
    assert not a.any()


@pytest.mark.parametrize("side", ["in", "inout"])
def test_each_dimension_as_the_reference_checks_it(mpi, side):
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data

    def call(sub, sz, st, p_in=pb):
        kw = dict(isz=sz, ist=st) if side == "in" else dict(osz=sz, ost=st)
        return _call(mpi, p_in, pa, sub, **kw)

    for d in (0, 1, 2):
        for what, (sub_d, sz_d, st_d) in {"size": (1, 0, 0), "size-": (1, -4, 0), "subsize": (0, 4, 0), "subsize-": (-1, 4, 0),
                                          "start": (2, 4, -1), "subsize>": (5, 4, 0), "start>": (2, 4, 3)}.items():
            sub, sz, st = [2, 2, 2], [4, 4, 4], [1, 1, 1]
            sub[d], sz[d], st[d] = sub_d, sz_d, st_d
            _refused(mpi, call(sub, sz, st), mpi.MPI_ERR_ARG, f"dimension {d}")
            # ... ahead of MPI_IN_PLACE
            _refused(mpi, call(sub, sz, st, mpi.MPI_IN_PLACE), mpi.MPI_ERR_ARG, f"dimension {d}")
    # two faults: the lower dimension's is the one reported
    _refused(mpi, call([2, 9, 2], [0, 4, 4], [0, 0, 0]), mpi.MPI_ERR_ARG, "dimension 0")
    _refused(mpi, call([2, 2, 0], [4, 4, 4], [0, 3, 0]), mpi.MPI_ERR_ARG, "dimension 1")
    # the largest start that fits, and a box that is the whole array
    assert mpi.error_class(call([2, 2, 2], [4, 4, 4], [2, 2, 2])) == mpi.MPI_ERR_BUFFER
    assert mpi.error_class(call([4, 4, 4], [4, 4, 4], [0, 0, 0])) == mpi.MPI_ERR_BUFFER
    assert not a.any()


def test_an_empty_box_and_a_packed_side_with_a_zero_subsize(mpi):
    a, b = _host()
    _refused(mpi, _call(mpi, b.ctypes.data, a.ctypes.data, [2, 0]), mpi.MPI_ERR_ARG, "dimension 1")
    _refused(mpi, _call(mpi, b.ctypes.data, a.ctypes.data, [0]), mpi.MPI_ERR_ARG, "dimension 0")


def test_an_array_that_does_not_fit_an_aint(mpi):
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    big = (1 << 31) - 1
    # 2^93 floats; the box itself is small
    for kw in (dict(isz=[big] * 3, ist=[0] * 3), dict(osz=[big] * 3, ost=[0] * 3)):
        _refused(mpi, _call(mpi, pb, pa, [2, 2, 2], **kw), mpi.MPI_ERR_ARG, "MPI_Aint")
        _refused(mpi, _call(mpi, mpi.MPI_IN_PLACE, pa, [2, 2, 2], **kw), mpi.MPI_ERR_ARG, "MPI_Aint")   # ahead of IN_PLACE
    # 2^62 elements: doubles pass 63 bits, bytes do not
    kw = dict(osz=[1 << 30, 1 << 30, 4], ost=[0] * 3)
    _refused(mpi, _call(mpi, pb, pa, [2, 2, 2], dt=mpi.MPI_DOUBLE, **kw), mpi.MPI_ERR_ARG, "MPI_Aint")
    assert mpi.error_class(_call(mpi, pb, pa, [2, 2, 2], dt=mpi.MPI_BYTE, op=mpi.MPI_BXOR, **kw)) == mpi.MPI_ERR_BUFFER
    # ... behind a bad dimension
    _refused(mpi, _call(mpi, pb, pa, [2, 2, 5], osz=[big, big, 4], ost=[0] * 3), mpi.MPI_ERR_ARG, "dimension 2")
    assert not a.any()


def test_in_place_and_aliased(mpi):
    assert os.environ.get("MPIR_CVAR_COLL_ALIAS_CHECK", "1") != "0"
    a, b = _host()
    pa, pb = a.ctypes.data, b.ctypes.data
    for pin, pio in ((mpi.MPI_IN_PLACE, pa), (pb, mpi.MPI_IN_PLACE), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE)):
        _refused(mpi, _call(mpi, pin, pio, **GOOD), mpi.MPI_ERR_BUFFER, "MPI_IN_PLACE")
    _refused(mpi, _call(mpi, pa, pa, **GOOD), mpi.MPI_ERR_BUFFER, "aliased")            # unequal sizes
    _refused(mpi, _call(mpi, pa, pa, [2, 3]), mpi.MPI_ERR_BUFFER, "aliased")            # both packed
    _refused(mpi, _call(mpi, pa, pa, [2, 3], isz=[8, 8], ist=[0, 0]), mpi.MPI_ERR_BUFFER, "aliased")   # one side packed
    _refused(mpi, _call(mpi, pa, pa, [2, 3], osz=[8, 8], ost=[0, 0]), mpi.MPI_ERR_BUFFER, "aliased")
    same = dict(isz=[8, 9], osz=[8, 9])
    # the periodic wrap: one array, equal sizes, the boxes apart in some dimension -- passes on to residency
    for ist, ost in (([0, 0], [2, 0]), ([0, 0], [0, 3]), ([6, 1], [0, 2]), ([1, 6], [1, 0]), ([0, 0], [6, 6])):
        _refused(mpi, _call(mpi, pa, pa, [2, 3], ist=ist, ost=ost, **same), mpi.MPI_ERR_BUFFER, "device-resident")
    # boxes that touch in every dimension: the same box, one short of apart in each
    for ist, ost in (([0, 0], [0, 0]), ([0, 0], [1, 2]), ([1, 2], [0, 0]), ([3, 3], [4, 1])):
        _refused(mpi, _call(mpi, pa, pa, [2, 3], ist=ist, ost=ost, **same), mpi.MPI_ERR_BUFFER, "aliased")
    # unequal sizes with boxes apart
    _refused(mpi, _call(mpi, pa, pa, [2, 3], isz=[8, 9], ist=[0, 0], osz=[9, 8], ost=[4, 4]), mpi.MPI_ERR_BUFFER, "aliased")
    assert not a.any()


_ALIAS_OFF = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import mpich_pip_amd as m
lib = m.load()
assert lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN) == 0
a = np.zeros(4096, np.float32)
for kw in (dict(isz=[8, 9], ist=[0, 0], osz=[8, 9], ost=[1, 1]), dict(isz=[8, 9], ist=[0, 0], osz=[9, 8], ost=[4, 4])):
    rc = m.reduce_local_subarray(a.ctypes.data, kw["isz"], kw["ist"], a.ctypes.data, kw["osz"], kw["ost"], [2, 3],
                                 m.MPI_ORDER_C, m.MPI_FLOAT, m.MPI_SUM)
    assert m.error_class(rc) == m.MPI_ERR_BUFFER and "device-resident" in m.error_string(rc), m.error_string(rc)
rc = m.reduce_local_subarray(m.MPI_IN_PLACE, None, None, a.ctypes.data, None, None, [2, 3], m.MPI_ORDER_C, m.MPI_FLOAT, m.MPI_SUM)
assert m.error_class(rc) == m.MPI_ERR_BUFFER and "MPI_IN_PLACE" in m.error_string(rc)
assert not a.any()
print("alias-off ok")
"""


def test_aliased_with_the_check_off():
    """MPIR_CVAR_COLL_ALIAS_CHECK=0 is read once per process: a fresh one.  Overlapping
    boxes of one array then pass the argument checks (and are refused as host memory)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPIR_CVAR_COLL_ALIAS_CHECK="0")
    r = subprocess.run([sys.executable, "-c", _ALIAS_OFF.format(paths=[os.path.join(root, "mpich-pip_amd"), root])],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "alias-off ok" in r.stdout, r.stdout + r.stderr


def test_the_shim_refuses_what_the_entry_point_refuses(mpi):
    """MPIR_Hip_subarray_plan_info answers MPIR_HIP_EARG where the arguments are no box."""
    for kw in (dict(sub=[0, 2]), dict(sub=[2, 2], isz=[1, 2], ist=[0, 0]), dict(sub=[2, 2], osz=[4, 4], ost=[3, 0]),
               dict(sub=[2, 2], osz=[4, 4], ost=[-1, 0]), dict(sub=[2] * 9), dict(sub=[]),
               dict(sub=[2, 2, 2], osz=[(1 << 31) - 1] * 3, ost=[0] * 3)):
        with pytest.raises(ValueError):
            _plan(mpi, **kw)


# ---------------------------------------------------------------- the normal form
def _norm_keys(p):
    return {k: p[k] for k in ("form", "launches", "groups", "per", "units_per_row", "rows_per_launch", "k", "blocklen",
                              "in_offset", "io_offset", "n", "in_stride", "io_stride", "strided_form", "tile_rows", "elem_rows")}


def test_c_order_and_fortran_order_reversed_give_one_plan(mpi):
    rng = np.random.default_rng(1)
    for _ in range(60):
        nd = int(rng.integers(1, 7))
        sub = rng.integers(1, 6, nd)
        isz, osz = sub + rng.integers(0, 4, nd), sub + rng.integers(0, 4, nd)
        ist, ost = [int(rng.integers(0, s - b + 1)) for s, b in zip(isz, sub)], [int(rng.integers(0, s - b + 1)) for s, b in zip(osz, sub)]
        l = lambda x: [int(v) for v in x]
        c = _plan(mpi, l(sub), l(isz), ist, l(osz), ost, C)
        f = _plan(mpi, l(sub)[::-1], l(isz)[::-1], ist[::-1], l(osz)[::-1], ost[::-1], F)
        assert _norm_keys(c) == _norm_keys(f), (l(sub), l(isz), ist, l(osz), ost)


def test_dimensions_of_size_one_vanish(mpi):
    ref = _plan(mpi, [3, 2, 4], [6, 5, 7], [1, 2, 1], [5, 4, 9], [0, 1, 3])
    assert ref["k"] == 2 and ref["blocklen"] == 4 and ref["n"] == [2, 3]
    assert ref["in_stride"] == [7 * 4, 35 * 4] and ref["io_stride"] == [9 * 4, 36 * 4]
    assert ref["in_offset"] == ((1 * 5 + 2) * 7 + 1) * 4 and ref["io_offset"] == ((0 * 4 + 1) * 9 + 3) * 4
    for pos in range(4):
        ins = lambda x, v: x[:pos] + [v] + x[pos:]
        p = _plan(mpi, ins([3, 2, 4], 1), ins([6, 5, 7], 1), ins([1, 2, 1], 0), ins([5, 4, 9], 1), ins([0, 1, 3], 0))
        assert _norm_keys(p) == _norm_keys(ref), pos
    # a subsize of 1 in a longer dimension only moves the base
    p = _plan(mpi, [3, 1, 2, 4], [6, 3, 5, 7], [1, 2, 2, 1], [5, 1, 4, 9], [0, 0, 1, 3])
    assert (p["k"], p["blocklen"], p["n"]) == (2, 4, [2, 3])
    assert p["in_stride"] == [28, 35 * 3 * 4] and p["in_offset"] == (((1 * 3 + 2) * 5 + 2) * 7 + 1) * 4
    # ... in the fastest dimension it leaves rows of one element
    p = _plan(mpi, [3, 2, 1], [6, 5, 7], [1, 2, 1], [5, 4, 9], [0, 1, 3])
    assert (p["k"], p["blocklen"], p["n"], p["in_stride"], p["io_stride"]) == (2, 1, [2, 3], [28, 140], [36, 144])
    # a box of one element
    p = _plan(mpi, [1, 1, 1], [6, 5, 7], [1, 2, 1], [5, 4, 9], [0, 1, 3])
    assert (p["form"], p["k"], p["blocklen"]) == (SINGLE, 0, 1)


def test_a_spanned_dimension_merges_only_when_both_sides_span_it(mpi):
    # the fastest dimension spanned on both sides: rows of 2 x 7
    p = _plan(mpi, [3, 2, 7], [6, 5, 7], [1, 2, 0], [5, 4, 7], [0, 1, 0])
    assert (p["form"], p["k"], p["blocklen"], p["n"]) == (STRIDED, 1, 14, [3])
    # ... on the input side only: nothing merges
    p = _plan(mpi, [3, 2, 7], [6, 5, 7], [1, 2, 0], [5, 4, 9], [0, 1, 0])
    assert (p["k"], p["blocklen"], p["n"]) == (2, 7, [2, 3])
    # ... on the output side only
    p = _plan(mpi, [3, 2, 7], [6, 5, 8], [1, 2, 0], [5, 4, 7], [0, 1, 0])
    assert (p["k"], p["blocklen"], p["n"]) == (2, 7, [2, 3])
    # the middle dimension spanned on both sides: one outer dimension of 3 x 5
    p = _plan(mpi, [3, 5, 4], [6, 5, 7], [1, 0, 1], [4, 5, 9], [0, 0, 3])
    assert (p["form"], p["k"], p["blocklen"], p["n"], p["in_stride"], p["io_stride"]) == (STRIDED, 1, 4, [15], [28], [36])
    # a packed input under a box: packed dimensions merge only where the box spans the output's too
    p = _plan(mpi, [3, 5, 4], None, None, [4, 5, 9], [0, 0, 3])
    assert (p["k"], p["blocklen"], p["n"], p["in_stride"], p["io_stride"]) == (1, 4, [15], [16], [36])
    p = _plan(mpi, [3, 5, 4], None, None, [4, 6, 9], [0, 0, 3])
    assert (p["k"], p["n"], p["in_stride"], p["io_stride"]) == (2, [5, 3], [16, 80], [36, 216])


def test_both_sides_packed_is_the_single_call(mpi):
    p = _plan(mpi, [3, 5, 4])
    assert (p["form"], p["k"], p["blocklen"], p["launches"]) == (SINGLE, 0, 60, 1)
    assert p["groups"] == mpi.plan_info(BASE, FAR, 60, mpi.MPI_FLOAT, mpi.MPI_SUM)["groups"]
    # a whole array on both sides, and one row of a larger one
    assert _plan(mpi, [3, 5, 4], [3, 5, 4], [0, 0, 0], [3, 5, 4], [0, 0, 0])["form"] == SINGLE
    p = _plan(mpi, [1, 1, 3], [6, 5, 7], [1, 2, 1], [5, 4, 9], [0, 1, 3])
    assert (p["form"], p["blocklen"], p["in_offset"], p["io_offset"]) == (SINGLE, 3, 200, 48)


@pytest.mark.parametrize("shape", ["2d", "3d-fastest-spanned", "3d-middle-spanned", "2d-wide", "2d-packed-input"])
def test_one_outer_dimension_is_the_strided_calls_plan(mpi, shape):
    thr = _plan(mpi, [2, 2], [3, 3], [0, 0], [3, 3], [0, 0])["threshold"]
    wide = thr // 4 + 37
    sub, isz, ist, osz, ost = {
        "2d": ([300, 12], [400, 16], [3, 4], [301, 20], [1, 8]),
        "3d-fastest-spanned": ([30, 10, 12], [40, 11, 12], [3, 1, 0], [31, 20, 12], [1, 2, 0]),
        "3d-middle-spanned": ([30, 10, 12], [40, 10, 16], [3, 0, 4], [31, 10, 20], [1, 0, 8]),
        "2d-wide": ([5, wide], [9, wide + 9], [3, 4], [6, wide + 5], [1, 1]),
        "2d-packed-input": ([300, 12], None, None, [301, 20], [1, 8]),
    }[shape]
    p = _plan(mpi, sub, isz, ist, osz, ost)
    assert p["form"] == STRIDED and p["k"] == 1
    s = mpi.strided_plan_info(BASE + p["in_offset"], p["in_stride"][0], FAR + p["io_offset"], p["io_stride"][0], p["n"][0],
                              p["blocklen"], mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert s["form"] == (2 if shape == "2d-wide" else 3)
    for mine, theirs in (("strided_form", "form"), ("launches", "launches"), ("groups", "groups"), ("per", "per"),
                         ("tile_rows", "tile_rows"), ("elem_rows", "elem_rows"), ("threshold", "threshold"),
                         ("rows_per_launch", "rows_per_launch")):
        assert p[mine] == s[theirs], (mine, p, s)
    # the five numbers are the box's: rows of the fastest dimension's subsize (times a merged one)
    want_bl = {"3d-fastest-spanned": 120}.get(shape, sub[-1])
    assert p["blocklen"] == want_bl and p["n"][0] * want_bl == int(np.prod(sub))


def test_five_dimensions_with_nothing_to_merge(mpi):
    p = _plan(mpi, [5, 2, 3, 2, 3], [6, 3, 4, 3, 4], [1, 1, 1, 1, 1], [7, 4, 5, 4, 5], [2, 2, 2, 2, 2])
    assert (p["k"], p["blocklen"], p["n"]) == (4, 3, [2, 3, 2, 5])
    assert p["launches"] == 5 and p["form"] == NARROW_ELEMS and p["groups"] == 5
    # six: the two outermost are looped
    p = _plan(mpi, [4, 5, 2, 3, 2, 3], [5, 6, 3, 4, 3, 4], [1] * 6, [6, 7, 4, 5, 4, 5], [2] * 6)
    assert (p["k"], p["launches"]) == (5, 20)


# ---------------------------------------------------------------- forms
def _set_threshold(mpi, b):
    return mpi.load().MPIR_Hip_set_strided_wide_bytes(b)


def test_wide_and_narrow_flip_at_the_reported_threshold(mpi):
    thr = _plan(mpi, [2, 2, 2], [3, 3, 3], [0] * 3, [3, 3, 3], [0] * 3)["threshold"]
    assert thr == mpi.strided_plan_info(BASE, 0, FAR, 0, 1, 1, mpi.MPI_FLOAT, mpi.MPI_SUM)["threshold"]
    n = thr // 4
    at = _plan(mpi, [3, 4, n], [4, 5, n + 4], [0] * 3, [4, 5, n + 8], [0] * 3)
    below = _plan(mpi, [3, 4, n - 1], [4, 5, n + 4], [0] * 3, [4, 5, n + 8], [0] * 3)
    assert at["form"] == WIDE and below["form"] == NARROW_ELEMS and at["threshold"] == below["threshold"] == thr
    assert _plan(mpi, [3, 4, n - 4], [4, 5, n + 4], [0] * 3, [4, 5, n + 8], [0] * 3)["form"] == NARROW_VEC
    prev = _set_threshold(mpi, 256)
    try:
        assert prev == thr
        assert _plan(mpi, [3, 4, 64], [4, 5, 68], [0] * 3, [4, 5, 72], [0] * 3)["form"] == WIDE
        assert _plan(mpi, [3, 4, 63], [4, 5, 68], [0] * 3, [4, 5, 72], [0] * 3)["form"] == NARROW_ELEMS
        assert _plan(mpi, [3, 4, 64], [4, 5, 68], [0] * 3, [4, 5, 72], [0] * 3)["threshold"] == 256
    finally:
        assert _set_threshold(mpi, prev) == 256


def test_narrow_vec_is_lost_to_each_alignment_condition(mpi):
    """fp32 (7,72,16) / (5,70,12) / (1,1,4): row bytes 48, outer strides 64 and 4608, both
    box bases multiples of 16 -- then each condition broken with the others kept.  An
    outer stride is a multiple of every one below it, so the second can only be lost
    together with the first: a fastest size of 17 with a start of 3 breaks the first
    stride (68) and keeps the second (4896) and the box's base (4976) multiples of 16;
    sizes (7,73,18) with a start of 4 break both strides (72 and 5256) and keep the base
    (5344)."""
    sub, sz, st = [5, 70, 12], [7, 72, 16], [1, 1, 4]
    good = _plan(mpi, sub, sz, st, sz, st)
    assert good["form"] == NARROW_VEC and good["n"] == [70, 5] and good["in_stride"] == good["io_stride"] == [64, 4608]
    assert good["in_offset"] % 16 == 0 and good["io_offset"] % 16 == 0
    assert good["per"] == TILE // 16 and good["units_per_row"] == 3 and good["groups"] == -(-1050 // 1024) == 2
    assert _plan(mpi, [5, 70, 11], sz, st, sz, st)["form"] == NARROW_ELEMS                       # the row's bytes: 44
    s17, st17 = [7, 72, 17], [1, 1, 3]
    for kw in (dict(isz=s17, ist=st17, osz=sz, ost=st), dict(isz=sz, ist=st, osz=s17, ost=st17)):
        p = _plan(mpi, sub, **kw)                                                                # the first outer stride of one side
        side = "in" if kw["isz"] is s17 else "io"
        assert p[side + "_stride"] == [68, 4896] and p[side + "_offset"] % 16 == 0 and p["form"] == NARROW_ELEMS, p
    s73, st73 = [7, 73, 18], [1, 1, 4]
    for kw in (dict(isz=s73, ist=st73, osz=sz, ost=st), dict(isz=sz, ist=st, osz=s73, ost=st73)):
        p = _plan(mpi, sub, **kw)                                                                # both outer strides of one side
        side = "in" if kw["isz"] is s73 else "io"
        assert p[side + "_stride"] == [72, 5256] and p[side + "_offset"] % 16 == 0 and p["form"] == NARROW_ELEMS, p
    for off in (4, 8):
        assert _plan(mpi, sub, sz, st, sz, st, ai=BASE + off)["form"] == NARROW_ELEMS            # the input array's origin
        assert _plan(mpi, sub, sz, st, sz, st, ao=FAR + off)["form"] == NARROW_ELEMS             # the output array's
    assert _plan(mpi, sub, sz, [1, 1, 3], sz, st)["form"] == NARROW_ELEMS                        # the input box's base: start 3
    assert _plan(mpi, sub, sz, st, sz, [1, 1, 1])["form"] == NARROW_ELEMS                        # the output box's base
    # an origin and a start that are each off and together a multiple of 16: the box's address is what counts
    assert _plan(mpi, sub, sz, [1, 1, 3], sz, st, ai=BASE + 4)["form"] == NARROW_VEC
    # the 32-byte class never takes vectors
    p = _plan(mpi, [3, 2, 2], [4, 3, 4], [0] * 3, [4, 3, 4], [0] * 3, t="MPI_LONG_DOUBLE_INT", op="MPI_MAXLOC")
    assert p["form"] == NARROW_ELEMS


def test_g_against_the_batchs_count_per_row(mpi):
    """G is never below what any row needs (the batch's planner on that row's pointers) and
    at most one above; exact where the output box's base and outer strides sit on the 16 KiB grid."""
    thr = _plan(mpi, [2, 2, 2], [3, 3, 3], [0] * 3, [3, 3, 3], [0] * 3)["threshold"]
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    rng = np.random.default_rng(3)
    for case in range(40):
        bl = thr // 4 + int(rng.integers(0, 3 * TILE // 4))
        osz = [4, 5, bl + int(rng.integers(1, 40))]
        isz = [4, 5, bl + int(rng.integers(1, 40))]
        sub, ist, ost = [3, 4, bl], [1, 0, int(rng.integers(0, isz[2] - bl + 1))], [0, 1, int(rng.integers(0, osz[2] - bl + 1))]
        ai, ao = BASE + 4 * int(rng.integers(0, 8)), FAR + 4 * int(rng.integers(0, 4096))
        p = _plan(mpi, sub, isz, ist, osz, ost, ai=ai, ao=ao)
        assert p["form"] == WIDE and p["groups"] == 12 * p["per"] and p["launches"] == 1
        need = 0
        for i2 in range(3):
            for i1 in range(4):
                pin = ai + p["in_offset"] + i1 * p["in_stride"][0] + i2 * p["in_stride"][1]
                pio = ao + p["io_offset"] + i1 * p["io_stride"][0] + i2 * p["io_stride"][1]
                need = max(need, mpi.batch_plan_info([(pin, pio, bl), (pin, pio, bl)], dt, o)["seg_groups"][0])
        assert need <= p["per"] <= need + 1, (case, need, p)
    # on the grid: rows of 2 tiles + 100 floats in an array whose rows are 3 tiles and planes 15
    bl = 2 * TILE // 4 + 100
    p = _plan(mpi, [3, 4, bl], None, None, [4, 5, 3 * TILE // 4], [0, 0, 0])
    assert p["form"] == WIDE and p["per"] == 3 and p["io_stride"] == [3 * TILE, 15 * TILE]
    p = _plan(mpi, [3, 4, bl], None, None, [4, 5, 3 * TILE // 4], [0, 0, 4])        # the box base off the grid
    assert p["per"] == 4
    p = _plan(mpi, [3, 4, bl], None, None, [4, 5, 3 * TILE // 4 + 4], [0, 0, 0])    # the strides off the grid
    assert p["per"] == 4


def test_launches_split_at_the_cap(mpi):
    lib = mpi.load()
    cap = mpi.BATCH_MAX_GROUPS
    # wide rows of one workgroup each: 2^23 + 2^22 rows are two launches
    prev = _set_threshold(mpi, 16)
    try:
        p = _plan(mpi, [3, 1 << 22, 4], [3, 1 << 23, 4096], [0] * 3, [3, 1 << 23, 4096], [0] * 3)
        assert (p["form"], p["per"], p["launches"], p["rows_per_launch"], p["groups"]) == (WIDE, 1, 2, cap, 3 << 22)
    finally:
        _set_threshold(mpi, prev)
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        # narrow vectors: 5 x 70 rows of 3 units, 1024 units a workgroup: 3 workgroups hold 1024 rows -- one launch
        sub, sz, st = [5, 70, 12], [7, 72, 16], [1, 1, 4]
        p = _plan(mpi, sub, sz, st, sz, st)
        assert (p["launches"], p["groups"]) == (1, 2)
        assert lib.MPIR_Hip_strided_test_max_groups(1) == 3
        p = _plan(mpi, sub, sz, st, sz, st)
        assert (p["launches"], p["rows_per_launch"], p["groups"]) == (2, 341, 2)        # the split falls inside outer index 4
        assert lib.MPIR_Hip_strided_test_max_groups(3) == 1
        # wide rows of 2 workgroups under a cap of 3: a row per launch
        thr = p["threshold"]
        bl = thr // 4 + TILE // 4
        p = _plan(mpi, [3, 4, bl], None, None, [4, 5, bl + 4], [0, 0, 0])
        assert p["form"] == WIDE and p["rows_per_launch"] == max(1, 3 // p["per"]) and p["launches"] == -(-12 // p["rows_per_launch"])
        # four outer dimensions: every peeled box splits alike
        p = _plan(mpi, [2, 3, 4, bl], None, None, [3, 4, 5, bl + 4], [0] * 4)
        assert p["k"] == 3 and p["launches"] == -(-24 // p["rows_per_launch"])
        p = _plan(mpi, [5, 2, 3, 4, bl], None, None, [6, 3, 4, 5, bl + 4], [0] * 5)
        assert p["k"] == 4 and p["launches"] == 5 * -(-24 // p["rows_per_launch"])
    finally:
        lib.MPIR_Hip_strided_test_max_groups(0)


# ---------------------------------------------------------------- the matrix
OP = dict(MAX=1, MIN=2, SUM=3, PROD=4, LAND=5, BAND=6, LOR=7, BOR=8, LXOR=9, BXOR=10, MINLOC=11, MAXLOC=12,
          REPLACE=13, NO_OP=14)
INTS = ["I8", "U8", "I16", "U16", "I32", "U32", "I64", "U64"]
REALS = ["F16", "F32", "F64"]
MATRIX = {
    "SUM": INTS + REALS + ["CF32", "CF64", "F80", "CF80"], "PROD": INTS + REALS + ["CF32", "CF64", "F80", "CF80"],
    "MAX": INTS + REALS + ["F80"], "MIN": INTS + REALS + ["F80"],
    "LAND": INTS, "LOR": INTS, "LXOR": INTS + REALS + ["F80"], "BAND": INTS, "BOR": INTS, "BXOR": INTS,
    "MAXLOC": ["P2INT", "PFLOATINT", "PLONGINT", "PSHORTINT", "PDOUBLEINT", "PLDOUBLEINT"],
    "MINLOC": ["P2INT", "PFLOATINT", "PLONGINT", "PSHORTINT", "PDOUBLEINT", "PLDOUBLEINT"],
}


def test_no_kernel_exactly_outside_the_matrix(mpi):
    lib = mpi.load()
    want = {(OP[o], mpi.ELEM[e]) for o, es in MATRIX.items() for e in es}
    assert len(want) == 118
    out = (ctypes.c_uint64 * 40)()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    sub, sz, st = ints(3, 2, 4), ints(6, 5, 7), ints(1, 2, 1)
    nelems = len(mpi.ELEM) + 1
    grid = [(o, e) for o in range(16) for e in range(nelems + 1)]
    rcs = {p: lib.MPIR_Hip_subarray_plan_info(BASE, sz, st, FAR, sz, st, 3, sub, 1, p[0], p[1], out) for p in grid}
    none = {p for p in grid if rcs[p] == ENOKERNEL}
    assert none == set(grid) - want, sorted(none ^ (set(grid) - want))
    assert all(rcs[p] == 0 for p in want)
    assert all(rcs[(OP["REPLACE"], e)] == ENOKERNEL for e in mpi.ELEM.values())
    # the pair is looked at before the box
    assert lib.MPIR_Hip_subarray_plan_info(BASE, sz, st, FAR, sz, st, 0, None, 1, OP["REPLACE"], mpi.ELEM["F32"], out) == ENOKERNEL
    assert lib.MPIR_Hip_subarray_plan_info(BASE, sz, st, FAR, sz, st, 0, None, 1, OP["SUM"], mpi.ELEM["F32"], out) == EARG


# ---------------------------------------------------------------- index arithmetic
def model_normal_form(sub, isz, ist, osz, ost, order, esz):
    """The planner's normal form restated: (blocklen, [(count, in byte stride, io byte stride)]
    fastest first, in byte offset, io byte offset).  isz / osz None: packed."""
    nd = len(sub)
    rev = (lambda x: list(x)[::-1]) if order == C else list
    sub = rev(sub)
    sides = []
    for sz, st in ((isz, ist), (osz, ost)):
        sz, st = (sub, [0] * nd) if sz is None else (rev(sz), rev(st))
        stride, base, acc = [], 0, 1
        for d in range(nd):
            stride.append(acc)
            base += st[d] * acc
            acc *= sz[d]
        sides.append((stride, base))
    dims = []
    for d in range(nd):
        if sub[d] == 1:
            continue
        si, so = sides[0][0][d], sides[1][0][d]
        if dims and si == dims[-1][0] * dims[-1][1] and so == dims[-1][0] * dims[-1][2]:
            dims[-1][0] *= sub[d]
        else:
            dims.append([sub[d], si, so])
    blocklen = 1
    if dims and dims[0][1] == 1 and dims[0][2] == 1:
        blocklen = dims.pop(0)[0]
    return blocklen, [(n, si * esz, so * esz) for n, si, so in dims], sides[0][1] * esz, sides[1][1] * esz


def model_offsets(blocklen, dims, base, side, esz):
    """Byte offsets of every element the kernel visits on one side, row by row in the
    kernel's row numbering (outer dimension 1 fastest)."""
    rows = [0]
    for n, si, so in dims:                  # each further dimension is slower than those before
        step = si if side == 0 else so
        rows = [r + i * step for i in range(n) for r in rows]
    return np.array([base + r + e * esz for r in rows for e in range(blocklen)], dtype=np.int64)


@pytest.mark.parametrize("seed", range(4))
def test_index_arithmetic_against_numpy(mpi, seed):
    """100 random shapes a seed, 1 to 6 dimensions of sizes 1 to 7: the model's offsets are
    numpy's for the same box (as a set on each side, and pairing the same elements), and
    the planner reports the model's normal form."""
    rng = np.random.default_rng(seed)
    for case in range(100):
        nd = int(rng.integers(1, 7))
        order = C if rng.integers(0, 2) else F
        esz, t, op = [(4, "MPI_FLOAT", "MPI_SUM"), (8, "MPI_DOUBLE", "MPI_SUM"), (1, "MPI_BYTE", "MPI_BXOR")][int(rng.integers(0, 3))]
        sides, sub = [], None
        isz = [int(v) for v in rng.integers(1, 8, nd)]
        sub = [int(rng.integers(1, s + 1)) for s in isz]
        osz = [int(b + rng.integers(0, 8 - b)) for b in sub]
        ist = [int(rng.integers(0, s - b + 1)) for s, b in zip(isz, sub)]
        ost = [int(rng.integers(0, s - b + 1)) for s, b in zip(osz, sub)]
        packed = int(rng.integers(0, 4))            # 1: input packed, 2: output packed
        args = [sub, None if packed == 1 else isz, None if packed == 1 else ist,
                None if packed == 2 else osz, None if packed == 2 else ost]
        bl, dims, bi, bo = model_normal_form(*args, order, esz)
        what = (args, order, esz)
        # numpy's view of each box: element byte offsets in the array's own layout
        want = []
        for sz, st in ((args[1], args[2]), (args[3], args[4])):
            sz, st = (sub, [0] * nd) if sz is None else (sz, st)
            whole = (np.arange(int(np.prod(sz)), dtype=np.int64) * esz).reshape(sz, order="C" if order == C else "F")
            want.append(whole[tuple(slice(s, s + b) for s, b in zip(st, sub))])
        got_in, got_io = model_offsets(bl, dims, bi, 0, esz), model_offsets(bl, dims, bo, 1, esz)
        assert got_in.size == int(np.prod(sub)) and np.array_equal(np.sort(got_in), np.sort(want[0].ravel())), what
        assert np.array_equal(np.sort(got_io), np.sort(want[1].ravel())), what
        # the pairing: element number j of the input box meets element number j of the output box
        pair = dict(zip(want[0].ravel().tolist(), want[1].ravel().tolist()))
        assert all(pair[i] == o for i, o in zip(got_in.tolist(), got_io.tolist())), what
        p = _plan(mpi, *args, order=order, t=t, op=op)
        assert (p["blocklen"], p["k"], p["in_offset"], p["io_offset"]) == (bl, len(dims), bi, bo), (what, p)
        assert list(zip(p["n"], p["in_stride"], p["io_stride"])) == dims, (what, p)
        assert p["form"] == (SINGLE if not dims else STRIDED if len(dims) == 1 else p["form"]) and p["form"] != 0
