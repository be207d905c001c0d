"""The (op, element class) matrix of every kernel family, pinned on its own.

The registration units fill one table per family from the four pair lists of
csrc/hip/kernel_table.hpp.  This test states the matrix once more, in Python
and independently of those lists, and asks the shim pair by pair: every op
index 0..15 against every element class index 0..MPIR_HIP_NELEMS - 1 and one
past it.  MPIR_Hip_has_kernel answers for the single call's table; each
family's *_plan_info entry point, on made-up addresses and a sound argument
set (those of the families' own *_cpu.py tests), answers MPIR_HIP_ENOKERNEL
exactly for the pairs outside the matrix.

MPI_REPLACE is a byte copy of every class in the single call and has no kernel
in the batch, strided, indexed, ordered and ragged families; the three fetching
families take MPI_NO_OP and MPI_REPLACE on every class that has a size.
"""
import ctypes

import pytest

BASE = 1 << 32               # inbuf's arena
FAR = 1 << 40                # inoutbuf's
FETCH = 1 << 41              # fetchbuf's
TAB_O, TAB_S, TAB_ORD = (1 << 44) + (1 << 30), (1 << 44) + (1 << 31), (1 << 44) + (1 << 29)
TILE = 16384
ENOKERNEL = 3

# op indices: the reference's MPIR_Op_table (include/mpir_hip_reduce.h)
OP = dict(MAX=1, MIN=2, SUM=3, PROD=4, LAND=5, BAND=6, LOR=7, BOR=8, LXOR=9, BXOR=10, MINLOC=11, MAXLOC=12,
          REPLACE=13, NO_OP=14)
INTS = ["I8", "U8", "I16", "U16", "I32", "U32", "I64", "U64"]
REALS = ["F16", "F32", "F64"]
CPLX = ["CF32", "CF64"]
PAIRS = ["P2INT", "PFLOATINT", "PLONGINT", "PSHORTINT", "PDOUBLEINT"]
# op -> the classes it is defined on (src/include/mpir_op_util.h); F80, CF80 and
# PLDOUBLEINT are long double, its _Complex and MPI_LONG_DOUBLE_INT
MATRIX = {
    "SUM": INTS + REALS + CPLX + ["F80", "CF80"], "PROD": INTS + REALS + CPLX + ["F80", "CF80"],
    "MAX": INTS + REALS + ["F80"], "MIN": INTS + REALS + ["F80"],
    "LAND": INTS, "LOR": INTS, "LXOR": INTS + REALS + ["F80"],
    "BAND": INTS, "BOR": INTS, "BXOR": INTS,
    "MAXLOC": PAIRS + ["PLDOUBLEINT"], "MINLOC": PAIRS + ["PLDOUBLEINT"],
}
# the pairs on the wide (32-byte class) launcher; every other one is on the ordinary launcher
WIDE = {("SUM", "CF80"), ("PROD", "CF80"), ("MAXLOC", "PLDOUBLEINT"), ("MINLOC", "PLDOUBLEINT")}
COMBINING = ("batch", "strided", "indexed", "indexed_ordered", "ragged")
FETCHING = ("fetch", "fetch_ragged", "fetch_indexed_ordered")


@pytest.fixture(scope="module")
def expected(mpi):
    pairs = {(OP[o], mpi.ELEM[e]) for o, es in MATRIX.items() for e in es}
    assert len(pairs) == 118 and len(pairs - {(OP[o], mpi.ELEM[e]) for o, e in WIDE}) == 114
    return pairs


@pytest.fixture(scope="module")
def asked(mpi):
    """rc of every family's plan_info for every (op, elem) asked, computed once."""
    lib = mpi.load()
    out = (ctypes.c_uint64 * 8)()
    segs = (mpi.HipSeg * 2)(mpi.HipSeg(BASE, BASE + TILE, 4), mpi.HipSeg(BASE + 64, BASE + TILE + 64, 4))
    info = {
        "batch": lambda o, e: lib.MPIR_Hip_batch_plan_info(segs, 2, o, e, out, None, None),
        # strides that hold a row of four elements of the widest (32-byte) class
        "strided": lambda o, e: lib.MPIR_Hip_strided_plan_info(BASE, 128, FAR, 256, 4, 4, o, e, out),
        "fetch": lambda o, e: lib.MPIR_Hip_fetch_plan_info(BASE, FAR, FETCH, 4, o, e, out),
        "indexed": lambda o, e: lib.MPIR_Hip_indexed_plan_info(BASE, None, FAR, TAB_O, 16, 4, 4, o, e, out),
        "indexed_ordered": lambda o, e: lib.MPIR_Hip_indexed_ordered_plan_info(BASE, None, FAR, TAB_O, TAB_ORD, 16, 4, 4,
                                                                                 o, e, out),
        "ragged": lambda o, e: lib.MPIR_Hip_ragged_plan_info(BASE, None, FAR, TAB_O, TAB_S, 16, 4, 16, o, e, out),
        "fetch_ragged": lambda o, e: lib.MPIR_Hip_fetch_ragged_plan_info(BASE, FAR, TAB_O, FETCH, TAB_S, 16, 4, 16, o, e, out),
        "fetch_indexed_ordered": lambda o, e: lib.MPIR_Hip_fetch_indexed_ordered_plan_info(
            BASE, None, FAR, TAB_O, FETCH, TAB_ORD, 16, 4, 4, o, e, out),
    }
    assert sorted(info) == sorted(COMBINING + FETCHING)
    nelems = len(mpi.ELEM) + 1                    # MPIR_HIP_NELEMS: classes count from 1
    assert lib.MPIR_Hip_elem_size(nelems - 1) and not lib.MPIR_Hip_elem_size(nelems) and not lib.MPIR_Hip_elem_size(0)
    grid = [(o, e) for o in range(16) for e in range(nelems + 1)]
    return grid, {f: {p: fn(*p) for p in grid} for f, fn in info.items()}


def test_the_matrix_counts(mpi, expected):
    assert len(mpi.ELEM) == 21 and sorted(OP.values()) == list(range(1, 15))
    assert sum(len(es) for es in MATRIX.values()) == 118


def test_has_kernel_is_the_matrix_plus_replace_on_every_class(mpi, expected, asked):
    lib = mpi.load()
    grid, _ = asked
    sized = {e for e in mpi.ELEM.values()}
    want = expected | {(OP["REPLACE"], e) for e in sized}
    got = {p for p in grid if lib.MPIR_Hip_has_kernel(*p)}
    assert got == want, (sorted(got - want), sorted(want - got))


@pytest.mark.parametrize("family", COMBINING)
def test_combining_families_hold_the_matrix_and_no_replace(mpi, expected, asked, family):
    grid, rcs = asked
    none = {p for p in grid if rcs[family][p] == ENOKERNEL}
    assert none == set(grid) - expected, (family, sorted(none ^ (set(grid) - expected)))
    assert all(rcs[family][(OP["REPLACE"], e)] == ENOKERNEL for e in mpi.ELEM.values())
    # a registered pair answers something else: the argument set is sound for every class
    assert all(rcs[family][p] == 0 for p in expected), [(p, rcs[family][p]) for p in expected if rcs[family][p]][:5]


@pytest.mark.parametrize("family", FETCHING)
def test_fetching_families_hold_the_matrix_and_the_byte_ops(mpi, expected, asked, family):
    grid, rcs = asked
    want = expected | {(o, e) for o in (OP["NO_OP"], OP["REPLACE"]) for e in mpi.ELEM.values()}
    none = {p for p in grid if rcs[family][p] == ENOKERNEL}
    assert none == set(grid) - want, (family, sorted(none ^ (set(grid) - want)))
    assert all(rcs[family][p] == 0 for p in want), [(p, rcs[family][p]) for p in want if rcs[family][p]][:5]
