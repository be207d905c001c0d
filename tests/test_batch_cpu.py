"""MPIX_Reduce_local_batch without a GPU: its argument checks through the C
ABI, and its launch planner (MPIR_Hip_batch_plan_info: the planner the launch
itself runs, host arithmetic on the pointer values) on made-up addresses.

What the planner must get right is what the kernel relies on: a workgroup finds
its segment from the first-workgroup column alone, so every segment's workgroup
count must be the one the kernel's own decomposition covers -- the single
call's tile grid on the tile path, fixed runs of 16384 / esz elements on the
element path -- and a launch may hold no more segments than its kernel
arguments carry and no more workgroups than the cap.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_plan_edges_gpu import CASES, CASE_IDS

TILE = 16384
BASE = 1 << 32
INT_MAX = 2 ** 31 - 1
LEAN, FULL = 0, 1
EMPTY, TILEPATH, ELEMS, SINGLE = range(4)
WILD = 0x10          # an address that would fault if touched


# ---------------------------------------------------------------- argument checks
def _host(n=8):
    return np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)


def test_negative_nsegs_and_null_segs(mpi):
    lib = mpi.load()
    a, b = _host()
    arr = (mpi.ReduceLocalSeg * 1)(mpi.ReduceLocalSeg(b.ctypes.data, a.ctypes.data, 4))
    rc = lib.MPIX_Reduce_local_batch(arr, -1, mpi.MPI_FLOAT, mpi.MPI_SUM, None)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG
    rc = lib.MPIX_Reduce_local_batch(None, 3, mpi.MPI_FLOAT, mpi.MPI_SUM, None)
    assert mpi.error_class(rc) == mpi.MPI_ERR_ARG
    assert not a.any()


def test_negative_count(mpi):
    a, b = _host()
    rc = mpi.reduce_local_batch([(b.ctypes.data, a.ctypes.data, 0), (b.ctypes.data, a.ctypes.data, -1)],
                                mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_COUNT
    assert not a.any()


@pytest.mark.parametrize("op", ["MPI_REPLACE", "MPI_NO_OP", "MPI_OP_NULL", "BAD_HANDLE"])
def test_ops_refused_as_in_reduce_local(mpi, op):
    handle = {"MPI_REPLACE": mpi.MPI_REPLACE, "MPI_NO_OP": mpi.MPI_NO_OP, "MPI_OP_NULL": mpi.MPI_OP_NULL,
              "BAD_HANDLE": 0x44000003}[op]
    a, b = _host()
    segs = [(b.ctypes.data, a.ctypes.data, 4), (b.ctypes.data + 16, a.ctypes.data + 16, 4)]
    rc = mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, handle)
    single = mpi.reduce_local(b.ctypes.data, a.ctypes.data, 4, mpi.MPI_FLOAT, handle)
    assert mpi.error_class(rc) == mpi.error_class(single) == mpi.MPI_ERR_OP
    assert not a.any()


def test_user_op_refused_with_the_stream_variants_text(mpi):
    lib = mpi.load()

    @mpi.MPI_User_function
    def noop(a, b, n, d):
        raise AssertionError("a user op must not run")

    op = ctypes.c_int(0)
    assert lib.MPI_Op_create(noop, 1, ctypes.byref(op)) == 0
    try:
        a, b = _host()
        segs = [(b.ctypes.data, a.ctypes.data, 4), (b.ctypes.data + 16, a.ctypes.data + 16, 4)]
        rc = mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, op.value)
        assert mpi.error_class(rc) == mpi.MPI_ERR_OP
        assert "user MPI_Op functions run on the host" in mpi.error_string(rc)
        rc_stream = mpi.reduce_local_stream(b.ctypes.data, a.ctypes.data, 4, mpi.MPI_FLOAT, op.value)
        assert "user MPI_Op functions run on the host" in mpi.error_string(rc_stream)
    finally:
        assert lib.MPI_Op_free(ctypes.byref(op)) == 0


def test_land_on_float_is_err_op(mpi):
    a, b = _host()
    segs = [(b.ctypes.data, a.ctypes.data, 4), (b.ctypes.data + 16, a.ctypes.data + 16, 4)]
    rc = mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, mpi.MPI_LAND)
    assert mpi.error_class(rc) == mpi.MPI_ERR_OP
    assert "not defined for this datatype" in mpi.error_string(rc)
    # an op the type's check_dtype refuses outright
    assert mpi.error_class(mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, mpi.MPI_BAND)) == mpi.MPI_ERR_OP


def test_aliased_segment_and_in_place(mpi):
    a, b = _host()
    rc = mpi.reduce_local_batch([(b.ctypes.data, a.ctypes.data, 4), (a.ctypes.data + 16, a.ctypes.data + 16, 2)],
                                mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc)
    for seg in ((mpi.MPI_IN_PLACE, a.ctypes.data, 4), (b.ctypes.data, mpi.MPI_IN_PLACE, 4)):
        rc = mpi.reduce_local_batch([(b.ctypes.data, a.ctypes.data, 4), seg], mpi.MPI_FLOAT, mpi.MPI_SUM)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "MPI_IN_PLACE" in mpi.error_string(rc)
    assert not a.any()


@pytest.mark.parametrize("nseg", [1, 2, 5])
def test_host_pointers_refused_as_non_device(mpi, nseg):
    """As MPIX_Reduce_local_multi refuses them (test_abi_cpu); one segment is no
    exception: the batch never takes the single call's host paths."""
    a, b = _host(64)
    segs = [(b.ctypes.data + 16 * k, a.ctypes.data + 16 * k, 4) for k in range(nseg)]
    rc = mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, mpi.MPI_SUM)
    assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER
    assert "device-resident" in mpi.error_string(rc) and "aliased" not in mpi.error_string(rc)
    assert not a.any()


def test_empty_batches_succeed_without_touching_a_pointer(mpi):
    lib = mpi.load()
    assert lib.MPIX_Reduce_local_batch(None, 0, mpi.MPI_FLOAT, mpi.MPI_SUM, None) == 0
    assert mpi.reduce_local_batch([], mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    # empty segments: wild, aliased and MPI_IN_PLACE pointers all pass unseen
    segs = [(WILD, WILD, 0), (WILD + 1, WILD + 3, 0), (mpi.MPI_IN_PLACE, mpi.MPI_IN_PLACE, 0), (0, 0, 0)]
    assert mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    assert mpi.reduce_local_batch(segs * 100, mpi.MPI_DOUBLE, mpi.MPI_MAX) == 0
    # ... but the op is still checked
    assert mpi.error_class(mpi.reduce_local_batch(segs, mpi.MPI_FLOAT, mpi.MPI_OP_NULL)) == mpi.MPI_ERR_OP


def test_shim_refuses_replace_and_unknown_pairs(mpi):
    lib = mpi.load()
    ENOKERNEL = 3
    out = (ctypes.c_uint64 * 6)()
    segs = (mpi.HipSeg * 2)(mpi.HipSeg(BASE, BASE + TILE, 4), mpi.HipSeg(BASE + 64, BASE + TILE + 64, 4))
    f32 = mpi.ELEM["F32"]
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, mpi.MPI_REPLACE & 0xF, f32, out, None, None) == ENOKERNEL
    assert lib.MPIR_Hip_reduce_batch(segs, 2, mpi.MPI_REPLACE & 0xF, f32, None, 1) == ENOKERNEL
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, mpi.MPI_BAND & 0xF, f32, out, None, None) == ENOKERNEL   # no BAND on floats
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, mpi.MPI_MAXLOC & 0xF, f32, out, None, None) == ENOKERNEL
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, 0, f32, out, None, None) == ENOKERNEL
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, mpi.MPI_SUM & 0xF, 99, out, None, None) == ENOKERNEL
    assert lib.MPIR_Hip_batch_plan_info(segs, 2, mpi.MPI_SUM & 0xF, f32, out, None, None) == 0


# ---------------------------------------------------------------- the planner
def _plan(mpi, segs, t, op):
    return mpi.batch_plan_info(segs, mpi.DATATYPES[t], mpi.OPS[op])


@pytest.mark.parametrize("op,t,align", CASES, ids=CASE_IDS)
def test_tile_segments_take_the_single_calls_grid(mpi, op, t, align):
    """A tile-path segment runs reduce_tile on the grid MPIR_Hip_plan_info reports
    for the same pointers (LEAN or FULL), so its workgroup count must be that
    plan's; every other shape must report the element path."""
    esz = T.elem_size(t)
    vec = max(16 // esz, 1)
    counts = sorted({1, 2, vec - 1, vec, vec + 1, 3 * vec, TILE // esz - 1, TILE // esz, TILE // esz + 1,
                     2 * TILE // esz + vec - 1, 5 * TILE // esz + 3} - {0})
    tiles = elems = 0
    for pio in (0, esz, 16, 4096, TILE - 16, TILE - 16 + esz, TILE - esz):
        for dpin in (0, 4096, TILE - 16, esz, 1, 4, 8):
            ao, ai = BASE + pio, BASE + 64 * TILE + pio + dpin
            for n in counts:
                # a neighbour on either side: the segment under test is never the only one
                segs = [(BASE + 200 * TILE, BASE + 300 * TILE, 3), (ai, ao, n), (BASE + 400 * TILE, BASE + 500 * TILE, 3)]
                info = _plan(mpi, segs, t, op)
                single = mpi.plan_info(ai, ao, n, mpi.DATATYPES[t], mpi.OPS[op])
                kind, groups = info["seg_kind"][1], info["seg_groups"][1]
                natural = ai % align == 0 and ao % align == 0
                head_ok = (-ao % 16) % esz == 0
                want_tile = esz <= 16 and natural and (ai - ao) % 16 == 0 and head_ok
                what = f"{t} in=+{ai - BASE} io=+{pio} n={n}: batch {info}, single {single}"
                assert kind == (TILEPATH if want_tile else ELEMS), what
                if want_tile:
                    assert single["kind"] in (LEAN, FULL), what
                    assert groups == single["groups"], what
                    # the grid covers the vector region on 16 KiB boundaries of inoutbuf's address
                    vs = ao + single["nhead"] * esz
                    assert groups == max(1, -(-(vs % TILE + single["vbytes"]) // TILE)), what
                    tiles += 1
                else:
                    assert single["kind"] not in (LEAN, FULL), what
                    assert groups == -(-n // (TILE // esz)), what
                    elems += 1
                assert info["launches"] == 1 and info["groups"] == sum(info["seg_groups"]), what
    assert elems and (tiles or esz == 32)


def test_paths_counted_and_empty_segments_reported(mpi):
    t, op = "MPI_FLOAT", "MPI_SUM"
    segs = [(WILD, WILD, 0),                               # empty, first
            (BASE, BASE + 64 * TILE, 1000),                # tile
            (BASE + 4, BASE + 65 * TILE, 1000),            # elements: inbuf 4 B off
            (WILD, WILD + 1, 0),                           # empty, middle
            (BASE + 2, BASE + 66 * TILE + 2, 5000),        # elements: off natural alignment
            (BASE + 32, BASE + 67 * TILE + 32, 5 * 4096),  # tile, five tiles and a sixth partial
            (0, 0, 0)]                                     # empty, last
    info = _plan(mpi, segs, t, op)
    assert info["seg_kind"] == [EMPTY, TILEPATH, ELEMS, EMPTY, ELEMS, TILEPATH, EMPTY]
    assert info["seg_groups"] == [0, 1, 1, 0, 2, 6, 0]
    assert (info["launches"], info["groups"], info["tile"], info["elems"], info["empty"]) == (1, 10, 2, 2, 3)
    # the 32-byte classes always take the element path, 512 elements per workgroup
    wide = _plan(mpi, [(BASE, BASE + 64 * TILE, 513), (BASE + 16, BASE + 65 * TILE, 512)], "MPI_LONG_DOUBLE_INT",
                 "MPI_MAXLOC")
    assert wide["seg_kind"] == [ELEMS, ELEMS] and wide["seg_groups"] == [2, 1]


def test_one_non_empty_segment_is_the_single_call(mpi):
    t, op = "MPI_FLOAT", "MPI_SUM"
    for ai, ao, n in ((BASE, BASE + 64 * TILE, 100000), (BASE + 4, BASE + 64 * TILE, 100000), (BASE + 4, BASE + 8, 3)):
        info = _plan(mpi, [(WILD, WILD, 0), (ai, ao, n), (WILD, WILD, 0)], t, op)
        single = mpi.plan_info(ai, ao, n, mpi.DATATYPES[t], mpi.OPS[op])
        assert info["seg_kind"] == [EMPTY, SINGLE, EMPTY]
        assert info["seg_groups"] == [0, single["groups"], 0]
        assert (info["launches"], info["groups"], info["tile"], info["elems"], info["empty"]) == \
            (1, single["groups"], 0, 0, 2)
    none = _plan(mpi, [(WILD, WILD, 0)] * 3, t, op)
    assert (none["launches"], none["groups"], none["empty"]) == (0, 0, 3) and none["seg_kind"] == [EMPTY] * 3
    assert _plan(mpi, [], t, op)["launches"] == 0


def test_launches_split_at_the_argument_table(mpi):
    t, op = "MPI_FLOAT", "MPI_SUM"
    K = _plan(mpi, [], t, op)["max_segs"]
    assert K >= 2 and 8 + 32 * K <= 4096          # {in, io, count, first} per segment within 4 KiB of arguments
    for n in (K - 1, K, K + 1, 2 * K + 1):
        segs = [(BASE + 4096 * k, BASE + (1 << 30) + 4096 * k, 1 + k % 700) for k in range(n)]
        info = _plan(mpi, segs, t, op)
        assert info["launches"] == -(-n // K), (n, K, info["launches"])
        assert info["max_segs"] == K and info["groups"] == n and info["tile"] == n
        # empty segments take no descriptor
        sparse = [s for seg in segs for s in (seg, (WILD, WILD, 0))]
        assert _plan(mpi, sparse, t, op)["launches"] == -(-n // K)


def test_launches_split_at_the_workgroup_cap(mpi):
    """INT_MAX-count segments: each alone is far below the cap, a launch closes
    before its total passes it, and the same addresses always plan the same."""
    t, op = "MPI_FLOAT", "MPI_SUM"
    cap = mpi.BATCH_MAX_GROUPS
    assert cap < 2 ** 31 and cap * 256 < 2 ** 32
    K = _plan(mpi, [], t, op)["max_segs"]
    n = 64
    assert n < K
    # every operand INT_MAX floats long at 16 GiB strides; inoutbuf 32 B past a grid boundary
    segs = [(BASE + (k << 34), BASE + (1 << 44) + (k << 34) + 32, INT_MAX) for k in range(n)]
    info = _plan(mpi, segs, t, op)
    per = info["seg_groups"][0]
    assert info["seg_kind"] == [TILEPATH] * n and info["seg_groups"] == [per] * n
    assert per == -(-(32 + (INT_MAX * 4 - 12)) // TILE)          # vector region: all but the 12 B tail, 32 B into a tile
    fit = cap // per                                             # whole segments under the cap
    assert 1 <= fit < n
    assert info["launches"] == -(-n // fit) and info["groups"] == n * per
    # the 32-byte classes' largest segment still fits one launch
    wide = _plan(mpi, [(BASE, BASE + (1 << 44), INT_MAX), (BASE + (1 << 40), BASE + (1 << 45), INT_MAX)],
                 "MPI_LONG_DOUBLE_INT", "MPI_MAXLOC")
    assert wide["seg_groups"] == [-(-INT_MAX // 512)] * 2 and wide["seg_groups"][0] <= cap
    assert wide["launches"] == (1 if 2 * wide["seg_groups"][0] <= cap else 2)
