"""MPIX_Reduce_local_subarray on the GPU: a sub-box of an N-dimensional array on
either side, every element of the box the oracle's MPI_Reduce_local on that pair
(bit-exact, test_parity_gpu.same's complex-NaN rule).

Each operand is a whole array inside an arena of its own filled with 0xA5, the
array's origin at a chosen byte phase of the 16 KiB grid.  The expected result
is built with numpy's own indexing: both boxes gathered (np.arange(...).reshape(
sizes, order=...)[box] names their elements), the oracle run on the packed
pair, the result scattered back.  After each call the box must equal it, every
other byte of the output arena -- the rest of the array included -- must be what
it was, and the input arena must be unchanged.  Before a shape runs,
MPIR_Hip_subarray_plan_info -- the call's own planner -- must report the form the
shape was built for.  Every shape runs twice: synchronously on the library
stream, and enqueued on a torch stream that is then synchronised.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import FILL, TILE

pytestmark = pytest.mark.gpu

SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS, STRIDED = range(1, 6)
FORMS = ["", "single", "wide", "narrow_vec", "narrow_elems", "strided"]
C, F = 56, 57


class Arena:
    """A device allocation filled with 0xA5 around a whole array of `elems`
    (n x element bytes), its origin `phase` bytes past a 16 KiB boundary."""

    def __init__(self, torch, elems, phase):
        self.torch = torch
        self.nbytes = elems.size
        self.t = torch.empty(self.nbytes + 4 * TILE, dtype=torch.uint8, device="cuda")
        self.off = -self.t.data_ptr() % TILE + TILE + phase
        self.ptr = self.t.data_ptr() + self.off
        self.host = np.full(self.t.numel(), FILL, np.uint8)
        self.load(elems)

    def load(self, elems):
        self.host[self.off:self.off + self.nbytes] = elems.reshape(-1)
        self.upload()

    def upload(self):
        self.t.copy_(self.torch.from_numpy(self.host))

    def check(self, what, box=None, esz=1):
        """The array's elements, after asserting that no byte of the arena outside
        the elements numbered `box` differs from what was uploaded."""
        self.torch.cuda.synchronize()
        whole = self.t.cpu().numpy()
        diff = whole != self.host
        if box is not None:
            inside = np.zeros(self.nbytes // esz, bool)
            inside[box] = True
            diff[self.off:self.off + self.nbytes] &= ~np.repeat(inside, esz)
        bad = np.nonzero(diff)[0]
        assert not bad.size, f"{what}: bytes outside the box written at array offsets {(bad[:8] - self.off).tolist()}"
        return whole[self.off:self.off + self.nbytes].reshape(-1, esz)


def box_elems(sizes, starts, sub, order):
    """The element numbers of a box in its array's layout, in the box's index order."""
    whole = np.arange(int(np.prod(sizes)), dtype=np.int64).reshape(sizes, order="C" if order == C else "F")
    return whole[tuple(slice(s, s + b) for s, b in zip(starts, sub))].ravel()


def threshold(mpi):
    return mpi.strided_plan_info(1 << 32, 0, 1 << 40, 0, 1, 1, mpi.MPI_FLOAT, mpi.MPI_SUM)["threshold"]


class wide_from:
    """The wide / narrow threshold lowered for the shapes inside, then restored."""

    def __init__(self, mpi, nbytes):
        self.lib, self.nbytes = mpi.load(), nbytes

    def __enter__(self):
        self.prev = self.lib.MPIR_Hip_set_strided_wide_bytes(self.nbytes)

    def __exit__(self, *exc):
        assert self.lib.MPIR_Hip_set_strided_wide_bytes(self.prev) == self.nbytes


def run(mpi, orc, torch, stream, op, t, sub, isz, ist, osz, ost, form, order=C, pin=0, pio=0, seed=0, expect=None,
        keep=None):
    """The box `sub` of the array isz at ist combined into the one of osz at ost
    (sizes None: packed).  Asserts the planner's form, runs the call both ways and
    checks both arenas.  expect(info): further plan checks.  keep: a dict that
    receives the output array's bytes after the synchronous call.  Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    nd = len(sub)
    full = lambda sz, st: (list(sub), [0] * nd) if sz is None else (list(sz), list(st))
    (fisz, fist), (fosz, fost) = full(isz, ist), full(osz, ost)
    rng = np.random.default_rng([seed, int(np.prod(sub)), nd])
    a = T.to_bytes(T.gen(t, int(np.prod(fosz)), rng, op)).reshape(-1, esz)         # the output array
    b = T.to_bytes(T.gen(t, int(np.prod(fisz)), rng, op)).reshape(-1, esz)         # the input array
    bi, bo = box_elems(fisz, fist, sub, order), box_elems(fosz, fost, sub, order)
    n = bi.size
    packed_in, want_box = np.ascontiguousarray(b[bi]).reshape(-1), np.ascontiguousarray(a[bo]).reshape(-1)
    old_box = want_box.copy()
    rc_want = orc.reduce_local(packed_in.copy(), want_box, n, dt, o)
    want_box = want_box.reshape(n, esz)
    ain, aio = Arena(torch, b, pin), Arena(torch, a, pio)
    what = f"{op} {t} sub={list(sub)} in={isz}@{ist} io={osz}@{ost} order={order} +{pin}/+{pio}"
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.subarray_plan_info(ain.ptr, isz, ist, aio.ptr, osz, ost, sub, order, dt, o)
        assert info["form"] == form, f"{what}: aimed at {FORMS[form]}, the planner says {info}"
        if expect:
            expect(info)
    for way in ("sync", "stream"):
        if way == "stream":
            aio.upload()
        torch.cuda.synchronize()
        rc = mpi.reduce_local_subarray(ain.ptr, isz, ist, aio.ptr, osz, ost, sub, order, dt, o,
                                       0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf", None if rc_want else bo, esz)
        ain.check(f"{what} {way} inbuf")
        if not rc_want and not same(got[bo].reshape(-1), want_box.reshape(-1), t):
            pytest.fail(f"{what} {way} ({FORMS[form]}):\n" + explain(got[bo].reshape(-1), want_box.reshape(-1), old_box,
                                                                     packed_in, esz))
        if keep is not None and way == "sync":
            keep["bytes"] = got.copy()
    return info


# ---------------------------------------------------------------- narrow, elements
@pytest.mark.parametrize("order", [C, F], ids=["c", "fortran"])
def test_doubles_in_both_orders(mpi, orc, cuda, order):
    """fp64 (6,5,7) / (3,2,4) / (1,2,1): rows of 4 doubles under two strides."""
    def two(info):
        want = dict(blocklen=4, n=[2, 3]) if order == C else dict(blocklen=3, n=[2, 4])
        assert info["k"] == 2 and all(info[k] == v for k, v in want.items()) and info["launches"] == 1, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_DOUBLE", [3, 2, 4], [6, 5, 7], [1, 2, 1], [6, 5, 7], [1, 2, 1],
        NARROW_ELEMS, order=order, expect=two)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_DOUBLE", [3, 2, 4], [6, 5, 7], [1, 2, 1], [5, 4, 9], [0, 1, 3],
        NARROW_ELEMS, order=order, pin=8, pio=24, seed=1)


def test_a_one_cell_face_across_the_fast_axis(mpi, orc, cuda):
    """Rows of one element under two strides: 60 x 70 doubles of a (62, 72, 9) array, 4200
    elements, three workgroups."""
    def face(info):
        assert (info["k"], info["blocklen"], info["n"], info["groups"]) == (2, 1, [70, 60], 3), info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_DOUBLE", [60, 70, 1], [62, 72, 9], [1, 1, 8], [61, 71, 5], [0, 1, 2],
        NARROW_ELEMS, expect=face)


def test_three_byte_rows_at_odd_starts(mpi, orc, cuda):
    """MPI_BYTE rows of 3 at odd starts in arrays of odd sizes, 6000 of them: 16384 is no
    multiple of 3, so a workgroup's span ends inside a row; no element is aligned."""
    def two(info):
        assert info["blocklen"] == 3 and info["groups"] == 2 and info["per"] % 3, info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_BYTE", [75, 80, 3], [77, 83, 7], [1, 3, 1], [79, 81, 5], [3, 1, 1],
        NARROW_ELEMS, pin=1, pio=3, expect=two)


# ---------------------------------------------------------------- narrow, vectors
def test_rows_of_three_vectors(mpi, orc, cuda):
    """fp32 (7,72,16) / (5,70,12) / (1,1,4): 1050 vectors, the boundary between the two
    workgroups inside row 341 = (61, 4); the second workgroup's span begins in outer index
    4 of dimension 2 ... and the first's crosses four of its boundaries."""
    def two(info):
        assert info["groups"] == 2 and info["units_per_row"] == 3 and info["n"] == [70, 5] and 1024 % 3, info

    sz, st = [7, 72, 16], [1, 1, 4]
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", [5, 70, 12], sz, st, sz, st, NARROW_VEC, expect=two)
    # 1400 rows: the second workgroup (rows 341 to 682) crosses the boundaries at rows 350, 420, ...
    sz = [22, 72, 16]
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", [20, 70, 12], sz, st, [21, 71, 20], [0, 1, 8], NARROW_VEC,
        seed=1, expect=lambda i: i["groups"] == 5 or pytest.fail(str(i)))


# ---------------------------------------------------------------- wide rows
@pytest.mark.parametrize("off", [0, 8192], ids=["on-grid", "8KiB-off"])
@pytest.mark.parametrize("tiles", [1, 2])
def test_wide_rows_of_whole_tiles(mpi, orc, cuda, tiles, off):
    """Rows of exactly one and of two tiles in an array whose rows are three: on the grid G
    is exact, 8 KiB off it every row takes one workgroup more."""
    bl = tiles * TILE // 4
    assert bl * 4 >= threshold(mpi)

    def grid(info):
        assert info["per"] == (tiles if off == 0 else tiles + 1) and info["groups"] == 6 * info["per"], info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", [2, 3, bl], None, None, [3, 4, 3 * TILE // 4], [1, 1, 0],
        WIDE, pin=off, pio=off, seed=tiles, expect=grid)


def test_threshold_and_one_element_below(mpi, orc, cuda):
    """Row bytes at the reported threshold take the wide form, one element less the narrow one."""
    stream = cuda.cuda.Stream()
    with wide_from(mpi, 256):
        assert threshold(mpi) == 256
        shape = lambda bl: ([3, 4, bl], [4, 5, 72], [1, 0, 4], [5, 6, 76], [0, 1, 8])
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", *shape(64), WIDE, seed=1)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", *shape(63), NARROW_ELEMS, seed=2)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", *shape(60), NARROW_VEC, seed=3)


def test_wide_rows_whose_sides_differ_mod_16(mpi, orc, cuda):
    """The input box one float further into its row than the output box: every row takes
    reduce_seg's element path; with a head and a tail where they agree."""
    stream = cuda.cuda.Stream()
    bl = threshold(mpi) // 4 + TILE // 4 + 7
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", [2, 3, bl], [3, 4, bl + 9], [1, 0, 1], [3, 4, bl + 12], [0, 1, 0], WIDE)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", [2, 3, bl], [3, 4, bl + 9], [1, 0, 1], [3, 4, bl + 12], [0, 1, 5], WIDE,
        seed=1)


@pytest.mark.parametrize("op,t", [("MPI_SUM", "MPI_C_LONG_DOUBLE_COMPLEX"), ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT")])
def test_wide_rows_of_the_32_byte_class(mpi, orc, cuda, op, t):
    bl = threshold(mpi) // 32 + 513
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, [2, 2, bl], [3, 3, bl + 1], [0, 1, 1], [3, 3, bl + 2], [1, 0, 0], WIDE,
        expect=lambda i: i["per"] == -(-bl // 512) or pytest.fail(str(i)))


# ---------------------------------------------------------------- sides
@pytest.mark.parametrize("side", ["unpack-accumulate", "pack-reduce"])
def test_one_side_packed(mpi, orc, cuda, side):
    box = ([6, 7, 9], [1, 2, 3])
    isz, ist, osz, ost = (None, None, *box) if side == "unpack-accumulate" else (*box, None, None)
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", [4, 3, 5], isz, ist, osz, ost, NARROW_ELEMS,
        expect=lambda i: i["k"] == 2 or pytest.fail(str(i)))
    with wide_from(mpi, 32):
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", [4, 3, 5], isz, ist, osz, ost, WIDE, seed=1)


def test_both_sides_boxes_of_different_arrays(mpi, orc, cuda):
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_PROD", "MPI_FLOAT", [4, 3, 8], [6, 7, 12], [2, 3, 4], [5, 4, 20], [0, 1, 8],
        NARROW_VEC, pin=16, pio=32)


# ---------------------------------------------------------------- one array on both sides
def test_a_periodic_fold_inside_one_array(mpi, orc, cuda):
    """inbuf == inoutbuf: the two ghost planes at the top folded onto the first two
    interior planes, and a corner onto a disjoint corner; overlapping boxes are refused
    with nothing written."""
    torch = cuda
    dt, o = mpi.MPI_DOUBLE, mpi.MPI_SUM
    sz = [10, 6, 9]
    rng = np.random.default_rng(7)
    a = T.to_bytes(T.gen("MPI_DOUBLE", int(np.prod(sz)), rng)).reshape(-1, 8)
    stream = torch.cuda.Stream()
    for sub, ist, ost in (([2, 4, 7], [8, 1, 1], [2, 1, 1]), ([3, 2, 4], [0, 0, 5], [1, 3, 1]), ([3, 2, 4], [0, 0, 0], [3, 1, 3])):
        bi, bo = box_elems(sz, ist, sub, C), box_elems(sz, ost, sub, C)
        assert not np.intersect1d(bi, bo).size
        want = np.ascontiguousarray(a[bo]).reshape(-1)
        assert orc.reduce_local(np.ascontiguousarray(a[bi]).reshape(-1), want, bi.size, dt, o) == 0
        arena = Arena(torch, a, 0)
        assert mpi.subarray_plan_info(arena.ptr, sz, ist, arena.ptr, sz, ost, sub, C, dt, o)["k"] == 2
        for way in ("sync", "stream"):
            arena.upload()
            torch.cuda.synchronize()
            rc = mpi.reduce_local_subarray(arena.ptr, sz, ist, arena.ptr, sz, ost, sub, C, dt, o,
                                           0 if way == "sync" else stream.cuda_stream)
            stream.synchronize()
            assert rc == 0, mpi.error_string(rc)
            got = arena.check(f"fold {sub} {way}", bo, 8)
            assert np.array_equal(got[bo].reshape(-1), want), f"fold {sub} {way}"
    arena = Arena(torch, a, 0)
    for ist, ost in (([0, 0, 0], [1, 1, 3]), ([2, 1, 1], [2, 1, 1])):
        rc = mpi.reduce_local_subarray(arena.ptr, sz, ist, arena.ptr, sz, ost, [2, 4, 7] if ist[0] else [3, 2, 4], C, dt, o)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "aliased" in mpi.error_string(rc), mpi.error_string(rc)
        arena.check("overlapping boxes")


# ---------------------------------------------------------------- dimensions
def test_one_dimension_and_collapsing_boxes_equal_the_calls_they_become(mpi, orc, cuda):
    """ndims 1, 2 and 3 that collapse give the bytes of the single and of the strided call on
    the equivalent arguments."""
    torch = cuda
    stream = torch.cuda.Stream()
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    for sub, isz, ist, osz, ost, form in (([1000], [1500], [100], [1200], [37], SINGLE),
                                          ([300, 12], [400, 16], [3, 4], [301, 20], [1, 8], STRIDED),
                                          ([30, 10, 12], [40, 11, 12], [3, 1, 0], [31, 20, 12], [1, 2, 0], STRIDED),
                                          ([30, 10, 12], [40, 10, 16], [3, 0, 4], [31, 10, 20], [1, 0, 8], STRIDED),
                                          ([4, 5, 6], [4, 5, 6], [0, 0, 0], None, None, SINGLE)):
        keep = {}
        p = run(mpi, orc, torch, stream, "MPI_SUM", "MPI_FLOAT", sub, isz, ist, osz, ost, form, seed=len(sub), keep=keep)
        # the same arrays through the call the box becomes
        nd = len(sub)
        fisz, fosz = isz or sub, osz or sub
        rng = np.random.default_rng([len(sub), int(np.prod(sub)), nd])
        a = T.to_bytes(T.gen("MPI_FLOAT", int(np.prod(fosz)), rng, "MPI_SUM")).reshape(-1, 4)
        b = T.to_bytes(T.gen("MPI_FLOAT", int(np.prod(fisz)), rng, "MPI_SUM")).reshape(-1, 4)
        ain, aio = Arena(torch, b, 0), Arena(torch, a, 0)
        pi, po = ain.ptr + p["in_offset"], aio.ptr + p["io_offset"]
        if form == SINGLE:
            rc = mpi.reduce_local(pi, po, p["blocklen"], dt, o)
        else:
            rc = mpi.reduce_local_strided(pi, p["in_stride"][0], po, p["io_stride"][0], p["n"][0], p["blocklen"], dt, o)
        assert rc == 0, mpi.error_string(rc)
        other = aio.check(f"{sub} the call it becomes", box_elems(fosz, ost or [0] * nd, sub, C), 4)
        assert np.array_equal(other, keep["bytes"]), f"{sub}: differs from the call it becomes"


def test_four_and_five_dimensions(mpi, orc, cuda):
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", [3, 4, 5, 6], [4, 6, 7, 8], [1, 1, 2, 1], [5, 5, 6, 9], [2, 0, 1, 3],
        NARROW_ELEMS, expect=lambda i: (i["k"], i["launches"]) == (3, 1) or pytest.fail(str(i)))
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", [3, 4, 5, 6], [4, 6, 7, 8], [1, 1, 2, 1], [5, 5, 6, 9], [2, 0, 1, 3],
        NARROW_ELEMS, order=F, seed=1, expect=lambda i: (i["k"], i["launches"]) == (3, 1) or pytest.fail(str(i)))
    # five with nothing to merge: the outermost is looped on the host
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", [3, 2, 3, 4, 8], [4, 3, 5, 6, 12], [1, 1, 2, 1, 4], [5, 4, 4, 5, 16],
        [2, 0, 1, 1, 8], NARROW_VEC, seed=2, expect=lambda i: (i["k"], i["launches"]) == (4, 3) or pytest.fail(str(i)))
    with wide_from(mpi, 32):
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", [2, 3, 2, 3, 4, 9], [3, 4, 3, 5, 6, 12], [1, 0, 1, 2, 1, 3],
            [4, 3, 4, 4, 5, 16], [2, 0, 0, 1, 1, 7], WIDE, seed=3,
            expect=lambda i: (i["k"], i["launches"]) == (5, 6) or pytest.fail(str(i)))


@pytest.mark.parametrize("pos", range(4))
def test_dimensions_of_size_one_in_every_position(mpi, orc, cuda, pos):
    ins = lambda x, v: x[:pos] + [v] + x[pos:]
    stream = cuda.cuda.Stream()
    # a subsize of 1 in an array dimension of 1, and in a longer one (which scales the strides above it)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", ins([3, 2, 4], 1), ins([6, 5, 7], 1), ins([1, 2, 1], 0),
        ins([5, 4, 9], 1), ins([0, 1, 3], 0), NARROW_ELEMS, seed=pos, expect=lambda i: i["n"] == [2, 3] or pytest.fail(str(i)))
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", ins([3, 2, 4], 1), ins([6, 5, 7], 3), ins([1, 2, 1], 2),
        ins([5, 4, 9], 2), ins([0, 1, 3], 1), NARROW_ELEMS, seed=pos + 4,
        expect=lambda i: (i["k"], i["blocklen"]) == ((2, 4) if pos < 3 else (3, 1)) or pytest.fail(str(i)))


# ---------------------------------------------------------------- launches
def test_lowered_cap_forces_several_launches(mpi, orc, cuda):
    """The per-launch workgroup cap lowered: later launches begin at a row whose outer
    indices are not zero (row 341 is (61, 4)), so the first-row argument matters.  The
    bytes equal the uncapped call's."""
    lib = mpi.load()
    stream = cuda.cuda.Stream()
    sz, st = [7, 72, 16], [1, 1, 4]
    shapes = [("MPI_SUM", "MPI_FLOAT", [5, 70, 12], sz, st, sz, st, NARROW_VEC),
              ("MPI_BXOR", "MPI_BYTE", [75, 80, 3], [77, 83, 7], [1, 3, 1], [79, 81, 5], [3, 1, 1], NARROW_ELEMS)]
    free = [dict() for _ in shapes]
    for s, k in zip(shapes, free):
        run(mpi, orc, cuda, stream, *s, seed=5, keep=k)
    bl = threshold(mpi) // 4 + TILE // 4 + 3
    wide = ("MPI_SUM", "MPI_FLOAT", [3, 5, bl], None, None, [4, 6, bl + 5], [1, 0, 4], WIDE)
    kw = {}
    run(mpi, orc, cuda, stream, *wide, seed=6, keep=kw)
    assert lib.MPIR_Hip_strided_test_max_groups(1) == 0
    try:
        capped = [dict() for _ in shapes]
        run(mpi, orc, cuda, stream, *shapes[0], seed=5, keep=capped[0],
            expect=lambda i: (i["launches"], i["rows_per_launch"]) == (2, 341) or pytest.fail(str(i)))
        run(mpi, orc, cuda, stream, *shapes[1], seed=5, keep=capped[1],
            expect=lambda i: (i["launches"], i["rows_per_launch"]) == (2, TILE // 3) or pytest.fail(str(i)))
        for k, c in zip(free, capped):
            assert np.array_equal(k["bytes"], c["bytes"])
        assert lib.MPIR_Hip_strided_test_max_groups(7) == 1
        kc = {}
        # wide rows of 3 workgroups under a cap of 7: two rows a launch, 15 rows, the launches begin at (2, 0), (4, 0), (1, 1), ...
        run(mpi, orc, cuda, stream, *wide, seed=6, keep=kc,
            expect=lambda i: (i["per"], i["rows_per_launch"], i["launches"]) == (3, 2, 8) or pytest.fail(str(i)))
        assert np.array_equal(kw["bytes"], kc["bytes"])
    finally:
        lib.MPIR_Hip_strided_test_max_groups(0)


# ---------------------------------------------------------------- the matrix
@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_subarray_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, once in each form at
    the smallest shape of that form.  What the reference's compute switch refuses (LAND /
    LOR on floating types) the call refuses with the same class, writing nothing."""
    esz = T.elem_size(t)
    stream = cuda.cuda.Stream()
    vec = max(16 // esz, 1)
    with wide_from(mpi, 256):
        bl = 256 // esz + vec + 1                # a head and a tail where the type has any
        run(mpi, orc, cuda, stream, op, t, [2, 3, bl], [3, 4, bl + 5], [1, 0, 1 if esz < 16 else 0], [3, 4, bl + 2 * vec + 1],
            [0, 1, 1 if esz < 16 else 0], WIDE, pin=4096, seed=1)
        run(mpi, orc, cuda, stream, op, t, [3, 4, 3], [4, 5, 5], [1, 0, 1], [4, 6, 4], [0, 1, 1], NARROW_ELEMS,
            pio=esz if esz < 16 else 8, seed=2)
        if esz <= 16:
            n = 48 // esz
            run(mpi, orc, cuda, stream, op, t, [3, 4, n], [4, 5, 64 // esz], [1, 0, 0], [4, 6, 80 // esz], [0, 1, 16 // esz],
                NARROW_VEC, pin=16, seed=3)


# ---------------------------------------------------------------- graph capture, failures
def test_captured_in_a_graph(mpi, orc, cuda):
    """Everything travels in the kernel arguments: one call captured into a graph (one
    stream, a linear chain) and replayed on fresh inputs twice equals the oracle each time."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    sub, sz, st = [5, 70, 12], [7, 72, 16], [1, 1, 4]
    box = box_elems(sz, st, sub, C)
    rng = np.random.default_rng(11)
    fresh = lambda: T.to_bytes(T.gen("MPI_FLOAT", int(np.prod(sz)), rng)).reshape(-1, 4)
    a, b = fresh(), fresh()
    ain, aio = Arena(torch, b, 0), Arena(torch, a, 16 * 3)
    # the argument arrays live only as long as the call: nothing is read from them afterwards
    assert mpi.subarray_plan_info(ain.ptr, sz, st, aio.ptr, sz, st, sub, C, dt, o)["form"] == NARROW_VEC
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_subarray(ain.ptr, list(sz), list(st), aio.ptr, list(sz), list(st), list(sub), C, dt, o, cs) == 0
    torch.cuda.synchronize()
    aio.check("captured inoutbuf")              # capture records, it does not run
    for replay in range(2):
        a, b = fresh(), fresh()
        ain.load(b)
        aio.load(a)
        want = np.ascontiguousarray(a[box]).reshape(-1)
        assert orc.reduce_local(np.ascontiguousarray(b[box]).reshape(-1), want, box.size, dt, o) == 0
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = aio.check(f"replay {replay}", box, 4)
        assert np.array_equal(got[box].reshape(-1), want), f"replay {replay}"
        ain.check(f"replay {replay} inbuf")


def test_no_partial_work(mpi, orc, cuda):
    """Residency is settled before the first launch: boxes whose first byte is in the arena
    and whose last byte is no device memory (arrays claimed to be 2^48 bytes: the last
    byte's address is past 2^47, which no allocation reaches), or a host operand, fail
    the call with both arenas untouched, however many launches it would have made."""
    torch = cuda
    lib = mpi.load()
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    rng = np.random.default_rng(5)
    sub, sz, st = [5, 70, 12], [7, 72, 16], [1, 1, 4]
    a = T.to_bytes(T.gen("MPI_FLOAT", int(np.prod(sz)), rng)).reshape(-1, 4)
    b = T.to_bytes(T.gen("MPI_FLOAT", int(np.prod(sz)), rng)).reshape(-1, 4)
    ain, aio = Arena(torch, b, 0), Arena(torch, a, 0)
    host = np.ones(int(np.prod(sz)), dtype=np.float32)
    # 2^15 planes of 2^33 bytes: the box's first byte is 8208 bytes into the arena, its last 2^48 further on
    far_sz, far_st, far_sub = [1 << 15, 1 << 20, 1 << 11], [0, 1, 4], [1 << 15, 70, 12]
    assert (((1 << 15) - 1) << 33) >= 1 << 47 and 8208 < ain.nbytes
    stream = torch.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(1) == 0          # several launches, had any been made
    try:
        for way in ("sync", "stream"):
            cs = 0 if way == "sync" else stream.cuda_stream
            torch.cuda.synchronize()
            for args in ((ain.ptr, far_sz, far_st, aio.ptr, far_sz, far_st, far_sub),
                         (host.ctypes.data, sz, st, aio.ptr, sz, st, sub), (ain.ptr, sz, st, host.ctypes.data, sz, st, sub)):
                rc = mpi.reduce_local_subarray(*args, C, dt, o, cs)
                stream.synchronize()
                assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER and "device-resident" in mpi.error_string(rc), mpi.error_string(rc)
                aio.check(f"{way}: inoutbuf written by a refused call")
                ain.check(f"{way}: inbuf written by a refused call")
            assert (host == 1).all()
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 1
