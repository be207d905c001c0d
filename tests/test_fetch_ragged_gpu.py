"""MPIX_Reduce_local_fetch_ragged on the GPU: the fetching reduction on a ragged
target, in one launch.  inbuf and fetchbuf are packed, the target's pieces sit
at the places a displacement table names.  After each call every target piece
must be the oracle's MPI_Reduce_local on it (bit-exact, test_parity_gpu.same's
complex-NaN rule) and fetchbuf must hold the bytes the pieces held before, a
numpy gather of the old target compared byte for byte.

Each operand sits in an arena of its own filled with 0xA5 (test_ragged_gpu.Arena);
fetchbuf is prefilled with the complement of the old image, so a byte that was
not written shows.  After each call the guard bytes around and between the
target's pieces and around fetchbuf's count x size bytes must still be 0xA5, and
inbuf and both tables must be unchanged.  The target's pieces are laid out in a
permuted order with gaps.  Every shape runs three ways: synchronously with
device tables, enqueued on a torch stream with device tables, and synchronously
with host (numpy) tables.

Every address a kernel forms here stays inside its arena, and every device
`starts` is consistent.
"""
import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import TILE
from test_ragged_gpu import Arena, mixed, place

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, RAGGED = range(3)
WAYS = ("sync", "stream", "host-tables")
# one type of each element size, for the two byte ops
BY_SIZE = {1: "MPI_UNSIGNED_CHAR", 2: "MPI_SHORT", 4: "MPI_FLOAT", 8: "MPI_DOUBLE", 16: "MPI_LONG_DOUBLE",
           32: "MPI_LONG_DOUBLE_INT"}


def op_handle(mpi, op):
    return getattr(mpi, op)


def run(mpi, orc, torch, stream, op, t, lens, unit, tio, pin, pio, pf, seed=0, ways=WAYS, a_all=None, null_in=False):
    """Pieces of lens[k] elements; tio: the target's displacement table (int64, in
    units of `unit` bytes); pin / pio / pf: the byte phases of inbuf, of the
    target's base and of fetchbuf.  a_all: the target's old bytes in packed order
    (generated if None).  null_in: pass a NULL inbuf (MPI_NO_OP).  Runs the call
    every way and checks the three arenas and the tables.  Returns the plan."""
    dt, o = mpi.DATATYPES[t], op_handle(mpi, op)
    esz = T.elem_size(t)
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = int(starts[-1])
    rng = np.random.default_rng([seed, n, count])
    gen_op = op if op in mpi.OPS else "MPI_SUM"
    if a_all is None:
        a_all = T.to_bytes(T.gen(t, count, rng, gen_op))
    b_all = T.to_bytes(T.gen(t, count, rng, gen_op))
    assert len(a_all) == len(b_all) == count * esz
    off_io = np.asarray(tio, np.int64) * unit
    a = [a_all[starts[k] * esz:starts[k + 1] * esz] for k in range(n)]
    b = [b_all[starts[k] * esz:starts[k + 1] * esz] for k in range(n)]
    if op == "MPI_NO_OP":
        want, rc_want = [x.copy() for x in a], 0
    elif op == "MPI_REPLACE":
        want, rc_want = [x.copy() for x in b], 0
    else:
        want = [x.copy() for x in a]
        rcs = {orc.reduce_local(b[k].copy(), want[k], int(lens[k]), dt, o) for k in range(n) if lens[k]}    # piece by piece
        assert len(rcs) == 1
        rc_want = rcs.pop()
    prefill = ~a_all                    # the complement of the old image
    ain = Arena(torch, [b_all], [0], pin)
    afe = Arena(torch, [prefill], [0], pf)
    aio = Arena(torch, a, off_io, pio)
    host = [np.ascontiguousarray(tio, dtype=np.int64), starts]
    devt = [torch.from_numpy(x).cuda() for x in host]
    dptr = [x.data_ptr() for x in devt]
    pb = 0 if null_in else ain.ptr
    what = f"{op} {t} {n} pieces, {count} elements, unit {unit} in=+{pin} io=+{pio}/table fetch=+{pf}"
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.fetch_ragged_plan_info(pb, aio.ptr, dptr[0], afe.ptr, dptr[1], unit, n, count, dt, o)
        assert (info["form"], info["launches"], info["groups"]) == (RAGGED, 1, -(-count * esz // TILE)), f"{what}: {info}"
        assert info == mpi.fetch_ragged_plan_info(pb, aio.ptr, host[0], afe.ptr, host[1], unit, n, count, dt, o)
    for i, way in enumerate(ways):
        if i:
            aio.upload()
            afe.upload()
        torch.cuda.synchronize()
        tabs = host if way == "host-tables" else dptr
        rc = mpi.reduce_local_fetch_ragged(pb, aio.ptr, tabs[0], afe.ptr, tabs[1], unit, n, count, dt, o,
                                           stream.cuda_stream if way == "stream" else 0)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        fetched = afe.check(f"{what} {way} fetchbuf")[0]
        assert np.array_equal(ain.check(f"{what} {way} inbuf")[0], b_all), f"{what} {way}: inbuf modified"
        if rc_want:                     # refused: nothing written
            assert np.array_equal(fetched, prefill), f"{what} {way}: fetchbuf written by a refused call"
            assert all(np.array_equal(x, y) for x, y in zip(got, a)), f"{what} {way}: inoutbuf written by a refused call"
            continue
        if not np.array_equal(fetched, a_all):
            bad = np.nonzero(fetched != a_all)[0]
            k = int(np.searchsorted(starts * esz, bad[0], side="right")) - 1
            pytest.fail(f"{what} {way}: fetchbuf differs from the old target at {bad.size} bytes, first at packed byte "
                        f"{bad[0]} (piece {k} of {lens[k]} elements): got {fetched[bad[0]]:#x}, old {a_all[bad[0]]:#x}, "
                        f"prefill {prefill[bad[0]]:#x}")
        for k in range(n):
            if not np.array_equal(got[k], want[k]) and not same(got[k], want[k], t):
                pytest.fail(f"{what} {way} piece {k} of {lens[k]} elements at packed {starts[k]}:\n" +
                            explain(got[k], want[k], a[k], b[k], esz))
    for x, h in zip(devt, host):
        assert np.array_equal(x.cpu().numpy(), h), f"{what}: a table was written"
    return info


def scatter(mpi, orc, cuda, lens, t="MPI_FLOAT", op="MPI_SUM", unit=None, align=None, gap=None, pin=0, pio=0, pf=0, seed=0,
            ways=WAYS):
    """the Get_accumulate target: packed origin data and response buffer, the
    target's pieces at permuted places"""
    esz = T.elem_size(t)
    unit = unit or esz
    align = align or unit
    tio = place(np.asarray(lens) * esz, unit, align, esz if gap is None else gap, seed)
    return run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, lens, unit, tio, pin, pio, pf, seed=seed, ways=ways)


# ---------------------------------------------------------------- spans and boundaries
def test_pieces_at_span_boundaries(mpi, orc, cuda):
    """fp32 spans are 4096 elements: pieces ending one short of a span's end, on
    it, one past it, a piece holding a whole span, two empty pieces on a
    boundary, a last short one"""
    lens = [4095, 2, 4095, 1, 8191, 0, 0, 5]
    assert sum(lens[:5]) == 4 * 4096
    info = scatter(mpi, orc, cuda, lens)
    assert info["groups"] == 5 and info["per"] == 4096 and info["rounds"] == 1


def test_empty_pieces_first_and_last(mpi, orc, cuda):
    scatter(mpi, orc, cuda, [0, 0, 5, 0, 4096, 3, 0, 0], seed=1)
    scatter(mpi, orc, cuda, [0, 9, 0], seed=2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_search_round_edges(mpi, orc, cuda, n):
    """both sides of every edge of the wave-wide search's round count, lengths 0-7"""
    info = scatter(mpi, orc, cuda, mixed(n, n), seed=n, gap=8)
    assert info["rounds"] == (1 if n <= 63 else 2 if n <= 4095 else 3)


@pytest.mark.parametrize("each", [1, 3])
def test_many_short_pieces(mpi, orc, cuda, each):
    """4097 pieces of 1 element: a span holds as many boundaries as elements,
    more than its LDS table; of 3 elements: a span's end falls inside a piece."""
    info = scatter(mpi, orc, cuda, [each] * 4097, seed=each)
    assert info["rounds"] == 3 and (each == 1 or 4096 % each)
    if each == 1:
        assert info["per"] > info["lds_entries"]


def test_span_with_more_boundaries_than_lds(mpi, orc, cuda):
    """16,385 one-byte pieces at odd byte displacements: the first span holds
    16,384 boundaries, its LDS table fewer, so most lanes search the global
    table from where LDS ends"""
    lens = [1] * 16385
    tio = place(np.ones(16385, np.int64), 1, 2, 1, 19) + 1
    assert (tio % 2 == 1).all()
    info = run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", lens, 1, tio, 1, 0, 3, seed=6)
    assert info["per"] == 16384 > info["lds_entries"] and info["groups"] == 2


# ---------------------------------------------------------------- vector and element chunks
VEC_LENS = 4 * np.random.default_rng(5).integers(0, 40, 300)


def test_every_chunk_a_vector(mpi, orc, cuda):
    """lengths multiples of 4 floats at 16-byte-aligned places, all three addresses aligned"""
    info = scatter(mpi, orc, cuda, VEC_LENS, unit=16, gap=16, pin=16, pio=32, pf=48, seed=5)
    assert info["packed_sides_aligned"] == 1
    # ... as good with byte displacements: the device decides chunk by chunk
    scatter(mpi, orc, cuda, VEC_LENS, unit=1, align=16, gap=16, pin=16, pio=32, pf=48, seed=6)


@pytest.mark.parametrize("off", ["target", "fetchbuf", "inbuf"])
def test_one_address_off_goes_by_elements(mpi, orc, cuda, off):
    """the same pieces with one of the three addresses 4 bytes off: no chunk is a vector"""
    pin, pio, pf = (20 if off == "inbuf" else 16), (36 if off == "target" else 32), (52 if off == "fetchbuf" else 48)
    info = scatter(mpi, orc, cuda, VEC_LENS, unit=16, gap=16, pin=pin, pio=pio, pf=pf, seed=7)
    assert info["packed_sides_aligned"] == int(off == "target")


def test_odd_lengths_straddle_chunks(mpi, orc, cuda):
    """odd lengths: chunks straddle pieces, and only some pieces sit congruent
    mod 16 with their packed offset"""
    lens = [3, 5, 1, 7, 12, 4, 4, 9, 16, 2, 33, 8, 1, 1, 1, 1, 64, 5] * 40
    scatter(mpi, orc, cuda, lens, unit=4, seed=8)
    scatter(mpi, orc, cuda, lens, unit=4, align=16, seed=9)


def test_negative_displacements(mpi, orc, cuda):
    """the base in the middle of the arena"""
    lens = mixed(90, 14, top=30)
    tio = place(lens * 4, 4, 4, 4, 15, centre=True)
    assert (tio < 0).sum() > 20 and (tio > 0).sum() > 20
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_FLOAT", lens, 4, tio, 0, 0, 16, seed=4)


def test_32_byte_class(mpi, orc, cuda):
    """MPI_LONG_DOUBLE_INT MAXLOC: element by element, 512 elements a span"""
    lens = [511, 2, 0, 700, 1, 1, 37]
    info = scatter(mpi, orc, cuda, lens, t="MPI_LONG_DOUBLE_INT", op="MPI_MAXLOC", unit=16, gap=16, seed=20)
    assert info["per"] == 512 and info["groups"] == 3


# ---------------------------------------------------------------- the matrix and the byte ops
def matrix_shape(t):
    """test_ragged_gpu's mixed shape: pieces that are whole vectors at aligned
    places, odd ones between them, an empty one, one that crosses the first
    span's end"""
    esz = T.elem_size(t)
    v = max(16 // esz, 1)
    per = TILE // esz
    lens = [4 * v, 3, 0, 2 * v, 1, per - 6 * v - 7, 5 * v + 1, 2, 8 * v]
    unit = min(esz, 16)
    return lens, unit, place(np.asarray(lens) * esz, unit, 16, unit, 21)


@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_fetch_ragged_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included.  What the
    reference's compute switch refuses (LAND / LOR on floating types) the call
    refuses with the same class, writing nothing."""
    lens, unit, tio = matrix_shape(t)
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, lens, unit, tio, 0, 0, 0, seed=21)


@pytest.mark.parametrize("size", sorted(BY_SIZE))
def test_no_op_is_a_pack(mpi, orc, cuda, size):
    """the target unchanged, fetchbuf the pieces gathered; inbuf not looked at"""
    t = BY_SIZE[size]
    lens, unit, tio = matrix_shape(t)
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_NO_OP", t, lens, unit, tio, 0, 0, 0, seed=22)
    run(mpi, orc, cuda, stream, "MPI_NO_OP", t, lens, unit, tio, 0, 0, 0, seed=23, null_in=True)
    # an inbuf off 16 bytes does not keep the chunks from moving as vectors, the target off does
    info = run(mpi, orc, cuda, stream, "MPI_NO_OP", t, lens, unit, tio, 4, 0, 0, seed=24, ways=("sync",))
    assert info["packed_sides_aligned"] == 1
    run(mpi, orc, cuda, stream, "MPI_NO_OP", t, lens, unit, tio, 0, max(size, 4) % 16 or 4, 0, seed=25, ways=("sync",))


@pytest.mark.parametrize("size", sorted(BY_SIZE))
def test_replace_is_a_swap(mpi, orc, cuda, size):
    """the target equals inbuf, fetchbuf the old bytes"""
    t = BY_SIZE[size]
    lens, unit, tio = matrix_shape(t)
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_REPLACE", t, lens, unit, tio, 0, 0, 0, seed=26)
    run(mpi, orc, cuda, stream, "MPI_REPLACE", t, lens, unit, tio, 0, 0, max(size, 4) % 16 or 4, seed=27, ways=("sync",))


# ---------------------------------------------------------------- the byte copy
@pytest.mark.parametrize("pio", [0, 4], ids=["vectors", "elements"])
def test_fetched_nans_keep_their_payloads(mpi, orc, cuda, pio):
    """an fp32 target of signalling and quiet NaNs with payloads, on the vector
    path and on the element path: the fetched bytes are the old bytes"""
    lens = np.asarray([8, 4, 0, 12, 4, 16, 4])
    count = int(lens.sum())
    pats = np.array([0x7F800001, 0x7FC12345, 0xFFA00123, 0xFFC00001, 0x7FBFFFFF, 0x7F812345, 0xFFFFFFFF, 0x3F800000],
                    np.uint32)
    a_all = T.to_bytes(pats[np.arange(count) % len(pats)])
    tio = place(lens * 4, 16, 16, 16, 30)
    info = run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", lens, 16, tio, 0, pio, 0, seed=30, a_all=a_all)
    assert info["packed_sides_aligned"] == 1


@pytest.mark.parametrize("pio", [0, 8], ids=["vectors", "elements"])
def test_fetched_long_doubles_keep_their_padding(mpi, orc, cuda, pio):
    """an MPI_LONG_DOUBLE target with non-zero bytes in each slot's six padding bytes"""
    lens = np.asarray([5, 1, 0, 9, 2, 30])
    count = int(lens.sum())
    rng = np.random.default_rng(31)
    a_all = T.to_bytes(T.gen("MPI_LONG_DOUBLE", count, rng)).copy().reshape(count, 16)
    a_all[:, 10:] = rng.integers(1, 256, (count, 6), dtype=np.uint8)
    assert (a_all[:, 10:] != 0).all()
    tio = place(lens * 16, 16, 16, 16, 31)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_LONG_DOUBLE", lens, 16, tio, 0, pio, 0, seed=31,
        a_all=a_all.reshape(-1))


# ---------------------------------------------------------------- routes, failures, graphs
def test_contiguous_target_is_the_fetch_call(mpi, orc, cuda):
    """inout_displs NULL is MPIX_Reduce_local_fetch on count elements (starts is
    not looked at): the same target and the same fetched bytes"""
    torch = cuda
    dt = mpi.MPI_FLOAT
    count = 37 * 2703
    rng = np.random.default_rng(count)
    a = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    b = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    ain, aio, afe = Arena(torch, [b], [0], 0), Arena(torch, [a], [0], 16), Arena(torch, [~a], [0], 32)
    stream = torch.cuda.Stream()
    for op in ("MPI_SUM", "MPI_NO_OP", "MPI_REPLACE"):
        o = op_handle(mpi, op)
        assert mpi.fetch_ragged_plan_info(ain.ptr, aio.ptr, None, afe.ptr, 0x10, 4, 37, count, dt, o)["form"] == SINGLE
        aio.upload()
        afe.upload()
        torch.cuda.synchronize()
        assert mpi.reduce_local_fetch(ain.ptr, aio.ptr, afe.ptr, count, dt, o) == 0
        want_io, want_fe = aio.check(f"{op} fetch call")[0], afe.check(f"{op} fetch call")[0]
        assert np.array_equal(want_fe, a)
        for way in ("sync", "stream"):
            aio.upload()
            afe.upload()
            torch.cuda.synchronize()
            rc = mpi.reduce_local_fetch_ragged(ain.ptr, aio.ptr, None, afe.ptr, 0x10, 4, 37, count, dt, o,
                                               0 if way == "sync" else stream.cuda_stream)
            stream.synchronize()
            assert rc == 0, mpi.error_string(rc)
            assert np.array_equal(aio.check(f"{op} {way}")[0], want_io), f"{op} {way}: inoutbuf differs from the fetch call's"
            assert np.array_equal(afe.check(f"{op} {way}")[0], want_fe), f"{op} {way}: fetchbuf differs from the fetch call's"
            assert np.array_equal(ain.check(f"{op} {way}")[0], b)


def test_no_partial_work(mpi, orc, cuda):
    """Everything is settled before anything is enqueued: each of these fails the
    call with its class and all three arenas are untouched."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    lens = mixed(3000, 22, top=12)
    n = len(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = int(starts[-1])
    rng = np.random.default_rng(5)
    a_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    b_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    a = [a_all[starts[k] * 4:starts[k + 1] * 4] for k in range(n)]
    tio = place(lens * 4, 4, 4, 4, 23)
    aio = Arena(torch, a, tio * 4, 0)
    ain = Arena(torch, [b_all], [0], 0)
    # (room behind fetchbuf's bytes for a range that starts inside inbuf's)
    afe = Arena(torch, [~a_all], [0], 0)
    dtio, dstarts = torch.from_numpy(tio).cuda(), torch.from_numpy(starts).cuda()
    stream = torch.cuda.Stream()
    host_fetch = np.ones(count, dtype=np.float32)
    top = int(np.argmax(np.where(lens > 0, tio, tio.min())))        # the highest non-empty piece
    low = int(np.argmin(np.where(lens > 0, tio, tio.max())))        # the lowest
    beyond = tio.copy()
    beyond[top] += 1 << 38                                          # ... 2^40 bytes past the arena
    big = tio.copy()
    big[7] = 1 << 62
    short = starts.copy()
    short[-1] -= 1

    def refused(rc, cls, what):
        stream.synchronize()
        assert mpi.error_class(rc) == cls, f"{what}: {mpi.error_string(rc)}"
        got = aio.check(what)
        assert all(np.array_equal(x, y) for x, y in zip(got, a)), f"{what}: inoutbuf written by a refused call"
        assert np.array_equal(ain.check(what)[0], b_all), f"{what}: inbuf written"
        assert np.array_equal(afe.check(what)[0], ~a_all) and (host_fetch == 1).all(), f"{what}: fetchbuf written"

    B, A = mpi.MPI_ERR_BUFFER, mpi.MPI_ERR_ARG
    call = mpi.reduce_local_fetch_ragged
    s = stream.cuda_stream
    refused(call(ain.ptr, aio.ptr, tio, afe.ptr, dstarts.data_ptr(), 4, n, count, dt, o, s), B, "host table on a stream")
    refused(call(ain.ptr, aio.ptr, dtio.data_ptr(), afe.ptr, starts, 4, n, count, dt, o, s), B, "host starts on a stream")
    refused(call(ain.ptr, aio.ptr, tio, afe.ptr, short, 4, n, count, dt, o), A, "starts ends short of count")
    refused(call(ain.ptr, aio.ptr, dtio.data_ptr(), afe.ptr, short, 4, n, count, dt, o), A, "starts ends short, device table")
    refused(call(ain.ptr, aio.ptr, beyond, afe.ptr, starts, 4, n, count, dt, o), B, "highest piece past the arena")
    refused(call(ain.ptr, aio.ptr, big, afe.ptr, starts, 4, n, count, dt, o), A, "overflowing displacement")
    refused(call(ain.ptr, aio.ptr, big, afe.ptr, dstarts.data_ptr(), 4, n, count, dt, o), A, "overflow beside a device starts")
    for way, st in (("sync", 0), ("stream", s)):
        refused(call(ain.ptr, aio.ptr, dtio.data_ptr(), host_fetch.ctypes.data, dstarts.data_ptr(), 4, n, count, dt, o, st),
                B, f"{way}: fetchbuf in host memory")
        for pf in (ain.ptr, ain.ptr + 4 * count - 4, ain.ptr - 4 * count + 4):
            refused(call(ain.ptr, aio.ptr, dtio.data_ptr(), pf, dstarts.data_ptr(), 4, n, count, dt, o, st), B,
                    f"{way}: fetchbuf overlapping inbuf")
    # with host tables the library knows the pieces' extent: fetchbuf anywhere in it, a gap included
    first = aio.ptr + int(tio[low]) * 4
    last = aio.ptr + int(tio[top]) * 4 + int(lens[top]) * 4 - 1
    assert last - first + 1 >= 4 * count
    for pf in (first, first + 4, last - 4 * count + 1, first - 4 * count + 4, last - 3):
        refused(call(ain.ptr, aio.ptr, tio, pf, starts, 4, n, count, dt, o), B, "fetchbuf inside the pieces' extent")
    # the same call with sound arguments runs
    want = a_all.copy()
    assert orc.reduce_local(b_all.copy(), want, count, dt, o) == 0
    assert call(ain.ptr, aio.ptr, tio, afe.ptr, starts, 4, n, count, dt, o) == 0
    got = aio.check("sound")
    assert all(np.array_equal(got[k], want[starts[k] * 4:starts[k + 1] * 4]) for k in range(n))
    assert np.array_equal(afe.check("sound")[0], a_all)


def test_captured_in_a_graph(mpi, orc, cuda):
    """With device tables the stream call carries everything else in its kernel
    arguments: captured into a graph (one stream, no parallel branches) and
    replayed twice, the target equals the oracle applied twice and fetchbuf the
    target after the first application."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    lens = mixed(400, 24, top=24)
    n = len(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = int(starts[-1])
    rng = np.random.default_rng(9)
    a_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng, specials=False))
    b_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng, specials=False))
    once = a_all.copy()
    assert orc.reduce_local(b_all.copy(), once, count, dt, o) == 0
    twice = once.copy()
    assert orc.reduce_local(b_all.copy(), twice, count, dt, o) == 0
    a = [a_all[starts[k] * 4:starts[k + 1] * 4] for k in range(n)]
    tio = place(lens * 4, 4, 4, 4, 25)
    ain, aio, afe = Arena(torch, [b_all], [0], 0), Arena(torch, a, tio * 4, 16), Arena(torch, [~a_all], [0], 0)
    dtio, dstarts = torch.from_numpy(tio).cuda(), torch.from_numpy(starts).cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_fetch_ragged(ain.ptr, aio.ptr, dtio.data_ptr(), afe.ptr, dstarts.data_ptr(), 4, n, count,
                                                 dt, o, cs) == 0
    torch.cuda.synchronize()
    # capture records, it does not run
    assert all(np.array_equal(x, y) for x, y in zip(aio.check("captured inoutbuf"), a))
    assert np.array_equal(afe.check("captured fetchbuf")[0], ~a_all)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got = aio.check("replayed twice")
    assert all(np.array_equal(got[k], twice[starts[k] * 4:starts[k + 1] * 4]) for k in range(n))
    assert np.array_equal(afe.check("replayed twice fetchbuf")[0], once)
    assert np.array_equal(ain.check("replayed twice inbuf")[0], b_all)
