"""MPIX_Reduce_local_ragged on the GPU: unequal pieces from a table of packed
element offsets, in one launch, every piece the oracle's MPI_Reduce_local on it
(bit-exact, test_parity_gpu.same's complex-NaN rule).

Each operand sits in an arena of its own, filled with 0xA5, its base pointer at
a chosen byte phase of the 16 KiB grid (in the middle of the arena where the
table holds negative displacements).  After each call every piece of inoutbuf
must equal the oracle's, every other byte of the arena -- the gaps between
pieces included -- must still be 0xA5, and the input arena and all three tables
must be unchanged: a workgroup that found the wrong first piece, a boundary
read one entry off, a chunk taken for a vector across a piece's end all show
there.  Output pieces are laid out in a permuted order with gaps, so no two
overlap.  The work is divided by packed element, so the shapes are chosen by
where the pieces' boundaries fall against the spans (16 KiB of packed elements:
4096 floats) and against the 16-byte chunks inside them.  Every shape runs
three ways: synchronously with device tables, enqueued on a torch stream with
device tables, and synchronously with host (numpy) tables.

Every address a kernel forms here stays inside its arena, and every device
`starts` is consistent.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import FILL, TILE

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, RAGGED = range(3)
WAYS = ("sync", "stream", "host-tables")


class Arena:
    """A device allocation filled with 0xA5 around pieces of unequal length:
    piece j is the bytes chunks[j] at byte offset offs[j] (signed) from a base
    pointer that sits `phase` bytes past a 16 KiB boundary."""

    def __init__(self, torch, chunks, offs, phase):
        offs = [int(o) for o in offs]
        assert len(offs) == len(chunks)
        lo = min([o for o, c in zip(offs, chunks) if len(c)], default=0)
        hi = max([o + len(c) for o, c in zip(offs, chunks) if len(c)], default=0)
        below = -(-max(-lo, 0) // TILE) * TILE              # room for negative displacements
        self.torch = torch
        self.t = torch.empty(below + max(hi, 0) + phase + 4 * TILE, dtype=torch.uint8, device="cuda")
        off = -self.t.data_ptr() % TILE + TILE + below + phase
        self.ptr = self.t.data_ptr() + off
        self.at = [off + o for o in offs]
        self.size = [len(c) for c in chunks]
        self.host = np.full(self.t.numel(), FILL, np.uint8)
        self.guard = np.ones(self.t.numel(), bool)
        for at, c in zip(self.at, chunks):
            if len(c):
                assert at >= TILE // 2 and at + len(c) <= self.t.numel() - TILE // 2
                assert self.guard[at:at + len(c)].all(), "pieces overlap"
                self.host[at:at + len(c)] = c
                self.guard[at:at + len(c)] = False
        self.upload()

    def upload(self):
        self.t.copy_(self.torch.from_numpy(self.host))

    def check(self, what):
        """The pieces' bytes, after asserting that nothing around or between them was written."""
        self.torch.cuda.synchronize()
        whole = self.t.cpu().numpy()
        bad = np.nonzero(self.guard & (whole != FILL))[0]
        assert not bad.size, f"{what}: guard bytes written at arena offsets {(bad[:8] - (self.ptr - self.t.data_ptr())).tolist()} from the base"
        return [whole[at:at + n] for at, n in zip(self.at, self.size)]


def place(nbytes, unit, align, gap, seed, centre=False):
    """Displacements (in `unit` bytes) that put pieces of nbytes[k] bytes at
    multiples of `align` bytes (a multiple of unit) plus `gap`-byte gaps, in a
    random order; centre: around zero, so that about half are negative."""
    rng = np.random.default_rng([seed, len(nbytes), 77])
    assert align % unit == 0
    out = np.zeros(len(nbytes), np.int64)
    cur = 0
    for k in rng.permutation(len(nbytes)):
        cur = -(-cur // align) * align
        out[k] = cur // unit
        cur += int(nbytes[k]) + (gap if nbytes[k] else 0)
    if centre:
        out -= (cur // 2 // align) * (align // unit)
    return out


def run(mpi, orc, torch, stream, op, t, lens, unit, tin, tio, pin, pio, seed=0, ways=WAYS):
    """Pieces of lens[k] elements.  tin / tio: the displacement tables (int64, in
    units of `unit` bytes) or None for a packed side; pin / pio: the bases' byte
    phases.  Pieces that share a tin entry read the same input (they must be of
    one length).  Runs the call every way and checks both arenas and the tables.
    Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = int(starts[-1])
    rng = np.random.default_rng([seed, n, count])
    off_in = starts[:-1] * esz if tin is None else np.asarray(tin, np.int64) * unit
    off_io = starts[:-1] * esz if tio is None else np.asarray(tio, np.int64) * unit
    a_all = T.to_bytes(T.gen(t, max(count, 1), rng, op))
    b_all = T.to_bytes(T.gen(t, max(count, 1), rng, op))
    a = [a_all[starts[k] * esz:starts[k + 1] * esz] for k in range(n)]
    # one input per placement: the first piece that names it supplies the bytes
    first = {}
    for k in range(n):
        if lens[k]:
            j = first.setdefault(int(off_in[k]), k)
            assert lens[j] == lens[k], "pieces that share an input are of one length"
    b = [b_all[starts[first[int(off_in[k])]] * esz:starts[first[int(off_in[k])] + 1] * esz] if lens[k] else b_all[:0]
         for k in range(n)]
    want = [x.copy() for x in a]
    rcs = {orc.reduce_local(b[k].copy(), want[k], int(lens[k]), dt, o) for k in range(n) if lens[k]}    # piece by piece
    assert len(rcs) == 1
    rc_want = rcs.pop()
    owners = sorted(set(first.values()))
    ain = Arena(torch, [b[k] for k in owners], [off_in[k] for k in owners], pin)
    aio = Arena(torch, a, off_io, pio)
    host = [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (tin, tio)] + [starts]
    devt = [None if x is None else torch.from_numpy(x).cuda() for x in host]
    dptr = [0 if x is None else x.data_ptr() for x in devt]
    what = (f"{op} {t} {n} pieces, {count} elements, unit {unit} in=+{pin}{'' if tin is None else '/table'} "
            f"io=+{pio}{'' if tio is None else '/table'}")
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.ragged_plan_info(ain.ptr, dptr[0], aio.ptr, dptr[1], dptr[2], unit, n, count, dt, o)
        assert (info["form"], info["launches"], info["groups"]) == (RAGGED, 1, -(-count * esz // TILE)), f"{what}: {info}"
        assert info == mpi.ragged_plan_info(ain.ptr, host[0], aio.ptr, host[1], host[2], unit, n, count, dt, o)
    for i, way in enumerate(ways):
        if i:
            aio.upload()
        torch.cuda.synchronize()
        tabs = host if way == "host-tables" else dptr
        rc = mpi.reduce_local_ragged(ain.ptr, tabs[0], aio.ptr, tabs[1], tabs[2], unit, n, count, dt, o,
                                     stream.cuda_stream if way == "stream" else 0)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        back = ain.check(f"{what} {way} inbuf")
        assert all(np.array_equal(x, b[k]) for x, k in zip(back, owners)), f"{what} {way}: inbuf modified"
        for k in range(n):
            if not np.array_equal(got[k], want[k]) and not same(got[k], want[k], t):
                pytest.fail(f"{what} {way} piece {k} of {lens[k]} elements at packed {starts[k]}:\n" +
                            explain(got[k], want[k], a[k], b[k], esz))
    for x, h in zip(devt, host):
        if x is not None:
            assert np.array_equal(x.cpu().numpy(), h), f"{what}: a table was written"
    return info


def scatter(mpi, orc, cuda, lens, t="MPI_FLOAT", op="MPI_SUM", unit=None, align=None, gap=None, pin=0, pio=0, seed=0,
            ways=WAYS):
    """the accumulate target: packed input, the output pieces at permuted places"""
    esz = T.elem_size(t)
    unit = unit or esz
    align = align or unit
    tio = place(np.asarray(lens) * esz, unit, align, esz if gap is None else gap, seed)
    return run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, lens, unit, None, tio, pin, pio, seed=seed, ways=ways)


def mixed(n, seed, top=7):
    """n lengths of 0..top elements, at least one element in all"""
    lens = np.random.default_rng([seed, n]).integers(0, top + 1, n)
    lens[n // 2] = max(lens[n // 2], 1)
    return lens


# ---------------------------------------------------------------- spans and boundaries
def test_pieces_at_span_boundaries(mpi, orc, cuda):
    """fp32 spans are 4096 elements.  Pieces ending one short of a span's end
    (4095), on it (+ 2 across it ... + 4095 + 1 = 8193: one past), a piece that
    holds a whole span in its interior (8191), two empty pieces on a boundary
    (8193 + 8191 = 16384 = 4 spans), and a last short one."""
    lens = [4095, 2, 4095, 1, 8191, 0, 0, 5]
    assert sum(lens[:5]) == 4 * 4096
    info = scatter(mpi, orc, cuda, lens)
    assert info["groups"] == 5 and info["per"] == 4096 and info["rounds"] == 1


def test_empty_pieces_first_and_last(mpi, orc, cuda):
    scatter(mpi, orc, cuda, [0, 0, 5, 0, 4096, 3, 0, 0], seed=1)
    scatter(mpi, orc, cuda, [0, 9, 0], seed=2)


@pytest.mark.parametrize("each", [1, 3])
def test_many_short_pieces(mpi, orc, cuda, each):
    """4097 pieces of 1 element: a span holds as many boundaries as elements,
    more than its LDS table; of 3 elements: a span's end falls inside a piece."""
    info = scatter(mpi, orc, cuda, [each] * 4097, seed=each)
    assert info["rounds"] == 3 and (each == 1 or 4096 % each)
    if each == 1:
        assert info["per"] > info["lds_entries"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_search_round_edges(mpi, orc, cuda, n):
    """both sides of every edge of the wave-wide search's round count, lengths 0-7"""
    info = scatter(mpi, orc, cuda, mixed(n, n), seed=n, gap=8)
    assert info["rounds"] == (0 if n < 1 else 1 if n <= 63 else 2 if n <= 4095 else 3)


def test_three_rounds_over_several_spans(mpi, orc, cuda):
    """4500 pieces of 0-15 elements: eight or so spans, each starting somewhere in
    a table that takes three rounds to search"""
    info = scatter(mpi, orc, cuda, mixed(4500, 3, top=15), seed=4)
    assert info["rounds"] == 3 and info["groups"] > 4


# ---------------------------------------------------------------- vector and element chunks
def test_every_chunk_a_vector(mpi, orc, cuda):
    """lengths multiples of 4 floats at 16-byte-aligned places on both sides"""
    lens = 4 * np.random.default_rng(5).integers(0, 40, 300)
    scatter(mpi, orc, cuda, lens, unit=16, gap=16, pin=16, pio=32, seed=5)
    # ... as good with byte displacements: the device decides chunk by chunk
    scatter(mpi, orc, cuda, lens, unit=1, align=16, gap=16, pin=16, pio=32, seed=6)


def test_every_chunk_by_elements(mpi, orc, cuda):
    """the same pieces with inoutbuf 4 bytes off: no address pair is congruent"""
    lens = 4 * np.random.default_rng(5).integers(0, 40, 300)
    scatter(mpi, orc, cuda, lens, unit=16, gap=16, pin=16, pio=36, seed=7)


def test_odd_lengths_straddle_chunks(mpi, orc, cuda):
    """odd lengths: chunks straddle pieces, and only some pieces sit congruent
    mod 16 with their packed offset"""
    lens = [3, 5, 1, 7, 12, 4, 4, 9, 16, 2, 33, 8, 1, 1, 1, 1, 64, 5] * 40
    scatter(mpi, orc, cuda, lens, unit=4, seed=8)
    scatter(mpi, orc, cuda, lens, unit=4, align=16, seed=9)


# ---------------------------------------------------------------- tables and sides
def test_gather_both_tables_and_repeats(mpi, orc, cuda):
    stream = cuda.cuda.Stream()
    lens = mixed(700, 10, top=20)
    nb = lens * 4
    tin = place(nb, 4, 4, 8, 11)
    tio = place(nb, 4, 16, 4, 12)
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", lens, 4, tin, None, 0, 16, seed=1)       # gather
    run(mpi, orc, cuda, stream, "MPI_PROD", "MPI_FLOAT", lens, 4, tin, tio, 32, 16, seed=2)      # both
    # one input piece of 8 floats combined into each of 500 output pieces
    same_len = [8] * 500
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", same_len, 16, np.zeros(500, np.int64),
        place(np.full(500, 32), 16, 16, 16, 13), 0, 16, seed=3)


def test_negative_displacements(mpi, orc, cuda):
    lens = mixed(90, 14, top=30)
    tio = place(lens * 4, 4, 4, 4, 15, centre=True)
    tin = place(lens * 4, 4, 16, 0, 16, centre=True)
    assert (tio < 0).sum() > 20 and (tio > 0).sum() > 20 and (tin < 0).sum() > 20
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_FLOAT", lens, 4, tin, tio, 0, 0, seed=4)


def test_bytes_at_odd_displacements(mpi, orc, cuda):
    """disp_unit 1, one-byte elements, every displacement odd"""
    lens = mixed(3000, 17, top=9)
    tio = place(lens, 1, 2, 2, 18) + 1
    assert (tio % 2 == 1).all()
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", lens, 1, None, tio, 1, 0, seed=5)


def test_span_with_more_boundaries_than_lds(mpi, orc, cuda):
    """16,385 one-byte pieces: the first span holds 16,384 boundaries, its LDS
    table fewer, so most lanes search the global table from where LDS ends"""
    lens = [1] * 16385
    tio = place(np.ones(16385, np.int64), 1, 1, 1, 19)
    info = run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", lens, 1, None, tio, 0, 3, seed=6)
    assert info["per"] == 16384 > info["lds_entries"] and info["groups"] == 2


def test_32_byte_class(mpi, orc, cuda):
    """MPI_LONG_DOUBLE_INT MAXLOC: element by element, 512 elements a span"""
    lens = [511, 2, 0, 700, 1, 1, 37]
    info = scatter(mpi, orc, cuda, lens, t="MPI_LONG_DOUBLE_INT", op="MPI_MAXLOC", unit=16, gap=16, seed=20)
    assert info["per"] == 512 and info["groups"] == 3


@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_ragged_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, on one
    mixed shape: pieces that are whole vectors at aligned places, odd ones
    between them, an empty one, and one that crosses the first span's end.  What
    the reference's compute switch refuses (LAND / LOR on floating types) the
    call refuses with the same class, writing nothing."""
    esz = T.elem_size(t)
    v = max(16 // esz, 1)
    per = TILE // esz
    lens = [4 * v, 3, 0, 2 * v, 1, per - 6 * v - 7, 5 * v + 1, 2, 8 * v]
    unit = min(esz, 16)
    tio = place(np.asarray(lens) * esz, unit, 16, unit, 21)
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, lens, unit, None, tio, 0, 0, seed=21)


# ---------------------------------------------------------------- routes, failures, graphs
def test_single_call_rule(mpi, orc, cuda):
    """Both tables NULL goes through MPIR_Hip_reduce on count elements (starts is
    not looked at): the same result, and synchronously the direct AQL dispatch
    where it is up."""
    torch = cuda
    lib = mpi.load()
    lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
    state = lib.MPIR_Hip_direct_prepare(torch.cuda.current_device())
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    count = 37 * 2703
    rng = np.random.default_rng(count)
    a = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    b = T.to_bytes(T.gen("MPI_FLOAT", count, rng))
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, count, dt, o) == 0
    ain, aio = Arena(torch, [b], [0], 0), Arena(torch, [a], [0], 0)
    assert mpi.ragged_plan_info(ain.ptr, 0, aio.ptr, 0, 0x10, 4, 37, count, dt, o)["form"] == SINGLE
    stream = torch.cuda.Stream()
    for way in ("sync", "stream"):
        aio.upload()
        torch.cuda.synchronize()
        d0 = lib.MPIR_Hip_direct_dispatches()
        rc = mpi.reduce_local_ragged(ain.ptr, None, aio.ptr, None, 0x10, 4, 37, count, dt, o,
                                     0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert rc == 0, mpi.error_string(rc)
        d1 = lib.MPIR_Hip_direct_dispatches()
        assert np.array_equal(aio.check(way)[0], want), f"{way}: differs from the oracle"
        if state == 1:
            assert d1 - d0 == (1 if way == "sync" else 0), f"{way}: direct dispatches {d1 - d0}"


def test_no_partial_work(mpi, orc, cuda):
    """Everything is settled before anything is enqueued: a host table on a
    stream, a host starts that ends short of count, a piece whose extreme lies
    outside device memory and an overflowing displacement each fail the call
    with their class and nothing written."""
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
    dtio, dstarts = torch.from_numpy(tio).cuda(), torch.from_numpy(starts).cuda()
    stream = torch.cuda.Stream()
    host_in = np.ones(count, dtype=np.float32)
    top = int(np.argmax(np.where(lens > 0, tio, tio.min())))        # the highest non-empty piece
    far = tio.copy()
    far[top] = (host_in.ctypes.data - aio.ptr) // 4                 # ... in this process's host memory
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
        assert np.array_equal(ain.check(what)[0], b_all) and (host_in == 1).all(), what

    B, A = mpi.MPI_ERR_BUFFER, mpi.MPI_ERR_ARG
    call = mpi.reduce_local_ragged
    s = stream.cuda_stream
    refused(call(ain.ptr, None, aio.ptr, tio, dstarts.data_ptr(), 4, n, count, dt, o, s), B, "host table on a stream")
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), starts, 4, n, count, dt, o, s), B, "host starts on a stream")
    refused(call(aio.ptr, tio, ain.ptr, None, dstarts.data_ptr(), 4, n, count, dt, o, s), B, "host input table on a stream")
    for way, st in (("sync", 0), ("stream", s)):
        refused(call(host_in.ctypes.data, None, aio.ptr, dtio.data_ptr(), dstarts.data_ptr(), 4, n, count, dt, o, st), B,
                f"{way}: host inbuf")
        refused(call(aio.ptr, dtio.data_ptr(), host_in.ctypes.data, None, dstarts.data_ptr(), 4, n, count, dt, o, st), B,
                f"{way}: host inoutbuf")
    refused(call(ain.ptr, None, aio.ptr, tio, short, 4, n, count, dt, o), A, "starts ends short of count")
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), short, 4, n, count, dt, o), A, "starts ends short, device table")
    refused(call(ain.ptr, None, aio.ptr, far, starts, 4, n, count, dt, o), B, "a piece in host memory")
    refused(call(ain.ptr, None, aio.ptr, beyond, starts, 4, n, count, dt, o), B, "highest piece past the arena")
    refused(call(ain.ptr, None, aio.ptr, big, starts, 4, n, count, dt, o), A, "overflowing displacement")
    refused(call(ain.ptr, None, aio.ptr, big, dstarts.data_ptr(), 4, n, count, dt, o), A, "overflow beside a device starts")
    # the same call with device operands and sound host tables runs
    want = a_all.copy()
    assert orc.reduce_local(b_all.copy(), want, count, dt, o) == 0
    assert call(ain.ptr, None, aio.ptr, tio, starts, 4, n, count, dt, o) == 0
    got = aio.check("all device")
    assert all(np.array_equal(got[k], want[starts[k] * 4:starts[k + 1] * 4]) for k in range(n))


def test_host_tables_of_growing_size_reuse_the_table_buffer(mpi, orc, cuda):
    """The library's table buffer holds all three tables and grows on demand: a
    small set, one past the buffer's first size, and the small one again."""
    stream = cuda.cuda.Stream()
    for n in (100, 9000, 100):
        lens = mixed(n, n, top=5)
        assert n < 9000 or 3 * 8 * n > (64 << 10)
        tin = place(lens * 8, 8, 8, 8, n)
        tio = place(lens * 8, 8, 16, 0, n + 1)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_DOUBLE", lens, 8, tin, tio, 0, 16, seed=n, ways=("host-tables",))


def test_captured_in_a_graph(mpi, orc, cuda):
    """With device tables the stream call carries everything else in its kernel
    arguments: captured into a graph (one stream, no parallel branches) and
    replayed twice it equals the oracle applied twice."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    lens = mixed(400, 24, top=24)
    n = len(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = int(starts[-1])
    rng = np.random.default_rng(9)
    a_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng, specials=False))
    b_all = T.to_bytes(T.gen("MPI_FLOAT", count, rng, specials=False))
    twice = a_all.copy()
    assert orc.reduce_local(b_all.copy(), twice, count, dt, o) == 0
    assert orc.reduce_local(b_all.copy(), twice, count, dt, o) == 0
    a = [a_all[starts[k] * 4:starts[k + 1] * 4] for k in range(n)]
    tio = place(lens * 4, 4, 4, 4, 25)
    ain, aio = Arena(torch, [b_all], [0], 0), Arena(torch, a, tio * 4, 16)
    dtio, dstarts = torch.from_numpy(tio).cuda(), torch.from_numpy(starts).cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_ragged(ain.ptr, None, aio.ptr, dtio.data_ptr(), dstarts.data_ptr(), 4, n, count, dt, o,
                                           cs) == 0
    torch.cuda.synchronize()
    # capture records, it does not run
    assert all(np.array_equal(x, y) for x, y in zip(aio.check("captured inoutbuf"), a))
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got = aio.check("replayed twice")
    assert all(np.array_equal(got[k], twice[starts[k] * 4:starts[k + 1] * 4]) for k in range(n))
    assert np.array_equal(ain.check("replayed twice inbuf")[0], b_all)
