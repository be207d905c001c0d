"""Every launch-plan edge of the single-operand kernels, on purpose.

test_parity_gpu varies what is computed; which kernel computes it, and where
that kernel's addressing has its edges, is chosen here.  Each shape names the
plan kind it aims at and asserts that MPIR_Hip_plan_info -- the launch's own
planner -- reports that kind before it runs, so a shape cannot drift to
another kernel when a threshold moves (tests/test_plan_cpu.py asserts the same
on made-up addresses, without a GPU).

Each operand lives in an arena of its own, filled with 0xA5, with the payload
at a chosen byte phase of the 16 KiB grid the tile kernels lay over inoutbuf's
address.  After every call the payload must equal the oracle's (bit-exact,
test_parity_gpu.same's complex-NaN rule) and every other byte of both arenas
must still be 0xA5: the head lanes, the tail lanes, tile 0's cut and the shift
kernel's rounded-up in-descriptor all work at the payload's edges.

Every shape runs three ways: MPI_Reduce_local on fresh arguments (a
kernarg-cache miss: the direct path's checked kernel), the same call again (a
verified hit: the unchecked kernel), and MPIX_Reduce_local_stream on a torch
stream (the HIP launch).  The whole sweep then runs again with
MPIR_Hip_set_keep_min_bytes(0), so that every small result takes the sc1 store.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_parity_gpu import explain, same

pytestmark = pytest.mark.gpu

TILE = 16384
FILL = 0xA5
LEAN, FULL, SHIFT, ELEMS, ELEMS_U, WIDE_TILE, WIDE_ELEMS = range(7)
STRIDE_COUNT = 2 * 1048576 + 4099          # the element kernels' grid covers 1,048,576 elements per stride

# (op, type, alignment of the device type)
CASES = [("MPI_BXOR", "MPI_UNSIGNED_CHAR", 1), ("MPI_SUM", "MPIX_C_FLOAT16", 2), ("MPI_SUM", "MPI_FLOAT", 4),
         ("MPI_MAX", "MPI_DOUBLE", 8), ("MPI_PROD", "MPI_C_FLOAT_COMPLEX", 4), ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX", 8),
         ("MPI_MINLOC", "MPI_DOUBLE_INT", 8), ("MPI_SUM", "MPI_LONG_DOUBLE", 16),
         ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT", 16)]
CASE_IDS = [f"{o}-{t}" for o, t, _ in CASES]


def shapes(t, align):
    """(count, phase of inbuf, phase of inoutbuf, intended kind) for type t; the
    phases are byte offsets from a 16 KiB boundary.  No duplicates: the first
    call of every shape must miss the kernarg cache."""
    esz = T.elem_size(t)
    out = {}

    def add(n, pin, pio, kind):
        assert n >= 1 and pin >= 0 and pio >= 0
        out.setdefault((n, pin, pio), kind)

    def elems_kind(pin, pio):
        return ELEMS if pin % align == 0 and pio % align == 0 else ELEMS_U

    if esz == 32:
        # wide: the LDS-transpose tile is 512 elements (256 lanes x 2); one tile +- one element
        for pin, pio in ((0, 0), (16, 16), (0, 16)):
            for n in (1, 511, 512, 513):
                add(n, pin, pio, WIDE_TILE)
        for pin, pio in ((8, 0), (0, 8), (8, 8), (1, 1)):
            for n in (1, 5, 513):
                add(n, pin, pio, WIDE_ELEMS)
        return [(n, pin, pio, k) for (n, pin, pio), k in out.items()]

    # ---- lean / full: equal alignment mod 16, the grid at every phase
    maxtail = 16 - esz                                   # bytes
    for pio in (0, 16, 4096, 8192 - 16, TILE - 16, esz, TILE - 16 + esz):
        head = -pio % 16
        s = (pio + head) % TILE                          # the vector region's phase on the grid
        to_edge = TILE - s                               # bytes to the first grid boundary
        lens = []                                        # (vector bytes, tail bytes)
        if to_edge > 48:
            lens.append((48, 0))                         # wholly inside tile 0
        lens.append((to_edge, 0))                        # ends exactly on a grid boundary
        lens.append((to_edge - 16 if to_edge > 16 else to_edge + TILE - 16, 0))     # 16 B before one
        lens.append((to_edge + 16, 0))                   # 16 B after one
        lens.append((to_edge + TILE, maxtail))           # exactly two grid tiles, and a tail
        if esz < 16:
            lens.append((0, esz))                        # no vector region: head and tail only
            lens.append((0, maxtail))
        for shift in (0, 4096, TILE - 16):
            pin = pio + shift                            # same phase mod 16, another mod 16 KiB
            for v, tail in lens:
                add((head + v + tail) // esz, pin, pio, FULL if head or tail else LEAN)
            add(1, pin, pio, LEAN if esz == 16 else FULL)

    # ---- shift: inbuf at another offset mod 16, inout element-aligned, from two tiles up.
    # The deltas the type's alignment allows (the 16 B-aligned long double has none:
    # there inbuf sits 4 or 8 bytes off its natural alignment, as
    # test_relative_misalignment_tile_path runs it).  The last tile's length `left`
    # is a multiple of 16, so (delta + left) mod 16 is delta itself: 1 and 15 come
    # with the byte type, 0 cannot occur; the in-descriptor's round-up is run at
    # last tiles of 16 B, a whole tile and one vector less than a tile.
    deltas = [d for d in range(1, 16) if d % align == 0] or [4, 8]
    heads = [0, esz] if esz < 16 else [0]
    for pio in heads:
        for d in deltas:
            for nbytes in (2 * TILE - esz, 2 * TILE, 2 * TILE + esz):
                add(nbytes // esz, pio + d, pio, SHIFT if nbytes >= 2 * TILE else elems_kind(pio + d, pio))
        for d in (deltas[0], deltas[-1]):
            head = -pio % 16
            for v in (2 * TILE + 16, 3 * TILE - 16):
                add((head + v) // esz, pio + d, pio, SHIFT)

    # ---- elements: small counts of unequal alignment; the 16 B classes of 8 B
    # alignment at offset 8 (no tile or shift plan at any count); unnatural offsets
    past = 2 * TILE // esz + 3
    for pin, pio in ((esz % 16 or 8, 0), (0, esz % 16 or 8)):
        for n in (1, 5, 257, 1001):
            add(n, pin, pio, elems_kind(pin, pio))
    if esz == 16 and align == 8:
        for n in (1, 5, 1001, past):
            add(n, 8, 8, ELEMS)
            add(n, 24, 8, ELEMS)
    if align > 1:
        for pin, pio in ((1, 1), (3, 3), (3, 1)):
            for n in (1, 5, 1001, past):
                add(n, pin, pio, ELEMS_U)
    return [(n, pin, pio, k) for (n, pin, pio), k in out.items()]


class Arena:
    """A device allocation filled with 0xA5 around one payload; `base` is its
    first 16 KiB boundary."""

    def __init__(self, torch, nbytes):
        self.torch = torch
        self.t = torch.empty(nbytes + TILE, dtype=torch.uint8, device="cuda")
        self.skew = -self.t.data_ptr() % TILE
        self.base = self.t.data_ptr() + self.skew
        self.room = nbytes

    def place(self, off, payload):
        assert off >= TILE and off + payload.size + TILE <= self.room, (off, payload.size, self.room)
        self.t.fill_(FILL)
        self.lo, self.hi = self.skew + off, self.skew + off + payload.size
        self.restore(payload)
        return self.base + off

    def restore(self, payload):
        self.t[self.lo:self.hi].copy_(self.torch.from_numpy(payload))

    def check(self, what):
        """The payload's bytes, after asserting that nothing around it was written."""
        self.torch.cuda.synchronize()
        whole = self.t.cpu().numpy()
        bad = np.nonzero(whole[:self.lo] != FILL)[0].tolist() + \
            (self.hi + np.nonzero(whole[self.hi:] != FILL)[0]).tolist()
        assert not bad, (f"{what}: guard bytes written at payload offsets {[i - self.lo for i in bad[:8]]} "
                         f"(payload {self.hi - self.lo} B)")
        return whole[self.lo:self.hi]


class Counters:
    def __init__(self, mpi, torch):
        self.lib = mpi.load()
        self.lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
        self.lib.MPIR_Hip_direct_kernarg_writes.restype = ctypes.c_uint64
        # 1: the nonce protocol (hits and misses as described); 2: direct, every write read back
        self.state = self.lib.MPIR_Hip_direct_prepare(torch.cuda.current_device())

    def read(self):
        return self.lib.MPIR_Hip_direct_dispatches(), self.lib.MPIR_Hip_direct_kernarg_writes()


def run_shape(mpi, orc, torch, ctr, ain, aio, stream, op, t, n, off_in, off_io, kind, keep_all, paths):
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    rng = np.random.default_rng([n, off_in, off_io])
    a = T.to_bytes(T.gen(t, n, rng, op))          # inout
    b = T.to_bytes(T.gen(t, n, rng, op))          # in
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, n, dt, o) == 0
    pin, pio = ain.place(off_in, b), aio.place(off_io, a)
    what = f"{op} {t} n={n} in=+{off_in % TILE} io=+{off_io % TILE}"
    info = mpi.plan_info(pin, pio, n, dt, o)
    assert info["kind"] == kind, f"{what}: aimed at {mpi.PLAN_NAMES[kind]}, the planner says {info}"
    if kind in (LEAN, FULL, SHIFT, WIDE_TILE):
        assert info["keep"] == (info["vbytes"] if keep_all else 0), f"{what}: store policy {info}"
    direct = kind < WIDE_TILE
    for path in paths:
        if path != paths[0]:
            aio.restore(a)
        torch.cuda.synchronize()
        d0, w0 = ctr.read()
        if path == "stream":
            rc = mpi.reduce_local_stream(pin, pio, n, dt, o, stream.cuda_stream)
            stream.synchronize()
        else:
            rc = mpi.reduce_local(pin, pio, n, dt, o)
        assert rc == 0, f"{what} {path}: {mpi.error_string(rc)}"
        d1, w1 = ctr.read()
        got = aio.check(f"{what} {path} inoutbuf")
        assert np.array_equal(ain.check(f"{what} {path} inbuf"), b), f"{what} {path}: inbuf modified"
        if not same(got, want, t):
            pytest.fail(f"{what} {path} ({mpi.PLAN_NAMES[kind]}):\n" + explain(got, want, a, b, T.elem_size(t)))
        if ctr.state in (1, 2):
            assert d1 - d0 == (1 if direct and path != "stream" else 0), f"{what} {path}: direct dispatches {d1 - d0}"
        if ctr.state == 1 and direct and path != "stream":
            # fresh arguments are written into a kernarg slot (checked kernel); the
            # repeat finds them verified there (unchecked kernel)
            assert w1 - w0 == (1 if path == "miss" else 0), f"{what} {path}: kernarg writes {w1 - w0}"


@pytest.mark.parametrize("store", ["nt", "sc1"])
@pytest.mark.parametrize("op,t,align", CASES, ids=CASE_IDS)
def test_plan_edges(mpi, orc, cuda, op, t, align, store):
    torch = cuda
    lib = mpi.load()
    ctr = Counters(mpi, torch)
    # payloads sit one to three tiles into the arena in the first sweep, three
    # tiles further in the second: no argument set repeats between them
    slot = TILE * (1 if store == "nt" else 4)
    room = 12 * TILE
    ain, aio = Arena(torch, room), Arena(torch, room)
    stream = torch.cuda.Stream()
    prev = lib.MPIR_Hip_set_keep_min_bytes(0) if store == "sc1" else None
    try:
        for n, pin, pio, kind in shapes(t, align):
            run_shape(mpi, orc, torch, ctr, ain, aio, stream, op, t, n, slot + pin, slot + pio, kind,
                      store == "sc1", ("miss", "hit", "stream"))
    finally:
        if prev is not None:
            lib.MPIR_Hip_set_keep_min_bytes(prev)


STRIDE = [("MPI_SUM", "MPI_FLOAT", 1, 1, ELEMS_U), ("MPI_SUM", "MPI_C_DOUBLE_COMPLEX", 8, 8, ELEMS),
          ("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT", 0, 8, WIDE_ELEMS)]


@pytest.mark.parametrize("op,t,pin,pio,kind", STRIDE, ids=[f"{o}-{t}" for o, t, *_ in STRIDE])
def test_element_kernels_take_a_third_stride(mpi, orc, cuda, op, t, pin, pio, kind):
    """The grid-stride element kernels cap their grid at 4096 workgroups
    (1,048,576 elements per stride): 2 x 1,048,576 + 4099 elements make every
    workgroup take a second stride and some a third -- through the direct
    dispatch (its `stride` argument and in_grid) and through the HIP launch."""
    torch = cuda
    ctr = Counters(mpi, torch)
    room = STRIDE_COUNT * T.elem_size(t) + 3 * TILE
    ain, aio = Arena(torch, room), Arena(torch, room)
    assert mpi.plan_info(ain.base + TILE + pin, aio.base + TILE + pio, STRIDE_COUNT, mpi.DATATYPES[t],
                         mpi.OPS[op])["groups"] == 4096
    run_shape(mpi, orc, torch, ctr, ain, aio, torch.cuda.Stream(), op, t, STRIDE_COUNT, TILE + pin, TILE + pio, kind,
              False, ("miss", "stream"))
