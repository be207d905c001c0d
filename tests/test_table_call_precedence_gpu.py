"""Which refusal wins when a table call breaks two rules at once.

The other GPU tests check each refusal of the table calls (MPIR_Hip_reduce_indexed,
_ragged, _fetch_ragged, _indexed_ordered, _fetch_indexed_ordered and
MPIR_Hip_cas_indexed_ordered) alone.  The calls do not make their checks in the
same order -- the indexed family looks at the bases before the tables, the ragged
family reads the host tables first -- and that order decides which error a
caller sees.  Every case here breaks two rules, names the one the shim must
report, and checks that nothing was written: a refused call has enqueued nothing.

The shim is called through ctypes, synchronously, on a few dozen blocks of a few
elements.  "A block in host memory" is a displacement computed from a host
array's address (as test_indexed_gpu.py::test_no_partial_work makes one): the
library looks the address up and dereferences nothing.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EBUFFER, EARG = 1, 5
NB, BL, UNIT = 32, 4, 16            # 32 blocks of 4 floats, displacements in units of a block's 16 bytes


class Bufs:
    def __init__(self, torch, mpi):
        self.torch = torch
        self.lib = mpi.load()
        self.sum, self.f32, self.i64 = mpi.MPI_SUM & 0xF, mpi.ELEM["F32"], mpi.ELEM["I64"]
        rng = np.random.default_rng(23)
        # the target arena (blocks at every other slot, so the gaps show a stray
        # write), the packed origin side, and two more packed buffers (fetchbuf or
        # result, and the compare-and-swap's compare)
        self.dev = [torch.from_numpy(rng.integers(0, 255, n, dtype=np.uint8)).cuda() for n in (1 << 16, 4096, 4096, 4096)]
        self.snap = [t.clone() for t in self.dev]
        self.io, self.inp, self.fetch, self.cmp = (t.data_ptr() for t in self.dev)
        assert self.io % 16 == 0
        self.host = np.full(8192, 0x5A, np.uint8)
        self.hptr = (self.host.ctypes.data + 1024 + 15) // 16 * 16      # 16 bytes apart from any device base
        # a sound output table; one whose highest block lies in host memory; one whose
        # product overflows; one with equal entries that are not neighbours
        self.tio = (rng.permutation(NB).astype(np.int64)) * 2
        self.far = self.tio.copy()
        self.far[np.argmax(self.tio)] = (self.hptr - self.io) // UNIT
        self.far_in = np.arange(NB, dtype=np.int64)
        self.far_in[NB - 1] = (self.hptr - self.inp) // UNIT
        self.big = self.tio.copy()
        self.big[7] = 1 << 60
        self.dup = self.tio.copy()
        self.dup[2] = self.dup[0]
        assert abs(self.hptr - self.io) > 1 << 20 and (self.hptr - self.io) % UNIT == 0 and (self.hptr - self.inp) % UNIT == 0
        self.inside = self.io + UNIT                # in the gap after slot 0: inside the targets' extent
        assert self.tio.min() == 0 and self.tio.max() * UNIT > UNIT + NB * BL * 4
        # ragged pieces of 0..4 floats, and a starts that does not end at count
        lens = rng.integers(0, BL + 1, NB)
        lens[np.argmin(self.tio)] = lens[np.argmax(self.tio)] = BL      # the extreme pieces are not empty
        self.starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        self.count = int(self.starts[-1])
        self.bad_starts = self.starts.copy()
        self.bad_starts[-1] += 1
        self.order = np.argsort(self.tio, kind="stable").astype(np.int32)
        self.bad_order = np.zeros(NB, np.int32)     # not a permutation
        self.tables = [x.copy() for x in self._tables()]

    def _tables(self):
        return (self.tio, self.far, self.far_in, self.big, self.dup, self.starts, self.bad_starts, self.order, self.bad_order)

    def untouched(self, what):
        self.torch.cuda.synchronize()
        for t, s in zip(self.dev, self.snap):
            assert self.torch.equal(t, s), f"{what}: device memory written by a refused call"
        assert (self.host == 0x5A).all(), f"{what}: host memory written by a refused call"
        for t, s in zip(self._tables(), self.tables):
            assert np.array_equal(t, s), f"{what}: a table written by a refused call"


@pytest.fixture(scope="module")
def bufs(mpi, cuda):
    return Bufs(cuda, mpi)


def p(a):
    return a.ctypes.data


def indexed(b, inbuf, tin, io, tio):
    return b.lib.MPIR_Hip_reduce_indexed(inbuf, tin, io, tio, UNIT, NB, BL, b.sum, b.f32, None, 1)


def ragged(b, inbuf, tio, starts):
    return b.lib.MPIR_Hip_reduce_ragged(inbuf, None, b.io, tio, starts, UNIT, NB, b.count, b.sum, b.f32, None, 1)


def fetch_ragged(b, fetch, tio, starts):
    return b.lib.MPIR_Hip_reduce_fetch_ragged(b.inp, b.io, tio, fetch, starts, UNIT, NB, b.count, b.sum, b.f32, None, 1)


def ordered(b, tin, tio, order):
    return b.lib.MPIR_Hip_reduce_indexed_ordered(b.inp, tin, b.io, tio, order, UNIT, NB, BL, b.sum, b.f32, None, 1)


def fetch_ordered(b, fetch):
    return b.lib.MPIR_Hip_reduce_fetch_indexed_ordered(b.inp, None, b.io, p(b.dup), fetch, None, UNIT, NB, BL, b.sum, b.f32,
                                                       None, 1)


def cas(b, result):
    # 32 longs at displacements of 8 bytes: origin, compare, target, displs, result, order
    return b.lib.MPIR_Hip_cas_indexed_ordered(b.inp, b.cmp, b.io, p(b.dup), result, None, 8, NB, b.i64, None, 1)


# (call, what the call breaks, the refusal that wins, the call itself)
CASES = [
    ("indexed", "in_displs overflows, io_displs' highest block in host memory", EARG,
     lambda b: indexed(b, b.inp, p(b.big), b.io, p(b.far))),
    ("indexed", "in_displs' last block in host memory, io_displs overflows", EBUFFER,
     lambda b: indexed(b, b.inp, p(b.far_in), b.io, p(b.big))),
    ("indexed", "host inoutbuf, in_displs overflows", EBUFFER,
     lambda b: indexed(b, b.inp, p(b.big), b.hptr, None)),
    ("ragged", "host inbuf, starts does not end at count", EARG,
     lambda b: ragged(b, b.hptr, p(b.tio), p(b.bad_starts))),
    ("ragged", "host inbuf, io_displs overflows", EARG,
     lambda b: ragged(b, b.hptr, p(b.big), p(b.starts))),
    ("fetch_ragged", "host fetchbuf, starts does not end at count", EARG,
     lambda b: fetch_ragged(b, b.hptr, p(b.tio), p(b.bad_starts))),
    ("fetch_ragged", "both tables sound host tables, fetchbuf inside the pieces' extent", EBUFFER,
     lambda b: fetch_ragged(b, b.inside, p(b.tio), p(b.starts))),
    ("indexed_ordered", "io_displs' highest block in host memory, order not a permutation", EBUFFER,
     lambda b: ordered(b, None, p(b.far), p(b.bad_order))),
    ("indexed_ordered", "in_displs overflows, order not a permutation", EARG,
     lambda b: ordered(b, p(b.big), p(b.tio), p(b.bad_order))),
    ("fetch_indexed_ordered", "no order, equal entries not adjacent, fetchbuf inside the targets' extent", EBUFFER,
     lambda b: fetch_ordered(b, b.inside)),
    ("fetch_indexed_ordered", "no order, equal entries not adjacent, fetchbuf clear of the extent", EARG,
     lambda b: fetch_ordered(b, b.fetch)),
    ("cas", "no order, equal entries not adjacent, result inside the targets' extent", EBUFFER,
     lambda b: cas(b, b.io + 8)),
    ("cas", "no order, equal entries not adjacent, result clear of the extent", EARG,
     lambda b: cas(b, b.fetch)),
]


@pytest.mark.parametrize("call,breaks,wins,run", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_the_earlier_check_wins(bufs, call, breaks, wins, run):
    rc = run(bufs)
    print(f"{call}: {breaks}: rc {rc}, expected {wins}")
    assert rc == wins, f"{call}: {breaks}: shim returned {rc}"
    bufs.untouched(f"{call}: {breaks}")
