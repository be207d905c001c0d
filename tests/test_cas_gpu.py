"""MPIX_Compare_and_swap_indexed_ordered on the GPU: count compare-and-swaps of one
element each, in table order.

Expected values come from the model below, a plain loop over k: result[k] is what
entry k's target holds, and where that equals compare[k] the target takes
origin[k].  Equality is the reference's MPIR_Compare_equal
(src/mpi/rma/rmatypeutil.c:53-76): `==` on the C type of every type
MPIR_Type_is_rma_atomic accepts (:23-43) -- integers, _Bool, and for MPI_BYTE
unsigned char (:65) -- which is equality of the element's bytes, so the model
compares the elements as unsigned integers of their size.

Every operand sits in its own 0xA5 arena (test_indexed_gpu.Arena), result
prefilled with the complement of the expected bytes.  After each call the targets
and every result[k] must be byte-equal to the model's, every guard byte of all
four arenas still 0xA5, origin, compare and the tables unchanged.  Each shape
with a table runs synchronously with device tables, on a stream with device
tables, and synchronously with host tables; a contiguous target, which has no
table, synchronously and on a stream.

Values come from a three-word alphabet per size: w, w ^ 1 and w ^ (1 << (bits -
1)), so a compare that ignores the top or the bottom of the element (32 bits of
an 8-byte type) sees equal where the model does not.  Before any GPU work the
model must show between 20 % and 60 % of the entries swapping and, where the
shape has at least 10 targets with repeats, at least 10 targets with a swap after
a failure and 10 with a failure after a swap.

Every address a kernel forms here stays inside its arena.
"""
import numpy as np
import pytest

from test_indexed_gpu import Arena, slots
from test_indexed_ordered_gpu import build_orders, repeated
from test_plan_edges_gpu import TILE

pytestmark = pytest.mark.gpu

EMPTY, CONTIG_TILE, CONTIG_ELEMS, INDEXED = range(4)
WAYS = ("sync", "stream", "host-tables")
SIZE = {"MPI_SIGNED_CHAR": 1, "MPI_SHORT": 2, "MPI_INT": 4, "MPI_LONG": 8, "MPI_UINT64_T": 8, "MPI_C_BOOL": 1,
        "MPI_CHAR": 1, "MPI_BYTE": 1, "MPI_UNSIGNED_CHAR": 1}
BY_SIZE = {1: "MPI_SIGNED_CHAR", 2: "MPI_SHORT", 4: "MPI_INT", 8: "MPI_LONG"}
W = 0x5A3C96E17B2D48F1


def alphabet(t):
    if t == "MPI_C_BOOL":
        return [0, 1]
    bits = 8 * SIZE[t]
    w = W & ((1 << bits) - 1)
    return [w, w ^ 1, w ^ (1 << (bits - 1))]


def model(tv, dst, ov, cv):
    """The targets after entries 0 .. count - 1 in that order, what each entry's target
    held just before it, and which entries swapped (values: unsigned integers of the
    element's size)"""
    want = tv.tolist()
    res, swapped = [], []
    for j, o, c in zip(dst.tolist(), ov.tolist(), cv.tolist()):
        res.append(want[j])
        swapped.append(want[j] == c)
        if want[j] == c:
            want[j] = o
    return np.array(want, tv.dtype), np.array(res, tv.dtype), np.array(swapped, bool)


def transitions(dst, swapped):
    """targets that see a swap after a failure, and a failure after a swap"""
    up, down = set(), set()
    last = {}
    for j, s in zip(dst.tolist(), swapped.tolist()):
        if j in last and last[j] != s:
            (up if s else down).add(j)
        last[j] = s
    return len(up), len(down)


def rows(v):
    return np.ascontiguousarray(v).view(np.uint8).reshape(len(v), v.dtype.itemsize)


class Case:
    """Operands of one shape: the four arenas, the tables, the model's outcome.
    tab: the displacement table in units of `unit` bytes, or None (contiguous)."""

    def __init__(self, mpi, torch, stream, t, tab, unit, count, phases=(0, 0, 0, 0), seed=0, order=True, repeats=True):
        self.mpi, self.torch, self.stream, self.t = mpi, torch, stream, t
        self.dt, self.n, self.unit, self.count = mpi.DATATYPES[t], SIZE[t], unit, count
        n = self.n
        u = np.dtype(f"uint{8 * n}")
        rng = np.random.default_rng([seed, count, n])
        letters = np.array(alphabet(t), u)
        packed = np.arange(count, dtype=np.int64) * n
        if tab is None:
            self.tab, self.uio, self.dst = None, packed, np.arange(count)
        else:
            self.tab = np.ascontiguousarray(tab, dtype=np.int64)
            assert len(self.tab) == count
            self.uio, self.dst = np.unique(self.tab * unit, return_inverse=True)
        self.tv = letters[rng.integers(0, len(letters), len(self.uio))]
        self.ov = letters[rng.integers(0, len(letters), count)]
        self.cv = letters[rng.integers(0, len(letters), count)]
        self.want, self.rwant, self.swapped = model(self.tv, self.dst, self.ov, self.cv)
        po, pc, pt, pr = phases
        self.what = f"{t} {count} onto {len(self.uio)} unit {unit} origin=+{po} compare=+{pc} target=+{pt} result=+{pr}"
        # the model must exercise both outcomes, and both orders of them on one target
        share = self.swapped.mean()
        assert count < 20 or 0.2 <= share <= 0.6, f"{self.what}: {share:.2f} of the entries swap"
        if repeats:
            up, down = transitions(self.dst, self.swapped)
            assert up >= 10 and down >= 10, f"{self.what}: swap after failure on {up} targets, failure after swap on {down}"
        self.ao, self.ac = Arena(torch, rows(self.ov), packed, po), Arena(torch, rows(self.cv), packed, pc)
        self.at = Arena(torch, rows(self.tv), self.uio, pt)
        self.ar = Arena(torch, ~rows(self.rwant), packed, pr)
        self.dtab = None if self.tab is None else torch.from_numpy(self.tab).cuda()
        self.dorder = self.horder = None
        if order and self.tab is not None:
            self.dorder, self.horder = build_orders(mpi, torch, stream, self.tab, self.dtab, self.what)

    def sorted_displs(self):
        return self.tab if self.horder is None else self.tab[self.horder]

    def plan(self):
        return self.mpi.cas_plan_info(self.ao.ptr, self.ac.ptr, self.at.ptr, None if self.tab is None else self.dtab.data_ptr(),
                                      self.ar.ptr, None if self.dorder is None else self.dorder.data_ptr(), self.unit,
                                      self.count, self.dt)

    def call(self, way, dt=None):
        if way == "host-tables":
            tab, order = self.tab, self.horder
        else:
            tab = None if self.tab is None else self.dtab.data_ptr()
            order = None if self.dorder is None else self.dorder.data_ptr()
        self.torch.cuda.synchronize()
        rc = self.mpi.compare_and_swap_indexed_ordered(self.ao.ptr, self.ac.ptr, self.at.ptr, tab, self.ar.ptr, order,
                                                       self.unit, self.count, self.dt if dt is None else dt,
                                                       self.stream.cuda_stream if way == "stream" else 0)
        self.stream.synchronize()
        return rc

    def reset(self):
        self.at.upload()
        self.ar.upload()

    def check(self, what, want=None, rwant=None):
        """every arena against the model; returns (targets' bytes, result's bytes)"""
        want = self.want if want is None else want
        rwant = self.rwant if rwant is None else rwant
        what = f"{self.what} {what}"
        got, rgot = self.at.check(f"{what} target"), self.ar.check(f"{what} result")
        assert np.array_equal(self.ao.check(f"{what} origin"), rows(self.ov)), f"{what}: origin modified"
        assert np.array_equal(self.ac.check(f"{what} compare"), rows(self.cv)), f"{what}: compare modified"
        bad = np.nonzero((rgot != rows(rwant)).any(axis=1))[0]
        assert not bad.size, (f"{what}: result[{bad[0]}] (target {self.dst[bad[0]]}, its entries "
                              f"{np.nonzero(self.dst == self.dst[bad[0]])[0].tolist()[:20]}) is {rgot[bad[0]].tobytes().hex()}, "
                              f"the model's {rows(rwant)[bad[0]].tobytes().hex()}; {bad.size} entries differ")
        bad = np.nonzero((got != rows(want)).any(axis=1))[0]
        assert not bad.size, (f"{what}: target {bad[0]} (entries {np.nonzero(self.dst == bad[0])[0].tolist()[:20]}) is "
                              f"{got[bad[0]].tobytes().hex()}, the model's {rows(want)[bad[0]].tobytes().hex()}; "
                              f"{bad.size} targets differ")
        return got, rgot

    def untouched(self, what):
        """a refused call wrote nothing"""
        self.stream.synchronize()
        what = f"{self.what} {what}"
        assert np.array_equal(self.at.check(what), rows(self.tv)), f"{what}: target written by a refused call"
        assert np.array_equal(self.ar.check(what), ~rows(self.rwant)), f"{what}: result written by a refused call"
        assert np.array_equal(self.ao.check(what), rows(self.ov)) and np.array_equal(self.ac.check(what), rows(self.cv)), what

    def tables_unchanged(self):
        for x, h in ((self.dtab, self.tab), (self.dorder, self.horder)):
            if x is not None:
                assert np.array_equal(x.cpu().numpy(), h), f"{self.what}: a table was written"


def run(mpi, torch, stream, t, tab, unit, count, form, phases=(0, 0, 0, 0), seed=0, order=True, repeats=True, expect=None):
    """One shape every way.  Returns the case (its last outputs still in the arenas)."""
    c = Case(mpi, torch, stream, t, tab, unit, count, phases, seed, order, repeats)
    info = c.plan()
    assert info["form"] == form, f"{c.what}: the planner says {info}"
    if expect:
        expect(info, c.sorted_displs() if tab is not None else None)
    for i, way in enumerate(WAYS if tab is not None else WAYS[:2]):
        if i:
            c.reset()
        rc = c.call(way)
        assert rc == 0, f"{c.what} {way}: {mpi.error_string(rc)}"
        c.check(way)
    c.tables_unchanged()
    return c


def table(n_unit, seed=1, count=400, distinct=37, lo=0):
    """count entries onto `distinct` targets two elements apart, in units of one element"""
    return slots(distinct, seed, gap=1, lo=lo)[repeated(count, distinct, seed)] * n_unit


# ---------------------------------------------------------------- 1. types and sizes
@pytest.mark.parametrize("t", ["MPI_SIGNED_CHAR", "MPI_SHORT", "MPI_INT", "MPI_LONG", "MPI_UINT64_T", "MPI_C_BOOL", "MPI_CHAR"])
def test_400_entries_onto_37_targets(mpi, cuda, t):
    n = SIZE[t]

    def one(info, sorted_displs):
        assert info["launches"] == 1 and info["groups"] == 1 and len(np.unique(sorted_displs)) == 37, info

    run(mpi, cuda, cuda.cuda.Stream(), t, table(1), n, 400, INDEXED, phases=(n, 2 * n, 3 * n, 4 * n), seed=1, expect=one)


def test_byte_is_compared_as_unsigned_char(mpi, cuda):
    """MPI_BYTE is in MPIR_Compare_equal's BYTE group (rmatypeutil.c:65, unsigned char):
    entries whose compare value is byte-equal to the target swap, and the outcome
    is MPI_UNSIGNED_CHAR's on the same operands."""
    stream = cuda.cuda.Stream()
    c = run(mpi, cuda, stream, "MPI_BYTE", table(1, seed=2), 1, 400, INDEXED, phases=(1, 2, 3, 5), seed=2)
    assert c.swapped.sum() >= 80 and not np.array_equal(c.want, c.tv)
    got = c.check("MPI_BYTE")
    c.reset()
    rc = c.call("sync", dt=mpi.DATATYPES["MPI_UNSIGNED_CHAR"])
    assert rc == 0, mpi.error_string(rc)
    same = c.check("MPI_UNSIGNED_CHAR")
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[1], same[1])


# ---------------------------------------------------------------- 2. edges of the run loop
@pytest.mark.parametrize("t", ["MPI_INT", "MPI_LONG"])
def test_run_loop_edges(mpi, cuda, t):
    """Runs of 1, 2, A, A + 1, 2A and 2A + 1 (A = kCasAhead), the first at sorted
    position 0, the last ending at the table's end, in a shuffled table; 300
    entries all on one target; no repeats at all."""
    n = SIZE[t]
    stream = cuda.cuda.Stream()
    A = mpi.cas_plan_info(1 << 32, 1 << 33, 1 << 40, 1 << 44, 1 << 41, 0, n, 1, mpi.DATATYPES[t])["ahead"]
    assert A >= 1
    lens = [1, 2, A, A + 1, 2 * A, 2 * A + 1] * 6 + [2 * A + 1, 2 * A, A + 1, A, 2, 1] * 6
    srt = np.repeat(np.arange(len(lens), dtype=np.int64) * 3 - 40, lens)      # negative ones too
    tab = np.random.default_rng(3).permutation(srt)

    def runs(info, sorted_displs):
        _, counts = np.unique(sorted_displs, return_counts=True)
        assert counts.tolist() == lens and np.array_equal(sorted_displs, srt)
        assert sorted_displs[0] != sorted_displs[1] and sorted_displs[-1] != sorted_displs[-2]     # runs of 1 at both ends

    run(mpi, cuda, stream, t, tab, n, len(tab), INDEXED, phases=(0, n, 2 * n, 3 * n), seed=3, expect=runs)
    # ... and with runs of 2A + 1 at both ends
    lens = [2 * A + 1, 1, 2, A, A + 1, 2 * A] * 6 + [2 * A + 1]
    tab = np.random.default_rng(4).permutation(np.repeat(np.arange(len(lens), dtype=np.int64) * 3 - 40, lens))
    run(mpi, cuda, stream, t, tab, n, len(tab), INDEXED, seed=4,
        expect=lambda i, s: (s[0] == s[2 * A] != s[2 * A + 1] and s[-1] == s[-1 - 2 * A] != s[-2 - 2 * A]) or
        pytest.fail("runs at the ends"))
    run(mpi, cuda, stream, t, np.full(300, 7, np.int64), n, 300, INDEXED, seed=5, repeats=False)
    run(mpi, cuda, stream, t, slots(400, 6, gap=1), n, 400, INDEXED, seed=6, repeats=False)
    run(mpi, cuda, stream, t, np.array([5], np.int64), n, 1, INDEXED, seed=7, repeats=False)


def test_a_run_across_a_workgroup_boundary(mpi, cuda):
    def crossing(info, sorted_displs):
        per = info["per"]
        assert info["groups"] == 2 and info["launches"] == 1 and len(sorted_displs) > per, info
        assert sorted_displs[per - 1] == sorted_displs[per]

    per = mpi.cas_plan_info(1 << 32, 1 << 33, 1 << 40, 1 << 44, 1 << 41, 0, 4, 1, mpi.MPI_INT)["per"]
    run(mpi, cuda, cuda.cuda.Stream(), "MPI_INT", table(1, seed=8, count=per + 400), 4, per + 400, INDEXED, seed=8,
        expect=crossing)


def test_a_run_across_a_launch_boundary(mpi, cuda):
    """The per-launch workgroup cap lowered to 1: three launches, runs across both boundaries."""
    lib = mpi.load()
    assert lib.MPIR_Hip_strided_test_max_groups(1) == 0
    try:
        def crossing(info, sorted_displs):
            rpl = info["rows_per_launch"]
            assert info["launches"] == 3 and rpl == info["per"] and info["groups"] == 3, info
            assert all(sorted_displs[p - 1] == sorted_displs[p] for p in (rpl, 2 * rpl))

        per = mpi.cas_plan_info(1 << 32, 1 << 33, 1 << 40, 1 << 44, 1 << 41, 0, 8, 1, mpi.MPI_LONG)["per"]
        run(mpi, cuda, cuda.cuda.Stream(), "MPI_LONG", table(1, seed=9, count=2 * per + 300, distinct=61), 8, 2 * per + 300,
            INDEXED, seed=9, expect=crossing)
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 1


# ---------------------------------------------------------------- 3. alignment and signs
@pytest.mark.parametrize("t", ["MPI_SHORT", "MPI_INT", "MPI_LONG"])
def test_byte_displacements_odd_and_negative(mpi, cuda, t):
    """disp_unit 1: every target at an odd byte offset, half of them below the base;
    the packed buffers at odd phases too."""
    n = SIZE[t]
    tab = table(2 * n, seed=10, lo=-18) + 1
    assert (tab % 2 == 1).all() and (tab < 0).sum() > 100 and (tab > 0).sum() > 100
    run(mpi, cuda, cuda.cuda.Stream(), t, tab, 1, 400, INDEXED, phases=(1, 3, 0, 5), seed=10)


@pytest.mark.parametrize("t", ["MPI_SIGNED_CHAR", "MPI_LONG"])
def test_order_null(mpi, cuda, t):
    """order NULL: equal entries adjacent (runs of 1 and 3, the runs themselves in no
    order), byte-equal to the call with the built order; and no repeats at all."""
    n = SIZE[t]
    stream = cuda.cuda.Stream()
    adj = np.concatenate([[s] * (1 if s % 2 else 3) for s in slots(200, 11, gap=1).tolist()]).astype(np.int64)
    assert not (np.diff(adj) >= 0).all()
    c = run(mpi, cuda, stream, t, adj, n, len(adj), INDEXED, seed=11)
    built = c.check("built order")
    c.dorder = c.horder = None
    assert c.plan()["form"] == INDEXED
    for way in WAYS:
        c.reset()
        rc = c.call(way)
        assert rc == 0, f"{c.what} order NULL {way}: {mpi.error_string(rc)}"
        nul = c.check(f"order NULL {way}")
        assert np.array_equal(nul[0], built[0]) and np.array_equal(nul[1], built[1])
    c.tables_unchanged()
    run(mpi, cuda, stream, t, slots(400, 12, gap=1), n, 400, INDEXED, seed=12, order=False, repeats=False)


# ---------------------------------------------------------------- 4. contiguous target
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_contiguous_target(mpi, cuda, n):
    """target_displs NULL.  Counts around 16 bytes and around one and two 16 KiB
    tiles with all four pointers on the grid (the tile form); one phase with a
    head and a tail (the tile form); origin, compare and result in turn off that
    phase (the element form)."""
    t = BY_SIZE[n]
    stream = cuda.cuda.Stream()
    per16, pert = 16 // n, TILE // n
    counts = sorted({1, per16 - 1, per16, per16 + 1, pert - 1, pert, pert + 1, 2 * pert + 3} - {0})
    for count in counts:
        run(mpi, cuda, stream, t, None, n, count, CONTIG_TILE, seed=count, repeats=False)
    ph = 24                                 # 8 bytes of head elements up to the next multiple of 16
    count = 2 * pert + 3 + (n == 8)         # ... and a ragged end after them

    def head_and_tail(info, _):
        assert info["nhead"] == 8 // n and info["ntail"] == (count * n - 8) % 16 // n > 0 and info["groups"] == 3, info

    run(mpi, cuda, stream, t, None, n, count, CONTIG_TILE, phases=(ph, ph + 32, ph, ph + TILE), seed=13, repeats=False,
        expect=head_and_tail)
    off = min(n, 4)                         # (an 8-byte element's buffer then sits off its own alignment too)
    for k in (0, 1, 3):
        phases = [ph] * 4
        phases[k] += off
        run(mpi, cuda, stream, t, None, n, count, CONTIG_ELEMS, phases=tuple(phases), seed=14 + k, repeats=False,
            expect=lambda i, _: i["groups"] == -(-count * n // TILE) or pytest.fail(str(i)))


# ---------------------------------------------------------------- 5. graph
def test_captured_in_a_graph(mpi, cuda):
    """Captured on one stream and replayed twice: the outcome is the model applied twice."""
    torch = cuda
    s = torch.cuda.Stream()
    c = Case(mpi, torch, s, "MPI_INT", table(1, seed=20), 4, 400, seed=20)
    twice, rsecond, sw = model(c.want, c.dst, c.ov, c.cv)
    assert not np.array_equal(rsecond, c.rwant) and sw.any()
    assert c.plan()["launches"] == 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.compare_and_swap_indexed_ordered(c.ao.ptr, c.ac.ptr, c.at.ptr, c.dtab.data_ptr(), c.ar.ptr,
                                                        c.dorder.data_ptr(), 4, 400, c.dt, cs) == 0
    torch.cuda.synchronize()
    c.untouched("captured: recorded, not run")
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    c.check("replayed twice", want=twice, rwant=rsecond)
    c.tables_unchanged()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_with_device_operands_write_nothing(mpi, cuda):
    torch = cuda
    stream = torch.cuda.Stream()
    count = 400
    c = Case(mpi, torch, stream, "MPI_INT", table(1, seed=21), 4, count, seed=21)
    call = mpi.compare_and_swap_indexed_ordered
    tab, horder, dtab, dorder = c.tab, c.horder, c.dtab.data_ptr(), c.dorder.data_ptr()
    po, pc, pt, pr = c.ao.ptr, c.ac.ptr, c.at.ptr, c.ar.ptr

    def refused(rc, cls, what):
        assert mpi.error_class(rc) == cls, f"{what}: {mpi.error_string(rc)}"
        c.untouched(what)

    cs = stream.cuda_stream
    refused(call(po, pc, pt, dtab, pr, horder, 4, count, c.dt, cs), mpi.MPI_ERR_BUFFER, "host order on a stream")
    refused(call(po, pc, pt, tab, pr, dorder, 4, count, c.dt, cs), mpi.MPI_ERR_BUFFER, "host target_displs on a stream")
    # a host order that is no stable sort of the host table
    twice = horder.copy()
    twice[7] = twice[8]
    wild = horder.copy()
    wild[3] = count
    neg = horder.copy()
    neg[3] = -1
    p = int(np.nonzero(tab[horder][1:] != tab[horder][:-1])[0][0])     # positions p, p + 1: two different targets
    desc = horder.copy()
    desc[[p, p + 1]] = desc[[p + 1, p]]
    q = int(np.nonzero(tab[horder][1:] == tab[horder][:-1])[0][0])     # positions q, q + 1: one target
    tie = horder.copy()
    tie[[q, q + 1]] = tie[[q + 1, q]]
    for bad, why in ((twice, "a repeated entry"), (wild, "an entry == count"), (neg, "a negative entry"),
                     (desc, "a descending pair"), (tie, "a tie out of table order")):
        refused(call(po, pc, pt, tab, pr, bad, 4, count, c.dt), mpi.MPI_ERR_ARG, f"host order with {why}")
    # order NULL promises that equal entries are adjacent
    apart = slots(count, 22, gap=1)
    apart[count - 1] = apart[3]
    refused(call(po, pc, pt, apart, pr, None, 4, count, c.dt), mpi.MPI_ERR_ARG,
            "order NULL with a non-adjacent repeat in a host table")
    # result inside the targets' span, which only a host table shows
    lo, hi = int(c.uio.min()), int(c.uio.max()) + 4
    for d in (lo, lo - 4 * count + 1, hi - 1, (lo + hi) // 2 // 4 * 4):
        refused(call(po, pc, pt, tab, pt + d, horder, 4, count, c.dt), mpi.MPI_ERR_BUFFER, f"result in the targets' span at {d}")
    refused(call(po, pc, pt, dtab, pr, dorder, 4, count, mpi.MPI_FLOAT), mpi.MPI_ERR_TYPE, "MPI_FLOAT")
    refused(call(po, pc, pt, None, pr, dorder, 4, count, c.dt), mpi.MPI_ERR_ARG, "device order without target_displs")
    # a device order with out-of-range values: undefined result, but the call returns
    # and writes no guard byte of any arena
    broken = horder.copy()
    broken[5], broken[9], broken[count - 1] = count + 1000, -3, 2 ** 31 - 1
    dbroken = torch.from_numpy(broken).cuda()
    torch.cuda.synchronize()
    rc = call(po, pc, pt, dtab, pr, dbroken.data_ptr(), 4, count, c.dt)
    assert rc == 0, mpi.error_string(rc)
    c.at.check("device order out of range: target guards")
    c.ar.check("device order out of range: result guards")
    assert np.array_equal(c.ao.check("origin"), rows(c.ov)) and np.array_equal(c.ac.check("compare"), rows(c.cv))
    # and the valid order on the same operands still gives the model's
    c.reset()
    assert c.call("sync") == 0
    c.check("valid order")
    c.tables_unchanged()
