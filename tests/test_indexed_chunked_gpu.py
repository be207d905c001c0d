"""MPIX_Reduce_local_indexed_chunked on the GPU: the ordered call's operands with
the blocks of one target folded in chunks of 64 counted from the run's first
block, then the partials folded into the target.  The expected bits are the
definition composed from the oracle's MPI_Reduce_local: one partial row per
chunk (a byte copy of the chunk's first input block, the rest reduced into it),
then the partials into the target row in order (bit-exact, test_parity_gpu.same's
complex-NaN rule).

The arenas are test_indexed_gpu's: 0xA5 around and between the blocks.  Every
shape runs three ways: synchronously with device tables and the library's
scratch, on a torch stream with device tables and the caller's work, and
synchronously with host tables.  After each run every target must equal the
definition's, every guard byte must still be 0xA5, the input arena and all four
tables must be unchanged, and the caller's work past its reported size must be
unwritten.  The runstart table comes from MPIX_Reduce_local_runs on device
tables and must equal the numpy statement of its definition.

For the fp32 chunk-edge shapes the data must be able to tell: before the GPU
runs, the expected bits must differ from the ordered call's, from chunks cut at
sorted positions instead of run-relative ones, and from chunk lengths 32 and 128.

Every address a kernel forms here stays inside its arena or the work.
"""
import ctypes

import numpy as np
import pytest

import _types as T
from test_indexed_chunked_cpu import runs_of
from test_indexed_gpu import Arena, slots, threshold
from test_indexed_ordered_gpu import oracle_rows
from test_parity_gpu import explain, same
from test_plan_edges_gpu import FILL, TILE

pytestmark = pytest.mark.gpu

EMPTY, SINGLE, WIDE, NARROW_VEC, NARROW_ELEMS = range(5)
FORMS = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
WAYS = ("sync", "stream", "host-tables")
TAIL = 4096                     # bytes of a caller's work allocation past the reported size
C = 64


def chunked_rows(orc, a, b, src, dst, bl, dt, o, chunk=C, by_position=False, descending=False):
    """a's rows (one per distinct target, in ascending displacement) after the
    definition: per run, a partial per chunk of `chunk` blocks in ascending block
    number, then the partials into the row.  by_position cuts the chunks at
    multiples of `chunk` of the sorted position instead of the run's own count;
    descending takes a run's blocks in descending number.  The classes returned."""
    want = a.copy()
    rcs = set()
    start = 0
    for j in range(len(a)):
        ks = np.nonzero(dst == j)[0]
        if descending:
            ks = ks[::-1]
        first = (-start) % chunk if by_position else chunk
        cuts = list(range(first, len(ks), chunk)) if by_position else list(range(chunk, len(ks), chunk))
        partials = []
        for part in np.split(ks, cuts):
            if not len(part):
                continue
            p = b[src[part[0]]].copy()
            for k in part[1:]:
                rcs.add(orc.reduce_local(b[src[k]].copy(), p, bl, dt, o))
            partials.append(p)
        for p in partials:
            rcs.add(orc.reduce_local(p, want[j], bl, dt, o))
        start += len(ks)
    assert len(rcs) == 1
    return want, rcs.pop()


def mixed_floats(n, rng):
    """fp32 values of mixed magnitude: sums whose association shows in the bits"""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 5, n)).astype(np.float32)


def table_of(lengths, rng, step):
    """A shuffled output table: target i (displacement i * step) named lengths[i] times"""
    ids = np.repeat(np.arange(len(lengths)), lengths)
    return rng.permutation(ids).astype(np.int64) * step


def runs_in(sorted_displs):
    """(start, length) of every run of the sorted table"""
    heads = np.nonzero(np.concatenate([[True], sorted_displs[1:] != sorted_displs[:-1]]))[0]
    return list(zip(heads.tolist(), np.diff(np.concatenate([heads, [len(sorted_displs)]])).tolist()))


def assert_two_slot_case(sorted_displs):
    """A multi-chunk run starts off a multiple of 64, and one window of 64
    positions holds a run's short last chunk and the next multi-chunk run's first."""
    multi = [(s, n) for s, n in runs_in(sorted_displs) if n > C]
    assert any(s % C for s, _ in multi), multi
    lasts = [s + (n // C) * C for s, n in multi if n % C]
    assert any(q // C == s // C and s > q for q in lasts for s, _ in multi), (lasts, multi)


def build_tables(mpi, torch, stream, tio, dtio, what):
    """order and runstart of tio: the order from numpy (MPIX_Reduce_local_order
    must agree), runstart from MPIX_Reduce_local_runs on device tables, both
    synchronously and on the stream, against the definition.  Returns the device
    tensors and the host tables."""
    nb = len(tio)
    horder = np.argsort(tio, kind="stable").astype(np.int32)
    hruns = runs_of(tio, horder)
    dorder = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = mpi.reduce_local_order(dtio.data_ptr(), nb, dorder.data_ptr())
    assert rc == 0 and np.array_equal(dorder.cpu().numpy(), horder), f"{what}: order: {mpi.error_string(rc)}"
    d1 = torch.full((nb + 2,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((nb + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = mpi.reduce_local_runs(dtio.data_ptr(), dorder.data_ptr(), nb, d1.data_ptr() + 4)
    assert rc == 0, f"{what}: runs: {mpi.error_string(rc)}"
    rc = mpi.reduce_local_runs(dtio.data_ptr(), dorder.data_ptr(), nb, d2.data_ptr() + 4, stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, f"{what}: runs on a stream: {mpi.error_string(rc)}"
    for d in (d1, d2):
        got = d.cpu().numpy()
        assert got[0] == got[-1] == -7, f"{what}: the runs build wrote outside its table"
        assert np.array_equal(got[1:-1], hruns), f"{what}: MPIX_Reduce_local_runs differs from the definition"
    assert np.array_equal(dtio.cpu().numpy(), tio) and np.array_equal(dorder.cpu().numpy(), horder), f"{what}: the build wrote an input"
    return dorder, d1[1:-1], horder, hruns


def run(mpi, orc, torch, stream, op, t, bl, unit, tin, tio, pin, pio, form, seed=0, expect=None, ways=WAYS, tell=False,
        against_indexed=False, data=None, operand_order=False):
    """len(tio) blocks of bl elements; tio (int64, units of `unit` bytes) may
    repeat, tin (or None: packed) too.  Asserts the planner's form, runs the call
    every way and checks both arenas, the tables and the work.  Returns the plan."""
    dt, o = mpi.DATATYPES[t], mpi.OPS[op]
    esz = T.elem_size(t)
    rb = bl * esz
    tio = np.ascontiguousarray(tio, dtype=np.int64)
    nb = len(tio)
    off_in = np.arange(nb, dtype=np.int64) * rb if tin is None else np.asarray(tin, np.int64) * unit
    uin, src = np.unique(off_in, return_inverse=True)
    uio, dst = np.unique(tio * unit, return_inverse=True)
    what = f"{op} {t} {nb} x {bl} onto {len(uio)} unit {unit} in=+{pin}{'' if tin is None else '/table'} io=+{pio}"
    for attempt in range(8):
        rng = np.random.default_rng([seed, nb, bl, attempt])
        gen = (lambda n: T.gen(t, n, rng, op)) if data is None else (lambda n: data(n, rng))
        a = T.to_bytes(gen(len(uio) * bl)).reshape(len(uio), rb)            # one row per distinct target
        b = T.to_bytes(gen(len(uin) * bl)).reshape(len(uin), rb)            # one per input placement
        want, rc_want = chunked_rows(orc, a, b, src, dst, bl, dt, o)
        if not tell and not operand_order:
            break
        # the case can tell a wrong implementation only if it gives other bits
        if operand_order:
            others = {"descending block numbers": chunked_rows(orc, a, b, src, dst, bl, dt, o, descending=True)[0]}
        else:
            others = {"the ordered call": oracle_rows(orc, a, b, src, dst, range(nb), bl, dt, o)[0],
                      "chunks cut at sorted positions": chunked_rows(orc, a, b, src, dst, bl, dt, o, by_position=True)[0],
                      "chunk length 32": chunked_rows(orc, a, b, src, dst, bl, dt, o, chunk=32)[0],
                      "chunk length 128": chunked_rows(orc, a, b, src, dst, bl, dt, o, chunk=128)[0]}
        differ = {n: int((want.reshape(-1, esz) != x.reshape(-1, esz)).any(axis=1).sum()) for n, x in others.items()}
        print(f"{what} (data {attempt}): elements that differ of {len(uio) * bl}: {differ}")
        if all(differ.values()):
            break
    else:
        pytest.fail(f"{what}: no data found that tells: {differ}")
    ain, aio = Arena(torch, b, uin, pin), Arena(torch, a, uio, pio)
    host = [None if tin is None else np.ascontiguousarray(tin, dtype=np.int64), tio]
    devt = [None if x is None else torch.from_numpy(x).cuda() for x in host]
    dptr = [0 if x is None else x.data_ptr() for x in devt]
    dorder, druns, horder, hruns = build_tables(mpi, torch, stream, tio, devt[1], what)
    ws = mpi.reduce_local_chunked_worksize(nb, bl, dt)
    work = torch.full((ws + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.indexed_chunked_plan_info(ain.ptr, dptr[0], aio.ptr, dptr[1], dorder.data_ptr(), druns.data_ptr(), unit,
                                             nb, bl, dt, o)
        assert info["form"] == form, f"{what}: aimed at {FORMS[form]}, the planner says {info}"
        assert info == mpi.indexed_chunked_plan_info(ain.ptr, host[0], aio.ptr, host[1], horder, hruns, unit, nb, bl, dt, o)
        assert info["work_bytes"] == ws and info["total_launches"] == 2 * info["launches"]
        if expect:
            expect(info, tio[horder])
    for n, way in enumerate(ways):
        if n:
            aio.upload()
        torch.cuda.synchronize()
        tabs = host + [horder, hruns] if way == "host-tables" else dptr + [dorder.data_ptr(), druns.data_ptr()]
        wk = (0, 0) if way == "sync" else (work.data_ptr(), ws)
        rc = mpi.reduce_local_indexed_chunked(ain.ptr, tabs[0], aio.ptr, tabs[1], tabs[2], tabs[3], unit, nb, bl, dt, o, *wk,
                                              stream.cuda_stream if way == "stream" else 0)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")
        assert np.array_equal(ain.check(f"{what} {way} inbuf"), b), f"{what} {way}: inbuf modified"
        assert (work[ws:].cpu().numpy() == FILL).all(), f"{what} {way}: work written past the reported {ws} bytes"
        if rc_want:
            assert (work.cpu().numpy() == FILL).all(), f"{what} {way}: a refused call wrote its work"
        for j in range(0 if not np.array_equal(got, want) else len(uio), len(uio)):
            if not same(got[j], want[j], t):
                ks = np.nonzero(dst == j)[0]
                pytest.fail(f"{what} {way} ({FORMS[form]}) target {j}, {len(ks)} blocks {ks.tolist()[:20]}:\n" +
                            explain(got[j], want[j], a[j], b[src[ks[-1]]], esz))
    if against_indexed:
        # all targets distinct: byte-equal to the indexed call on the same operands
        aio.upload()
        torch.cuda.synchronize()
        assert mpi.reduce_local_indexed(ain.ptr, dptr[0], aio.ptr, dptr[1], unit, nb, bl, dt, o) == 0
        plain = aio.check(f"{what} indexed")
        assert np.array_equal(plain, got), f"{what}: differs from MPIX_Reduce_local_indexed"
    for x, h in zip(devt + [dorder, druns], host + [horder, hruns]):
        if x is not None:
            assert np.array_equal(x.cpu().numpy(), h), f"{what}: a table was written"
    return info


# ---------------------------------------------------------------- chunk edges
EDGE_LENGTHS = [1, 65, 129, 2, 63, 200, 64, 128]        # in ascending displacement: 65 then 129 share a window


def edge_table(step, seed):
    tio = table_of(EDGE_LENGTHS, np.random.default_rng(seed), step)
    assert sorted(EDGE_LENGTHS) == [1, 2, 63, 64, 65, 128, 129, 200]
    assert_two_slot_case(np.sort(tio))
    return tio


def test_chunk_edges_narrow_vectors(mpi, orc, cuda):
    """fp32 MPI_SUM, 48-byte blocks, runs of 1, 2, 63, 64, 65, 128, 129 and 200:
    652 blocks, two workgroups; the run of 129 starts at sorted position 66, in
    the window that holds the run of 65's last chunk of one block."""
    assert 48 < threshold(mpi)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 12, 16, None, edge_table(4, 1), 16, 32, NARROW_VEC,
        seed=1, tell=True, data=mixed_floats, expect=lambda i, s: i["groups"] == 2 or pytest.fail(str(i)))


def test_chunk_edges_narrow_elements(mpi, orc, cuda):
    """The same runs with 4-byte blocks, 8 bytes apart."""
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 1, 4, None, edge_table(2, 2), 16, 36, NARROW_ELEMS,
        seed=2, tell=True, data=mixed_floats)


def test_chunk_edges_wide(mpi, orc, cuda):
    """Blocks of the threshold's bytes and 12 more (no multiple of 16), the base 4
    bytes off the tile grid: runs of 1, 65, 130 and 64, the run of 130 starting in
    the window of the run of 65's last chunk.  The packed input blocks fall at
    every residue mod 16 that a multiple of 4 has, so some are read through the
    descriptor and some element by element."""
    bl = threshold(mpi) // 4 + 3
    assert bl * 4 >= threshold(mpi) and (bl * 4) % 16
    tio = table_of([1, 65, 130, 64], np.random.default_rng(3), bl + 5)
    assert_two_slot_case(np.sort(tio))

    def two_tiles(info, sorted_displs):
        assert info["per"] >= 2 and info["groups"] == len(tio) * info["per"], info

    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", bl, 4, None, tio, 4, 4, WIDE, seed=3, tell=True,
        data=mixed_floats, expect=two_tiles)


def test_one_target_only(mpi, orc, cuda):
    """4097 blocks of 16 bytes onto one target: 65 partials, the last of one block."""
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 4, 16, None, np.full(4097, 5, np.int64), 16, 32,
        NARROW_VEC, seed=4, data=mixed_floats)


def test_all_targets_distinct_is_the_indexed_call(mpi, orc, cuda):
    for unit, pio, form in ((16, 32, NARROW_VEC), (4, 36, NARROW_ELEMS)):
        run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 12, unit, None, slots(400, 5, gap=0) * (64 // unit),
            16, pio, form, seed=5, against_indexed=True)


# ---------------------------------------------------------------- launches
def test_lowered_cap_runs_and_chunks_cross_launch_boundaries(mpi, orc, cuda):
    """The per-launch workgroup cap lowered to 3: 2731 blocks of 48 bytes make
    three launches of 1024 sorted positions for either kernel.  Runs of 7, 1500
    and 1224: chunks start at 7 + 64 i and 1507 + 64 i, so a chunk lies across
    each boundary (kernel 1), and both long runs' partials lie on both sides of
    one (kernel 2).  The wide shape becomes one launch per block."""
    lib = mpi.load()
    stream = cuda.cuda.Stream()
    assert lib.MPIR_Hip_strided_test_max_groups(3) == 0
    try:
        def crossing(info, sorted_displs):
            rpl = info["rows_per_launch"]
            assert info["launches"] == 3 and rpl == 1024 and info["total_launches"] == 6, info
            for edge in range(rpl, len(sorted_displs), rpl):
                s, n = next((s, n) for s, n in runs_in(sorted_displs) if s < edge < s + n)
                assert n > C and (edge - s) % C, (edge, s, n)      # inside a run, and inside one of its chunks

        tio = table_of([7, 1500, 1224], np.random.default_rng(6), 4)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 12, 16, None, tio, 16, 32, NARROW_VEC, seed=6, expect=crossing,
            tell=True, data=mixed_floats)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 12, 4, None, tio * 4, 16, 36, NARROW_ELEMS, seed=7,
            expect=lambda i, s: i["launches"] > 1 or pytest.fail(str(i)), data=mixed_floats)
        bl = threshold(mpi) // 4 + 3
        wide = table_of([3, 70], np.random.default_rng(8), bl + 5)
        run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", bl, 4, None, wide, 4, 4, WIDE, seed=8, data=mixed_floats,
            expect=lambda i, s: i["launches"] == -(-73 // max(1, 3 // i["per"])) > 1 or pytest.fail(str(i)))
    finally:
        assert lib.MPIR_Hip_strided_test_max_groups(0) == 3


# ---------------------------------------------------------------- input placement
def test_input_blocks_off_the_targets_phase(mpi, orc, cuda):
    """An input table in units of 4 bytes whose blocks sit at residues 4, 8, 12
    and 0 mod 16 while every target sits at residue 4 (wide) or 0 (elements)."""
    bl = threshold(mpi) // 4 + 3
    rng = np.random.default_rng(9)
    tio = table_of([2, 70, 5], rng, bl + 5)
    tin = rng.permutation(77).astype(np.int64) * (bl + 2)
    assert set((tin * 4 + 8) % 16) == {0, 4, 8, 12}
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", bl, 4, tin, tio, 8, 4, WIDE, seed=9, data=mixed_floats)
    tio = table_of([2, 70, 5], rng, 16)
    tin = rng.permutation(77).astype(np.int64) * 13
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 12, 4, tin, tio, 4, 0, NARROW_ELEMS, seed=10,
        data=mixed_floats)


@pytest.mark.parametrize("unit,form", [(16, NARROW_VEC), (4, NARROW_ELEMS)], ids=["vec", "elems"])
def test_an_input_table_with_repeated_entries(mpi, orc, cuda, unit, form):
    rng = np.random.default_rng(11)
    tio = table_of([1, 64, 135, 30, 70], rng, 64 // unit)
    tin = rng.integers(0, 50, len(tio)).astype(np.int64) * (48 // unit)
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 12, unit, tin, tio, 0, 16 if unit == 16 else 20, form,
        seed=11, data=mixed_floats)


# ---------------------------------------------------------------- every pair of the matrix
CLASSES = ["MPI_INT8_T", "MPI_UINT8_T", "MPI_INT16_T", "MPI_UINT16_T", "MPI_INT32_T", "MPI_UINT32_T", "MPI_INT64_T",
           "MPI_UINT64_T", "MPIX_C_FLOAT16", "MPI_FLOAT", "MPI_DOUBLE", "MPI_LONG_DOUBLE", "MPI_C_FLOAT_COMPLEX",
           "MPI_C_DOUBLE_COMPLEX", "MPI_C_LONG_DOUBLE_COMPLEX", "MPI_2INT", "MPI_FLOAT_INT", "MPI_LONG_INT", "MPI_SHORT_INT",
           "MPI_DOUBLE_INT", "MPI_LONG_DOUBLE_INT"]
PAIRS = [(op, t) for op in T.OPS for t in CLASSES if T.compute_ok(op, t)]


def test_the_pairs_are_the_matrix():
    assert len(CLASSES) == 21 and len(PAIRS) == 118


@pytest.mark.parametrize("op,t", PAIRS, ids=[f"{o}-{t}" for o, t in PAIRS])
def test_every_pair(mpi, orc, cuda, op, t):
    """200 blocks of 96 bytes onto 3 targets, runs of 1, 64 and 135: a direct
    combine, a single full chunk and three partials, the last of 7 blocks.  The
    32-byte classes take the element form, every other the vector form."""
    esz = T.elem_size(t)
    assert 96 % esz == 0
    tio = table_of([64, 1, 135], np.random.default_rng(12), 8)
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, 96 // esz, 16, None, tio, 16, 32, NARROW_VEC if esz <= 16 else NARROW_ELEMS,
        seed=12)


def nans_of_distinct_payloads(n, rng):
    """fp32: one element in three a quiet or signalling NaN whose payload is its own"""
    x = rng.standard_normal(n).astype(np.float32).view(np.uint32)
    idx = np.nonzero(rng.integers(0, 3, n) == 0)[0]
    x[idx] = (0x7F800001 + (rng.integers(0, 2, len(idx)) << 22) + rng.permutation(len(idx)) * 2 +
              (rng.integers(0, 2, len(idx)) << 31)).astype(np.uint32)
    return x.view(np.float32)


@pytest.mark.parametrize("op", ["MPI_MAX", "MPI_MIN"])
def test_float_max_min_over_nans_where_the_operand_order_shows(mpi, orc, cuda, op):
    tio = table_of([64, 1, 135], np.random.default_rng(13), 4)
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, "MPI_FLOAT", 12, 16, None, tio, 16, 32, NARROW_VEC, seed=13,
        data=nans_of_distinct_payloads, operand_order=True)


def test_a_pair_the_library_refuses(mpi, orc, cuda):
    """MPI_LAND on MPI_FLOAT: the oracle's class, nothing written, in the target or in work (run checks both)."""
    assert not T.compute_ok("MPI_LAND", "MPI_FLOAT")
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_LAND", "MPI_FLOAT", 12, 16, None, table_of([64, 1, 135],
        np.random.default_rng(14), 4), 16, 32, NARROW_VEC, seed=14)


# ---------------------------------------------------------------- the runstart build
def test_runs_on_device_tables(mpi, cuda):
    """The four cases of the CPU test and the chunk-edge table."""
    torch = cuda
    rng = np.random.default_rng(15)
    stream = torch.cuda.Stream()
    for name, displs in (("signed with repeats", rng.integers(-50, 50, 1000)), ("one", np.array([-5])),
                         ("all equal", np.full(257, 7)), ("all distinct", rng.permutation(4099) - 2000),
                         ("chunk edges", edge_table(4, 1))):
        tio = np.ascontiguousarray(displs, dtype=np.int64)
        dtio = torch.from_numpy(tio).cuda()
        _, _, horder, hruns = build_tables(mpi, torch, stream, tio, dtio, name)
        # mixed residency in the synchronous call
        mixed = np.full(len(tio), -1, np.int32)
        assert mpi.reduce_local_runs(dtio.data_ptr(), horder, len(tio), mixed) == 0 and np.array_equal(mixed, hruns), name
        dr = torch.full((len(tio),), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert mpi.reduce_local_runs(tio, horder, len(tio), dr.data_ptr()) == 0 and np.array_equal(dr.cpu().numpy(), hruns), name
        # a host table with a stream
        rc = mpi.reduce_local_runs(tio, horder, len(tio), dr.data_ptr(), stream.cuda_stream)
        assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)


# ---------------------------------------------------------------- graph capture
def loaded_hip():
    """The HIP runtime this process already uses (torch's and the library's), for the graph queries"""
    with open("/proc/self/maps") as maps:
        return ctypes.CDLL(next(line.split()[-1] for line in maps if "libamdhip64.so" in line))


def linear_chain(hip, graph):
    """(nodes, True where the captured graph is one chain: no parallel branch)"""
    n, roots, edges = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    assert hip.hipGraphGetRootNodes(graph, None, ctypes.byref(roots)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(edges)) == 0
    src = (ctypes.c_void_p * max(1, edges.value))()
    dst = (ctypes.c_void_p * max(1, edges.value))()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(edges)) == 0
    froms, tos = [src[i] for i in range(edges.value)], [dst[i] for i in range(edges.value)]
    chain = roots.value == 1 and edges.value == n.value - 1 and len(set(froms)) == len(froms) and len(set(tos)) == len(tos)
    return n.value, chain


def test_captured_in_a_graph(mpi, orc, cuda):
    """With device tables and the caller's work the call is captured once on one
    stream: a chain of two kernel nodes, no parallel branch.  It is replayed
    twice with other input bytes uploaded in between; each replay is bit-exact."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    bl = 12
    rng = np.random.default_rng(16)
    tio = edge_table(4, 16)
    nb = len(tio)
    uio, dst = np.unique(tio * 16, return_inverse=True)
    a = T.to_bytes(mixed_floats(len(uio) * bl, rng)).reshape(len(uio), bl * 4)
    b1 = T.to_bytes(mixed_floats(nb * bl, rng)).reshape(nb, bl * 4)
    b2 = T.to_bytes(mixed_floats(nb * bl, rng)).reshape(nb, bl * 4)
    src = np.arange(nb)
    once, rc = chunked_rows(orc, a, b1, src, dst, bl, dt, o)
    assert rc == 0
    twice, _ = chunked_rows(orc, once, b2, src, dst, bl, dt, o)
    ain, aio = Arena(torch, b1, np.arange(nb) * bl * 4, 0), Arena(torch, a, uio, 16)
    dtio = torch.from_numpy(tio).cuda()
    s = torch.cuda.Stream()
    dorder, druns, _, _ = build_tables(mpi, torch, s, tio, dtio, "graph")
    ws = mpi.reduce_local_chunked_worksize(nb, bl, dt)
    work = torch.full((ws + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def enqueue(cs):
        return mpi.reduce_local_indexed_chunked(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(),
                                                16, nb, bl, dt, o, work.data_ptr(), ws, cs)

    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert enqueue(torch.cuda.current_stream().cuda_stream) == 0
    # the shape of the captured graph: the two kernels, one after the other
    nodes, chain = linear_chain(loaded_hip(), ctypes.c_void_p(g.raw_cuda_graph()))
    assert nodes == 2 and chain, (nodes, chain)
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("captured inoutbuf"), a)        # capture records, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("replayed once"), once)
    ain.host[ain.idx] = b2
    ain.upload()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(aio.check("replayed twice"), twice)
    assert np.array_equal(ain.check("replayed twice inbuf"), b2)
    assert (work[ws:].cpu().numpy() == FILL).all()


# ---------------------------------------------------------------- routes and failures
def test_routes_and_failures(mpi, orc, cuda):
    """Both tables NULL is the indexed call; one of them NULL, either with a packed
    target, a host runstart off its definition, a host table on a stream, short
    work_bytes and no work on a stream are refused with nothing written, in the
    target or in work; a device runstart and order holding out-of-range values
    return and write no guard byte and nothing past the work's size."""
    torch = cuda
    dt, o = mpi.MPI_FLOAT, mpi.MPI_SUM
    bl = 12
    rng = np.random.default_rng(17)
    tio = edge_table(4, 17)
    nb = len(tio)
    uio, dst = np.unique(tio * 16, return_inverse=True)
    a = T.to_bytes(mixed_floats(len(uio) * bl, rng)).reshape(len(uio), bl * 4)
    b = T.to_bytes(mixed_floats(nb * bl, rng)).reshape(nb, bl * 4)
    ain, aio = Arena(torch, b, np.arange(nb) * bl * 4, 0), Arena(torch, a, uio, 16)
    dtio = torch.from_numpy(tio).cuda()
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    dorder, druns, horder, hruns = build_tables(mpi, torch, stream, tio, dtio, "routes")
    ws = mpi.reduce_local_chunked_worksize(nb, bl, dt)
    work = torch.full((ws + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    wp = work.data_ptr()

    def refused(rc, cls, what):
        stream.synchronize()
        assert mpi.error_class(rc) == cls, f"{what}: {mpi.error_string(rc)}"
        assert np.array_equal(aio.check(what), a), f"{what}: inoutbuf written by a refused call"
        assert np.array_equal(ain.check(what), b), what
        assert (work.cpu().numpy() == FILL).all(), f"{what}: work written by a refused call"

    call = mpi.reduce_local_indexed_chunked
    tail = (16, nb, bl, dt, o)
    # both NULL: the indexed call, here on a table without repeats
    tdist = slots(len(uio), 17, gap=0) * 4
    adist = Arena(torch, a, tdist * 16, 16)
    bdist = Arena(torch, b[:len(uio)], np.arange(len(uio)) * bl * 4, 0)
    assert call(bdist.ptr, None, adist.ptr, tdist, None, None, 16, len(uio), bl, dt, o) == 0
    first = adist.check("both tables NULL")
    adist.upload()
    assert mpi.reduce_local_indexed(bdist.ptr, None, adist.ptr, tdist, 16, len(uio), bl, dt, o) == 0
    assert np.array_equal(adist.check("indexed"), first)
    # exactly one of them, and either with a packed target
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), None, *tail, wp, ws), mpi.MPI_ERR_ARG, "no runstart")
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), None, druns.data_ptr(), *tail, wp, ws), mpi.MPI_ERR_ARG, "no order")
    refused(call(ain.ptr, None, aio.ptr, None, dorder.data_ptr(), druns.data_ptr(), *tail, wp, ws), mpi.MPI_ERR_ARG,
            "tables with a packed target")
    # a host runstart: off its definition beside host tables; out of range beside a device order
    for p in (0, 1, 65, 66, nb - 1):
        for step in (-1, 1):
            bad = hruns.copy()
            bad[p] += step
            refused(call(ain.ptr, None, aio.ptr, tio, horder, bad, *tail, wp, ws), mpi.MPI_ERR_ARG, f"runstart[{p}] {step:+d}")
    bad = hruns.copy()
    bad[70] = 71
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), bad, *tail, wp, ws), mpi.MPI_ERR_ARG,
            "host runstart past its position beside device tables")
    # a host table with a stream, whichever it is; no work on a stream; short work
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), hruns, *tail, wp, ws, cs), mpi.MPI_ERR_BUFFER,
            "host runstart on a stream")
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), horder, druns.data_ptr(), *tail, wp, ws, cs), mpi.MPI_ERR_BUFFER,
            "host order on a stream")
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(), *tail, 0, 0, cs),
            mpi.MPI_ERR_BUFFER, "no work on a stream")
    for st in (0, cs):
        refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(), *tail, wp, ws - 1, st),
                mpi.MPI_ERR_ARG, "short work_bytes")
    hostwork = np.zeros(ws, np.uint8)
    refused(call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(), *tail, hostwork.ctypes.data, ws),
            mpi.MPI_ERR_BUFFER, "work in host memory")
    assert not hostwork.any()
    # device tables with out-of-range values: undefined result, but the call returns
    # and every address stays inside the blocks and the work
    broken_o, broken_r = horder.copy(), hruns.copy()
    broken_o[5], broken_o[9], broken_o[nb - 1] = nb + 1000, -3, 2 ** 31 - 1
    broken_r[3], broken_r[100], broken_r[nb - 1], broken_r[200] = -1, 2 ** 31 - 1, nb + 7, 199
    dbo, dbr = torch.from_numpy(broken_o).cuda(), torch.from_numpy(broken_r).cuda()
    torch.cuda.synchronize()
    rc = call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dbo.data_ptr(), dbr.data_ptr(), *tail, wp, ws)
    assert rc == 0, mpi.error_string(rc)
    aio.check("device tables out of range: inoutbuf guards")
    assert np.array_equal(ain.check("device tables out of range: inbuf"), b)
    assert (work[ws:].cpu().numpy() == FILL).all(), "work written past its size"
    # and the valid tables on the same operands still give the definition's rows
    aio.upload()
    want, _ = chunked_rows(orc, a, b, np.arange(nb), dst, bl, dt, o)
    assert call(ain.ptr, None, aio.ptr, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(), *tail, wp, ws) == 0
    assert np.array_equal(aio.check("valid tables"), want)
