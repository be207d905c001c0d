"""MPIX_Reduce_local_fetch on the GPU: fetchbuf receives the bytes inoutbuf held,
inoutbuf the oracle's MPI_Reduce_local (bit-exact, test_parity_gpu.same's
complex-NaN rule), in one launch.

Each of the three operands sits in an arena of its own, filled with 0xA5, at a
chosen byte phase of the 16 KiB grid (test_strided_gpu's Image).  Before each
call fetchbuf's payload holds the bitwise complement of the old inoutbuf image,
so that any byte left unwritten shows.  After each call inoutbuf must equal the
oracle's, fetchbuf must equal the old inoutbuf image byte for byte (NaN payloads,
the padding of the x87 slots and of the pair types included), every guard byte
of all three arenas must still be 0xA5 and inbuf must be unchanged.  Before a
shape runs MPIR_Hip_fetch_plan_info -- the launch's own planner -- must report the
path the shape was built for.  Every shape runs twice: synchronously on the
library stream, and enqueued on a torch stream that is then synchronised.
"""
import numpy as np
import pytest

import _types as T
from test_parity_gpu import MATRIX, explain, same
from test_plan_edges_gpu import TILE
from test_strided_gpu import Image

pytestmark = pytest.mark.gpu

EMPTY, COPY, TILEP, ELEMS = range(4)
PATHS = ["empty", "copy", "tile", "elems"]


def handles(mpi, op, t):
    return mpi.DATATYPES[t], getattr(mpi, op)


def run(mpi, orc, torch, stream, op, t, n, pin, pio, pfe, path, seed=0, null_in=False, expect=None):
    """n elements; inbuf / inoutbuf / fetchbuf at byte phases pin / pio / pfe of the
    16 KiB grid.  Asserts the planner's path, runs the call both ways and checks
    all three arenas.  expect(info): further plan checks.  Returns the plan."""
    dt, o = handles(mpi, op, t)
    esz = T.elem_size(t)
    gen_op = op if op in T.OPS else "MPI_SUM"
    rng = np.random.default_rng([seed, n, esz])
    a = T.to_bytes(T.gen(t, n, rng, gen_op))            # inout
    b = T.to_bytes(T.gen(t, n, rng, gen_op))            # in
    want = a.copy()
    # (the oracle's validation refuses MPI_NO_OP and MPI_REPLACE as MPI_Reduce_local does; its kernels compute them)
    rc_want = orc.reduce_local(b.copy(), want, n, dt, o, check=op in T.OPS)
    ain = None if null_in else Image(torch, b.reshape(1, -1), 0, pin)
    aio = Image(torch, a.reshape(1, -1), 0, pio)
    afe = Image(torch, (~a).reshape(1, -1), 0, pfe)
    p_in = 0 if null_in else ain.ptr
    what = f"{op} {t} n={n} in=+{pin} io=+{pio} fetch=+{pfe}"
    info = None
    if not rc_want:                     # (a refused pair has no kernel, so no plan)
        info = mpi.fetch_plan_info(p_in, aio.ptr, afe.ptr, n, dt, o)
        assert info["path"] == path, f"{what}: aimed at {PATHS[path]}, the planner says {info}"
        if expect:
            expect(info)
    for way in ("sync", "stream"):
        if way == "stream":
            aio.upload()
            afe.upload()
        torch.cuda.synchronize()
        rc = mpi.reduce_local_fetch(p_in, aio.ptr, afe.ptr, n, dt, o, 0 if way == "sync" else stream.cuda_stream)
        stream.synchronize()
        assert mpi.error_class(rc) == rc_want, f"{what} {way}: {mpi.error_string(rc)}"
        got = aio.check(f"{what} {way} inoutbuf")[0]
        old = afe.check(f"{what} {way} fetchbuf")[0]
        if ain is not None:
            assert np.array_equal(ain.check(f"{what} {way} inbuf")[0], b), f"{what} {way}: inbuf modified"
        if rc_want:                     # refused: nothing written
            assert np.array_equal(got, a) and np.array_equal(old, ~a), f"{what} {way}: a refused call wrote"
            continue
        if not same(got, want, t):
            pytest.fail(f"{what} {way} ({PATHS[path]}) inoutbuf:\n" + explain(got, want, a, b, esz))
        if not np.array_equal(old, a):
            pytest.fail(f"{what} {way} ({PATHS[path]}) fetchbuf is not the old inoutbuf:\n" + explain(old, a, a, b, esz))
    return info


def groups(n):
    return lambda info: info["groups"] == n or pytest.fail(f"expected {n} workgroups: {info}")


# ---------------------------------------------------------------- the tile path
def test_count_one(mpi, orc, cuda):
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 1, 0, 0, 0, TILEP, expect=groups(1))
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 1, 12, 12, 12, TILEP, seed=1,
        expect=lambda i: (i["nhead"], i["ntail"]) == (1, 0) or pytest.fail(str(i)))
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", 1, 0, 0, 4, ELEMS, seed=2, expect=groups(1))


def test_tile_path_with_head_and_tail(mpi, orc, cuda):
    """Floats, all phases 4, 2 x 4096 + 7: three head elements, then whole vectors
    over two tiles and a sliver of a third; one element less leaves three tail
    elements."""
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 2 * 4096 + 7, 4, 4, 4, TILEP,
        expect=lambda i: (i["groups"], i["nhead"], i["ntail"]) == (3, 3, 0) or pytest.fail(str(i)))
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 2 * 4096 + 6, 4, 4, 4, TILEP, seed=1,
        expect=lambda i: (i["groups"], i["nhead"], i["ntail"]) == (3, 3, 3) or pytest.fail(str(i)))


def test_exactly_one_tile_and_one_vector_more(mpi, orc, cuda):
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", TILE // 4, 0, 0, 0, TILEP, expect=groups(1))
    run(mpi, orc, cuda, stream, "MPI_SUM", "MPI_FLOAT", TILE // 4 + 4, 0, 0, 0, TILEP, seed=1, expect=groups(2))


def test_three_descriptors_clip_at_different_places(mpi, orc, cuda):
    """inoutbuf 8 KiB off the grid, fetchbuf on it, inbuf 4 KiB off: tile 0 is cut at
    inoutbuf's first grid line, which is the middle of fetchbuf's tile and three
    quarters through inbuf's."""
    n = 2 * 4096 + 7
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", n, 4096, 8192, 0, TILEP,
        expect=lambda i: (i["groups"], i["nhead"], i["ntail"]) == (3, 0, 3) or pytest.fail(str(i)))
    # ... and with head elements, every phase another 16 KiB residue
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_MAX", "MPI_DOUBLE", 4096 + 3, 4096 + 8, 8192 + 8, 12288 + 8, TILEP, seed=1,
        expect=lambda i: (i["groups"], i["nhead"]) == (3, 1) or pytest.fail(str(i)))


# ---------------------------------------------------------------- the element path
@pytest.mark.parametrize("pin,pio,pfe", [(0, 0, 4), (4, 0, 0), (1, 1, 1)], ids=["fetch-4-off", "in-4-off", "unaligned"])
def test_element_path_for_each_reason(mpi, orc, cuda, pin, pio, pfe):
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 1003, pin, pio, pfe, ELEMS, seed=pin + pfe,
        expect=groups(1))


def test_element_path_three_workgroups_ragged(mpi, orc, cuda):
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_SUM", "MPI_FLOAT", 2 * 4096 + 101, 16, 16, 20, ELEMS, expect=groups(3))
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_BXOR", "MPI_UNSIGNED_CHAR", 2 * TILE + 1, 3, 5, 7, ELEMS, seed=1,
        expect=groups(3))


@pytest.mark.parametrize("op,t", [("MPI_MAXLOC", "MPI_LONG_DOUBLE_INT"), ("MPI_SUM", "MPI_C_LONG_DOUBLE_COMPLEX"),
                                  ("MPI_PROD", "MPI_C_LONG_DOUBLE_COMPLEX")])
def test_32_byte_classes(mpi, orc, cuda, op, t):
    """700 elements: two workgroups of 512, whatever the alignment; the x87
    slots' padding arrives in fetchbuf as it was."""
    stream = cuda.cuda.Stream()
    run(mpi, orc, cuda, stream, op, t, 700, 0, 0, 0, ELEMS, expect=groups(2))
    run(mpi, orc, cuda, stream, op, t, 700, 16, 0, 8, ELEMS, seed=1, expect=groups(2))


# ---------------------------------------------------------------- the matrix
@pytest.mark.parametrize("op,t", MATRIX, ids=[f"{o}-{t}" for o, t in MATRIX])
def test_fetch_matrix_vs_oracle(mpi, orc, cuda, op, t):
    """Every (op, type) the reference accepts, special values included, at one
    small count on each path: head elements where the type has any, whole
    vectors and tail elements on the tile path; fetchbuf off inoutbuf's residue
    mod 16 on the element path.  What the reference's compute switch refuses
    (LAND / LOR on floating types) the call refuses with the same class, writing
    nothing."""
    esz = T.elem_size(t)
    stream = cuda.cuda.Stream()
    n = 37
    ph = esz if esz < 16 else 0
    if esz <= 16:
        run(mpi, orc, cuda, stream, op, t, n, 4096 + ph, ph, 8192 + ph, TILEP, seed=1)
    run(mpi, orc, cuda, stream, op, t, n, 4096 + ph, ph, 8192 + ph + (esz if esz < 16 else 8), ELEMS, seed=2)


# ---------------------------------------------------------------- MPI_NO_OP and MPI_REPLACE
def test_no_op_with_null_inbuf(mpi, orc, cuda):
    """An atomic get: fetchbuf the copy, inoutbuf byte-identical afterwards (run()
    checks it against the oracle's MPI_NO_OP, which leaves it alone)."""
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_NO_OP", "MPI_FLOAT", 2 * 4096 + 7, 0, 4, 8, COPY, null_in=True,
        expect=groups(0))


def test_replace(mpi, orc, cuda):
    """A swap: fetchbuf the old bytes, inoutbuf = inbuf."""
    run(mpi, orc, cuda, cuda.cuda.Stream(), "MPI_REPLACE", "MPI_FLOAT", 2 * 4096 + 7, 4, 8, 12, COPY, expect=groups(0))


@pytest.mark.parametrize("t", ["MPI_UNSIGNED_CHAR", "MPI_LONG_DOUBLE", "MPI_LONG_DOUBLE_INT"], ids=["1B", "16B", "32B"])
@pytest.mark.parametrize("op", ["MPI_NO_OP", "MPI_REPLACE"])
def test_copy_ops_on_every_size_at_an_odd_phase(mpi, orc, cuda, op, t):
    run(mpi, orc, cuda, cuda.cuda.Stream(), op, t, 1001, 1, 3, 5, COPY, seed=T.elem_size(t))


# ---------------------------------------------------------------- failures, graphs
def test_no_partial_work(mpi, orc, cuda):
    """Residency is settled before anything is enqueued: a pinned-host fetchbuf
    fails the call, and inoutbuf, the arenas and the pinned buffer are untouched."""
    torch = cuda
    n = 3 * 4096 + 5
    rng = np.random.default_rng(9)
    a = T.to_bytes(T.gen("MPI_FLOAT", n, rng))
    b = T.to_bytes(T.gen("MPI_FLOAT", n, rng))
    ain, aio = Image(torch, b.reshape(1, -1), 0, 0), Image(torch, a.reshape(1, -1), 0, 0)
    pinned = torch.full((n * 4,), 0x5A, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream()
    for op in ("MPI_SUM", "MPI_NO_OP", "MPI_REPLACE"):
        for way in ("sync", "stream"):
            torch.cuda.synchronize()
            rc = mpi.reduce_local_fetch(ain.ptr, aio.ptr, pinned.data_ptr(), n, mpi.MPI_FLOAT, getattr(mpi, op),
                                        0 if way == "sync" else stream.cuda_stream)
            stream.synchronize()
            assert mpi.error_class(rc) == mpi.MPI_ERR_BUFFER, mpi.error_string(rc)
            assert "device-resident" in mpi.error_string(rc)
            assert np.array_equal(aio.check(f"{op} {way} inoutbuf")[0], a), f"{op} {way}: inoutbuf written by a refused call"
            assert np.array_equal(ain.check(f"{op} {way} inbuf")[0], b)
            assert (pinned.numpy() == 0x5A).all(), f"{op} {way}: the pinned fetchbuf was written"
    # the same call with a device fetchbuf runs
    afe = Image(torch, (~a).reshape(1, -1), 0, 0)
    want = a.copy()
    assert orc.reduce_local(b.copy(), want, n, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    assert mpi.reduce_local_fetch(ain.ptr, aio.ptr, afe.ptr, n, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    assert np.array_equal(aio.check("all device")[0], want) and np.array_equal(afe.check("all device")[0], a)


def test_fetch_in_hip_graph(mpi, orc, cuda):
    """The call is self-contained in its kernel arguments: one fp32 MPI_SUM fetch
    captured on a side stream (a single kernel node) and replayed twice leaves in
    fetchbuf the oracle's value after the first application, in inoutbuf the
    value after two."""
    torch = cuda
    n = 70001
    rng = np.random.default_rng(5)
    a = T.to_bytes(T.gen("MPI_FLOAT", n, rng, specials=False))
    b = T.to_bytes(T.gen("MPI_FLOAT", n, rng, specials=False))
    once = a.copy()
    assert orc.reduce_local(b.copy(), once, n, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    twice = once.copy()
    assert orc.reduce_local(b.copy(), twice, n, mpi.MPI_FLOAT, mpi.MPI_SUM) == 0
    ain, aio = Image(torch, b.reshape(1, -1), 0, 0), Image(torch, a.reshape(1, -1), 0, 0)
    afe = Image(torch, (~a).reshape(1, -1), 0, 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            assert mpi.reduce_local_fetch(ain.ptr, aio.ptr, afe.ptr, n, mpi.MPI_FLOAT, mpi.MPI_SUM, cs) == 0
    torch.cuda.synchronize()
    # capture records, it does not run
    assert np.array_equal(aio.check("captured inoutbuf")[0], a) and np.array_equal(afe.check("captured fetchbuf")[0], ~a)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(afe.check("replayed fetchbuf")[0], once)
    assert np.array_equal(aio.check("replayed inoutbuf")[0], twice)
    assert np.array_equal(ain.check("replayed inbuf")[0], b)
