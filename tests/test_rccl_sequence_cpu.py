"""The device collectives' RCCL call sequences at N = 2..8 ranks, without a GPU
(VERDICT r5 item 3).

csrc/host/coll_hip.c -- the product source, compiled unchanged -- runs one
process per rank against a recording librccl stand-in (tests/progs/rccl_stub.c,
loaded through MPIR_TEST_RCCL_LIBRARY) with its HIP calls and kernels replaced
by stand-ins that move no data (tests/progs/coll_trace.c), so configs 4 and 5
run at their full counts in no memory.  Checked, per plan and rank count:
  * every rank's grouped ncclSend / ncclRecv sit inside balanced
    ncclGroupStart / ncclGroupEnd brackets;
  * for every ordered pair of ranks (a, b), the k-th send a -> b and the k-th
    recv at b from a carry equal bytes and type and fall in the same group epoch
    (the i-th group on each rank): no rank waits on a transfer its peer posts in
    a later group;
  * ncclAllReduce / ncclReduceScatter / ncclReduce are issued by every rank in
    the same order, with the same count, type, op and root, after the same number
    of groups;
  * config 4 (MPI_Allreduce fp32 SUM, 256 MiB): ncclAllReduce count 67,108,864;
    config 5 (MPI_Reduce_scatter_block fp16 SUM, 1 GiB per rank): ncclReduceScatter
    recvcount 2^29 / N (67,108,864 at N = 8); the reference-order schedules move
    the bytes their reference schedules move;
  * bench_coll.py's own sequence of calls (bench_coll.call_plan) at N = 2 and 8.
A checker that missed a changed sequence would be worthless: one test alters
one rank's log in several ways and expects each to be caught.

The pinned sweep (below the sequence tests) goes further: over plans that walk
every branch of coll_hip.c at N = 1..8 it compares each rank's complete log --
every HIP call, kernel launch and RCCL call with its buffers, streams and events
by name -- with digests recorded from the source before a rewrite, and checks
that small edits to the source change them.

Reference schedules: reduce_scatter_block_intra_pairwise.c:97-134,
allreduce_intra_reduce_scatter_allgather.c:170-260 / reduce_intra_reduce_scatter_gather.c
(coll_hip.c's reference order); RCCL mode: MPIR_Allreduce -> ncclAllReduce.
"""
import collections
import hashlib
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mpich-pip_amd", "csrc", "host")
ROCM_INC = "/opt/rocm/include"
NCCL_F16, NCCL_F32, NCCL_SUM = 6, 7, 0       # rccl.h ncclDataType_t / ncclRedOp_t

CONFIG4 = [("allreduce", 67108864, "f32", "sum", "rccl"), ("allreduce", 67108864, "f32", "sum", "ref")]


def config5(n):
    rc = (1 << 29) // n          # 1 GiB of fp16 per rank
    return [("reduce_scatter_block", rc, "f16", "sum", "rccl"), ("reduce_scatter_block", rc, "f16", "sum", "ref")]


def build_harness(d, source=None):
    """The stub library and the one-rank program, built in directory d from
    `source` (default: the tree's coll_hip.c)."""
    d = pathlib.Path(d)
    stub = str(d / "librccl_stub.so")
    exe = str(d / "coll_trace")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-Wall", "-I" + ROCM_INC, "-D__HIP_PLATFORM_AMD__", "-o", stub,
                    os.path.join(ROOT, "tests", "progs", "rccl_stub.c"), "-ldl"], check=True)
    # -rdynamic: the stub finds the harness's name lookups with dlsym
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                    "-I" + ROCM_INC, "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(ROOT, "tests", "progs", "coll_trace.c"), source or os.path.join(HOST, "coll_hip.c")] +
                   [os.path.join(HOST, f) for f in ("op_kernels.c", "errutil.c", "reduce_local.c",
                                                   "op_objects.c")] + ["-ldl", "-lpthread"], check=True)
    return d, stub, exe


def have_headers():
    return os.path.exists(os.path.join(ROCM_INC, "rccl", "rccl.h"))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not have_headers():
        pytest.skip("needs the ROCm headers (rccl.h, hip_runtime_api.h) to compile against")
    return build_harness(tmp_path_factory.mktemp("rccl_trace"))


def run_plan(harness, n, plan, tag, env=None):
    d, stub, exe = harness
    text = "".join(" ".join(str(x) for x in step) + "\n" for step in plan)
    log = str(d / f"{tag}_n{n}")
    # a run with an environment of its own (the pinned sweep) inherits no CVAR
    base = os.environ if env is None else {k: v for k, v in os.environ.items() if not k.startswith("MPIR_CVAR_")}
    env = dict(base, MPIR_TEST_RCCL_LIBRARY=stub, RCCL_STUB_LOG=log, **(env or {}))
    procs = [subprocess.Popen([exe, str(r), str(n)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env) for r in range(n)]
    for r, p in enumerate(procs):
        out, err = p.communicate(text, timeout=120)
        assert p.returncode == 0, f"rank {r}: exit {p.returncode}: {err}"
    logs = []
    for r in range(n):
        with open(f"{log}.{r}") as f:
            logs.append([ln.split() for ln in f.read().splitlines()])
    return logs


class Mismatch(AssertionError):
    pass


def check(logs):
    """The cross-rank rules of the module docstring; returns, per rank, the
    collectives issued and the bytes received per call of the plan."""
    n = len(logs)
    per_rank = []
    for r, log in enumerate(logs):
        if log[0] != ["init", str(r), str(n)] or log[-1] != ["destroy"]:
            raise Mismatch(f"rank {r}: log not framed by init / destroy")
        depth, groups, call = 0, 0, -1
        sends, recvs, colls = collections.defaultdict(list), collections.defaultdict(list), []
        recv_bytes = collections.Counter()
        for ev in log[1:-1]:
            kind = ev[0]
            if kind == "group_start":
                if depth:
                    raise Mismatch(f"rank {r}: nested group")
                depth = 1
            elif kind == "group_end":
                if not depth:
                    raise Mismatch(f"rank {r}: group_end without group_start")
                depth = 0
                groups += 1
            elif kind in ("send", "recv"):
                if not depth:
                    raise Mismatch(f"rank {r}: {kind} outside a group")
                nbytes, ty, peer = int(ev[1]), int(ev[2]), int(ev[3])
                (sends if kind == "send" else recvs)[peer].append((nbytes, ty, groups))
                if kind == "recv":
                    recv_bytes[call] += nbytes
            elif kind in ("allreduce", "reduce_scatter", "reduce"):
                if depth:
                    raise Mismatch(f"rank {r}: collective inside a group")
                colls.append((kind, tuple(ev[1:]), groups))
            elif kind == "note" and ev[1] == "call":
                call = int(ev[2])
        if depth:
            raise Mismatch(f"rank {r}: unterminated group")
        per_rank.append({"groups": groups, "sends": sends, "recvs": recvs, "colls": colls, "recv_bytes": recv_bytes})
    # the same number of groups and the same collectives, at the same places
    for r in range(1, n):
        if per_rank[r]["groups"] != per_rank[0]["groups"]:
            raise Mismatch(f"rank {r}: {per_rank[r]['groups']} groups against {per_rank[0]['groups']} on rank 0")
        if per_rank[r]["colls"] != per_rank[0]["colls"]:
            raise Mismatch(f"rank {r}: collectives differ from rank 0's")
    # every send matched by its peer's recv: bytes, type, group epoch
    for a in range(n):
        for b in range(n):
            s, v = per_rank[a]["sends"].get(b, []), per_rank[b]["recvs"].get(a, [])
            if s != v:
                raise Mismatch(f"sends {a}->{b} {s[:4]}... against recvs at {b} from {a} {v[:4]}...")
    return per_rank


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_config4_allreduce_sequences(harness, n):
    res = check(run_plan(harness, n, CONFIG4, "c4"))
    # RCCL mode: one ncclAllReduce of the whole vector
    kind, args, _ = res[0]["colls"][0]
    assert kind == "allreduce" and args == ("67108864", str(NCCL_F32), str(NCCL_SUM))
    assert len(res[0]["colls"]) == 1          # the reference order uses send / recv only
    # reference order: the reduce-scatter moves the pof2 blocks, the allgather brings
    # back the rest -- every rank ends holding the whole 256 MiB
    pof2 = 1 << (n.bit_length() - 1)
    for r, pr in enumerate(res):
        got = pr["recv_bytes"][1]
        assert got > 0
        if n == pof2:
            # (p - 1) blocks in the reduce-scatter + (p - 1) in the allgather
            assert got == 2 * (n - 1) * (256 << 20) // n, (r, got)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_config5_reduce_scatter_block_sequences(harness, n):
    res = check(run_plan(harness, n, config5(n), "c5"))
    kind, args, _ = res[0]["colls"][0]
    assert kind == "reduce_scatter" and args == (str((1 << 29) // n), str(NCCL_F16), str(NCCL_SUM))
    if n == 8:
        assert args[0] == "67108864"
    # the pairwise schedule: block r from every other rank, one exchange
    for r, pr in enumerate(res):
        assert pr["recv_bytes"][1] == (n - 1) * ((1 << 29) // n) * 2, r
        assert sorted(pr["recvs"]) == sorted(set(range(n)) - {r})


@pytest.mark.parametrize("n", [2, 8])
def test_bench_coll_plan_sequences(harness, n):
    sys.path.insert(0, ROOT)
    import bench_coll
    plan = bench_coll.call_plan(n, warmup=1, steps=2)
    res = check(run_plan(harness, n, plan, "bench"))
    # its RCCL collectives: the self-check's three (+ the flags), then per
    # algorithm pair of each config a barrier and a per-rank gather around the
    # timed calls (3 RCCL calls per RCCL-mode config, 2 per reference-order one)
    kinds = [c[0] for c in res[0]["colls"]]
    assert kinds.count("reduce_scatter") == 1 + 3     # self-check + config 5 rccl x (1 warm-up + 2 timed)
    counts = {c[1][0] for c in res[0]["colls"] if c[0] == "allreduce"}
    assert "67108864" in counts and str(bench_coll.INT_N) in counts


def test_checker_catches_changed_sequences(harness):
    n = 4
    good = run_plan(harness, n, CONFIG4 + config5(n), "mut")
    check(good)

    def mutated(fn):
        logs = [list(map(list, log)) for log in good]
        fn(logs)
        with pytest.raises(Mismatch):
            check(logs)
    # one recv's byte count
    def bytes_(logs):
        i = next(i for i, ev in enumerate(logs[2]) if ev[0] == "recv")
        logs[2][i][1] = str(int(logs[2][i][1]) + 2)
    mutated(bytes_)
    # a send dropped
    def drop(logs):
        i = next(i for i, ev in enumerate(logs[1]) if ev[0] == "send")
        del logs[1][i]
    mutated(drop)
    # a send moved into the next group
    def move(logs):
        i = next(i for i, ev in enumerate(logs[3]) if ev[0] == "send")
        ev = logs[3].pop(i)
        j = next(j for j in range(i, len(logs[3])) if logs[3][j][0] == "group_start")
        logs[3].insert(j + 1, ev)
    mutated(move)
    # a collective's count
    def count(logs):
        i = next(i for i, ev in enumerate(logs[0]) if ev[0] == "reduce_scatter")
        logs[0][i][1] = "1"
    mutated(count)
    # a collective issued inside a group
    def inside(logs):
        i = next(i for i, ev in enumerate(logs[1]) if ev[0] == "allreduce")
        ev = logs[1].pop(i)
        j = next(j for j, e in enumerate(logs[1]) if e[0] == "group_start")
        logs[1].insert(j + 1, ev)
    mutated(inside)


@pytest.mark.parametrize("kb,chunks", [(0, 1), (32768, 4), (65536, 2)])
def test_pipelined_reference_order_chunks(harness, kb, chunks, monkeypatch):
    """Config 5's reference order at N = 8 (8 x 128 MiB blocks): with
    MPIR_CVAR_DEVICE_COLL_PIPELINE_KB = chunk, the exchange runs in
    128 MiB / chunk groups and the CHAIN8 fold in as many chunk folds, each
    chunk's fold after its group (coll_hip.c exchange_fold_pipelined); 0 turns
    the pipeline off.  The cross-rank rules hold either way."""
    monkeypatch.setenv("MPIR_CVAR_DEVICE_COLL_PIPELINE_KB", str(kb))
    n = 8
    logs = run_plan(harness, n, [config5(n)[1]], f"pipe{kb}")
    res = check(logs)
    for r, log in enumerate(logs):
        assert res[r]["groups"] == chunks
        folds = [ev for ev in log if ev[:2] == ["note", "combine"]]
        assert len(folds) == chunks
        assert sum(int(ev[3]) for ev in folds) == (1 << 29) // n          # every element folded once
        assert all(ev[2] == "8" and ev[-1] == "chain" for ev in folds)
        # each fold follows its chunk's group
        pos = [i for i, ev in enumerate(log) if ev[0] == "group_end"]
        fpos = [i for i, ev in enumerate(log) if ev[:2] == ["note", "combine"]]
        assert all(f > g for f, g in zip(fpos, pos))


@pytest.mark.parametrize("n", [3, 5, 6, 7])
def test_pipelined_allreduce_non_pof2(harness, n):
    """Config 4's reference order at rank counts with a pre-fold (excluded
    ranks take part in every chunk's group with no transfers): the blocks of
    256 MiB / pof2 are pipelined, and the sequences still match."""
    logs = run_plan(harness, n, [CONFIG4[1]], "arnp")
    res = check(logs)
    pof2 = 1 << (n.bit_length() - 1)
    block = (256 << 20) // pof2
    chunks = -(-block // (32 << 20))
    # pre-fold group + reduce-scatter chunks + allgather chunks
    assert all(pr["groups"] == 1 + 2 * chunks for pr in res), [pr["groups"] for pr in res]


# ---------------------------------------------------------------- the pinned sweep
# Every rank's complete log -- every HIP call, kernel launch and RCCL call of
# coll_hip.c with its operands, streams and events by name (coll_trace.c) -- over
# a plan that walks every branch of the file, hashed and compared with the
# digests in tests/golden/coll_trace/digests.txt.  The digests are generated from
# the coll_hip.c of the commit BEFORE a rewrite, never from the rewritten file:
#     git show <parent>:mpich-pip_amd/csrc/host/coll_hip.c > /tmp/coll_hip_parent.c
#     python tests/test_rccl_sequence_cpu.py --write-golden --source /tmp/coll_hip_parent.c
# reproduces the committed file byte for byte; --dump DIR writes the full logs
# (DIR/<case>_n<n>.<rank>) to diff when a digest differs.
GOLDEN = os.path.join(ROOT, "tests", "golden", "coll_trace", "digests.txt")
SWEEP_ENVS = {
    "default": {},
    "flat": {"MPIR_CVAR_ENABLE_SMP_COLLECTIVES": "0"},                  # recursive doubling
    "maxsmp1": {"MPIR_CVAR_MAX_SMP_ALLREDUCE_MSG_SIZE": "1"},           # recursive doubling / Rabenseifner
    "pipe1": {"MPIR_CVAR_DEVICE_COLL_PIPELINE_KB": "1"},                # pipelined at small sizes
    "pipe0": {"MPIR_CVAR_DEVICE_COLL_PIPELINE_KB": "0"},
}
LONG = 100003        # fp32: 400012 bytes, odd (not divisible by pof2), one chunk at the default
                     # 32 MiB; at PIPELINE_KB=1 its blocks take 16 chunks, more than MAX_PIPE at n = 8
RS_LONG = 131072     # fp32 elements in 524288 bytes (RSB_COMMUTATIVE_LONG_MSG_SIZE)
VARIANTS = [(), ("inplace",), ("ustream",), ("inplace", "ustream")]


def ragged(total, n):
    """Per-rank counts summing to total: a zero count (n >= 3) and, at rank 1, a
    block that starts inside its own length (in place it overlaps the output)."""
    if n == 1:
        return [[total]]
    if n == 2:
        return [[3, total - 3], [0, total]]
    q = (total - 3) // (n - 1)
    return [[3, total - 3 - q * (n - 3), 0] + [q] * (n - 3)]


def sweep_plan(n):
    pof2 = 1 << (n.bit_length() - 1)
    counts = sorted({1, pof2 - 1, 512, 513, LONG} - {0})
    # reduce-scatter totals just below and at 524288 bytes
    at = -(-RS_LONG // n)
    rsb = sorted(set(counts) | {at - 1, at})
    rs = [[3, 5, 0, 2, 7, 1, 4, 6][:n]] + ragged(RS_LONG - 1, n) + ragged(RS_LONG, n)
    plan = []
    for v in VARIANTS:
        for alg in ("rccl", "ref"):
            for c in counts:
                plan.append(("allreduce", c, "f32", "sum", alg) + v)
                for root in sorted({0, n - 1}):
                    plan.append(("reduce", c, "f32", "sum", alg, root) + v)
            for c in rsb:
                plan.append(("reduce_scatter_block", c, "f32", "sum", alg) + v)
        for cs in rs:
            plan.append(("reduce_scatter", ",".join(map(str, cs)), "f32", "sum", "ref") + v)
        for c in counts:
            plan.append(("scan", c, "f32", "sum") + v)
            plan.append(("exscan", c, "f32", "max") + v)
    # esz != 4: 1025 fp16 elements are 2050 bytes, just past the short-message switch
    for what in ("allreduce", "reduce", "reduce_scatter_block", "scan"):
        plan.append((what, 1025, "f16", "sum", "ref"))
    # called from another device than the communicator's: switched and put back
    plan.append(("device", 1))
    for what in ("allreduce", "reduce", "reduce_scatter_block", "scan"):
        plan += [(what, 513, "f32", "sum", "ref"), (what, 513, "f32", "sum", "rccl", "ustream")]
    plan.append(("device", 0))
    return plan


def pinned_cases():
    for name in SWEEP_ENVS:
        for n in range(1, 9):
            yield name, n
    for n in range(2, 9):
        yield "config4", n
        yield "config5", n


def run_case(harness, name, n):
    """check() on the case's logs; returns the digest of each rank's log file."""
    if name == "config4":
        plan, env = CONFIG4, {}
    elif name == "config5":
        plan, env = config5(n), {}
    else:
        plan, env = sweep_plan(n), SWEEP_ENVS[name]
    check(run_plan(harness, n, plan, name, env=env))
    out = []
    for r in range(n):
        with open(harness[0] / f"{name}_n{n}.{r}", "rb") as f:
            out.append(hashlib.sha256(f.read()).hexdigest())
    return out


def read_golden():
    with open(GOLDEN) as f:
        return {tuple(ln.split()[:3]): ln.split()[3] for ln in f if ln.strip() and not ln.startswith("#")}


def differing(harness, cases, golden):
    bad = []
    for name, n in cases:
        for r, h in enumerate(run_case(harness, name, n)):
            if golden.get((name, str(n), str(r))) != h:
                bad.append(f"{name} n={n} rank {r}")
    return bad


@pytest.mark.parametrize("name", list(SWEEP_ENVS) + ["config4", "config5"])
def test_pinned_trace(harness, name):
    golden = read_golden()
    cases = [c for c in pinned_cases() if c[0] == name]
    assert len(golden) == sum(n for _, n in pinned_cases())
    bad = differing(harness, cases, golden)
    assert not bad, (f"{len(bad)} logs differ from {os.path.relpath(GOLDEN, ROOT)}: {bad[:6]}...  Dump the logs of the "
                     "commit the digests came from and of this tree with `python tests/test_rccl_sequence_cpu.py "
                     "--dump DIR [--source PATH]` and diff DIR/<case>_n<n>.<rank>")


# one small edit to coll_hip.c at a time; each must change some digest
def in_function(name, edit):
    def apply(src):
        a = src.index("\nstatic int " + name + "(")
        b = src.index("\n}\n", a)
        body = edit(src[a:b])
        assert body != src[a:b], name
        return src[:a] + body + src[b:]
    return apply


def swap_streams(body):
    body = body.replace("c->fold_stream", "\0")
    body = body.replace(", s)", ", c->fold_stream)").replace("(s, ", "(c->fold_stream, ")
    return body.replace("\0", "s")


MUTANTS = {
    # the exchanges and their events on the fold stream, the folds on the exchange's
    "streams_swapped": in_function("exchange_fold_pipelined", swap_streams),
    "fold_step_operands_swapped": in_function(
        "fold_step", lambda b: b.replace("MPIR_Hip_reduce(src, dst,", "MPIR_Hip_reduce(dst, src,")),
    # the owner's received blocks read one staging slot too far
    "slot_off_by_one": in_function(
        "rsg_phase", lambda b: b.replace("scr + (size_t) (i - 1) * ", "scr + (size_t) i * ")),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_pinned_trace_catches_mutants(tmp_path, mutant):
    if not have_headers():
        pytest.skip("needs the ROCm headers (rccl.h, hip_runtime_api.h) to compile against")
    with open(os.path.join(HOST, "coll_hip.c")) as f:
        src = MUTANTS[mutant](f.read())
    (tmp_path / "coll_hip.c").write_text(src)
    h = build_harness(tmp_path, str(tmp_path / "coll_hip.c"))
    # n = 5: a pre-fold (fold_step), pof2 = 4 (staging slots); pipe1: the pipeline runs
    assert differing(h, [("pipe1", 5)], read_golden())


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description="write the pinned sweep's digests or full logs")
    ap.add_argument("--write-golden", action="store_true", help="write " + os.path.relpath(GOLDEN, ROOT))
    ap.add_argument("--dump", metavar="DIR", help="write every case's full logs into DIR")
    ap.add_argument("--source", metavar="PATH", help="the coll_hip.c to build against (default: the tree's)")
    args = ap.parse_args(argv)
    if not (args.write_golden or args.dump):
        ap.error("nothing to do")
    with tempfile.TemporaryDirectory() as d:
        h = build_harness(d, args.source and os.path.abspath(args.source))
        lines = []
        for name, n in pinned_cases():
            for r, digest in enumerate(run_case(h, name, n)):
                lines.append(f"{name} {n} {r} {digest}\n")
                if args.dump:
                    os.makedirs(args.dump, exist_ok=True)
                    shutil.copyfile(h[0] / f"{name}_n{n}.{r}", os.path.join(args.dump, f"{name}_n{n}.{r}"))
    if args.write_golden:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            f.write("# <case> <ranks> <rank> <sha256 of the rank's log>; generated by\n"
                    "# python tests/test_rccl_sequence_cpu.py --write-golden --source <coll_hip.c of the parent commit>\n")
            f.writelines(lines)


if __name__ == "__main__":
    main(sys.argv[1:])
