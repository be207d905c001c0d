"""When the device collectives' steps run relative to one another, without a GPU.

csrc/host/coll_hip.c spreads one collective over two streams (the exchanges on
the call's stream, the pipelined folds on fold_stream, tied by xev[k] / fev[k]),
reuses one staging scratch per communicator, and on a caller's stream never
synchronises with the host, so two calls in a row overlap.  Every correct result
then rests on a handful of hipStreamWaitEvent lines.  test_rccl_sequence_cpu.py
already runs the unchanged coll_hip.c against recording stand-ins and logs
every copy, fold, send, recv, event record, stream wait, sync, malloc and free;
its digests say the sequence did not change.  tests/_coll_order.py builds the
happens-before order from the same logs and says whether the sequence is free
of races (its docstring has the model and the six rules).  Checked here:
  * every pinned case of test_rccl_sequence_cpu.py (the five SWEEP_ENVS at
    N = 1..8, config 4 and 5 at N = 2..8; their `ustream` lines run back to back);
  * a plan in which every line is `ustream` with no synchronisation between
    them (stream_plan), at N = 2, 3, 5, 8 with MPIR_CVAR_DEVICE_COLL_PIPELINE_KB
    = 64, 1 (more than MAX_PIPE chunks, re-sized) and 0;
  * source mutants: each removes or misplaces one wait (or one index) in a
    temporary copy of coll_hip.c and must be reported under its rule, while
    the unmutated copy is reported clean.
The mutants run stream_plan at N = 5 and N = 8 at PIPELINE_KB = 64 and 1: at 64
the plan's reduce-scatters are pipelined (blocks of 160004 bytes and more), its
Allreduce / Reduce (blocks of 65540 bytes, under two chunks) only at 1, and
exchange_after_folds and the wait before rsg_gather run in those alone.
"""
import os

import pytest

import _coll_order as O
from test_rccl_sequence_cpu import (CONFIG4, HOST, MUTANTS, SWEEP_ENVS, build_harness, config5, have_headers,
                                    in_function, run_plan, sweep_plan)

PIPE = "MPIR_CVAR_DEVICE_COLL_PIPELINE_KB"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not have_headers():
        pytest.skip("needs the ROCm headers (rccl.h, hip_runtime_api.h) to compile against")
    return build_harness(tmp_path_factory.mktemp("coll_order"))


def ragged_pipe(n):
    """Reduce_scatter counts in the manner of test_coll_loopback_gpu._pipe_counts
    (fp32, 64 KiB chunks): a block of several chunks with a ragged end, a zero
    count (n >= 3), a block shorter than one chunk, counts larger than their
    displacement (in place the own block overlaps the output and is staged);
    >= 524288 bytes in all, so the pairwise schedule runs."""
    counts = {2: [5000, 160003], 3: [5000, 0, 160003], 5: [5000, 0, 40001, 1, 200003],
              8: [5000, 0, 40001, 70001, 1, 33000, 16384, 200003]}[n]
    disps = [sum(counts[:i]) for i in range(n)]
    assert sum(counts) * 4 >= 524288 and max(counts) * 4 >= 4 * 65536 and 0 < counts[0] * 4 < 65536
    assert 0 < disps[-1] < counts[-1]
    return counts


def stream_plan(n):
    """Every line on the caller's stream, nothing between them; twice: where
    the scratch grows comm_scratch synchronises the device, which orders
    everything, and the second pass finds the scratch grown."""
    pof2 = 1 << (n.bit_length() - 1)
    big = pof2 * 16384 + 5
    u = ("ustream",)
    return 2 * [("allreduce", big, "f32", "sum", "ref") + u,
            ("allreduce", big, "f32", "sum", "ref", "inplace") + u,
            ("reduce", big, "f32", "sum", "ref", 0) + u,
            ("reduce", big, "f32", "sum", "ref", n - 1) + u,
            ("reduce_scatter_block", 40001, "f32", "sum", "ref") + u,
            ("reduce_scatter", ",".join(map(str, ragged_pipe(n))), "f32", "sum", "ref", "inplace") + u,
            ("allreduce", 3, "f32", "sum", "ref") + u,
            ("scan", big, "f32", "sum") + u,
            ("exscan", big, "f32", "sum") + u]


@pytest.mark.parametrize("name", list(SWEEP_ENVS) + ["config4", "config5"])
def test_pinned_cases_are_ordered(harness, name):
    for n in range(1 if name in SWEEP_ENVS else 2, 9):
        if name == "config4":
            plan, env = CONFIG4, {}
        elif name == "config5":
            plan, env = config5(n), {}
        else:
            plan, env = sweep_plan(n), SWEEP_ENVS[name]
        O.check_order(run_plan(harness, n, plan, "ord_" + name, env=env), f"{name} n={n}")


@pytest.mark.parametrize("kb", [64, 1, 0])
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_back_to_back_on_a_callers_stream(harness, n, kb):
    logs = run_plan(harness, n, stream_plan(n), f"stream{kb}", env={PIPE: str(kb)})
    O.check_order(logs, f"stream_plan n={n} PIPELINE_KB={kb}")
    # the plan does what it is there for: no host synchronisation anywhere but
    # where the scratch grows (and when the communicator is freed), none at all
    # in the second pass, and (kb > 0) folds on a second stream
    for log in logs:
        syncs = [i for i, ev in enumerate(log) if ev[:2] in (["note", "stream_sync"], ["note", "device_sync"])]
        assert all(log[i + 1][:2] in (["note", "device_sync"], ["note", "free"], ["destroy"]) for i in syncs)
        second = log.index(["note", "call", str(len(stream_plan(n)) // 2), "allreduce"])
        assert all(i < second or log[i + 1] == ["destroy"] for i in syncs)
    # (a rank the pre-fold excludes, with a zero count of its own, folds nothing)
    folds = {ev[5] for log in logs for ev in log if ev[:3] == ["note", "+", "combine"]}
    assert ("stream=s1" in folds) == (kb > 0), folds


def test_checker_on_edited_logs(harness):
    """The rules that no source mutant reaches, on logs edited by hand: a wait
    for an event that was never recorded is an error; a call on the
    communicator's stream whose closing hipStreamSynchronize is gone breaks the
    exit rule in that mode too."""
    n = 5
    plan = [("reduce_scatter_block", 40001, "f32", "sum", "ref"), ("allreduce", 3, "f32", "sum", "ref")]
    good = run_plan(harness, n, plan, "edit", env={PIPE: "64"})
    assert O.analyse(good) == []

    def edited(rank, match):
        logs = [list(log) for log in good]
        del logs[rank][next(i for i, ev in enumerate(logs[rank]) if match(ev))]
        return O.analyse(logs)
    bad = edited(2, lambda ev: ev[:2] == ["note", "event_record"])
    assert 0 in O.rules_of(bad) and all(v.rank == 2 for v in bad)
    bad = edited(3, lambda ev: ev[:2] == ["note", "stream_sync"])
    assert O.rules_of(bad) == [3] and all(v.rank == 3 and v.call == 0 for v in bad)


def without(text):
    def edit(body):
        assert body.count(text) == 1, text
        return body.replace(text, "")
    return edit


ORDER_MUTANTS = {
    # the fold of chunk k no longer waits for chunk k's exchange
    "fold_without_xev_wait": (1, in_function("exchange_fold_pipelined", lambda b: b.replace(
        " ||\n            (e = hipStreamWaitEvent(c->fold_stream, c->xev[k], 0)) != hipSuccess)", ")"))),
    # chunk k of the allgather leaves without waiting for its fold / waits for fold 0 only
    "allgather_without_fev_wait": (1, in_function("exchange_after_folds", without(
        "        HIPTRY(hipStreamWaitEvent(f->s, f->c->fev[k], 0));\n"))),
    "allgather_waits_for_fev0": (1, in_function("exchange_after_folds", lambda b: b.replace(
        "f->c->fev[k]", "f->c->fev[0]"))),
    # the call's stream never joins the fold stream at the end of a reduce-scatter
    "reduce_scatter_without_final_wait": (3, in_function("reduce_scatter_schedule", without(
        "        HIPTRY(hipStreamWaitEvent(s, c->fev[nchunk - 1], 0));\n"))),
    # the gather to the root leaves before the last fold
    "reduce_gather_without_wait": ((1, 3), in_function("reduce_schedule", without(
        "    if (g.nchunk > 1)\n        HIPTRY(hipStreamWaitEvent(s, c->fev[g.nchunk - 1], 0));     /* every fold done */\n"))),
    # the scratch is freed while earlier calls may still use it
    "free_without_syncs": (5, in_function("comm_scratch", lambda b: without(
        "            (void) hipDeviceSynchronize();\n")(without("            (void) hipStreamSynchronize(c->stream);\n")(b)))),
    # (test_rccl_sequence_cpu.MUTANTS) the owner's received blocks read one staging slot too far
    "slot_off_by_one": (4, MUTANTS["slot_off_by_one"]),
}
# test_rccl_sequence_cpu.MUTANTS' other two have tests of their own below


def run_source(tmp_path, src):
    """The violations of stream_plan at N = 5 and 8, PIPELINE_KB = 64 and 1,
    with the harness built from `src`: {n: [Violation]}."""
    (tmp_path / "coll_hip.c").write_text(src)
    h = build_harness(tmp_path, str(tmp_path / "coll_hip.c"))
    return {n: [v for kb in (64, 1) for v in O.analyse(run_plan(h, n, stream_plan(n), f"m{kb}", env={PIPE: str(kb)}))]
            for n in (5, 8)}


@pytest.fixture(scope="module")
def source():
    if not have_headers():
        pytest.skip("needs the ROCm headers (rccl.h, hip_runtime_api.h) to compile against")
    with open(os.path.join(HOST, "coll_hip.c")) as f:
        return f.read()


@pytest.fixture(scope="module")
def control(source, tmp_path_factory):
    """An unmutated temporary copy, built and run the way the mutants are."""
    return run_source(tmp_path_factory.mktemp("control"), source)


@pytest.mark.parametrize("mutant", list(ORDER_MUTANTS))
def test_checker_reports_mutants(tmp_path, source, control, mutant):
    rules, edit = ORDER_MUTANTS[mutant]
    rules = rules if isinstance(rules, tuple) else (rules,)
    assert control == {5: [], 8: []}, O.describe((control[5] + control[8])[0])
    for n, bad in run_source(tmp_path, edit(source)).items():
        assert set(rules) & set(O.rules_of(bad)), (f"{mutant} at n={n}: expected rule {rules}, reported "
                                                   f"{O.rules_of(bad)}: " + "; ".join(map(O.describe, bad[:3])))
        for v in bad:       # each report names the rank, the call, both log lines and the bytes
            assert 0 <= v.rank < n and v.call >= 0 and v.first and v.second and (v.rule in (0,) or v.hi > v.lo)


def test_streams_swapped_is_an_entry_violation(tmp_path, source):
    """The streams_swapped mutant puts the exchanges on the fold stream and
    the folds on the call's.  The call's stream still waits for xev[k] before
    each fold, so it joins every exchange: behind the call nothing is left
    unordered and the exit rule (3) holds.  What breaks is the entry: the
    exchanges read send / recv on a stream that never waited for the caller's
    (rule 2), and race with the call's own copies and pre-fold (rule 1)."""
    for n, bad in run_source(tmp_path, MUTANTS["streams_swapped"](source)).items():
        assert {1, 2} <= set(O.rules_of(bad)) and 3 not in O.rules_of(bad), (n, O.rules_of(bad))


def test_fold_step_operands_swapped_is_out_of_reach(tmp_path, source):
    """fold_step_operands_swapped changes which operand a pre-fold step
    overwrites: data flow, not ordering.  Every step stays on the call's
    stream, reads bytes the same call wrote and writes a slot (or the partner's
    staged vector) that only the same stream touches afterwards, so no rule of
    the checker is broken: it is outside its reach.  The digests of
    test_pinned_trace_catches_mutants and the bit-exact GPU tests catch it."""
    assert run_source(tmp_path, MUTANTS["fold_step_operands_swapped"](source)) == {5: [], 8: []}
