#!/usr/bin/env python3
"""MPIX_Compare_and_swap_indexed_ordered against the nearest calls a caller had
before it, whose code the compare-and-swap does not touch.

Indexed shapes: 65,536 entries of MPI_INT and of MPI_LONG, every target named
exactly R times (R = 1, 4, 64) in a shuffled table, and `one`: every entry on one
target.  Targets sit two elements apart, disp_unit the element's size; origin,
compare and result are packed.  Two ways alternate:
  cas      one MPIX_Compare_and_swap_indexed_ordered, the order table built before
  replace  one MPIX_Reduce_local_fetch_indexed_ordered with MPI_REPLACE and
           blocklen 1 on the same tables: the unconditional swap.  The CAS reads
           one more packed stream: at most 5 : 4 by the bytes per entry, the
           tables not counted.
Contiguous shapes: MPI_LONG, 16 KiB and 256 MiB per operand, target_displs NULL:
  cas      one MPIX_Compare_and_swap_indexed_ordered (five streams)
  fetch    one MPIX_Reduce_local_fetch with MPI_BXOR (four streams): the byte
           bound of cas / fetch is 1.25.  For cas the bytes of its five streams
           over the time of the whole synchronous call are printed as a share of
           the 8 TB/s peak (a call's share, not a kernel trace's).
Values come from three words per size, so about a third of the compares succeed
(the kernel stores a target only where a run swapped).  Before a shape is timed
the CAS is checked against a loop in table order (contiguous: against torch).

The parent starts one child process per step -- a library and a group of shapes --
each under its own time limit, over `rounds` alternated rounds, and stops at the
first step that fails.  A child warms every way, then alternates the ways over
five inner rounds, host clock stamps around synchronous calls, and prints the
median per way.  The parent reports the median of the rounds' medians and their
lowest and highest, and writes the log.

kCasAhead: a second library built with -DMPIR_CAS_AHEAD=1 (the same sources) can
be named with --alt DIR (DIR holds libmpich_reduce_local.so and libmpir_hip.so);
its indexed steps then alternate with the default library's, round by round.

    python3 tools/cas_ab.py [--rounds 3] [--alt DIR] [--out profiles/cas/cas_ab.log]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
sys.path.insert(0, ROOT)

KIB, MIB = 1 << 10, 1 << 20
COUNT = 65536
FACTORS = ["1", "4", "64", "one"]
W = 0x5A3C96E17B2D48F1
STEP_LIMIT = 420            # seconds per child
PEAK = 8e12                 # bytes/s


def letters(np, n):
    bits = 8 * n
    w = W & ((1 << bits) - 1)
    return np.array([w, w ^ 1, w ^ (1 << (bits - 1))], np.dtype(f"uint{bits}")).view(np.dtype(f"int{bits}"))


def timed(run, ways, inner=5):
    """every way warmed, then alternated over `inner` rounds; the median per way, us"""
    import numpy as np
    for w in ways:
        run(w)
        run(w)
    est = {}
    for w in ways:
        t0 = time.perf_counter_ns()
        run(w)
        est[w] = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
    reps = {w: int(min(100, max(3, 10000 / est[w]))) for w in ways}
    t = {w: [] for w in ways}
    for r in range(inner):
        for w in (ways if r % 2 == 0 else ways[::-1]):
            for _ in range(reps[w]):
                t0 = time.perf_counter_ns()
                run(w)
                t[w].append((time.perf_counter_ns() - t0) / 1e3)
    return {w: float(np.median(t[w])) for w in ways}


def child(group, libdir):
    import numpy as np
    import mpich_pip_amd as m
    lib = m.load(os.path.join(libdir, "libmpich_reduce_local.so") if libdir else None)
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    bench.bind_near_gpu(m, 0)
    out = {"build": m.build_id(), "device": torch.cuda.get_device_name(0), "rows": {}}
    if group == "indexed":
        for t, n, tdt in (("MPI_INT", 4, torch.int32), ("MPI_LONG", 8, torch.int64)):
            dt = m.DATATYPES[t]
            al = letters(np, n)
            for f in FACTORS:
                R = COUNT if f == "one" else int(f)
                distinct = COUNT // R
                rng = np.random.default_rng([n, R])
                which = rng.permutation(np.repeat(np.arange(distinct), R))
                tab = (rng.permutation(COUNT)[:distinct][which] * 2).astype(np.int64)
                horder = np.argsort(tab, kind="stable").astype(np.int32)
                tv = al[rng.integers(0, 3, 2 * COUNT)]
                ov, cv = al[rng.integers(0, 3, COUNT)], al[rng.integers(0, 3, COUNT)]
                dtab, dtv, dov, dcv = (torch.from_numpy(x).cuda() for x in (tab, tv, ov, cv))
                dres = torch.empty(COUNT, dtype=tdt, device="cuda")
                dorder = torch.empty(COUNT, dtype=torch.int32, device="cuda")
                rc = m.reduce_local_order(dtab.data_ptr(), COUNT, dorder.data_ptr())
                assert rc == 0, m.error_string(rc)
                assert np.array_equal(dorder.cpu().numpy(), horder), "MPIX_Reduce_local_order != stable argsort"
                info = m.cas_plan_info(dov.data_ptr(), dcv.data_ptr(), dtv.data_ptr(), dtab.data_ptr(), dres.data_ptr(),
                                       dorder.data_ptr(), n, COUNT, dt)

                def run(way):
                    if way == "cas":
                        rc = m.compare_and_swap_indexed_ordered(dov.data_ptr(), dcv.data_ptr(), dtv.data_ptr(), dtab.data_ptr(),
                                                                dres.data_ptr(), dorder.data_ptr(), n, COUNT, dt)
                    else:
                        rc = m.reduce_local_fetch_indexed_ordered(dov.data_ptr(), None, dtv.data_ptr(), dtab.data_ptr(),
                                                                  dres.data_ptr(), dorder.data_ptr(), n, COUNT, 1, dt,
                                                                  m.MPI_REPLACE)
                    assert rc == 0, m.error_string(rc)

                # the CAS against a loop in table order
                want, rwant, swaps = tv.tolist(), [], 0
                for j, o, c in zip(tab.tolist(), ov.tolist(), cv.tolist()):
                    rwant.append(want[j])
                    if want[j] == c:
                        want[j] = o
                        swaps += 1
                run("cas")
                assert np.array_equal(dtv.cpu().numpy(), np.array(want, tv.dtype)), f"{t} R {f}: targets != the loop's"
                assert np.array_equal(dres.cpu().numpy(), np.array(rwant, tv.dtype)), f"{t} R {f}: result != the loop's"
                med = timed(run, ["cas", "replace"])
                out["rows"][f"{t} R {f}"] = {"cas": med["cas"], "replace": med["replace"], "ahead": info["ahead"],
                                             "groups": info["groups"], "swap_share": round(swaps / COUNT, 3)}
    else:
        t, n, dt = "MPI_LONG", 8, m.DATATYPES["MPI_LONG"]
        al = torch.from_numpy(letters(np, n)).cuda()
        for nbytes in (16 * KIB, 256 * MIB):
            count = nbytes // n
            g = torch.Generator(device="cuda").manual_seed(nbytes)
            tv, ov, cv = (al[torch.randint(0, 3, (count,), device="cuda", generator=g)] for _ in range(3))
            res = torch.empty_like(tv)
            info = m.cas_plan_info(ov.data_ptr(), cv.data_ptr(), tv.data_ptr(), None, res.data_ptr(), None, n, count, dt)
            assert info["form"] == m.CAS_CONTIG_TILE, info

            def run(way):
                if way == "cas":
                    rc = m.compare_and_swap_indexed_ordered(ov.data_ptr(), cv.data_ptr(), tv.data_ptr(), None, res.data_ptr(),
                                                            None, n, count, dt)
                else:
                    rc = m.reduce_local_fetch(ov.data_ptr(), tv.data_ptr(), res.data_ptr(), count, dt, m.MPI_BXOR)
                assert rc == 0, m.error_string(rc)

            old = tv.clone()
            run("cas")
            assert torch.equal(res, old) and torch.equal(tv, torch.where(old == cv, ov, old)), f"{nbytes} B: cas != torch"
            share = float((old == cv).float().mean())
            del old
            med = timed(run, ["cas", "fetch"])
            out["rows"][f"{t} contiguous {nbytes} B"] = {"cas": med["cas"], "fetch": med["fetch"], "groups": info["groups"],
                                                         "swap_share": round(share, 3)}
            del tv, ov, cv, res
            torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)


def main(rounds, alt, outpath):
    import numpy as np
    steps = [("indexed", None, "default")] + ([("indexed", alt, "alt")] if alt else []) + [("contig", None, "default")]
    got = {}                # (label, row) -> way -> [a median per round]
    lines = []
    for r in range(rounds):
        for group, libdir, label in (steps if r % 2 == 0 else steps[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", group] + (["--lib", libdir] if libdir else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            rec = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode or not rec:
                sys.exit(f"step {group} ({label}) round {r} failed with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            d = json.loads(rec[-1][6:])
            print(f"round {r}: {group} ({label} library) done", flush=True)
            if r == 0:
                lines.append(f"{label} library, {group}: build {d['build']}; {d['device']}")
            for row, v in d["rows"].items():
                for way in ("cas", "replace", "fetch"):
                    if way in v:
                        got.setdefault((label, row), {}).setdefault(way, []).append(v[way])
                got[(label, row)]["meta"] = {k: v[k] for k in v if k not in ("cas", "replace", "fetch")}
    for (label, row), ways in got.items():
        meta = ways.pop("meta")
        med = {w: float(np.median(v)) for w, v in ways.items()}
        base = "replace" if "replace" in med else "fetch"
        text = f"{label:7s} {row:32s} " + "  ".join(f"{w} {med[w]:.2f} us [{min(v):.2f}, {max(v):.2f}]" for w, v in ways.items())
        text += f"  cas/{base} {med['cas'] / med[base]:.3f}  {meta}"
        if "contiguous" in row:
            nbytes = int(row.split()[2])
            text += f"  cas: {5 * nbytes / med['cas'] / 1e-6 / PEAK:.3f} of the 8 TB/s peak by the call's time"
        lines.append(text)
    lines.append(f"rounds {rounds} (each a fresh process per step; medians of the rounds' medians, [lowest, highest])")
    os.makedirs(os.path.dirname(os.path.abspath(outpath)), exist_ok=True)
    with open(outpath, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    a = sys.argv[1:]

    def opt(name, default):
        return a[a.index(name) + 1] if name in a else default

    if "--child" in a:
        child(opt("--child", "indexed"), opt("--lib", None))
    else:
        main(int(opt("--rounds", "3")), opt("--alt", None), opt("--out", os.path.join(ROOT, "profiles", "cas", "cas_ab.log")))
