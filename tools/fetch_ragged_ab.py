#!/usr/bin/env python3
"""MPIX_Reduce_local_fetch_ragged against what exists without it.  Per shape --
tools/ragged_ab.py's: pieces of unequal length, the origin data and the response
buffer packed, the target's pieces laid out in a random order (a permuted table
of displacements in units of 16 bytes, or of the element where the pieces are
not 16-byte multiples) -- these ways alternate over rounds in one process,
MPI_SUM on device buffers, fp32 and fp64:
  fetch_ragged   one synchronous MPIX_Reduce_local_fetch_ragged, device tables
  copies+ragged  what a caller does today: one device copy per piece of the
                 target into fetchbuf (MPIR_Hip_memcpy, driven from this script),
                 then one synchronous MPIX_Reduce_local_ragged.  Up to 256
                 pieces only: at 65,536 pieces the copy loop alone runs to about
                 half a second, and is not timed.
  ragged         MPIX_Reduce_local_ragged alone on the same pieces: three
                 streams where the new call moves four
  fetch          MPIX_Reduce_local_fetch on the same byte count, all three
                 buffers contiguous: the price of the shape
The last three are the yardsticks and run the code this call did not change.
Every shape is warmed in every way; each repetition takes the next of several
distinct buffer sets (at least 1 GiB of operands in rotation once a set is above
1 MiB); host clock stamps around calls that end in completion; medians over all
repetitions, us, with the lowest and highest median of a single round.  Before a
shape is timed the ways' results are compared bit for bit: the target against
the ragged call's, fetchbuf against a gather of the old target (and against the
per-piece copies where those run), and the plan's launch count is read.

    python3 tools/fetch_ragged_ab.py [rounds = 5] [shapes = all] [ways = all]
    shapes: comma-separated names out of SHAPES below
    ways: comma-separated, e.g. fetch_ragged alone for a profiler run
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mpich_pip_amd as m  # noqa: E402  (the library first: VRAM rings)
from ragged_ab import lengths, spread  # noqa: E402

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
SHAPES = ["64k_1to127", "64k_16Bx", "4k_32to96K", "n2", "n8", "n32", "n128", "n256"]
COPY_LOOP_MAX = 256


def set_count(total):
    return 4 if total <= MIB else max(4, min(16, -(-GIB // (4 * total))))


def main(rounds, shapes, only):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    state = lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    vp = ctypes.c_void_p
    lib.MPIR_Hip_memcpy.argtypes = [vp, vp, ctypes.c_size_t]
    lib.MPIR_Hip_memcpy.restype = ctypes.c_int
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for name in shapes:
        for esz in (4, 8):
            dt = m.MPI_DOUBLE if esz == 8 else m.MPI_FLOAT
            fdt = torch.float64 if esz == 8 else torch.float32
            ity = torch.int64 if esz == 8 else torch.int32
            rng = np.random.default_rng([len(name), esz])
            nbytes = lengths(name, esz, rng).astype(np.int64)
            nb = len(nbytes)
            unit = 16 if not (nbytes % 16).any() else esz
            # the pieces one after the other in a random order, each at the next multiple of unit
            order = rng.permutation(nb)
            at = np.zeros(nb, np.int64)
            at[order] = np.concatenate(([0], np.cumsum(-(-nbytes[order] // unit) * unit)[:-1]))
            tab = at // unit
            extent = int((-(-nbytes // unit) * unit).sum())
            lens = nbytes // esz
            starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
            count = int(starts[-1])
            total = count * esz
            nsets = set_count(total)
            pk_set = -(-total // 16384) * 16384
            io_set = -(-extent // 16384) * 16384
            pool_in = torch.rand((nsets * pk_set + 16384) // esz, device="cuda", dtype=fdt) * 1e-3
            pool_fe = torch.zeros((nsets * pk_set + 16384) // esz, device="cuda", dtype=fdt)
            pool_io = torch.rand((nsets * io_set + 16384) // esz, device="cuda", dtype=fdt)
            base = {k: p.data_ptr() + (-p.data_ptr() % 16384) for k, p in (("in", pool_in), ("fe", pool_fe), ("io", pool_io))}
            pools = {"in": (pool_in, pk_set), "fe": (pool_fe, pk_set), "io": (pool_io, io_set)}
            dtab, dstarts = torch.from_numpy(tab).cuda(), torch.from_numpy(starts).cuda()
            # the old target's element behind each packed element
            gather = torch.from_numpy(np.repeat(at // esz - starts[:-1], lens) + np.arange(count)).cuda()
            torch.cuda.synchronize()

            def ptr(k, s):
                return base[k] + s * pools[k][1]

            def view(k, s):
                pool, size = pools[k]
                lo = (ptr(k, s) - pool.data_ptr()) // esz
                return pool[lo:lo + size // esz]

            ways = tuple(w for w in ("fetch_ragged", "copies+ragged", "ragged", "fetch")
                         if (w != "copies+ragged" or nb <= COPY_LOOP_MAX) and (not only or w in only))
            info = m.fetch_ragged_plan_info(ptr("in", 0), ptr("io", 0), dtab.data_ptr(), ptr("fe", 0), dstarts.data_ptr(), unit,
                                            nb, count, dt, m.MPI_SUM)
            assert info["launches"] == 1, info

            def run(way, s):
                pi, po, pf = ptr("in", s), ptr("io", s), ptr("fe", s)
                if way == "fetch_ragged":
                    rc = lib.MPIX_Reduce_local_fetch_ragged(vp(pi), vp(po), vp(dtab.data_ptr()), vp(pf), vp(dstarts.data_ptr()),
                                                            unit, nb, count, dt, m.MPI_SUM, None)
                elif way == "fetch":
                    rc = lib.MPIX_Reduce_local_fetch(vp(pi), vp(po), vp(pf), count, dt, m.MPI_SUM, None)
                else:
                    if way == "copies+ragged":
                        for k in range(nb):
                            assert lib.MPIR_Hip_memcpy(pf + int(starts[k]) * esz, po + int(at[k]), int(nbytes[k])) == 0
                    rc = lib.MPIX_Reduce_local_ragged(vp(pi), None, vp(po), vp(dtab.data_ptr()), vp(dstarts.data_ptr()), unit,
                                                      nb, count, dt, m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

            # ---- the ways agree bit for bit at this shape (sets 1 to 3 copies of set 0)
            for s in (1, 2, 3):
                view("io", s).copy_(view("io", 0))
                view("in", s).copy_(view("in", 0))
            torch.cuda.synchronize()
            old = view("io", 3)[gather].clone()
            run("fetch_ragged", 0)
            run("copies+ragged" if nb <= COPY_LOOP_MAX else "ragged", 1)
            run("fetch", 2)
            torch.cuda.synchronize()
            assert torch.equal(view("io", 0).view(ity), view("io", 1).view(ity)), f"target != the ragged call's at {name}"
            assert not torch.equal(view("io", 0).view(ity), view("io", 3).view(ity)), "nothing was combined"
            assert torch.equal(view("fe", 0)[:count].view(ity), old.view(ity)), f"fetchbuf != the old target at {name}"
            if nb <= COPY_LOOP_MAX:
                assert torch.equal(view("fe", 0).view(ity), view("fe", 1).view(ity)), f"fetchbuf != the copies' at {name}"
            assert torch.equal(view("fe", 2)[:count].view(ity), view("io", 3)[:count].view(ity)), "the fetch call's fetchbuf"
            # ---- warm every way over every set
            for s in range(nsets):
                for way in ways:
                    run(way, s)
            t0 = time.perf_counter_ns()
            run("ragged", 0)
            est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = int(min(200, max(40, 20000 / est_us)))
            per_round = {w: [] for w in ways}
            k = 0
            for r in range(rounds):
                order_ = ways[r % len(ways):] + ways[:r % len(ways)]
                for way in (order_ if r % 2 == 0 else order_[::-1]):
                    mine = []
                    for _ in range(max(10, reps // 8) if way == "copies+ragged" else reps):
                        s = k % nsets
                        k += 1
                        t0 = time.perf_counter_ns()
                        run(way, s)
                        mine.append((time.perf_counter_ns() - t0) / 1e3)
                    per_round[way].append(mine)
            med = {w: float(np.median(sum(per_round[w], []))) for w in ways}
            row = {"shape": name, "pieces": nb, "bytes": total, "type": "fp64" if esz == 8 else "fp32", "disp_unit": unit,
                   "launches": info["launches"], "groups": info["groups"], "rounds_of_search": info["rounds"],
                   "packed_sides_aligned": info["packed_sides_aligned"], "sets": nsets}
            for w in ways:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
            if "fetch_ragged" in med:
                row["GBps_4_streams"] = round(4.0 * total / med["fetch_ragged"] / 1e3, 1)
                for w in ways[1:]:
                    row[f"fetch_ragged/{w}"] = round(med["fetch_ragged"] / med[w], 3)
            rows.append(row)
            print(f"{name:12s} {row['type']} {nb:6d} pieces {total / MIB:9.3f} MiB  " +
                  "  ".join(f"{w} {med[w]:.2f} {row[w + '_rounds']}" for w in ways) + "  " +
                  "  ".join(f"/{w} {row[f'fetch_ragged/{w}']:.3f}" for w in ways[1:] if "fetch_ragged" in med) +
                  f"  launches {info['launches']}" + ("" if nb <= COPY_LOOP_MAX else "  (copy loop not timed)"), flush=True)
            del pool_in, pool_fe, pool_io, pools, dtab, dstarts, gather, old
            torch.cuda.empty_cache()
    slower = [(r["shape"], r["type"]) for r in rows
              if "copies+ragged_us" in r and "fetch_ragged_us" in r and not r["fetch_ragged_us"] < r["copies+ragged_us"]]
    print("shapes where the call does not take less time than the copies and the ragged call:", slower)
    print(json.dumps({"rows": rows, "rounds": rounds, "not_faster_than_copies+ragged": slower}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5, args[1].split(",") if len(args) > 1 and args[1] != "all" else SHAPES,
         args[2].split(",") if len(args) > 2 else None)
