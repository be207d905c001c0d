#!/usr/bin/env python3
"""MPIX_Reduce_local_ragged against the routes a caller had before it.  Per
shape -- pieces of unequal length, the input packed, the output pieces laid out
in a random order (a scatter with a permuted table of byte displacements in
units of 16 bytes, or of the element where the pieces are not 16-byte
multiples) -- these ways of doing the same work alternate over rounds in one
process, MPI_SUM on device buffers, fp32 and fp64:
  loop        one synchronous MPI_Reduce_local per piece from the C loop
              (fast_reduce_local_loop)
  batch       one synchronous MPIX_Reduce_local_batch on the same pieces
  ragged      one synchronous MPIX_Reduce_local_ragged, device tables
and on the equal-piece shapes (slots twice the piece apart, the table holding
slot numbers) the identity and a permuted placement each:
  idx_id / idx_perm        MPIX_Reduce_local_indexed
  rag_id / rag_perm        MPIX_Reduce_local_ragged on the same table, with
                           starts = k x blocklen: the price of raggedness
loop, batch and indexed exist without the ragged call: they are the yardstick.
Every shape is warmed in every way; each repetition takes the next of several
distinct buffer sets (at least 1 GiB of operands in rotation once a set is
above 1 MiB, so that the 256 MiB Infinity Cache holds nothing of the set's last
use; the loop and the batch, bound by their launches at these piece counts,
rotate over four of them); host clock stamps around calls that end in
completion; medians over all repetitions, us, and the lowest and highest median
of a single round (the spread between alternated rounds).  Before a shape is
timed the ways' results are compared bit for bit on it, and the planners'
launch counts are read.

    python3 tools/ragged_ab.py [rounds = 5] [shapes = all]
    shapes: comma-separated names out of SHAPES below, or eq:NxBYTES
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
sys.path.insert(0, ROOT)

import mpich_pip_amd as m  # noqa: E402  (the library first: VRAM rings)

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30


def lengths(name, esz, rng):
    """piece lengths in bytes"""
    import numpy as np
    if name == "64k_1to127":                # 65,536 pieces of 1-127 elements
        return rng.integers(1, 128, 65536) * esz
    if name == "64k_16Bx":                  # 65,536 pieces, multiples of 16 bytes averaging 256
        return rng.integers(1, 32, 65536) * 16
    if name == "4k_32to96K":                # 4,096 pieces of 32-96 KiB
        return rng.integers(32 * KIB // 16, 96 * KIB // 16 + 1, 4096) * 16
    if name.startswith("n"):                # n pieces around 16 KiB (12-20 KiB)
        return rng.integers(12 * KIB // 16, 20 * KIB // 16 + 1, int(name[1:])) * 16
    raise SystemExit(f"unknown shape {name}")


SHAPES = ["64k_1to127", "64k_16Bx", "4k_32to96K", "n2", "n8", "n32", "n127", "n128", "n256",
          "eq:65536x256", "eq:4096x65536"]


def set_count(total):
    return 4 if total <= MIB else max(4, min(16, -(-GIB // (3 * total))))


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return [round(min(meds), 2), round(max(meds), 2)]


def main(rounds, shapes):
    import ctypes
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    state = lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    loop = m.fast_reduce_local_loop()
    batch = lib.MPIX_Reduce_local_batch
    vp = ctypes.c_void_p
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for name in shapes:
        for esz in (4, 8):
            dt = m.MPI_DOUBLE if esz == 8 else m.MPI_FLOAT
            fdt = torch.float64 if esz == 8 else torch.float32
            ity = torch.int64 if esz == 8 else torch.int32
            rng = np.random.default_rng([len(name), esz])
            equal = name.startswith("eq:")
            if equal:
                nb, rb = (int(v) for v in name[3:].split("x"))
                nbytes = np.full(nb, rb, np.int64)
                slot = 2 * rb
                unit = slot
                tabs = {"id": np.arange(nb, dtype=np.int64), "perm": rng.permutation(nb).astype(np.int64)}
                extent = nb * slot
            else:
                nbytes = lengths(name, esz, rng).astype(np.int64)
                nb = len(nbytes)
                unit = 16 if not (nbytes % 16).any() else esz
                # the pieces one after the other in a random order, each at the next multiple of unit
                order = rng.permutation(nb)
                at = np.zeros(nb, np.int64)
                at[order] = np.concatenate(([0], np.cumsum(-(-nbytes[order] // unit) * unit)[:-1]))
                tabs = {"perm": at // unit}
                extent = int((-(-nbytes // unit) * unit).sum())
            starts = np.concatenate(([0], np.cumsum(nbytes // esz))).astype(np.int64)
            count = int(starts[-1])
            total = count * esz
            nsets = set_count(total)
            few = min(nsets, 4)
            in_set = -(-total // 16384) * 16384
            io_set = -(-extent // 16384) * 16384
            pool_in = torch.rand((nsets * in_set + 16384) // esz, device="cuda", dtype=fdt) * 1e-3
            pool_io = torch.rand((nsets * io_set + 16384) // esz, device="cuda", dtype=fdt)
            base_in = pool_in.data_ptr() + (-pool_in.data_ptr() % 16384)
            base_io = pool_io.data_ptr() + (-pool_io.data_ptr() % 16384)
            dtab = {k: torch.from_numpy(v).cuda() for k, v in tabs.items()}
            dstarts = torch.from_numpy(starts).cuda()
            torch.cuda.synchronize()

            def ptrs(s):
                return base_in + s * in_set, base_io + s * io_set

            def io_view(s):
                lo = (base_io + s * io_set - pool_io.data_ptr()) // esz
                return pool_io[lo:lo + io_set // esz]

            def in_view(s):
                lo = (base_in + s * in_set - pool_in.data_ptr()) // esz
                return pool_in[lo:lo + in_set // esz]

            def segs(s, table):
                pi, po = ptrs(s)
                return [(pi + int(starts[k]) * esz, po + int(table[k]) * unit, int(nbytes[k]) // esz) for k in range(nb)]

            which = "perm"
            sets = [tuple((i, o, c, dt, m.MPI_SUM) for i, o, c in segs(s, tabs[which])) for s in range(few)]
            arrs = [(m.ReduceLocalSeg * nb)(*[m.ReduceLocalSeg(i, o, c) for i, o, c in segs(s, tabs[which])])
                    for s in range(few)]
            ways = ("loop", "batch") + (("idx_id", "idx_perm", "rag_id", "rag_perm") if equal else ("ragged",))
            rinfo = m.ragged_plan_info(ptrs(0)[0], None, ptrs(0)[1], dtab["perm"].data_ptr(), dstarts.data_ptr(), unit, nb,
                                       count, dt, m.MPI_SUM)
            binfo = m.batch_plan_info(segs(0, tabs["perm"]), dt, m.MPI_SUM)
            st = np.zeros(nb + 1, np.int64)

            def run(way, s, stamps=None):
                if way == "loop":
                    assert loop(sets[s % few], 0, nb, stamps) == 0
                    return
                pi, po = ptrs(s)
                if way == "batch":
                    rc = batch(arrs[s % few], nb, dt, m.MPI_SUM, None)
                elif way.startswith("idx"):
                    rc = lib.MPIX_Reduce_local_indexed(pi, None, po, dtab[way[4:]].data_ptr(), unit, nb, rb // esz, dt,
                                                       m.MPI_SUM, None)
                else:
                    t = dtab[way[4:] if equal else "perm"]
                    rc = lib.MPIX_Reduce_local_ragged(vp(pi), None, vp(po), vp(t.data_ptr()), vp(dstarts.data_ptr()), unit,
                                                      nb, count, dt, m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

            # ---- the ways agree bit for bit at this shape (sets 1 to 3 copies of set 0)
            for s in (1, 2, 3):
                io_view(s).copy_(io_view(0))
                in_view(s).copy_(in_view(0))
            torch.cuda.synchronize()
            run("rag_perm" if equal else "ragged", 0)
            run("batch", 1)
            if equal:
                run("idx_perm", 2)
            torch.cuda.synchronize()
            assert torch.equal(io_view(0).view(ity), io_view(1).view(ity)), f"ragged != batch at {name}"
            assert not equal or torch.equal(io_view(0).view(ity), io_view(2).view(ity)), f"ragged != indexed at {name}"
            assert not torch.equal(io_view(0).view(ity), io_view(3).view(ity)), "nothing was combined"
            if equal:
                io_view(0).copy_(io_view(3))
                io_view(1).copy_(io_view(3))
                torch.cuda.synchronize()
                run("rag_id", 0)
                run("idx_id", 1)
                torch.cuda.synchronize()
                assert torch.equal(io_view(0).view(ity), io_view(1).view(ity)), f"ragged != indexed (id) at {name}"
            # ---- warm every way over every set
            for s in range(nsets):
                for way in ways:
                    if way not in ("loop", "batch") or s < few:
                        run(way, s)
            t0 = time.perf_counter_ns()
            run("batch", 0)
            est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = int(min(200, max(5, 20000 / est_us)))
            loop_reps = int(max(1, min(reps, 100000 / (nb * 6.0))))
            per_round = {w: [] for w in ways}
            k = 0
            for r in range(rounds):
                order = ways[r % len(ways):] + ways[:r % len(ways)]
                for way in (order if r % 2 == 0 else order[::-1]):
                    mine = []
                    for _ in range(loop_reps if way == "loop" else reps if way == "batch" else max(reps, 40)):
                        s = k % nsets
                        k += 1
                        if way == "loop":
                            run(way, s, st)
                            mine.append((st[nb] - st[0]) / 1e3)
                        else:
                            t0 = time.perf_counter_ns()
                            run(way, s)
                            mine.append((time.perf_counter_ns() - t0) / 1e3)
                    per_round[way].append(mine)
            med = {w: float(np.median(sum(per_round[w], []))) for w in ways}
            row = {"shape": name, "pieces": nb, "bytes": total, "type": "fp64" if esz == 8 else "fp32", "disp_unit": unit,
                   "ragged_launches": rinfo["launches"], "ragged_groups": rinfo["groups"], "rounds_of_search": rinfo["rounds"],
                   "batch_launches": binfo["launches"], "sets": nsets}
            for w in ways:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
            mine = "rag_perm" if equal else "ragged"
            row["batch/ragged"] = round(med["batch"] / med[mine], 2)
            row["ragged_GBps"] = round(3.0 * total / med[mine] / 1e3, 1)
            if equal:
                row["rag_id/idx_id"] = round(med["rag_id"] / med["idx_id"], 3)
                row["rag_perm/idx_perm"] = round(med["rag_perm"] / med["idx_perm"], 3)
            rows.append(row)
            print(f"{name:14s} {row['type']} {nb:6d} pieces {total / MIB:9.3f} MiB  " +
                  "  ".join(f"{w} {med[w]:.2f} {row[w + '_rounds']}" for w in ways) +
                  f"  batch/ragged {row['batch/ragged']:.2f}  launches {binfo['launches']} -> {rinfo['launches']}" +
                  (f"  rag/idx id {row['rag_id/idx_id']:.3f} perm {row['rag_perm/idx_perm']:.3f}" if equal else ""),
                  flush=True)
            del sets, arrs, pool_in, pool_io, dtab
            torch.cuda.empty_cache()
    slower = [(r["shape"], r["type"]) for r in rows
              if not r["rag_perm_us" if "rag_perm_us" in r else "ragged_us"] < r["batch_us"]]
    print("shapes where the ragged call does not take less time than the batch:", slower)
    print(json.dumps({"rows": rows, "rounds": rounds, "not_faster_than_batch": slower}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5, args[1].split(",") if len(args) > 1 else SHAPES)
