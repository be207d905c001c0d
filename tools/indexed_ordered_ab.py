#!/usr/bin/env python3
"""MPIX_Reduce_local_indexed_ordered against what a caller with repeated
targets had before it, and against the indexed call where nothing repeats.  Per
shape -- nblocks blocks of block_bytes, the input packed, the targets in slots
twice the block apart, disp_unit the block's bytes -- and per repeat factor R
(blocks / distinct targets: every target named exactly R times, the table
shuffled; `one`: every block on one target) these ways alternate over rounds in
one process, MPI_SUM on fp32 device buffers, every call synchronous:
  indexed   one MPIX_Reduce_local_indexed (R = 1 only: the same duplicate-free
            operands; ordered / indexed is the price of the order table and the
            head test)
  ordered   one MPIX_Reduce_local_indexed_ordered, the order table built before
  rounds    what a caller does today: the table split into R duplicate-free
            rounds (round j: each target's j-th block in table order) and one
            MPIX_Reduce_local_indexed per round, both tables given.  The split
            is made once, outside the timed window, so the host's share of it is
            not charged to this way.  Not run past R = 64 (it is the per-block
            loop there).
  order     MPIX_Reduce_local_order alone, the caller's work buffer
  one_shot  order + ordered: a caller who uses the pattern once
By the bytes moved the ordered call reads nblocks input blocks and reads and
writes each distinct target once, nblocks + 2 x distinct blocks, where the rounds
move 3 x nblocks: `bound` is that ratio, printed beside the measured
rounds / ordered.  Every shape is warmed in every way; each repetition takes the
next of several buffer sets; host clock stamps around calls that end in
completion; medians over all repetitions, us, and the lowest and highest median
of a single round.  Before a shape is timed, ordered, rounds and (R = 1)
indexed are compared bit for bit on copies of one set.

    python3 tools/indexed_ordered_ab.py [rounds = 5] [shapes = 65536x256,4096x65536] [factors = 1,4,64,one]
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
DEFAULT = [(65536, 256), (4096, 64 * KIB)]
FACTORS = ["1", "4", "64", "one"]
ROUNDS_MAX_R = 64


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return [round(min(meds), 2), round(max(meds), 2)]


def main(rounds, shapes, factors):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    bench.bind_near_gpu(m, 0)
    print(f"build {m.build_id()}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    dt, op = m.MPI_FLOAT, m.MPI_SUM
    rows = []
    for nb, rb in shapes:
        bl = rb // 4
        total = nb * rb
        nsets = 4 if total <= MIB else max(4, min(16, -(-GIB // (3 * total))))
        in_set = -(-nb * rb // 16384) * 16384
        io_set = -(-nb * 2 * rb // 16384) * 16384
        pool_in = torch.rand((nsets * in_set + 16384) // 4, device="cuda") * 1e-3
        pool_io = torch.rand((nsets * io_set + 16384) // 4, device="cuda")
        torch.cuda.synchronize()
        base_in = pool_in.data_ptr() + (-pool_in.data_ptr() % 16384)
        base_io = pool_io.data_ptr() + (-pool_io.data_ptr() % 16384)

        def io_view(s):
            lo = (base_io + s * io_set - pool_io.data_ptr()) // 4
            return pool_io[lo:lo + io_set // 4]

        ws = m.reduce_local_order_worksize(nb)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        for f in factors:
            R = nb if f == "one" else int(f)
            distinct = nb // R
            rng = np.random.default_rng([nb, R])
            # every target R times, shuffled; the targets' slots a permutation (units of rb: 2 per slot)
            which = rng.permutation(np.repeat(np.arange(distinct), R))
            tio = (rng.permutation(nb)[:distinct][which] * 2).astype(np.int64)
            horder = np.argsort(tio, kind="stable").astype(np.int32)
            dtio = torch.from_numpy(tio).cuda()
            dorder = torch.empty(nb, dtype=torch.int32, device="cuda")
            rc = lib.MPIX_Reduce_local_order(dtio.data_ptr(), nb, dorder.data_ptr(), work.data_ptr(), ws, None)
            assert rc == 0, m.error_string(rc)
            assert np.array_equal(dorder.cpu().numpy(), horder), "MPIX_Reduce_local_order != stable argsort"
            ways = (["indexed"] if R == 1 else []) + ["ordered"] + (["rounds"] if R <= ROUNDS_MAX_R else []) + \
                ["order", "one_shot"]
            # the rounds: occurrence number of each block within its target, in table order
            occ = np.empty(nb, np.int64)
            occ[horder] = np.arange(nb) - np.searchsorted(tio[horder], tio[horder], side="left")
            rtabs = []
            if "rounds" in ways:
                for j in range(R):
                    ks = np.nonzero(occ == j)[0].astype(np.int64)
                    rtabs.append((torch.from_numpy(ks).cuda(), torch.from_numpy(tio[ks]).cuda(), len(ks)))
            info = m.indexed_ordered_plan_info(base_in, None, base_io, dtio.data_ptr(), dorder.data_ptr(), rb, nb, bl, dt, op)
            scratch_order = torch.empty(nb, dtype=torch.int32, device="cuda")

            def run(way, s):
                pi, po = base_in + s * in_set, base_io + s * io_set
                if way == "indexed":
                    rc = lib.MPIX_Reduce_local_indexed(pi, None, po, dtio.data_ptr(), rb, nb, bl, dt, op, None)
                elif way == "ordered":
                    rc = lib.MPIX_Reduce_local_indexed_ordered(pi, None, po, dtio.data_ptr(), dorder.data_ptr(), rb, nb, bl,
                                                               dt, op, None)
                elif way == "rounds":
                    rc = 0
                    for tin_j, tio_j, n in rtabs:
                        rc = rc or lib.MPIX_Reduce_local_indexed(pi, tin_j.data_ptr(), po, tio_j.data_ptr(), rb, n, bl, dt,
                                                                 op, None)
                elif way == "order":
                    rc = lib.MPIX_Reduce_local_order(dtio.data_ptr(), nb, scratch_order.data_ptr(), work.data_ptr(), ws, None)
                else:
                    rc = lib.MPIX_Reduce_local_order(dtio.data_ptr(), nb, scratch_order.data_ptr(), work.data_ptr(), ws, None)
                    rc = rc or lib.MPIX_Reduce_local_indexed_ordered(pi, None, po, dtio.data_ptr(), scratch_order.data_ptr(),
                                                                     rb, nb, bl, dt, op, None)
                assert rc == 0, m.error_string(rc)

            # ---- the ways agree bit for bit at this shape (sets 1 and 2 copies of set 0)
            keep = io_view(0).clone()
            same_in = pool_in[(base_in - pool_in.data_ptr()) // 4:][:in_set // 4]
            for s in (1, 2):
                io_view(s).copy_(keep)
                pool_in[(base_in + s * in_set - pool_in.data_ptr()) // 4:][:in_set // 4].copy_(same_in)
            torch.cuda.synchronize()
            run("ordered", 0)
            checked = []
            for s, way in ((1, "rounds"), (2, "indexed")):
                if way in ways:
                    run(way, s)
                    torch.cuda.synchronize()
                    assert torch.equal(io_view(0).view(torch.int32), io_view(s).view(torch.int32)), f"ordered != {way} at {nb} x {rb} R {f}"
                    checked.append(way)
            io_view(0).copy_(keep)
            del keep
            # ---- warm every way over every set
            for s in range(nsets):
                for way in ways:
                    run(way, s)
            est = {}
            for way in ways:
                t0 = time.perf_counter_ns()
                run(way, 0)
                est[way] = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = {w: int(min(200, max(3, 20000 / est[w]))) for w in ways}
            t = {w: [] for w in ways}
            per_round = {w: [] for w in ways}
            k = 0
            for r in range(rounds):
                seq = ways[r % len(ways):] + ways[:r % len(ways)]
                for way in (seq if r % 2 == 0 else seq[::-1]):
                    mine = []
                    for _ in range(reps[way]):
                        s = k % nsets
                        k += 1
                        t0 = time.perf_counter_ns()
                        run(way, s)
                        mine.append((time.perf_counter_ns() - t0) / 1e3)
                    t[way] += mine
                    per_round[way].append(mine)
            med = {w: float(np.median(t[w])) for w in ways}
            row = {"blocks": nb, "block_B": rb, "R": f, "distinct": distinct, "form": m.INDEXED_NAMES[info["form"]],
                   "launches": info["launches"], "groups": info["groups"], "sets": nsets, "checked_against": checked,
                   "ordered_GBps": round((nb + 2.0 * distinct) * rb / med["ordered"] / 1e3, 1),
                   "bound_rounds/ordered": round(3.0 * nb / (nb + 2.0 * distinct), 2)}
            for w in ways:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
                row[w + "_reps"] = reps[w] * rounds
            if "indexed" in ways:
                row["ordered/indexed"] = round(med["ordered"] / med["indexed"], 3)
            if "rounds" in ways:
                row["rounds/ordered"] = round(med["rounds"] / med["ordered"], 2)
                row["rounds/one_shot"] = round(med["rounds"] / med["one_shot"], 2)
            rows.append(row)
            print(f"{nb:6d} x {rb:6d} B R {f:>3s} ({distinct:6d} targets) {row['form']:10s} " +
                  "  ".join(f"{w} {med[w]:.2f} {row[w + '_rounds']}" for w in ways) +
                  (f"  ordered/indexed {row['ordered/indexed']:.3f}" if "indexed" in ways else "") +
                  (f"  rounds/ordered {row['rounds/ordered']:.2f} (bound {row['bound_rounds/ordered']:.2f})"
                   f"  rounds/one_shot {row['rounds/one_shot']:.2f}" if "rounds" in ways else "") +
                  f"  ordered {row['ordered_GBps']} GB/s of its own bytes", flush=True)
            del rtabs, dtio, dorder, scratch_order
        del pool_in, pool_io, work
        torch.cuda.empty_cache()
    print(json.dumps({"rows": rows, "rounds": rounds}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5,
         [tuple(int(v) for v in x.split("x")) for x in args[1].split(",")] if len(args) > 1 else DEFAULT,
         args[2].split(",") if len(args) > 2 else FACTORS)
