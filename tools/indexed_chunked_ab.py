#!/usr/bin/env python3
"""MPIX_Reduce_local_indexed_chunked against MPIX_Reduce_local_indexed_ordered
on the same operands, and MPIX_Reduce_local_runs beside MPIX_Reduce_local_order.
Per shape -- nblocks blocks of block_bytes, the input packed, the targets in
slots twice the block apart, disp_unit the block's bytes -- and per repeat factor
R (blocks / distinct targets: every target named exactly R times, the table
shuffled; `one`: every block on one target, the hot row) these ways alternate
over rounds in one process, MPI_SUM on fp32 device buffers, every call
synchronous:
  ordered   one MPIX_Reduce_local_indexed_ordered, the order table built before:
            the reference, existing code that this tool does not touch
  chunked   one MPIX_Reduce_local_indexed_chunked, order and runstart built
            before, the caller's work
  order     MPIX_Reduce_local_order alone, the caller's work buffer
  runs      MPIX_Reduce_local_runs alone, device tables
`depth` is the serial depth of the longest run: R for the ordered call, min(R,
64) + ceil(R / 64) for the chunked one (R for R = 1: no partial is made), and
depth_ratio their quotient, printed beside the measured ordered / chunked.
Every shape is warmed in every way; each repetition takes the next of several
buffer sets; host clock stamps around calls that end in completion; medians
over all repetitions, us, and the lowest and highest median of a single round.
Before a shape is timed the chunked call is run twice on copies of one set and
must give the same bits both times; at R = 1 it must give the ordered call's.

    python3 tools/indexed_chunked_ab.py [rounds = 5] [shapes = 65536x256,4096x65536] [factors = 1,4,64,one]
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
WAYS = ["ordered", "chunked", "order", "runs"]
C = m.REDUCE_LOCAL_CHUNK


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
        cws = m.reduce_local_chunked_worksize(nb, bl, dt)
        cwork = torch.empty(cws, dtype=torch.uint8, device="cuda")
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
            druns = torch.empty(nb, dtype=torch.int32, device="cuda")
            rc = lib.MPIX_Reduce_local_order(dtio.data_ptr(), nb, dorder.data_ptr(), work.data_ptr(), ws, None)
            assert rc == 0, m.error_string(rc)
            assert np.array_equal(dorder.cpu().numpy(), horder), "MPIX_Reduce_local_order != stable argsort"
            rc = lib.MPIX_Reduce_local_runs(dtio.data_ptr(), dorder.data_ptr(), nb, druns.data_ptr(), None)
            assert rc == 0, m.error_string(rc)
            sd = tio[horder]
            heads = np.concatenate([[True], sd[1:] != sd[:-1]])
            assert np.array_equal(druns.cpu().numpy(), np.maximum.accumulate(np.where(heads, np.arange(nb), 0))), \
                "MPIX_Reduce_local_runs != its definition"
            info = m.indexed_chunked_plan_info(base_in, None, base_io, dtio.data_ptr(), dorder.data_ptr(), druns.data_ptr(), rb,
                                               nb, bl, dt, op)
            scratch_order = torch.empty(nb, dtype=torch.int32, device="cuda")
            scratch_runs = torch.empty(nb, dtype=torch.int32, device="cuda")

            def run(way, s):
                pi, po = base_in + s * in_set, base_io + s * io_set
                if way == "ordered":
                    rc = lib.MPIX_Reduce_local_indexed_ordered(pi, None, po, dtio.data_ptr(), dorder.data_ptr(), rb, nb, bl,
                                                               dt, op, None)
                elif way == "chunked":
                    rc = lib.MPIX_Reduce_local_indexed_chunked(pi, None, po, dtio.data_ptr(), dorder.data_ptr(),
                                                               druns.data_ptr(), rb, nb, bl, dt, op, cwork.data_ptr(), cws, None)
                elif way == "order":
                    rc = lib.MPIX_Reduce_local_order(dtio.data_ptr(), nb, scratch_order.data_ptr(), work.data_ptr(), ws, None)
                else:
                    rc = lib.MPIX_Reduce_local_runs(dtio.data_ptr(), dorder.data_ptr(), nb, scratch_runs.data_ptr(), None)
                assert rc == 0, m.error_string(rc)

            # ---- the same bits twice (sets 1 and 2 copies of set 0), and at R = 1 the ordered call's
            keep = io_view(0).clone()
            same_in = pool_in[(base_in - pool_in.data_ptr()) // 4:][:in_set // 4]
            for s in (1, 2):
                io_view(s).copy_(keep)
                pool_in[(base_in + s * in_set - pool_in.data_ptr()) // 4:][:in_set // 4].copy_(same_in)
            torch.cuda.synchronize()
            run("chunked", 0)
            run("chunked", 1)
            torch.cuda.synchronize()
            assert torch.equal(io_view(0).view(torch.int32), io_view(1).view(torch.int32)), f"chunked twice differs at {nb} x {rb} R {f}"
            checked = ["itself"]
            if R == 1:
                run("ordered", 2)
                torch.cuda.synchronize()
                assert torch.equal(io_view(0).view(torch.int32), io_view(2).view(torch.int32)), f"chunked != ordered at {nb} x {rb} R 1"
                checked.append("ordered")
            io_view(0).copy_(keep)
            del keep
            # ---- warm every way over every set
            for s in range(nsets):
                for way in WAYS:
                    run(way, s)
            est = {}
            for way in WAYS:
                t0 = time.perf_counter_ns()
                run(way, 0)
                est[way] = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = {w: int(min(200, max(3, 20000 / est[w]))) for w in WAYS}
            t = {w: [] for w in WAYS}
            per_round = {w: [] for w in WAYS}
            k = 0
            for r in range(rounds):
                seq = WAYS[r % len(WAYS):] + WAYS[:r % len(WAYS)]
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
            med = {w: float(np.median(t[w])) for w in WAYS}
            depth = R if R == 1 else min(R, C) + -(-R // C)
            row = {"blocks": nb, "block_B": rb, "R": f, "distinct": distinct, "form": m.INDEXED_NAMES[info["form"]],
                   "launches": info["total_launches"], "groups_per_kernel": info["groups"], "work_B": info["work_bytes"],
                   "sets": nsets, "checked_against": checked, "depth_ordered": R, "depth_chunked": depth,
                   "depth_ratio": round(R / depth, 2)}
            for w in WAYS:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
                row[w + "_reps"] = reps[w] * rounds
            row["ordered/chunked"] = round(med["ordered"] / med["chunked"], 3)
            row["runs/order"] = round(med["runs"] / med["order"], 3)
            rows.append(row)
            print(f"{nb:6d} x {rb:6d} B R {f:>3s} ({distinct:6d} targets) {row['form']:10s} " +
                  "  ".join(f"{w} {med[w]:.2f} {row[w + '_rounds']}" for w in WAYS) +
                  f"  ordered/chunked {row['ordered/chunked']:.3f} (depth ratio {row['depth_ratio']:.2f})", flush=True)
            del dtio, dorder, druns, scratch_order, scratch_runs
        del pool_in, pool_io, work, cwork
        torch.cuda.empty_cache()
    print(json.dumps({"rows": rows, "rounds": rounds}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5,
         [tuple(int(v) for v in x.split("x")) for x in args[1].split(",")] if len(args) > 1 else DEFAULT,
         args[2].split(",") if len(args) > 2 else FACTORS)
