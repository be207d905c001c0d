#!/usr/bin/env python3
"""MPIX_Reduce_local_batch against the loop it replaces.  A caller with nsegs
small combines to make pays the synchronous call's fixed cost nsegs times
today; the batch pays it once.  Per shape, in one process, two ways of doing
the same work alternate over rounds, fp32 MPI_SUM on device buffers:
  loop    nsegs synchronous MPI_Reduce_local calls from the C loop
          (fast_reduce_local_loop) -- the code path this library had before
  batch   one synchronous MPIX_Reduce_local_batch over the same segments
          (through ctypes: its ~1-2 us of call overhead is on the batch's side)
Shapes: nsegs x segment bytes, total at most 1 GiB, each in a tile-path
variant (16 KiB-aligned operands) and an element-path one (inbuf 4 B off);
nsegs = 1 is the single call either way (the batch hands it to MPI_Reduce_local's path).
Every shape is warmed; each repetition takes the next of enough distinct
buffer sets that segments above 1 MiB are not served from the Infinity Cache
(at least 1 GiB of operands in rotation); host clock stamps around calls that
end in completion; medians over all repetitions, us.  Before a shape is timed
the two ways' results are compared bit for bit on it.

    python3 tools/batch_ab.py [rounds = 7] [nsegs list] [segment KiB list]
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
SLOT_PAD = 16 * KIB          # between segments of a pool: every segment starts on a 16 KiB boundary


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    nsegs_list = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 2, 4, 16, 64, 256, 1024]
    sizes = [int(x) * KIB for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else \
        [4 * KIB, 16 * KIB, 256 * KIB, 4 * MIB]
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
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for nb in sizes:
        count = nb // 4
        for nsegs in nsegs_list:
            if nsegs * nb > GIB:
                continue
            # sets in rotation: at least 1 GiB of operands when a segment is above 1 MiB, else 4
            nsets = max(4, -(-GIB // (2 * nsegs * nb))) if nb > MIB else 4
            slot = nb + SLOT_PAD
            pool_in = torch.rand(nsets * nsegs * slot // 4 + 4, device="cuda") * 1e-3
            pool_io = torch.rand(nsets * nsegs * slot // 4, device="cuda")
            torch.cuda.synchronize()
            base_in = pool_in.data_ptr() + (-pool_in.data_ptr() % SLOT_PAD)
            base_io = pool_io.data_ptr() + (-pool_io.data_ptr() % SLOT_PAD)
            for variant, off in (("tile", 0), ("elems", 4)):
                sets, arrs = [], []
                for s in range(nsets):
                    segs = [(base_in + (s * nsegs + k) * slot + off, base_io + (s * nsegs + k) * slot, count)
                            for k in range(nsegs)]
                    sets.append(tuple((i, o, c, m.MPI_FLOAT, m.MPI_SUM) for i, o, c in segs))
                    arrs.append((m.ReduceLocalSeg * nsegs)(*[m.ReduceLocalSeg(i, o, c) for i, o, c in segs]))
                info = m.batch_plan_info([(i, o, c) for i, o, c, _, _ in sets[0]], m.MPI_FLOAT, m.MPI_SUM)
                want = {"tile": m.BATCH_SEG_TILE, "elems": m.BATCH_SEG_ELEMS}[variant] if nsegs > 1 else m.BATCH_SEG_SINGLE
                assert set(info["seg_kind"]) == {want}, info

                def run_loop(s, stamps=None):
                    assert loop(sets[s], 0, nsegs, stamps) == 0

                def run_batch(s):
                    rc = batch(arrs[s], nsegs, m.MPI_FLOAT, m.MPI_SUM, None)
                    assert rc == 0, m.error_string(rc)

                # ---- the two ways agree bit for bit at this shape (set 0 against a copy of it in set 1)
                lo0 = (sets[0][0][1] - pool_io.data_ptr()) // 4
                lo1 = (sets[1][0][1] - pool_io.data_ptr()) // 4
                span = nsegs * slot // 4
                i0 = (sets[0][0][0] - off - pool_in.data_ptr()) // 4
                i1 = (sets[1][0][0] - off - pool_in.data_ptr()) // 4
                pool_io[lo1:lo1 + span].copy_(pool_io[lo0:lo0 + span])
                pool_in[i1:i1 + span + 1].copy_(pool_in[i0:i0 + span + 1].clone())
                torch.cuda.synchronize()
                run_loop(0)
                run_batch(1)
                torch.cuda.synchronize()
                assert torch.equal(pool_io[lo0:lo0 + span].view(torch.int32), pool_io[lo1:lo1 + span].view(torch.int32)), \
                    f"batch != loop at nsegs={nsegs} bytes={nb} {variant}"
                # ---- warm both ways over every set
                for s in range(nsets):
                    run_loop(s)
                    run_batch(s)
                t0 = time.perf_counter_ns()
                run_batch(0)
                est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
                reps = int(min(200, max(5, 20000 / max(est_us, nsegs * 6.0))))
                t_loop, t_batch = [], []
                st = np.zeros(nsegs + 1, np.int64)
                k = 0
                for r in range(rounds):
                    for way in (("loop", "batch") if r % 2 == 0 else ("batch", "loop")):
                        for _ in range(reps):
                            s = k % nsets
                            k += 1
                            if way == "loop":
                                run_loop(s, st)
                                t_loop.append((st[nsegs] - st[0]) / 1e3)
                            else:
                                t0 = time.perf_counter_ns()
                                run_batch(s)
                                t_batch.append((time.perf_counter_ns() - t0) / 1e3)
                lu, bu = float(np.median(t_loop)), float(np.median(t_batch))
                moved = 3.0 * nsegs * nb
                rows.append({"nsegs": nsegs, "KiB": nb // KIB, "path": variant,
                             "loop_us": round(lu, 2), "batch_us": round(bu, 2), "ratio": round(lu / bu, 2),
                             "loop_GBps": round(moved / lu / 1e3, 1), "batch_GBps": round(moved / bu / 1e3, 1),
                             "launches": info["launches"], "groups": info["groups"], "sets": nsets, "reps": reps * rounds})
                del sets, arrs
            del pool_in, pool_io
            torch.cuda.empty_cache()
    print("seg KiB | nsegs | path   | loop us (nsegs calls) | batch us (one call) | loop / batch | loop GB/s | batch GB/s")
    for r in rows:
        print(f"{r['KiB']:7d} | {r['nsegs']:5d} | {r['path']:6s} | {r['loop_us']:10.2f} | {r['batch_us']:10.2f} | "
              f"{r['ratio']:6.2f} | {r['loop_GBps']:8.1f} | {r['batch_GBps']:8.1f}")
    print("crossover (the smallest measured nsegs from which the batch takes less time than the loop at every larger one):")
    cross = {}
    for nb in sizes:
        for variant in ("tile", "elems"):
            sel = sorted((r["nsegs"], r["batch_us"] < r["loop_us"]) for r in rows
                         if r["KiB"] == nb // KIB and r["path"] == variant)
            win = None
            for n, ok in reversed(sel):
                if not ok:
                    break
                win = n
            cross[f"{nb // KIB}KiB/{variant}"] = win
            print(f"  {nb // KIB:5d} KiB {variant:5s}: {win}")
    lost = [r for r in rows if r["path"] == "tile" and r["nsegs"] >= 4 and not r["batch_us"] < r["loop_us"]]
    print("acceptance (batch < loop at every measured nsegs >= 4 on the tile path):", "HOLDS" if not lost else f"FAILS at {lost}")
    print(json.dumps({"rows": rows, "crossover": cross, "rounds": rounds, "accept": not lost}))


if __name__ == "__main__":
    main()
