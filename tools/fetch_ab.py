#!/usr/bin/env python3
"""MPIX_Reduce_local_fetch against what a caller does without it.  Per operand
size two ways of doing the same work alternate over rounds in one process, fp32
MPI_SUM on device buffers:
  pair   a device-to-device copy of inoutbuf into fetchbuf through the library's
         own HIP runtime (MPIR_Hip_memcpy), then a synchronous MPI_Reduce_local
         (the direct AQL dispatch): two launches, inoutbuf read twice, five
         streams through memory
  fetch  one synchronous MPIX_Reduce_local_fetch: one launch, four streams
The pair exists without the fetching call: it is the yardstick.  Two columns of
the fetching call: all three buffers 16 KiB-aligned (the tile path), and fetchbuf
4 bytes off the other two (the element path; the pair copies to the same place).
Every shape is warmed both ways over every buffer set; each repetition takes the
next of several distinct sets (at least 1 GiB of operands in rotation once an
operand is above 1 MiB, so that large operands are not re-read from the Infinity
Cache); host clock stamps around calls that end in completion; medians over all
repetitions, us, with the lowest and highest median of a single round (the
spread between alternated rounds).  Before a shape is timed both ways' results,
inoutbuf and fetchbuf, are compared bit for bit on it.

    python3 tools/fetch_ab.py [rounds = 5] [operand bytes list] [paths = tile,elems]

The kernel's own time: run one size and one path under `rocprofv3 --kernel-trace
--stats`, in a run of its own, and read k_reduce_fetch's average.
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
sys.path.insert(0, ROOT)

import mpich_pip_amd as m  # noqa: E402  (the library first: VRAM rings)

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
HBM_PEAK = 8.0e12           # bytes / s


class Sets:
    """nsets buffer sets of one size: in / inout / fetch, each 16 KiB-aligned, and a
    second fetch buffer 4 bytes off."""

    def __init__(self, torch, nbytes, nsets):
        self.nbytes, self.nsets, self.n = nbytes, nsets, nbytes // 4
        self.span = -(-(nbytes + 16) // 16384) * 16384
        words = (nsets * self.span + 16384) // 4
        self.pool_in = torch.rand(words, device="cuda", dtype=torch.float32) * 1e-3
        self.pool_io = torch.rand(words, device="cuda", dtype=torch.float32)
        self.pool_fe = torch.zeros(words, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        self.base = [p.data_ptr() + (-p.data_ptr() % 16384) for p in (self.pool_in, self.pool_io, self.pool_fe)]

    def ptrs(self, s, off=0):
        return self.base[0] + s * self.span, self.base[1] + s * self.span, self.base[2] + s * self.span + off

    def view(self, which, s, off=0):
        pool = (self.pool_in, self.pool_io, self.pool_fe)[which]
        lo = (self.base[which] + s * self.span + off - pool.data_ptr()) // 4
        return pool[lo:lo + self.n]


def set_count(nbytes):
    return 4 if nbytes <= MIB else max(4, min(32, -(-GIB // (3 * nbytes))))


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return round(min(meds), 2), round(max(meds), 2)


def main(rounds, sizes, paths):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    state = lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    fetch, reduce_local, memcpy = lib.MPIX_Reduce_local_fetch, m.fast_reduce_local(), lib.MPIR_Hip_memcpy
    memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    memcpy.restype = ctypes.c_int
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for nbytes in sizes:
        nsets = set_count(nbytes)
        sh = Sets(torch, nbytes, nsets)
        n = sh.n
        for col, off in (("tile", 0), ("elems", 4)):
            if col not in paths:
                continue
            info = m.fetch_plan_info(*sh.ptrs(0, off), n, m.MPI_FLOAT, m.MPI_SUM)
            assert m.FETCH_NAMES[info["path"]] == col, info

            def run_pair(s):
                pi, po, pf = sh.ptrs(s, off)
                assert memcpy(pf, po, nbytes) == 0
                assert reduce_local(pi, po, n, m.MPI_FLOAT, m.MPI_SUM) == 0

            def run_fetch(s):
                pi, po, pf = sh.ptrs(s, off)
                rc = fetch(pi, po, pf, n, m.MPI_FLOAT, m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

            # ---- both ways agree bit for bit at this shape (set 1 a copy of set 0)
            sh.view(0, 1).copy_(sh.view(0, 0))
            sh.view(1, 1).copy_(sh.view(1, 0))
            torch.cuda.synchronize()
            run_fetch(0)
            run_pair(1)
            torch.cuda.synchronize()
            for which in (1, 2):
                o = off if which == 2 else 0
                assert torch.equal(sh.view(which, 0, o).view(torch.int32), sh.view(which, 1, o).view(torch.int32)), \
                    f"fetch != pair ({'inoutbuf' if which == 1 else 'fetchbuf'}) at {nbytes} B, {col}"
            # ---- warm both ways over every set
            for s in range(nsets):
                run_pair(s)
                run_fetch(s)
            t0 = time.perf_counter_ns()
            run_pair(0)
            est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = int(min(200, max(8, 20000 / est_us)))
            t = {"pair": [], "fetch": []}
            per_round = {"pair": [], "fetch": []}
            k = 0
            for r in range(rounds):
                for way in (("pair", "fetch") if r % 2 == 0 else ("fetch", "pair")):
                    fn = run_pair if way == "pair" else run_fetch
                    mine = []
                    for _ in range(reps):
                        s = k % nsets
                        k += 1
                        t0 = time.perf_counter_ns()
                        fn(s)
                        mine.append((time.perf_counter_ns() - t0) / 1e3)
                    t[way] += mine
                    per_round[way].append(mine)
            pu, fu = float(np.median(t["pair"])), float(np.median(t["fetch"]))
            rows.append({"bytes": nbytes, "path": col, "pair_us": round(pu, 2), "fetch_us": round(fu, 2),
                         "pair_rounds": spread(per_round["pair"]), "fetch_rounds": spread(per_round["fetch"]),
                         "pair/fetch": round(pu / fu, 3), "fetch_GBps": round(4.0 * nbytes / fu / 1e3, 1),
                         "fetch_of_peak_host_clock": round(4.0 * nbytes / (fu * 1e-6) / HBM_PEAK, 3),
                         "groups": info["groups"], "sets": nsets, "reps": reps * rounds})
            r = rows[-1]
            print(f"{nbytes:10d} B {col:5s} pair {pu:9.2f} {r['pair_rounds']}  fetch {fu:9.2f} {r['fetch_rounds']}  "
                  f"pair/fetch {r['pair/fetch']:6.3f}  fetch {r['fetch_GBps']:7.1f} GB/s  groups {info['groups']}  "
                  f"sets {nsets}  reps {reps} x {rounds}", flush=True)
        del sh
        torch.cuda.empty_cache()
    slower = [(r["bytes"], r["path"]) for r in rows if not r["fetch_us"] < r["pair_us"]]
    print("shapes where the fetching call does not take less time than the pair (bytes, path):", slower)
    print(json.dumps({"rows": rows, "rounds": rounds, "slower_than_pair": slower}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5,
         [int(x) for x in args[1].split(",")] if len(args) > 1 else [4 * KIB, 64 * KIB, MIB, 16 * MIB, 256 * MIB],
         args[2].split(",") if len(args) > 2 else ["tile", "elems"])
