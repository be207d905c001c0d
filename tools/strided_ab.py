#!/usr/bin/env python3
"""MPIX_Reduce_local_strided against the two ways a caller had before it.  Per
shape -- nrows rows of row_bytes, the input packed, the output rows at a larger
stride (a sub-matrix; 8-byte rows are a column of doubles in a matrix 128 wide)
-- three ways of doing the same work alternate over rounds in one process,
MPI_SUM on device buffers (fp64 for the 8-byte rows, else fp32):
  loop     nrows synchronous MPI_Reduce_local calls from the C loop
           (fast_reduce_local_loop)
  batch    one synchronous MPIX_Reduce_local_batch over the same rows
  strided  one synchronous MPIX_Reduce_local_strided
loop and batch exist without the strided call: they are the yardstick.  Every
shape is warmed in every way; each repetition takes the next of several distinct
buffer sets (at least 1 GiB of operands in rotation once a set is above 1 MiB,
so that large shapes are not served from the Infinity Cache); host clock stamps
around calls that end in completion; medians over all repetitions, us, and for
batch and strided the lowest and highest median of a single round (the spread
between alternated rounds).  Before a shape is timed the three ways' results
are compared bit for bit on it.

    python3 tools/strided_ab.py [rounds = 5] [nrows list] [row bytes list]
    python3 tools/strided_ab.py sweep [rounds = 5] [nrows list] [row bytes list]

sweep: the wide / narrow threshold.  Row bytes from 256 B to 64 KiB, each form
forced in turn through MPIR_Hip_set_strided_wide_bytes (0: every row wide;
1 GiB: every row narrow), alternated over rounds; the default threshold is set
where the medians cross.
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


def out_stride(rb):
    return 1024 if rb == 8 else 2 * rb


class Shape:
    """nsets buffer sets of one shape: packed input rows, output rows out_stride apart."""

    def __init__(self, torch, nrows, rb, nsets):
        self.nrows, self.rb, self.nsets = nrows, rb, nsets
        self.dt = m.MPI_DOUBLE if rb == 8 else m.MPI_FLOAT
        self.esz = 8 if rb == 8 else 4
        self.bl = rb // self.esz
        self.so = out_stride(rb)
        fdt = torch.float64 if rb == 8 else torch.float32
        self.in_set = -(-nrows * rb // 16384) * 16384           # bytes per set, 16 KiB-aligned starts
        self.io_set = -(-nrows * self.so // 16384) * 16384
        self.pool_in = torch.rand((nsets * self.in_set + 16384) // self.esz, device="cuda", dtype=fdt) * 1e-3
        self.pool_io = torch.rand((nsets * self.io_set + 16384) // self.esz, device="cuda", dtype=fdt)
        torch.cuda.synchronize()
        self.base_in = self.pool_in.data_ptr() + (-self.pool_in.data_ptr() % 16384)
        self.base_io = self.pool_io.data_ptr() + (-self.pool_io.data_ptr() % 16384)

    def ptrs(self, s):
        return self.base_in + s * self.in_set, self.base_io + s * self.io_set

    def io_view(self, s):
        lo = (self.base_io + s * self.io_set - self.pool_io.data_ptr()) // self.esz
        return self.pool_io[lo:lo + self.io_set // self.esz]

    def in_view(self, s):
        lo = (self.base_in + s * self.in_set - self.pool_in.data_ptr()) // self.esz
        return self.pool_in[lo:lo + self.in_set // self.esz]

    def segs(self, s):
        pi, po = self.ptrs(s)
        return [(pi + r * self.rb, po + r * self.so, self.bl) for r in range(self.nrows)]


def set_count(nrows, rb):
    total = nrows * rb
    return 4 if total <= MIB else max(4, min(16, -(-GIB // (3 * total))))


def run_strided(lib, sh, s):
    pi, po = sh.ptrs(s)
    rc = lib.MPIX_Reduce_local_strided(pi, sh.rb, po, sh.so, sh.nrows, sh.bl, sh.dt, m.MPI_SUM, None)
    assert rc == 0, m.error_string(rc)


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return round(min(meds), 2), round(max(meds), 2)


def main_ab(rounds, nrows_list, sizes):
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
    for rb in sizes:
        for nrows in nrows_list:
            if nrows * rb > GIB:
                continue
            nsets = set_count(nrows, rb)
            sh = Shape(torch, nrows, rb, nsets)
            info = m.strided_plan_info(*sh.ptrs(0)[:1], sh.rb, sh.ptrs(0)[1], sh.so, nrows, sh.bl, sh.dt, m.MPI_SUM)
            binfo = m.batch_plan_info(sh.segs(0), sh.dt, m.MPI_SUM)
            sets = [tuple((i, o, c, sh.dt, m.MPI_SUM) for i, o, c in sh.segs(s)) for s in range(nsets)]
            arrs = [(m.ReduceLocalSeg * nrows)(*[m.ReduceLocalSeg(i, o, c) for i, o, c in sh.segs(s)]) for s in range(nsets)]

            def run_loop(s, stamps=None):
                assert loop(sets[s], 0, nrows, stamps) == 0

            def run_batch(s):
                rc = batch(arrs[s], nrows, sh.dt, m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

            # ---- the three ways agree bit for bit at this shape (sets 1 and 2 copies of set 0)
            for s in (1, 2):
                sh.io_view(s).copy_(sh.io_view(0))
                sh.in_view(s).copy_(sh.in_view(0))
            torch.cuda.synchronize()
            run_strided(lib, sh, 0)
            run_batch(1)
            run_loop(2)
            torch.cuda.synchronize()
            ity = torch.int64 if rb == 8 else torch.int32
            assert torch.equal(sh.io_view(0).view(ity), sh.io_view(1).view(ity)), f"strided != batch at {nrows} x {rb}"
            assert torch.equal(sh.io_view(0).view(ity), sh.io_view(2).view(ity)), f"strided != loop at {nrows} x {rb}"
            # ---- warm every way over every set
            for s in range(nsets):
                run_loop(s)
                run_batch(s)
                run_strided(lib, sh, s)
            t0 = time.perf_counter_ns()
            run_batch(0)
            est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = int(min(200, max(5, 20000 / est_us)))
            loop_reps = int(max(2, min(reps, 300000 / (nrows * 6.0))))
            t = {"loop": [], "batch": [], "strided": []}
            per_round = {"batch": [], "strided": []}
            st = np.zeros(nrows + 1, np.int64)
            k = 0
            orders = (("loop", "batch", "strided"), ("strided", "batch", "loop"), ("batch", "strided", "loop"))
            for r in range(rounds):
                for way in orders[r % 3]:
                    mine = []
                    for _ in range(loop_reps if way == "loop" else reps):
                        s = k % nsets
                        k += 1
                        if way == "loop":
                            run_loop(s, st)
                            mine.append((st[nrows] - st[0]) / 1e3)
                        else:
                            t0 = time.perf_counter_ns()
                            if way == "batch":
                                run_batch(s)
                            else:
                                run_strided(lib, sh, s)
                            mine.append((time.perf_counter_ns() - t0) / 1e3)
                    t[way] += mine
                    if way in per_round:
                        per_round[way].append(mine)
            lu, bu, su = (float(np.median(t[w])) for w in ("loop", "batch", "strided"))
            moved = 3.0 * nrows * rb
            rows.append({"rows": nrows, "row_B": rb, "form": m.STRIDED_NAMES[info["form"]],
                         "loop_us": round(lu, 2), "batch_us": round(bu, 2), "strided_us": round(su, 2),
                         "batch_rounds": spread(per_round["batch"]), "strided_rounds": spread(per_round["strided"]),
                         "batch/strided": round(bu / su, 2), "loop/strided": round(lu / su, 2),
                         "strided_GBps": round(moved / su / 1e3, 1), "batch_GBps": round(moved / bu / 1e3, 1),
                         "strided_launches": info["launches"], "strided_groups": info["groups"],
                         "batch_launches": binfo["launches"], "batch_groups": binfo["groups"],
                         "sets": nsets, "reps": reps * rounds})
            r = rows[-1]
            print(f"{rb:8d} B x {nrows:6d} {r['form']:12s} loop {lu:11.2f}  batch {bu:10.2f} {r['batch_rounds']}  "
                  f"strided {su:10.2f} {r['strided_rounds']}  batch/strided {r['batch/strided']:6.2f}  "
                  f"launches {binfo['launches']} -> {info['launches']}  groups {binfo['groups']} -> {info['groups']}",
                  flush=True)
            del sets, arrs, sh
            torch.cuda.empty_cache()
    slower = [(r["rows"], r["row_B"]) for r in rows if not r["strided_us"] < r["batch_us"]]
    print("shapes where the strided call does not take less time than the batch (rows, row bytes):", slower)
    print(json.dumps({"rows": rows, "rounds": rounds, "slower_than_batch": slower}))


def main_sweep(rounds, nrows_list, sizes):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    default = lib.MPIR_Hip_set_strided_wide_bytes(0)
    lib.MPIR_Hip_set_strided_wide_bytes(default)
    print(f"build {m.build_id()}; {torch.cuda.get_device_name(0)}; rounds {rounds}; default threshold {default} B")
    force = {"wide": 0, "narrow": GIB}
    rows = []
    try:
        for nrows in nrows_list:
            for rb in sizes:
                nsets = set_count(nrows, rb)
                sh = Shape(torch, nrows, rb, nsets)
                forms = {}
                for way, thr in force.items():
                    lib.MPIR_Hip_set_strided_wide_bytes(thr)
                    forms[way] = m.STRIDED_NAMES[m.strided_plan_info(sh.ptrs(0)[0], sh.rb, sh.ptrs(0)[1], sh.so, nrows,
                                                                     sh.bl, sh.dt, m.MPI_SUM)["form"]]
                    for s in range(nsets):
                        run_strided(lib, sh, s)
                # the two forms agree bit for bit
                sh.io_view(1).copy_(sh.io_view(0))
                sh.in_view(1).copy_(sh.in_view(0))
                torch.cuda.synchronize()
                lib.MPIR_Hip_set_strided_wide_bytes(force["wide"])
                run_strided(lib, sh, 0)
                lib.MPIR_Hip_set_strided_wide_bytes(force["narrow"])
                run_strided(lib, sh, 1)
                torch.cuda.synchronize()
                assert torch.equal(sh.io_view(0).view(torch.int32), sh.io_view(1).view(torch.int32)), (nrows, rb)
                t = {"wide": [], "narrow": []}
                k = 0
                for r in range(rounds):
                    for way in (("wide", "narrow") if r % 2 == 0 else ("narrow", "wide")):
                        lib.MPIR_Hip_set_strided_wide_bytes(force[way])
                        for _ in range(100):
                            s = k % nsets
                            k += 1
                            t0 = time.perf_counter_ns()
                            run_strided(lib, sh, s)
                            t[way].append((time.perf_counter_ns() - t0) / 1e3)
                wu, nu = float(np.median(t["wide"])), float(np.median(t["narrow"]))
                rows.append({"rows": nrows, "row_B": rb, "wide_us": round(wu, 2), "narrow_us": round(nu, 2),
                             "narrow_form": forms["narrow"], "wide/narrow": round(wu / nu, 2)})
                print(f"{nrows:6d} rows x {rb:6d} B  wide {wu:9.2f}  {forms['narrow']} {nu:9.2f}  wide/narrow {wu / nu:5.2f}",
                      flush=True)
                del sh
                torch.cuda.empty_cache()
    finally:
        lib.MPIR_Hip_set_strided_wide_bytes(default)
    print(json.dumps({"sweep": rows, "rounds": rounds, "default_threshold": default}))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "sweep":
        main_sweep(int(args[1]) if len(args) > 1 else 5,
                   [int(x) for x in args[2].split(",")] if len(args) > 2 else [256, 4096],
                   [int(x) for x in args[3].split(",")] if len(args) > 3 else [256 << k for k in range(9)])
    else:
        main_ab(int(args[0]) if args else 5,
                [int(x) for x in args[1].split(",")] if len(args) > 1 else [16, 256, 4096, 65536],
                [int(x) for x in args[2].split(",")] if len(args) > 2 else [8, 64, KIB, 4 * KIB, 64 * KIB, 4 * MIB])
