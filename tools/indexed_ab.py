#!/usr/bin/env python3
"""MPIX_Reduce_local_indexed against the routes a caller had before it.  Per
shape -- nblocks blocks of block_bytes, the input packed, the output blocks in
slots twice the block apart (at least 16 bytes), the table holding slot numbers
(disp_unit = the slot's bytes) -- these ways of doing the same work alternate
over rounds in one process, MPI_SUM on device buffers, fp32 and fp64:
  loop        nblocks synchronous MPI_Reduce_local calls from the C loop
              (fast_reduce_local_loop), identity placement
  batch_id    one synchronous MPIX_Reduce_local_batch, identity placement
  batch_perm  the same, the blocks at a random permutation of the slots
  strided     one synchronous MPIX_Reduce_local_strided: what the identity
              placement is without a table
  idx_id      one synchronous MPIX_Reduce_local_indexed, identity table (device)
  idx_perm    the same, the random-permutation table (device)
loop, batch and strided exist without the indexed call: they are the yardstick,
and idx_id against strided is what reading the table costs.  Every shape is
warmed in every way; each repetition takes the next of several distinct buffer
sets (at least 1 GiB of operands in rotation once a set is above 1 MiB); host
clock stamps around calls that end in completion; medians over all repetitions,
us, and the lowest and highest median of a single round (the spread between
alternated rounds).  Before a shape is timed the ways' results are compared bit
for bit on it, and the planner's launch count and the direct-dispatch counter
are read: the indexed call is `launches` HIP launches and no direct dispatch.

    python3 tools/indexed_ab.py [rounds = 5] [shapes = default]
    shapes: comma-separated nblocks x block_bytes, e.g. 65536x256,4096x65536
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
WAYS = ("loop", "batch_id", "batch_perm", "strided", "idx_id", "idx_perm")
DEFAULT = [(65536, 0), (65536, 256), (4096, 64 * KIB)] + [(n, 16 * KIB) for n in (2, 8, 32, 64, 127, 128, 256)]


class Shape:
    """nsets buffer sets of one shape: packed input blocks, output slots `so` apart."""

    def __init__(self, torch, nb, rb, esz, nsets):
        self.nb, self.rb, self.esz, self.nsets = nb, rb, esz, nsets
        self.dt = m.MPI_DOUBLE if esz == 8 else m.MPI_FLOAT
        self.bl = rb // esz
        self.so = max(2 * rb, 16)
        fdt = torch.float64 if esz == 8 else torch.float32
        self.in_set = -(-nb * rb // 16384) * 16384              # bytes per set, 16 KiB-aligned starts
        self.io_set = -(-nb * self.so // 16384) * 16384
        self.pool_in = torch.rand((nsets * self.in_set + 16384) // esz, device="cuda", dtype=fdt) * 1e-3
        self.pool_io = torch.rand((nsets * self.io_set + 16384) // esz, device="cuda", dtype=fdt)
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

    def segs(self, s, table):
        pi, po = self.ptrs(s)
        return [(pi + k * self.rb, po + int(table[k]) * self.so, self.bl) for k in range(self.nb)]


def set_count(nb, rb):
    total = nb * rb
    return 4 if total <= MIB else max(4, min(16, -(-GIB // (3 * total))))


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return [round(min(meds), 2), round(max(meds), 2)]


def main(rounds, shapes):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    lib.MPIR_Hip_direct_dispatches.restype = __import__("ctypes").c_uint64
    torch.cuda.set_device(0)
    state = lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    loop = m.fast_reduce_local_loop()
    batch = lib.MPIX_Reduce_local_batch
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for nb, rb0 in shapes:
        for esz in (4, 8):
            rb = rb0 or esz                                     # 0: blocks of one element
            if nb * rb > GIB:
                continue
            nsets = set_count(nb, rb)
            sh = Shape(torch, nb, rb, esz, nsets)
            tabs = {"id": np.arange(nb, dtype=np.int64),
                    "perm": np.random.default_rng(nb).permutation(nb).astype(np.int64)}
            dtab = {k: torch.from_numpy(v).cuda() for k, v in tabs.items()}
            info = m.indexed_plan_info(sh.ptrs(0)[0], None, sh.ptrs(0)[1], dtab["perm"].data_ptr(), sh.so, nb, sh.bl,
                                       sh.dt, m.MPI_SUM)
            sinfo = m.strided_plan_info(sh.ptrs(0)[0], rb, sh.ptrs(0)[1], sh.so, nb, sh.bl, sh.dt, m.MPI_SUM)
            binfo = m.batch_plan_info(sh.segs(0, tabs["perm"]), sh.dt, m.MPI_SUM)
            sets = [tuple((i, o, c, sh.dt, m.MPI_SUM) for i, o, c in sh.segs(s, tabs["id"])) for s in range(nsets)]
            arrs = {k: [(m.ReduceLocalSeg * nb)(*[m.ReduceLocalSeg(i, o, c) for i, o, c in sh.segs(s, v)])
                        for s in range(nsets)] for k, v in tabs.items()}
            st = np.zeros(nb + 1, np.int64)

            def run(way, s, stamps=None):
                pi, po = sh.ptrs(s)
                if way == "loop":
                    assert loop(sets[s], 0, nb, stamps) == 0
                    return
                if way.startswith("batch"):
                    rc = batch(arrs[way[6:]][s], nb, sh.dt, m.MPI_SUM, None)
                elif way == "strided":
                    rc = lib.MPIX_Reduce_local_strided(pi, rb, po, sh.so, nb, sh.bl, sh.dt, m.MPI_SUM, None)
                else:
                    rc = lib.MPIX_Reduce_local_indexed(pi, None, po, dtab[way[4:]].data_ptr(), sh.so, nb, sh.bl, sh.dt,
                                                       m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

            # ---- the ways agree bit for bit at this shape (sets 1 to 3 copies of set 0)
            for s in (1, 2, 3):
                sh.io_view(s).copy_(sh.io_view(0))
                sh.in_view(s).copy_(sh.in_view(0))
            torch.cuda.synchronize()
            d0 = lib.MPIR_Hip_direct_dispatches()
            run("idx_id", 0)
            direct = lib.MPIR_Hip_direct_dispatches() - d0
            run("strided", 1)
            run("batch_id", 2)
            torch.cuda.synchronize()
            ity = torch.int64 if esz == 8 else torch.int32
            assert torch.equal(sh.io_view(0).view(ity), sh.io_view(1).view(ity)), f"indexed != strided at {nb} x {rb}"
            assert torch.equal(sh.io_view(0).view(ity), sh.io_view(2).view(ity)), f"indexed != batch at {nb} x {rb}"
            sh.io_view(0).copy_(sh.io_view(3))
            sh.io_view(1).copy_(sh.io_view(3))
            torch.cuda.synchronize()
            run("idx_perm", 0)
            run("batch_perm", 1)
            torch.cuda.synchronize()
            assert torch.equal(sh.io_view(0).view(ity), sh.io_view(1).view(ity)), f"indexed != batch (perm) at {nb} x {rb}"
            # ---- warm every way over every set
            for s in range(nsets):
                for way in WAYS:
                    run(way, s)
            t0 = time.perf_counter_ns()
            run("batch_perm", 0)
            est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
            reps = int(min(200, max(5, 20000 / est_us)))
            loop_reps = int(max(2, min(reps, 300000 / (nb * 6.0))))
            t = {w: [] for w in WAYS}
            per_round = {w: [] for w in WAYS}
            k = 0
            for r in range(rounds):
                order = WAYS[r % len(WAYS):] + WAYS[:r % len(WAYS)]
                for way in (order if r % 2 == 0 else order[::-1]):
                    mine = []
                    for _ in range(loop_reps if way == "loop" else reps):
                        s = k % nsets
                        k += 1
                        if way == "loop":
                            run(way, s, st)
                            mine.append((st[nb] - st[0]) / 1e3)
                        else:
                            t0 = time.perf_counter_ns()
                            run(way, s)
                            mine.append((time.perf_counter_ns() - t0) / 1e3)
                    t[way] += mine
                    per_round[way].append(mine)
            med = {w: float(np.median(t[w])) for w in WAYS}
            moved = 3.0 * nb * rb
            row = {"blocks": nb, "block_B": rb, "type": "fp64" if esz == 8 else "fp32",
                   "form": m.INDEXED_NAMES[info["form"]], "strided_form": m.STRIDED_NAMES[sinfo["form"]],
                   "indexed_launches": info["launches"], "indexed_groups": info["groups"], "indexed_direct": int(direct),
                   "strided_groups": sinfo["groups"], "batch_launches": binfo["launches"], "batch_groups": binfo["groups"],
                   "idx_perm_GBps": round(moved / med["idx_perm"] / 1e3, 1), "sets": nsets, "reps": reps * rounds}
            for w in WAYS:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
            row["idx_id/strided"] = round(med["idx_id"] / med["strided"], 3)
            row["batch_perm/idx_perm"] = round(med["batch_perm"] / med["idx_perm"], 2)
            rows.append(row)
            print(f"{nb:6d} x {rb:6d} B {row['type']} {row['form']:12s} loop {med['loop']:11.2f}  "
                  f"batch id {med['batch_id']:9.2f} perm {med['batch_perm']:9.2f} {row['batch_perm_rounds']}  "
                  f"strided {med['strided']:9.2f} {row['strided_rounds']}  "
                  f"indexed id {med['idx_id']:9.2f} {row['idx_id_rounds']} perm {med['idx_perm']:9.2f} {row['idx_perm_rounds']}  "
                  f"id/strided {row['idx_id/strided']:.3f}  batch/indexed {row['batch_perm/idx_perm']:.2f}  "
                  f"launches {binfo['launches']} -> {info['launches']} (direct {direct})", flush=True)
            del sets, arrs, sh, dtab
            torch.cuda.empty_cache()
    slower = [(r["blocks"], r["block_B"], r["type"]) for r in rows
              if r["blocks"] >= 128 and not r["idx_perm_us"] < r["batch_perm_us"]]
    print("shapes of 128 or more blocks where the indexed call does not take less time than the batch:", slower)
    print(json.dumps({"rows": rows, "rounds": rounds, "slower_than_batch_from_128": slower}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5,
         [tuple(int(v) for v in x.split("x")) for x in args[1].split(",")] if len(args) > 1 else DEFAULT)
