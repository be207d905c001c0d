#!/usr/bin/env python3
"""MPIX_Reduce_local_subarray against the two ways a caller had before it.  Per
shape -- a sub-box of an N-dimensional array on either side, MPI_SUM on device
buffers, MPI_ORDER_C -- three ways of doing the same work alternate over rounds
in one process:
  planes    the loop of synchronous MPIX_Reduce_local_strided calls, one per
            index of the outermost dimension the box's normal form keeps
  indexed   one synchronous MPIX_Reduce_local_indexed over device displacement
            tables of the same rows (disp_unit 16 where every row's offset is a
            multiple of 16, so that it may take vectors, else the element's
            size); building and uploading the tables is timed once, apart
  subarray  one synchronous MPIX_Reduce_local_subarray
planes and indexed exist without the subarray call: they are the yardstick.
Every shape is warmed in every way; each repetition takes the next of several
distinct buffer sets; host clock stamps around calls that end in completion;
medians over all repetitions, us, and the lowest and highest median of a single
round (the spread between alternated rounds).  Before a shape is timed the three
ways' results are compared bit for bit on it.  A shape whose normal form keeps
one outer dimension is the strided call itself: there `planes` is that one call.

    python3 tools/subarray_ab.py [rounds = 5] [shape names, comma separated]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpich-pip_amd"))
sys.path.insert(0, ROOT)

import mpich_pip_amd as m  # noqa: E402  (the library first: VRAM rings)

MIB, GIB = 1 << 20, 1 << 30
C3 = [256, 256, 256]
SLAB = [64, 512, 512]
# name: (type, subsizes, in sizes, in starts, inout sizes, inout starts); sizes None: packed
SHAPES = {
    "interior-254^3": ("f64", [254, 254, 254], C3, [1, 1, 1], C3, [1, 1, 1]),
    "face-1-slow": ("f64", [1, 254, 254], C3, [255, 1, 1], C3, [1, 1, 1]),
    "face-1-middle": ("f64", [254, 1, 254], C3, [1, 255, 1], C3, [1, 1, 1]),
    "face-1-fast": ("f64", [254, 254, 1], C3, [1, 1, 255], C3, [1, 1, 1]),
    "face-2-slow": ("f64", [2, 254, 254], C3, [254, 1, 1], C3, [1, 1, 1]),
    "face-2-middle": ("f64", [254, 2, 254], C3, [1, 254, 1], C3, [1, 1, 1]),
    "face-2-fast": ("f64", [254, 254, 2], C3, [1, 1, 254], C3, [1, 1, 1]),
    "slab-32-of-64x512^2": ("f32", [32, 510, 510], SLAB, [16, 1, 1], SLAB, [16, 1, 1]),
    "packed-to-interior": ("f64", [254, 254, 254], None, None, C3, [1, 1, 1]),
    "interior-to-packed": ("f64", [254, 254, 254], C3, [1, 1, 1], None, None),
    "collapsing-254x(254x256)": ("f64", [254, 254, 256], C3, [1, 1, 0], C3, [1, 1, 0]),
}


def prod(v):
    n = 1
    for x in v:
        n *= x
    return n


class Shape:
    """nsets buffer sets of one shape, each array's origin on a 16 KiB boundary."""

    def __init__(self, torch, name, nsets):
        ty, self.sub, self.isz, self.ist, self.osz, self.ost = SHAPES[name]
        self.name, self.nsets = name, nsets
        self.dt, self.esz, fdt = (m.MPI_DOUBLE, 8, torch.float64) if ty == "f64" else (m.MPI_FLOAT, 4, torch.float32)
        self.ity = torch.int64 if ty == "f64" else torch.int32
        up = lambda b: -(-b // 16384) * 16384
        self.in_set = up(prod(self.isz or self.sub) * self.esz)
        self.io_set = up(prod(self.osz or self.sub) * self.esz)
        self.pool_in = torch.rand((nsets * self.in_set + 16384) // self.esz, device="cuda", dtype=fdt) * 1e-3
        self.pool_io = torch.rand((nsets * self.io_set + 16384) // self.esz, device="cuda", dtype=fdt)
        torch.cuda.synchronize()
        self.base_in = self.pool_in.data_ptr() + (-self.pool_in.data_ptr() % 16384)
        self.base_io = self.pool_io.data_ptr() + (-self.pool_io.data_ptr() % 16384)
        self.plan = m.subarray_plan_info(self.base_in, self.isz, self.ist, self.base_io, self.osz, self.ost, self.sub,
                                         m.MPI_ORDER_C, self.dt, m.MPI_SUM)
        self.args = [m._ints(x) for x in (self.isz, self.ist, self.osz, self.ost, self.sub)]

    def ptrs(self, s):
        return self.base_in + s * self.in_set, self.base_io + s * self.io_set

    def view(self, which, s):
        pool, base, size = (self.pool_in, self.base_in, self.in_set) if which == "in" else (self.pool_io, self.base_io, self.io_set)
        lo = (base + s * size - pool.data_ptr()) // self.esz
        return pool[lo:lo + size // self.esz]


def spread(per_round):
    import numpy as np
    meds = [float(np.median(r)) for r in per_round if r]
    return round(min(meds), 2), round(max(meds), 2)


def main(rounds, names):
    import numpy as np
    lib = m.load()
    import torch
    import bench
    lib.MPIX_Reduce_local_set_errhandler(m.MPI_ERRORS_RETURN)
    torch.cuda.set_device(0)
    state = lib.MPIR_Hip_direct_prepare(0)
    bench.bind_near_gpu(m, 0)
    print(f"build {m.build_id()}; direct state {state}; {torch.cuda.get_device_name(0)}; rounds {rounds}")
    rows = []
    for name in names:
        ty, sub = SHAPES[name][0], SHAPES[name][1]
        moved = 3 * prod(sub) * (8 if ty == "f64" else 4)
        nsets = 4 if moved > 64 * MIB else 8
        sh = Shape(torch, name, nsets)
        p = sh.plan
        k, bl = p["k"], p["blocklen"]
        assert k in (1, 2), (name, p)
        n1, si1, so1 = p["n"][0], p["in_stride"][0], p["io_stride"][0]
        planes = p["n"][1] if k == 2 else 1
        si2, so2 = (p["in_stride"][1], p["io_stride"][1]) if k == 2 else (0, 0)
        # ---- the rows' displacement tables for the indexed call (built and uploaded once, timed apart)
        t0 = time.perf_counter_ns()
        i2, i1 = np.meshgrid(np.arange(planes, dtype=np.int64), np.arange(n1, dtype=np.int64), indexing="ij")
        din = (p["in_offset"] + i1 * si1 + i2 * si2).ravel()
        dio = (p["io_offset"] + i1 * so1 + i2 * so2).ravel()
        unit = 16 if not ((din | dio) & 15).any() else sh.esz
        din //= unit
        dio //= unit
        t_build = (time.perf_counter_ns() - t0) / 1e3
        t0 = time.perf_counter_ns()
        tin, tio = torch.from_numpy(din).cuda(), torch.from_numpy(dio).cuda()
        torch.cuda.synchronize()
        t_upload = (time.perf_counter_ns() - t0) / 1e3
        nrows = din.size
        iinfo = m.indexed_plan_info(sh.base_in, tin.data_ptr(), sh.base_io, tio.data_ptr(), unit, nrows, bl, sh.dt, m.MPI_SUM)

        def run_subarray(s):
            pi, po = sh.ptrs(s)
            a = sh.args
            rc = lib.MPIX_Reduce_local_subarray(pi, a[0], a[1], po, a[2], a[3], len(sh.sub), a[4], m.MPI_ORDER_C, sh.dt,
                                                m.MPI_SUM, None)
            assert rc == 0, m.error_string(rc)

        def run_planes(s):
            pi, po = sh.ptrs(s)
            pi += p["in_offset"]
            po += p["io_offset"]
            for j in range(planes):
                rc = lib.MPIX_Reduce_local_strided(pi + j * si2, si1, po + j * so2, so1, n1, bl, sh.dt, m.MPI_SUM, None)
                assert rc == 0, m.error_string(rc)

        def run_indexed(s):
            pi, po = sh.ptrs(s)
            rc = lib.MPIX_Reduce_local_indexed(pi, tin.data_ptr(), po, tio.data_ptr(), unit, nrows, bl, sh.dt, m.MPI_SUM, None)
            assert rc == 0, m.error_string(rc)

        ways = {"planes": run_planes, "indexed": run_indexed, "subarray": run_subarray}
        # ---- the three ways agree bit for bit at this shape (sets 1 and 2 copies of set 0)
        for s in (1, 2):
            sh.view("io", s).copy_(sh.view("io", 0))
            sh.view("in", s).copy_(sh.view("in", 0))
        torch.cuda.synchronize()
        before = sh.view("io", 0).clone()
        run_subarray(0)
        run_planes(1)
        run_indexed(2)
        torch.cuda.synchronize()
        assert not torch.equal(sh.view("io", 0).view(sh.ity), before.view(sh.ity)), f"{name}: nothing written"
        assert torch.equal(sh.view("io", 0).view(sh.ity), sh.view("io", 1).view(sh.ity)), f"subarray != planes at {name}"
        assert torch.equal(sh.view("io", 0).view(sh.ity), sh.view("io", 2).view(sh.ity)), f"subarray != indexed at {name}"
        del before
        for s in range(nsets):
            for fn in ways.values():
                fn(s)
        t0 = time.perf_counter_ns()
        run_subarray(0)
        est_us = max((time.perf_counter_ns() - t0) / 1e3, 1.0)
        reps = int(min(100, max(5, 10000 / est_us)))
        plane_reps = int(max(2, min(reps, 40000 / (planes * 10.0))))
        t = {w: [] for w in ways}
        per_round = {w: [] for w in ways}
        orders = (("planes", "indexed", "subarray"), ("subarray", "indexed", "planes"), ("indexed", "subarray", "planes"))
        kk = 0
        for r in range(rounds):
            for way in orders[r % 3]:
                mine = []
                for _ in range(plane_reps if way == "planes" else reps):
                    s = kk % nsets
                    kk += 1
                    t0 = time.perf_counter_ns()
                    ways[way](s)
                    mine.append((time.perf_counter_ns() - t0) / 1e3)
                t[way] += mine
                per_round[way].append(mine)
        med = {w: float(np.median(t[w])) for w in ways}
        row = {"shape": name, "sub": sub, "form": m.SUBARRAY_NAMES[p["form"]], "k": k, "rows": nrows, "row_B": bl * sh.esz,
               "planes": planes, "planes_us": round(med["planes"], 2), "indexed_us": round(med["indexed"], 2),
               "subarray_us": round(med["subarray"], 2), "planes_rounds": spread(per_round["planes"]),
               "indexed_rounds": spread(per_round["indexed"]), "subarray_rounds": spread(per_round["subarray"]),
               "planes/subarray": round(med["planes"] / med["subarray"], 2),
               "indexed/subarray": round(med["indexed"] / med["subarray"], 3),
               "per_plane_us": round(med["planes"] / planes, 2),
               "subarray_GBps": round(moved / med["subarray"] / 1e3, 1),
               "launches": p["launches"], "groups": p["groups"], "indexed_form": m.INDEXED_NAMES[iinfo["form"]],
               "indexed_groups": iinfo["groups"], "disp_unit": unit, "table_build_us": round(t_build, 1),
               "table_upload_us": round(t_upload, 1), "sets": nsets, "reps": reps * rounds}
        rows.append(row)
        print(f"{name:26s} {row['form']:12s} k={k} rows {nrows:6d} x {row['row_B']:7d} B  planes({planes}) {med['planes']:10.2f} "
              f"{row['planes_rounds']}  indexed {med['indexed']:9.2f} {row['indexed_rounds']}  subarray {med['subarray']:9.2f} "
              f"{row['subarray_rounds']}  planes/sub {row['planes/subarray']:7.2f}  indexed/sub {row['indexed/subarray']:6.3f}  "
              f"tables {t_build:.0f} + {t_upload:.0f} us", flush=True)
        del sh, tin, tio
        torch.cuda.empty_cache()
    slower = [r["shape"] for r in rows if not r["subarray_us"] < r["indexed_us"]]
    print("shapes where the subarray call does not take less time than the indexed call:", slower)
    # planes from which one call beats the loop: the call's time over the loop's time per plane
    for r in rows:
        if r["planes"] > 1:
            print(f"{r['shape']}: one call equals {r['subarray_us'] / r['per_plane_us']:.1f} planes of the loop")
    print(json.dumps({"rows": rows, "rounds": rounds, "slower_than_indexed": slower}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5, args[1].split(",") if len(args) > 1 else list(SHAPES))
