#!/usr/bin/env python3
"""MPIX_Reduce_local_fetch_indexed_ordered against the ordered call it extends
and against what a caller who needed every intermediate value had before it.
Per shape -- nblocks blocks of block_bytes, the input and fetchbuf packed, the
targets in slots twice the block apart, disp_unit the block's bytes -- and per
repeat factor R (blocks / distinct targets: every target named exactly R times,
the table shuffled; `one`: every block on one target, the hot row) these ways
alternate over rounds in one process, MPI_SUM on fp32 device buffers, every call
synchronous:
  fetch_ordered  one MPIX_Reduce_local_fetch_indexed_ordered, the order table
                 built before
  ordered        (a) one MPIX_Reduce_local_indexed_ordered on the same operands:
                 fetch_ordered / ordered is the cost of the extra store stream.
                 By the bytes moved it is bounded by (2 nblocks + 2 distinct) /
                 (nblocks + 2 distinct), printed as `bound`.
  rounds         (b) what a caller did before: the table split into R
                 duplicate-free rounds (round j: each target's j-th block in
                 table order) and one MPIX_Reduce_local_fetch_ragged with uniform
                 starts per round.  That call wants its input and its fetchbuf
                 packed per round; the split, the packing of each round's input
                 blocks and the unpacking of its fetched blocks are all outside
                 the timed window.  Not run past R = 64.
  no_order       (c, R = 1 only) the new call with order NULL
  fetch_ragged   (c, R = 1 only) a single MPIX_Reduce_local_fetch_ragged with
                 uniform starts on the same operands
Every shape is warmed in every way; each repetition takes the next of several
buffer sets; host clock stamps around calls that end in completion; medians over
all repetitions, us, and the lowest and highest median of a single round.
Before a shape is timed the ways are compared bit for bit on copies of one set:
the targets of all of them, and the fetched blocks of fetch_ordered against the
rounds' (unpacked), no_order's and fetch_ragged's.

    python3 tools/fetch_ordered_ab.py [rounds = 5] [shapes = 65536x256,4096x65536] [factors = 1,4,64,one]
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
        fetch = torch.empty(total // 4, dtype=torch.float32, device="cuda")          # fetchbuf, packed by block number
        fetch2 = torch.empty(total // 4, dtype=torch.float32, device="cuda")         # the other ways' (rounds: packed per round)
        packed = torch.empty(total // 4, dtype=torch.float32, device="cuda")         # the rounds' input, packed per round
        torch.cuda.synchronize()
        base_in = pool_in.data_ptr() + (-pool_in.data_ptr() % 16384)
        base_io = pool_io.data_ptr() + (-pool_io.data_ptr() % 16384)

        def io_view(s):
            lo = (base_io + s * io_set - pool_io.data_ptr()) // 4
            return pool_io[lo:lo + io_set // 4]

        def in_view(s):
            lo = (base_in + s * in_set - pool_in.data_ptr()) // 4
            return pool_in[lo:lo + in_set // 4]

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
            ways = ["fetch_ordered", "ordered"] + (["rounds"] if R <= ROUNDS_MAX_R else []) + \
                (["no_order", "fetch_ragged"] if R == 1 else [])
            # the rounds: occurrence number of each block within its target, in table order
            occ = np.empty(nb, np.int64)
            occ[horder] = np.arange(nb) - np.searchsorted(tio[horder], tio[horder], side="left")
            rtabs, first = [], 0
            if "rounds" in ways:
                for j in range(R):
                    ks = np.nonzero(occ == j)[0].astype(np.int64)
                    starts = torch.from_numpy(np.arange(len(ks) + 1, dtype=np.int64) * bl).cuda()
                    rtabs.append((torch.from_numpy(ks).cuda(), torch.from_numpy(tio[ks]).cuda(), starts, len(ks), first))
                    first += len(ks)
            starts_all = torch.from_numpy(np.arange(nb + 1, dtype=np.int64) * bl).cuda()
            info = m.fetch_indexed_ordered_plan_info(base_in, None, base_io, dtio.data_ptr(), fetch.data_ptr(), dorder.data_ptr(),
                                                     rb, nb, bl, dt, op)

            def pack_rounds(s):
                """the rounds' input blocks of set s, round after round (outside the timed window)"""
                src = in_view(s)[:nb * bl].view(nb, bl)
                for ks, _, _, n, at in rtabs:
                    packed[at * bl:(at + n) * bl].view(n, bl).copy_(src[ks])
                torch.cuda.synchronize()

            def run(way, s):
                pi, po = base_in + s * in_set, base_io + s * io_set
                if way == "fetch_ordered":
                    rc = lib.MPIX_Reduce_local_fetch_indexed_ordered(pi, None, po, dtio.data_ptr(), fetch.data_ptr(),
                                                                     dorder.data_ptr(), rb, nb, bl, dt, op, None)
                elif way == "ordered":
                    rc = lib.MPIX_Reduce_local_indexed_ordered(pi, None, po, dtio.data_ptr(), dorder.data_ptr(), rb, nb, bl,
                                                               dt, op, None)
                elif way == "rounds":
                    rc = 0
                    for _, tio_j, starts_j, n, at in rtabs:
                        rc = rc or lib.MPIX_Reduce_local_fetch_ragged(packed.data_ptr() + at * rb, po, tio_j.data_ptr(),
                                                                      fetch2.data_ptr() + at * rb, starts_j.data_ptr(), rb, n,
                                                                      n * bl, dt, op, None)
                elif way == "no_order":
                    rc = lib.MPIX_Reduce_local_fetch_indexed_ordered(pi, None, po, dtio.data_ptr(), fetch2.data_ptr(), None,
                                                                     rb, nb, bl, dt, op, None)
                else:
                    rc = lib.MPIX_Reduce_local_fetch_ragged(pi, po, dtio.data_ptr(), fetch2.data_ptr(), starts_all.data_ptr(),
                                                            rb, nb, nb * bl, dt, op, None)
                assert rc == 0, m.error_string(rc)

            # ---- the ways agree bit for bit at this shape (the other sets copies of set 0)
            keep = io_view(0).clone()
            for s in range(1, nsets):
                in_view(s).copy_(in_view(0))
            torch.cuda.synchronize()
            if "rounds" in ways:
                pack_rounds(0)          # every set holds the same input from here on
            run("fetch_ordered", 0)
            checked = []
            for way in ways[1:]:
                io_view(1).copy_(keep)
                torch.cuda.synchronize()
                run(way, 1)
                torch.cuda.synchronize()
                assert torch.equal(io_view(0).view(torch.int32), io_view(1).view(torch.int32)), \
                    f"fetch_ordered's target != {way}'s at {nb} x {rb} R {f}"
                if way == "rounds":
                    got = torch.empty_like(fetch).view(nb, bl)
                    for ks, _, _, n, at in rtabs:
                        got[ks] = fetch2[at * bl:(at + n) * bl].view(n, bl)
                    assert torch.equal(fetch.view(torch.int32), got.view(-1).view(torch.int32)), \
                        f"fetch_ordered's fetchbuf != the rounds' at {nb} x {rb} R {f}"
                    del got
                elif way != "ordered":
                    assert torch.equal(fetch.view(torch.int32), fetch2.view(torch.int32)), \
                        f"fetch_ordered's fetchbuf != {way}'s at {nb} x {rb} R {f}"
                checked.append(way)
            for s in range(nsets):
                io_view(s).copy_(keep)
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
                   "fetch_ordered_GBps": round((2.0 * nb + 2.0 * distinct) * rb / med["fetch_ordered"] / 1e3, 1),
                   "fetch_ordered/ordered": round(med["fetch_ordered"] / med["ordered"], 3),
                   "bound_fetch_ordered/ordered": round((2.0 * nb + 2.0 * distinct) / (nb + 2.0 * distinct), 2),
                   "us_per_contribution": round(med["fetch_ordered"] / R, 3)}
            for w in ways:
                row[w + "_us"] = round(med[w], 2)
                row[w + "_rounds"] = spread(per_round[w])
                row[w + "_reps"] = reps[w] * rounds
            if "rounds" in ways:
                row["rounds/fetch_ordered"] = round(med["rounds"] / med["fetch_ordered"], 2)
            if "fetch_ragged" in ways:
                row["no_order/fetch_ragged"] = round(med["no_order"] / med["fetch_ragged"], 3)
            rows.append(row)
            print(f"{nb:6d} x {rb:6d} B R {f:>3s} ({distinct:6d} targets) {row['form']:10s} " +
                  "  ".join(f"{w} {med[w]:.2f} {row[w + '_rounds']}" for w in ways) +
                  f"  fetch_ordered/ordered {row['fetch_ordered/ordered']:.3f} (bound {row['bound_fetch_ordered/ordered']:.2f})" +
                  (f"  rounds/fetch_ordered {row['rounds/fetch_ordered']:.2f}" if "rounds" in ways else "") +
                  (f"  no_order/fetch_ragged {row['no_order/fetch_ragged']:.3f}" if "fetch_ragged" in ways else "") +
                  f"  fetch_ordered {row['fetch_ordered_GBps']} GB/s of its own bytes", flush=True)
            del rtabs, dtio, dorder, starts_all
        del pool_in, pool_io, work, fetch, fetch2, packed
        torch.cuda.empty_cache()
    print(json.dumps({"rows": rows, "rounds": rounds}))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 5,
         [tuple(int(v) for v in x.split("x")) for x in args[1].split(",")] if len(args) > 1 else DEFAULT,
         args[2].split(",") if len(args) > 2 else FACTORS)
