"""The launch planner, swept on made-up addresses (no GPU): MPIR_Hip_plan_info
and MPIR_Hip_combine_plan_info report the plan the launch itself computes
(plan_reduce / plan_reduce_wide / combine_split, reduce_kernels.hpp), and the
properties below are what the kernels rely on -- the head / body / tail
partition, the 16-byte alignment of the vector region, the lane ranges
workgroup 0 gives head and tail, the 16 KiB address grid's cover, and when
each kind may be chosen at all.  They are stated from the kernels' needs, not
from the planner's code.

The sweep runs in child processes (one per element class, side by side) that
never open the GPU: the functions only do arithmetic on the pointer values.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (label, element class, op, element size, alignment): one class per size, and
# the 16-byte class with 8-byte alignment
CLASSES = [("u8", "U8", 3, 1, 1), ("f16", "F16", 3, 2, 2), ("f32", "F32", 3, 4, 4), ("f64", "F64", 3, 8, 8),
           ("cf64", "CF64", 3, 16, 8), ("x80", "F80", 3, 16, 16)]

CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import mpich_pip_amd as m
lib = m.load()
elem, op, esz, align = m.ELEM[sys.argv[2]], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
TILE = 16384
BASE = 1 << 32
LEAN, FULL, SHIFT, ELEMS, ELEMS_U = range(5)
f = lib.MPIR_Hip_plan_info
out, out2 = (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 6)()
vec = 16 // esz
counts = set(range(1, 2 * vec + 3))
for tiles in (1, 2, 3):
    b = tiles * TILE // esz
    counts |= set(range(b - vec - 2, b + vec + 3))
counts = sorted(c for c in counts if c >= 1)
assert counts[-1] * esz > 3 * TILE
phases = sorted({0, 16, 4096, TILE - 16, TILE - esz})
seen = {k: 0 for k in range(5)}
cases = 0


def fail(msg, ai, ao, count, got):
    raise SystemExit(f"{sys.argv[2]}: {msg}: in=BASE+{ai - BASE} io=BASE+{ao - BASE} count={count} plan={got}")


for phase in phases:
    for off_io in range(32):
        ao = BASE + phase + off_io
        for off_in in range(32):
            ai = BASE + 8 * TILE + phase + off_in
            natural = ai % align == 0 and ao % align == 0
            for count in counts:
                if f(ai, ao, count, op, elem, out) != 0 or f(ai, ao, count, op, elem, out2) != 0:
                    fail("no plan", ai, ao, count, None)
                got = tuple(out)
                if got != tuple(out2):
                    fail("two answers for one question", ai, ao, count, (got, tuple(out2)))
                kind, groups, nhead, ntail, vbytes, keep = got
                nbytes = count * esz
                cases += 1
                if kind not in seen:
                    fail("unknown kind", ai, ao, count, got)
                seen[kind] += 1
                if keep not in (0, vbytes):
                    fail("keep is neither none nor all of the vector region", ai, ao, count, got)
                if kind in (LEAN, FULL, SHIFT):
                    vs = ao + nhead * esz               # where the vector region of inout starts
                    if nhead * esz + vbytes + ntail * esz != nbytes:
                        fail("head + body + tail != payload", ai, ao, count, got)
                    if vbytes % 16:
                        fail("vector region not whole vectors", ai, ao, count, got)
                    if vbytes and vs % 16:
                        fail("vector region of inout not 16 B-aligned", ai, ao, count, got)
                    if nhead * esz >= 16 or ntail * esz >= 16:
                        fail("head or tail holds a whole vector", ai, ao, count, got)
                    if nhead > 64 or ntail > 192:
                        fail("head / tail exceed workgroup 0's lane ranges", ai, ao, count, got)
                    if ao % align:
                        fail("element stores to an unaligned inout", ai, ao, count, got)
                if kind in (LEAN, FULL):
                    if (kind == LEAN) != (nhead == 0 and ntail == 0):
                        fail("lean <=> no head and no tail", ai, ao, count, got)
                    if (ai - ao) % 16 or not natural:
                        fail("aligned tile kernel on operands of unequal or unnatural alignment", ai, ao, count, got)
                    if groups < 1:
                        fail("empty grid", ai, ao, count, got)
                    t0 = vs // TILE                     # first tile of the address grid
                    if (t0 + groups) * TILE < vs + vbytes:
                        fail("grid does not cover the vector region", ai, ao, count, got)
                    last_lo = max((t0 + groups - 1) * TILE, vs)
                    if last_lo >= vs + vbytes and not (vbytes == 0 and groups == 1):
                        fail("last tile empty", ai, ao, count, got)
                elif kind == SHIFT:
                    if (ai - ao) % 16 == 0 or nbytes < 2 * TILE:
                        fail("shift kernel outside its domain", ai, ao, count, got)
                    if groups != -(-vbytes // TILE) or groups < 1:
                        fail("shift grid != ceil(vbytes / tile)", ai, ao, count, got)
                else:
                    if groups != min(4096, -(-count // 256)):
                        fail("element grid", ai, ao, count, got)
                    if (kind == ELEMS) != natural:
                        fail("natural element kernel <=> both pointers naturally aligned", ai, ao, count, got)
                    if nhead or ntail or vbytes or keep:
                        fail("element plan reports a split", ai, ao, count, got)
                    # operands the tile kernels serve must not end up here
                    if natural and (ai - ao) % 16 == 0 and ao % esz == 0:
                        fail("aligned operands on the element kernel", ai, ao, count, got)
                    if ao % align == 0 and ao % esz == 0 and nbytes >= 2 * TILE:
                        fail("two tiles or more with an aligned inout on the element kernel", ai, ao, count, got)
print(cases, *[seen[k] for k in range(5)])
"""

COMBINE_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import mpich_pip_amd as m
lib = m.load()
TREE, CHAIN = 0, 1
COPY, VECTOR, ELEMENTS, ANY = range(4)
BASE = 1 << 32
f = lib.MPIR_Hip_combine_plan_info
out = (ctypes.c_uint64 * 4)()
cases = 0


def ask(ins, o, count, op, elem, order):
    arr = (ctypes.c_void_p * len(ins))(*ins)
    rc = f(arr, len(ins), o, count, op, elem, order, out)
    assert rc == 0, (rc, ins, o, count, op, elem, order)
    return tuple(out)


# pairs with fused folds: SUM over one class per element size, and the 16-byte
# class with 8-byte alignment
for name, esz, align in (("U8", 1, 1), ("F16", 2, 2), ("F32", 4, 4), ("F64", 8, 8), ("CF64", 16, 8)):
    elem, op = m.ELEM[name], 3
    vec = 16 // esz
    counts = sorted(set(range(1, 2 * vec + 3)) | {3001, 16384 // esz - 1, 16384 // esz, 16384 // esz + 1})
    for order, n in ((TREE, 2), (TREE, 4), (TREE, 8), (CHAIN, 2), (CHAIN, 3), (CHAIN, 5), (CHAIN, 8)):
        for off_out in range(32):
            o = BASE + off_out
            # every operand at the output's offset; then operand n - 1 at every other
            for off_last in range(32):
                ins = [BASE + (j + 1) * (1 << 20) + off_out for j in range(n - 1)]
                ins.append(BASE + n * (1 << 20) + off_last)
                natural = o % align == 0 and all(a % align == 0 for a in ins)
                equal = all((a - o) % 16 == 0 for a in ins)
                for count in counts:
                    path, passes, nhead, ntail = ask(ins, o, count, op, elem, order)
                    cases += 1
                    nbytes = count * esz
                    assert passes == 1, (name, order, n, passes)
                    assert path in (VECTOR, ELEMENTS), (name, order, n, path)
                    unfit = (not natural) or (not equal) or o % esz != 0
                    assert (path == ELEMENTS) == unfit, (name, order, n, off_out, off_last, count, path)
                    if path == ELEMENTS:
                        assert nhead == 0 and ntail == 0
                        continue
                    vbytes = nbytes - (nhead + ntail) * esz
                    assert vbytes >= 0 and vbytes % 16 == 0, (name, off_out, count, nhead, ntail)
                    assert nhead * esz < 16 and ntail * esz < 16 and nhead <= 64 and ntail <= 192
                    assert nhead * esz <= nbytes, "head clamped to the payload"
                    if vbytes or ntail:
                        assert (o + nhead * esz) % 16 == 0, (name, off_out, count, nhead)
                    else:
                        # the whole payload is head: it ends at or before the next 16 B boundary
                        assert (o % 16) + nbytes <= 16, (name, off_out, count, nhead)

# passes: one for n <= 8, two for CHAIN 9-15; TREE beyond 8 and the classes without
# a fused fold take the any-kernel; one operand, or REPLACE, is a copy
F32 = m.ELEM["F32"]
for n in range(2, 9):
    assert ask([BASE + j * 4096 for j in range(n)], BASE + 64 * 4096, 100, 3, F32, CHAIN)[:2] == (VECTOR, 1)
for n in range(9, 16):
    assert ask([BASE + j * 4096 for j in range(n)], BASE + 64 * 4096, 100, 3, F32, CHAIN)[:2] == (VECTOR, 2)
assert ask([BASE + j * 4096 for j in range(16)], BASE + 64 * 4096, 100, 3, F32, CHAIN)[:2] == (VECTOR, 3)
# a later pass's misaligned operand shows
ins = [BASE + j * 4096 for j in range(12)]
ins[10] += 4
assert ask(ins, BASE + 64 * 4096, 100, 3, F32, CHAIN)[:2] == (ELEMENTS, 2)
assert ask([BASE + j * 4096 for j in range(16)], BASE + 64 * 4096, 100, 3, F32, TREE)[0] == ANY
# the 32-byte classes have no fused fold
assert ask([BASE, BASE + 4096, BASE + 8192], BASE, 100, 12, m.ELEM["PLDOUBLEINT"], CHAIN)[:2] == (ANY, 1)
assert ask([BASE + j * 4096 for j in range(13)], BASE, 100, 3, m.ELEM["CF80"], CHAIN)[:2] == (ANY, 1)
assert ask([BASE], BASE + 4096, 100, 3, F32, CHAIN)[0] == COPY
assert ask([BASE, BASE + 4096], BASE + 8192, 100, 13, F32, CHAIN)[0] == COPY                # REPLACE
arr = (ctypes.c_void_p * 3)(BASE, BASE, BASE)
assert f(arr, 3, BASE, 10, 3, F32, TREE, out) == 3                                          # TREE of 3: refused
assert f(arr, 3, BASE, 10, 3, 0, CHAIN, out) == 3
print(cases)
"""

WIDE_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import mpich_pip_amd as m
lib = m.load()
f = lib.MPIR_Hip_plan_info
out = (ctypes.c_uint64 * 6)()
BASE = 1 << 32
WIDE_TILE, WIDE_ELEMS = 5, 6
# (class, op, bytes of one workgroup's tile): MAXLOC pairs 2 elements per lane, complex PROD 1 or 2
for name, op in (("PLDOUBLEINT", 12), ("PLDOUBLEINT", 11), ("CF80", 3), ("CF80", 4)):
    elem = m.ELEM[name]
    for off_io in range(0, 33):
        for off_in in range(0, 33):
            for count in (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2 * 1048576 + 4099):
                assert f(BASE + (1 << 30) + off_in, BASE + off_io, count, op, elem, out) == 0
                kind, groups, nhead, ntail, vbytes, keep = tuple(out)
                assert kind == (WIDE_TILE if off_io % 16 == 0 and off_in % 16 == 0 else WIDE_ELEMS), (name, off_in, off_io)
                assert nhead == 0 and ntail == 0
                if kind == WIDE_TILE:
                    assert vbytes == 32 * count and keep in (0, vbytes)
                    # whole tiles of 256 lanes x 1 or 2 elements cover the payload, the last one not empty
                    assert any(groups == -(-vbytes // t) for t in (8192, 16384)), (name, count, groups)
                else:
                    assert vbytes == 0 and keep == 0 and groups == min(4096, -(-count // 256))
# no kernel: REPLACE's byte copy has no plan; float BAND does not exist
assert f(BASE, BASE, 10, 13, m.ELEM["F32"], out) == 3
assert f(BASE, BASE, 10, 6, m.ELEM["F32"], out) == 3
assert f(BASE, BASE, 10, 3, 0, out) == 3 and f(BASE, BASE, 10, 0, 1, out) == 3
# the keep window: above MPIR_Hip_set_keep_min_bytes and at most MPIR_Hip_set_keep_bytes
prev = lib.MPIR_Hip_set_keep_min_bytes(0)
assert f(BASE + 4096, BASE, 1000, 3, m.ELEM["F32"], out) == 0 and out[5] == out[4] == 4000 - 4000 % 16
lib.MPIR_Hip_set_keep_min_bytes(prev)
assert f(BASE + 4096, BASE, 1000, 3, m.ELEM["F32"], out) == 0 and out[5] == 0
print("ok")
"""


def child(code, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MPIR_CVAR_REDUCE_LOCAL_KEEP")}
    return subprocess.Popen([sys.executable, "-c", code, os.path.join(ROOT, "mpich-pip_amd"), *map(str, args)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def finish(p, timeout=120):
    out, err = p.communicate(timeout=timeout)
    assert p.returncode == 0, (out + err)[-3000:]
    return out.split()


@pytest.fixture(scope="module")
def sweep():
    """Every class's sweep, run side by side: {label: [cases, per-kind counts...]}."""
    procs = {label: child(CHILD, cls, op, esz, align) for label, cls, op, esz, align in CLASSES}
    res = {}
    for label, p in procs.items():
        try:
            res[label] = finish(p)
        except AssertionError as e:
            res[label] = e
    return res


@pytest.mark.parametrize("label", [c[0] for c in CLASSES])
def test_single_operand_plan_properties(sweep, label):
    """in and inout at every offset 0-31, inout at five phases of the 16 KiB grid,
    counts from 1 to past three tiles and all within two elements (and one
    head) of a vector, tile, two-tile or three-tile boundary."""
    r = sweep[label]
    if isinstance(r, AssertionError):
        raise r
    cases, lean, full, shift, elems, elems_u = (int(x) for x in r)
    esz, align = next((c[3], c[4]) for c in CLASSES if c[0] == label)
    assert cases == lean + full + shift + elems + elems_u and cases > 100000
    # the sweep reached every kind the class has (an unnatural offset needs alignment > 1;
    # naturally aligned pointers of unequal alignment mod 16, alignment < 16)
    assert lean and shift, r
    assert (elems > 0) == (align < 16), r
    assert full or esz == 16, r
    assert (elems_u > 0) == (align > 1), r


def test_combine_plan_properties():
    assert int(finish(child(COMBINE_CHILD))[0]) > 100000


def test_wide_plan_no_kernel_and_keep():
    assert finish(child(WIDE_CHILD)) == ["ok"]


def test_gpu_sweep_shapes_land_on_their_kinds(mpi):
    """The shapes tests/test_plan_edges_gpu.py runs, on made-up arenas: each lands
    on the plan kind it aims at (the GPU test asserts the same on its real
    addresses before every call), and together they reach every kind."""
    import _types as T
    import test_plan_edges_gpu as E
    reached = set()
    for op, t, align in E.CASES:
        sh = E.shapes(t, align)
        assert len(sh) == len({s[:3] for s in sh})
        for slot in (E.TILE, 4 * E.TILE):
            for n, pin, pio, kind in sh:
                info = mpi.plan_info((1 << 32) + slot + pin, (1 << 33) + slot + pio, n, mpi.DATATYPES[t], mpi.OPS[op])
                assert info["kind"] == kind, (op, t, n, pin, pio, mpi.PLAN_NAMES[kind], info)
                assert (slot + max(pin, pio)) + n * T.elem_size(t) + E.TILE <= 12 * E.TILE
                reached.add(kind)
    for op, t, pin, pio, kind in E.STRIDE:
        info = mpi.plan_info((1 << 32) + pin, (1 << 33) + pio, E.STRIDE_COUNT, mpi.DATATYPES[t], mpi.OPS[op])
        assert (info["kind"], info["groups"]) == (kind, 4096), (op, t, info)
    assert reached == set(range(7))
