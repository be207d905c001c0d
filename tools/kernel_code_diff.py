#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.  CPU only.

    tools/kernel_code_diff.py PARENT_TREE NEW_TREE [--arch gfx950] [--llvm DIR]

Each tree holds a finished `make -C mpich-pip_amd`: mpich-pip_amd/build/*.o
and mpich-pip_amd/lib/libmpir_hip_tiles.hsaco.  For a refactor that must leave
the kernels alone this answers "did it": per unit, the functions present on
one side only, and the functions whose code or metadata differ.

Per object the .hip_fatbin section is dumped with llvm-objcopy and the
architecture's code object unbundled with clang-offload-bundler (the .hsaco is
a code object already).  Of every function symbol of the code object the tool
records the size and a hash of its code bytes; of a kernel (a function with a
.kd descriptor) also a hash of the descriptor, the code's offset from it
masked because it is layout, and the kernel's metadata from the ELF notes:
VGPR, SGPR and AGPR counts, LDS and scratch bytes, kernarg bytes, workgroup
limit.  Only hashes and numbers are compared and printed; no instruction is
decoded.  Code is position independent within a function, so a kernel that
moved inside its code object still compares equal.

Exit status 0 when both builds hold the same functions with the same code and
metadata in every unit, 1 otherwise.
"""
import argparse
import glob
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack")
EM_AMDGPU = 224
STT_OBJECT, STT_FUNC = 1, 2


def code_object(path, arch, llvm, tmp):
    """The path of `path`'s device code object for `arch`, or None if it has no device code."""
    with open(path, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF" and struct.unpack_from("<H", head, 18)[0] == EM_AMDGPU:
        return path
    fat = os.path.join(tmp, os.path.basename(path) + ".fatbin")
    r = subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path,
                        os.path.join(tmp, "discard.o")], capture_output=True, text=True)
    if r.returncode and "not found" in r.stderr:
        return None                               # an object of host code only
    if r.returncode:
        sys.exit(f"llvm-objcopy {path}: {r.stderr.strip()}")
    out = os.path.join(tmp, os.path.basename(path) + ".co")
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--output=" + out], check=True, capture_output=True)
    return out if os.path.getsize(out) else None


def functions(co):
    """{name: (size, code hash, descriptor hash or None)} of an ELF64 little-endian code object."""
    data = open(co, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    symtab = next((s for s in secs if s[1] == 2), None) or next(s for s in secs if s[1] == 11)    # SHT_SYMTAB, else SHT_DYNSYM
    strtab = secs[symtab[6]]

    def name_at(off):
        start = strtab[4] + off
        return data[start:data.index(b"\0", start)].decode()

    def body(value, size, shndx):
        sec = secs[shndx]
        start = value - sec[3] + sec[4]
        return data[start:start + size]

    syms = {}
    for i in range(symtab[5] // symtab[9]):
        st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", data, symtab[4] + i * symtab[9])
        if (st_info & 0xF) in (STT_OBJECT, STT_FUNC) and 0 < st_shndx < shnum:
            syms[name_at(st_name)] = (st_info & 0xF, st_shndx, st_value, st_size)
    out = {}
    for name, (kind, shndx, value, size) in syms.items():
        if kind != STT_FUNC:
            continue
        kd = syms.get(name + ".kd")
        kd_hash = None
        if kd:
            desc = bytearray(body(kd[2], kd[3], kd[1]))
            desc[16:24] = bytes(8)                # kernel_code_entry_byte_offset: where the code lies, not what it is
            kd_hash = hashlib.sha256(desc).hexdigest()[:16]
        out[name] = (size, hashlib.sha256(body(value, size, shndx)).hexdigest()[:16], kd_hash)
    return out


def metadata(co, llvm):
    """{kernel name: {field: value}} from the code object's AMDGPU metadata note."""
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                           check=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count", "\n" + notes)[1:]:
        block = "    .agpr_count" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: m.group(1) for k in META for m in [re.search(r"\.%s:\s+(\S+)" % k, block)] if m}
    return out


def unit(path, arch, llvm, tmp):
    co = code_object(path, arch, llvm, tmp)
    if co is None:
        return {}
    meta = metadata(co, llvm)
    return {name: rec + (tuple(sorted(meta.get(name, {}).items())),) for name, rec in functions(co).items()}


def units(tree):
    pkg = os.path.join(tree, "mpich-pip_amd")
    files = sorted(glob.glob(os.path.join(pkg, "build", "*.o"))) + [os.path.join(pkg, "lib", "libmpir_hip_tiles.hsaco")]
    return {os.path.basename(f): f for f in files if os.path.exists(f)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"))
    args = ap.parse_args()
    a, b = units(args.parent), units(args.new)
    bad = 0
    totals = [0, 0]
    print(f"kernel_code_diff: {args.arch} code of {len(a)} units (parent) against {len(b)} (new)")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in the {'parent' if name in a else 'new'} build")
            bad += 1
            continue
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            fa, fb = unit(a[name], args.arch, args.llvm, ta), unit(b[name], args.arch, args.llvm, tb)
        if not fa and not fb:
            continue                              # host code only
        only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
        differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
        kernels = sum(1 for rec in fb.values() if rec[2])
        totals[0] += len(fb)
        totals[1] += kernels
        verdict = "identical" if not (only_a or only_b or differ) else "DIFFERENT"
        print(f"{name}: {len(fb)} functions, {kernels} of them kernels, {len(only_a)} only in parent, {len(only_b)} only in new, "
              f"{len(differ)} differ: {verdict}")
        for k in only_a:
            print(f"    only in parent: {k}")
        for k in only_b:
            print(f"    only in new:    {k}")
        for k in differ:
            what = [w for w, x, y in zip(("size", "code", "descriptor", "metadata"), fa[k], fb[k]) if x != y]
            print(f"    differs in {', '.join(what)}: {k}")
            if "size" in what:
                print(f"        size {fa[k][0]} -> {fb[k][0]}")
            if "metadata" in what:
                print(f"        metadata {dict(set(fa[k][3]) - set(fb[k][3]))} -> {dict(set(fb[k][3]) - set(fa[k][3]))}")
        bad += bool(only_a or only_b or differ)
    print(f"kernel_code_diff: {totals[0]} functions, {totals[1]} kernels; "
          + ("every unit identical in kernel set, code and metadata" if not bad else f"{bad} units differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
