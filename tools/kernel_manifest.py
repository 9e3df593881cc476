#!/usr/bin/env python3
"""Per-kernel manifest of the gfx950 device code in a build directory, and the comparison of two.

    tools/kernel_manifest.py BUILD_DIR > manifest.tsv     one line per kernel of every BUILD_DIR/*.hip.o
    tools/kernel_manifest.py --compare A.tsv B.tsv        the two as sets; exit status 1 when they differ
    tools/kernel_manifest.py --digest A.tsv               per object: kernels, SHA-256 of its sorted lines

A line holds: object, mangled name, symbol size, vgpr_count, sgpr_count, group_segment_fixed_size,
private_segment_fixed_size (the code object's metadata note) and the SHA-256 of the kernel's disassembly
(instruction text only: no addresses, no encodings). Kernels are compared one by one because the order
in which a translation unit emits them is not part of what it computes.
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    run("llvm-objdump", "--offloading", obj, cwd=tmp)  # writes the bundles beside the copy
    found = glob.glob(os.path.join(tmp, os.path.basename(obj) + ".*gfx950"))
    return found[0] if found else None  # (an object of host code only has none)


def kernels(obj):
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        os.symlink(os.path.abspath(obj), local)
        co = code_object(local, tmp)
        if co is None:
            return []
        meta = {}
        for block in re.split(r"\n  - (?=\.)", run("llvm-readelf", "--notes", co)):
            f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", "    " + block, re.M))
            if "symbol" in f:
                meta[f["name"].strip("'")] = [f[k] for k in FIELDS]
        size = {}
        for line in run("llvm-readelf", "--symbols", "-W", co).splitlines():
            w = line.split()
            if len(w) == 8 and w[3] == "FUNC" and w[7] in meta:
                size[w[7]] = w[2]
        text = {}
        cur = None
        for line in run("llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co).splitlines():
            m = re.match(r"^<(\S+)>:$", line)
            if m:
                cur = text.setdefault(m.group(1), []) if m.group(1) in meta else None
            elif cur is not None and line.strip():
                cur.append(line.split("//")[0].strip())
    base = os.path.basename(obj).split(".")[0]
    return [[base, k, size[k], *meta[k], hashlib.sha256("\n".join(text[k]).encode()).hexdigest()] for k in sorted(meta)]


def compare(a, b):
    A, B = (set(open(p).read().splitlines()) for p in (a, b))
    names = lambda s: {tuple(l.split("\t")[:2]) for l in s}
    lost, added = names(A) - names(B), names(B) - names(A)
    changed = names(A - B) & names(B - A)
    print(f"{a}: {len(A)} kernels\n{b}: {len(B)} kernels")
    print(f"lost {len(lost)}, added {len(added)}, changed {len(changed)}")
    for tag, s in (("lost", lost), ("added", added), ("changed", changed)):
        for o, k in sorted(s):
            print(f"  {tag}: {o} {k}")
    print("EQUAL" if A == B else "DIFFERENT")
    return 0 if A == B else 1


def digest(a):
    """The short form that is kept on record: a manifest runs to 200 bytes a kernel."""
    rows = sorted(open(a).read().splitlines())
    for obj in sorted({r.split("\t")[0] for r in rows}):
        mine = [r for r in rows if r.split("\t")[0] == obj]
        print(f"{obj}\t{len(mine)}\t{hashlib.sha256(chr(10).join(mine).encode()).hexdigest()}")
    print(f"total\t{len(rows)}\t{hashlib.sha256(chr(10).join(rows).encode()).hexdigest()}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--digest":
        sys.exit(digest(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    for obj in sorted(glob.glob(os.path.join(sys.argv[1], "*.hip.o"))):
        for row in kernels(obj):
            print("\t".join(row))
