#!/usr/bin/env python3
"""Is the device code of two trees the same?  python tools/device_asm_diff.py [--rename REGEX=REPL] OTHER_TREE [THIS_TREE]

Compiles every file of _build.SOURCES in both trees to device-only assembly with the build's own flags (_build._flags(source)
+ --cuda-device-only -S) and compares. Lines naming __hip_cuid_ (a hash of the translation unit) may differ. A file whose
lines differ otherwise is compared kernel by kernel (a host-side change of dispatch order makes the compiler emit the same
kernels in another order, which renumbers the local labels): same set of kernels, same body and .amdhsa_ block per kernel,
same metadata entry per kernel; every kernel that differs is named. `--rename REGEX=REPL` rewrites THIS tree's assembly first:
a kernel template that gained a parameter keeps its old symbol for the instances that existed (the new instances are then the
only kernels named). Exit status 0 = the same device code. No GPU needed."""
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))), os.path.join(tree, "unsloth_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(tree, out):
    b = load_build(tree)

    def one(s):
        dst = os.path.join(out, s.replace(".hip", ".s"))
        cmd = [b._hipcc()] + b._flags(s) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, s), "-o", dst]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stderr)
        return s, open(dst).read()

    with ThreadPoolExecutor(8) as ex:
        return dict(ex.map(one, b.SOURCES))


def kernels(text):
    """{symbol: text from its section line to the next function's}, {kernel name: its metadata entry}"""
    code, _, meta = text.partition("\t.amdgpu_metadata")
    begin = r"\t\.(?:protected|globl|weak)\t(\S+)\s*; -- Begin function"
    parts = re.split(r"(?m)^(?=(?:\t\.section\t\.text\.\S+\n|\t\.text\n)?" + begin.replace("(\\S+)", "\\S+") + ")", code)
    out, carry = {"": parts[0]}, ""
    for p in parts[1:]:
        p, carry = carry + p, ""
        m = re.search("(?m)^" + begin, p)
        if m is None:                                    # (the split also stops between a section line and its function)
            carry = p
            continue
        p = re.sub(r"\.L(func_end|func_begin|BB|tmp|sec_end)\d+", r".L\1#", p)      # running number of the function
        p = re.sub(r"\bBB\d+(_\d+)", r"BB#\1", p)
        p = re.sub(r"[ \t]+;", " ;", p)                  # the comment column depends on the label's width
        out[m.group(1)] = "\n".join(l for l in p.split("\n") if "__hip_cuid_" not in l)
    md = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"(?m)^(?=  - \.a)", meta)[1:]}
    return out, md


def main():
    argv, renames = sys.argv[1:], []
    while argv and argv[0] == "--rename":
        renames.append(argv[1].split("=", 1))
        argv = argv[2:]
    other = os.path.abspath(argv[0])
    this = os.path.abspath(argv[1]) if len(argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = assemble(other, ta), assemble(this, tb)
    for pat, repl in renames:
        b = {s: re.sub(pat, repl, t) for s, t in b.items()}
    if set(a) != set(b):
        print("different SOURCES:", sorted(set(a) ^ set(b)))
        return 1
    foreign_total = reordered = bad = 0
    for s in sorted(a):
        d = [l for l in difflib.unified_diff(a[s].split("\n"), b[s].split("\n"), lineterm="", n=0)
             if l[:1] in "+-" and not l.startswith(("+++", "---"))]
        foreign = [l for l in d if "__hip_cuid_" not in l]
        msg = f"{s:24s} {len(d) - len(foreign):3d} __hip_cuid_ lines, {len(foreign)} foreign lines"
        if foreign:
            (ka, ma), (kb, mb) = kernels(a[s]), kernels(b[s])
            diff = sorted({k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k)} | {k for k in set(ma) | set(mb) if ma.get(k) != mb.get(k)})
            if diff:
                bad += 1
                msg += f" -- DEVICE CODE DIFFERS: {len(diff)} kernels" + "".join("\n    " + k for k in diff)
            else:
                reordered += 1
                foreign = []
                msg += f" -- emitted in another order; kernel by kernel: {len(ka) - 1} kernels, bodies, .amdhsa_ blocks and metadata identical"
        foreign_total += len(foreign)
        print(msg)
    print(f"{len(a)} files, {foreign_total} foreign lines, {reordered} compared kernel by kernel, {bad} with different device code")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
