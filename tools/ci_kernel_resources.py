#!/usr/bin/env python3
"""Per-kernel resources and code digests of the CI kernel files, for comparing two source trees.

Compiles each given .hip file to gfx950 device assembly with the Makefile's flags and writes, per
function (kernels and out-of-line device functions alike), a digest of its instructions with local
labels normalised, and per kernel the metadata's register, scratch and LDS figures with the waves per
SIMD the VGPR count allows (512 registers per lane, granule 8, at most 8 waves).

    python tools/ci_kernel_resources.py --csrc fastbn_amd/csrc --out head.json ci_kernels.hip pc_small.hip ...
    python tools/ci_kernel_resources.py --diff parent.json head.json
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "--offload-arch=gfx950", "-munsafe-fp-atomics", "-x", "hip", "--cuda-device-only", "-S", "-fuse-cuid=none"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)( \[clone.*\])?$", "", name))


def functions(asm):
    """name -> normalised body text, for every .type NAME,@function"""
    names = re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M)
    out = {}
    for n in names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(n), asm, re.M | re.S)
        if not m:
            continue
        body = []
        for line in m.group(1).split("\n"):
            line = re.sub(r"\s*;.*$", "", line).strip()
            if line.startswith(".section") or line.startswith(".amdhsa_kernel"):
                break  # a kernel's descriptor follows its code
            if not line or line.startswith(".p2align") or line.startswith(".loc") or line.startswith(".cfi"):
                continue
            line = re.sub(r"\.L(BB|tmp|post_getpc|JTI)\d+(_\d+)?", r".L\1", line)
            body.append(line)
        out[n] = "\n".join(body)
    return out


def metadata(asm):
    out = {}
    for chunk in re.split(r"^  - \.", asm[asm.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"^\s*\.?name:\s+(\S+)", chunk, re.M)
        if not name:
            continue
        rec = {}
        for key in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, chunk)
            rec[key] = int(m.group(1)) if m else None
        alloc = -(-max(rec["vgpr_count"], 1) // 8) * 8
        rec["waves_per_simd"] = min(8, 512 // alloc)
        out[name.group(1)] = rec
    return out


def collect(csrc, files):
    res = {}
    with tempfile.TemporaryDirectory() as td:
        def compile_one(f):
            s = os.path.join(td, f + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I" + os.path.join(csrc, "..", "..", "include"),
                            os.path.join(csrc, f), "-o", s], check=True)
            return open(s).read()
        with ThreadPoolExecutor(8) as ex:
            asms = list(ex.map(compile_one, files))
        for f, asm in zip(files, asms):
            fn, md = functions(asm), metadata(asm)
            dm = demangle(list(fn))
            for n, body in fn.items():
                rec = {"file": f, "lines": body.count("\n") + 1, "digest": hashlib.sha256(body.encode()).hexdigest()[:16],
                       "kernel": n in md}
                rec.update(md.get(n, {}))
                # device functions every code object has its own copy of are told apart by file
                res[short(dm[n]) + ("" if rec["kernel"] else " @" + f)] = rec
    return res


def diff(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    keys = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "waves_per_simd")
    bad = 0
    print("| function | code | vgpr | sgpr | scratch | lds | waves/SIMD |")
    print("|---|---|---|---|---|---|---|")
    for n in sorted(set(A) | set(B)):
        x, y = A.get(n), B.get(n)
        if x is None or y is None:
            print("| `%s` | only in %s (%d lines) | | | | | |" % (n, "parent" if y is None else "head", (x or y)["lines"]))
            continue
        same = x["digest"] == y["digest"]
        cells = []
        for k in keys:
            cells.append("" if x.get(k) is None else (str(x[k]) if x[k] == y[k] else "%s -> %s" % (x[k], y[k])))
        if x["kernel"]:
            if (x["private_segment_fixed_size"] == 0 and y["private_segment_fixed_size"] != 0) or \
               x["group_segment_fixed_size"] != y["group_segment_fixed_size"] or x["waves_per_simd"] != y["waves_per_simd"]:
                bad += 1
        print("| `%s` | %s | %s |" % (n, "identical" if same else "%d -> %d lines" % (x["lines"], y["lines"]),
                                      " | ".join(cells)))
    print("\nkernels failing the scratch / LDS / waves conditions: %d" % bad)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fastbn_amd", "csrc"))
    ap.add_argument("--out")
    ap.add_argument("--diff", nargs=2, metavar=("PARENT", "HEAD"))
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    if args.diff:
        sys.exit(1 if diff(*args.diff) else 0)
    res = collect(args.csrc, args.files)
    json.dump(res, open(args.out, "w") if args.out else sys.stdout, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
