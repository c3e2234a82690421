"""Static counts of a plan-specialized JT kernel's machine code (no GPU: the kernel is generated and
compiled with device=-1, then disassembled with the ROCm LLVM's llvm-objdump).

    python tools/jt_isa_stats.py [--xml NET] [--layout 0|1] [--exact] [KNOB=VALUE ...]

prints, for the whole kernel (one block iteration plus the few instructions around the loop):
  * instructions, and fp64 arithmetic per opcode class (v_mul / v_add / v_fma+v_fmac / v_rcp _f64);
  * the loads of initial potentials (s_load_dwordx16: a batch of 16 potentials is two of them) by
    the number of fp64 instructions between a load and the next `s_waitcnt` that waits for
    lgkmcnt(0) -- scalar loads return out of order, so that wait is the first that covers the load;
    a load with fewer than 8 in between was waited on as good as at once;
  * adjacent fp64 instruction pairs, and those where the second reads the first's result;
  * v_accvgpr moves, lgkmcnt(0) waits, vmcnt(0) waits in front of the first fp64 instruction (the
    evidence prologue);
  * the code object's register metadata (spills, private segment).
"""
import os
import re
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64 = {"v_mul_f64": "mul", "v_add_f64": "add", "v_fma_f64": "fma", "v_fmac_f64": "fma", "v_rcp_f64": "rcp"}
NEAR = 8  # fp64 instructions between a load and its wait below which the load was not in flight


def _llvm(tool):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (shutil.which(tool), os.path.join(rocm, "llvm", "bin", tool), os.path.join(rocm, "lib", "llvm", "bin", tool)):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("%s of the ROCm LLVM not found (PATH, $ROCM_PATH/llvm/bin)" % tool)


def compiler_version():
    out = subprocess.run([_llvm("llvm-objdump"), "--version"], capture_output=True, text=True, check=True).stdout
    return re.search(r"LLVM version (\S+)", out).group(1)


def disassemble(path):
    """[(mnemonic, operand text)] of the code object's one kernel."""
    text = subprocess.run([_llvm("llvm-objdump"), "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    ins = []
    for line in text.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(?://.*)?$", line)
        if m and not line.lstrip().startswith("//"):
            ins.append((m.group(1).replace("_e32", "").replace("_e64", ""), m.group(2)))
    return ins


def _regs(operand):
    """The registers an operand names: a set of ('v' | 'a' | 's', index)."""
    out = set()
    for kind, lo, hi, one in re.findall(r"\b([vas])(?:\[(\d+):(\d+)\]|(\d+))", operand):
        for k in range(int(lo or one), int(hi or one) + 1):
            out.add((kind, k))
    return out


def metadata(path):
    notes = subprocess.run([_llvm("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, notes).group(1))
            for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}


def stats(path):
    ins = disassemble(path)
    is64 = [m in FP64 for m, _ in ins]
    s = {"instructions": len(ins), "fp64": sum(is64), "accvgpr_moves": sum(m.startswith("v_accvgpr") for m, _ in ins)}
    for cls in ("mul", "add", "fma", "rcp"):
        s["fp64_" + cls] = sum(FP64.get(m) == cls for m, _ in ins)
    waits = [i for i, (m, a) in enumerate(ins) if m == "s_waitcnt" and "lgkmcnt(0)" in a]
    s["lgkmcnt0_waits"] = len(waits)
    first64 = is64.index(True) if any(is64) else len(ins)
    s["prologue_vmcnt0_waits"] = sum(m == "s_waitcnt" and "vmcnt(0)" in a for m, a in ins[:first64])
    cum = [0]
    for f in is64:
        cum.append(cum[-1] + f)
    loads = [i for i, (m, _) in enumerate(ins) if m == "s_load_dwordx16"]
    s["potential_loads"] = len(loads)
    near, w = 0, 0
    for i in loads:
        while w < len(waits) and waits[w] < i:
            w += 1
        if w < len(waits) and cum[waits[w]] - cum[i] < NEAR:
            near += 1
    s["potential_loads_near_wait"] = near
    pairs = dep = 0
    for i in range(1, len(ins)):
        if is64[i - 1] and is64[i]:
            pairs += 1
            dst = _regs(ins[i - 1][1].split(",")[0])
            # (v_fmac reads its own destination too: every operand of the second counts as read)
            rd = ins[i][1] if ins[i][0] == "v_fmac_f64" else ins[i][1].split(",", 1)[1]
            dep += bool(dst & _regs(rd))
    s["fp64_adjacent_pairs"], s["fp64_adjacent_dependent_pairs"] = pairs, dep
    s.update(metadata(path))
    return s


def build(xml=None, layout=1, exact=False, env=None):
    """Path of the code object of `xml`'s kernel (default: ALARM) generated under `env`."""
    sys.path.insert(0, REPO)
    import fastbn_amd as F
    from fastbn_amd import prebuild
    keep = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        jt = F.JunctionTree(F.Network(xml or prebuild.ALARM_XML), device=-1)
        jt.set_exact(True if exact else None)
        jt.set_output_layout(layout)
        return jt.build_kernel()
    finally:
        for k, v in keep.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--xml", default=None)
    ap.add_argument("--layout", type=int, default=1)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("knobs", nargs="*", metavar="KNOB=VALUE")
    a = ap.parse_args(argv)
    path = build(a.xml, a.layout, a.exact, dict(k.split("=", 1) for k in a.knobs))
    print("%s  (LLVM %s)" % (os.path.basename(path), compiler_version()))
    for k, v in stats(path).items():
        print("%-34s %d" % (k, v))


if __name__ == "__main__":
    main(sys.argv[1:])
