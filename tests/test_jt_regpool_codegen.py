"""Register pool of the plan-specialized ALARM kernel, checked without a GPU (device=-1): the
placement the generator reports, the compiled kernel's register metadata, and the sources the pool
must not touch.  The constants are those of the commit before the pool (same compiler, gfx950):

  variable-major fast kernel (bench.py's): 494 registers (256 VGPRs + 238 AGPRs), no VGPR spill,
      27 spilled SGPRs, no private segment; key 42c0ea438b7007fb
  case-major fast kernel: 508 registers (256 + 252), no VGPR spill, 34 spilled SGPRs, no private
      segment; key 75cfe56681168056
  both: 195 rows of per-wave global workspace (Collect 195, Distribute 36 sharing them), 79 LDS rows

(The keys are those sources plus the one line that writes label 0 for a case whose query is
observed, which every kernel has since tests/test_gpu_jt_range.py; before it they were 1ed7462c5bf20a18,
7824a06c22f2f4fb, fcf3f8779048f2a5 and 9e56e7fd8c720034, and each source differs from its
predecessor by that line alone.)

The pool is the variable-major default.  The case-major kernel takes it on request only: with it
every slack tried compiled to 42-44 spilled SGPRs against the 34 above."""
import os
import re
import shutil
import subprocess

import pytest

import fastbn_amd as F
from fastbn_amd import prebuild

PARENT_WORKSPACE_ROWS = 195
PARENT_GLOBAL_ROWS = 195 + 36
PARENT_META = {"vgpr_spill_count": 0, "sgpr_spill_count": 27, "private_segment_fixed_size": 0}
PARENT_KEYS = {  # (layout, exact) -> cache key of the kernel before the pool
    (0, False): "75cfe56681168056", (1, False): "42c0ea438b7007fb",
    (0, True): "81b5a715d3ea0f76", (1, True): "e132e51334d05753",
}


def _key(jt):
    return re.search(r"fbn_jt_([0-9a-f]{16})\.hsaco$", jt.kernel_cache_path()).group(1)


@pytest.fixture()
def jt(monkeypatch):
    monkeypatch.delenv("FBN_JT_REG_POOL", raising=False)
    j = F.JunctionTree(F.Network(prebuild.ALARM_XML), device=-1)
    j.set_exact(None)
    j.set_output_layout(1)
    return j


def _readelf():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (shutil.which("llvm-readelf"), os.path.join(rocm, "llvm", "bin", "llvm-readelf"),
                 os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError("llvm-readelf of the ROCm LLVM not found (PATH, $ROCM_PATH/llvm/bin)")


def _metadata(path):
    notes = subprocess.run([_readelf(), "--notes", path], capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, notes).group(1))
            for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}


def test_placement_summary(jt):
    info = jt.refresh_info()
    reg = info["place_rows_reg_collect"] + info["place_rows_reg_distribute"]
    print({k: v for k, v in info.items() if k.startswith("place_")})
    assert reg > 0
    assert info["place_rows_workspace"] < PARENT_WORKSPACE_ROWS
    assert info["place_rows_global_collect"] + info["place_rows_global_distribute"] < PARENT_GLOBAL_ROWS
    assert info["place_rows_lds_pool"] <= 80
    # every stored message entry has exactly one place
    total = sum(v for k, v in info.items() if k.startswith("place_rows_") and k.split("_")[-1] in ("collect", "distribute"))
    off = _info_with(jt, "0")
    assert total == sum(v for k, v in off.items()
                        if k.startswith("place_rows_") and k.split("_")[-1] in ("collect", "distribute"))


def _info_with(jt, pool):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("FBN_JT_REG_POOL", pool)
        return dict(jt.refresh_info())


def test_default_kernel_metadata(jt):
    """No VGPR spill, no larger private segment and no more spilled SGPRs than before the pool."""
    meta = _metadata(jt.build_kernel())
    print(meta)
    assert meta["vgpr_spill_count"] == 0
    assert meta["private_segment_fixed_size"] <= PARENT_META["private_segment_fixed_size"]
    assert meta["sgpr_spill_count"] <= PARENT_META["sgpr_spill_count"]


def test_pool_off_and_exact_sources_unchanged(jt, monkeypatch):
    """FBN_JT_REG_POOL=0 generates the kernel of before (plan order, no register place), the exact
    order never has a pool (bit-pinned to the reference: its cache key must not move), and the
    case-major kernel has none unless asked."""
    for layout in (0, 1):
        jt.set_output_layout(layout)
        jt.set_exact(True)
        assert _key(jt) == PARENT_KEYS[(layout, True)]
        monkeypatch.setenv("FBN_JT_REG_POOL", "64")
        assert _key(jt) == PARENT_KEYS[(layout, True)]
        jt.set_exact(None)
        assert _key(jt) != PARENT_KEYS[(layout, False)]
        monkeypatch.setenv("FBN_JT_REG_POOL", "0")
        assert _key(jt) == PARENT_KEYS[(layout, False)]
        monkeypatch.delenv("FBN_JT_REG_POOL")
    jt.set_output_layout(0)
    assert _key(jt) == PARENT_KEYS[(0, False)]
    jt.set_output_layout(1)
    assert _key(jt) != PARENT_KEYS[(1, False)]


def test_parked_entries_are_block_local_registers(jt):
    """A parked entry is a named double declared in the block loop's body, assigned before it is
    read, and in no op boundary's operand list."""
    src = jt.kernel_source()
    body = src[src.index("for (long long blk"):]
    names = re.findall(r"\b(r[cd]\d+_\d+)\b", "".join(re.findall(r"^ {8}double (?:r[cd]\d+_\d+(?:, )?)+;$", body, re.M)))
    info = jt.refresh_info()
    assert len(names) == len(set(names)) == info["place_rows_reg_collect"] + info["place_rows_reg_distribute"]
    boundary = re.search(r"#define FBN_OP_BOUNDARY\(\).*", src).group(0)
    for nm in names:
        assert nm not in boundary
        first_write = re.search(r"\b%s = " % nm, body)
        first_read = re.search(r"= %s;" % nm, body)
        assert first_write and first_read and first_write.start() < first_read.start(), nm
