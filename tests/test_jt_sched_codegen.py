"""Load pipeline and level-wise products of the plan-specialized ALARM kernel (jt_gen_emit.cpp IvLoads,
Levels, FBN_JT_SCHED), checked without a GPU on the machine code of the default variable-major fast
kernel (tools/jt_isa_stats.py: device=-1 build, llvm-objdump).  Figures of the commit before (= the
FBN_JT_SCHED=0 build here, the same source byte for byte) and of this one, hiprtc / LLVM 22.0.0git
of ROCm 7, gfx950:

                                                   before    now
  instructions                                     15,038    14,992
  fp64 arithmetic (mul 5,255 add 2,514 fma 816 rcp 302)  8,887  8,887
  potential loads (s_load_dwordx16)                   226       251
  ... waited on within 8 fp64 instructions of issue   162         9
  s_waitcnt lgkmcnt(0)                                 210       188
  adjacent fp64 pairs / second reads the first  7,001 / 1,603   6,943 / 1,112
  VGPR / SGPR spills, private segment            0 / 27, 0     0 / 17, 0

(The load pipeline alone leaves 2,087 dependent neighbours; the products and Collect sums written
level by level in pairs bring them to 1,112 at no cost in time)
"""
import importlib.util
import os
import re

import pytest

import fastbn_amd as F
from fastbn_amd import prebuild

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_FP64 = 8887  # commit before the pipeline, measured with this tool; LLVM 22.0.0git (ROCm 7 hiprtc)
FUSED_OPS = 27 + 26  # Collect + Distribute fused products: one first batch each


def _tool():
    spec = importlib.util.spec_from_file_location("jt_isa_stats", os.path.join(REPO, "tools", "jt_isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def stats():
    """(default build, FBN_JT_SCHED=0 build) of the variable-major fast kernel."""
    tool = _tool()
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FBN_JT_REG_POOL", raising=False)
        mp.delenv("FBN_JT_SCHED", raising=False)
        new = tool.stats(tool.build(layout=1))
        old = tool.stats(tool.build(layout=1, env={"FBN_JT_SCHED": "0"}))
    print("LLVM", tool.compiler_version())
    print("default        ", new)
    print("FBN_JT_SCHED=0 ", old)
    return new, old


def test_fp64_instructions_unchanged(stats):
    new, old = stats
    assert new["fp64"] == old["fp64"] == PARENT_FP64
    for cls in ("mul", "add", "fma", "rcp"):
        assert new["fp64_" + cls] == old["fp64_" + cls]


def test_potential_loads_are_in_flight(stats):
    new, old = stats
    print(new["potential_loads_near_wait"], "of", new["potential_loads"], "against", old["potential_loads_near_wait"])
    assert new["potential_loads_near_wait"] <= FUSED_OPS
    assert new["vgpr_spill_count"] == 0 and new["private_segment_fixed_size"] == 0
    assert new["sgpr_spill_count"] <= old["sgpr_spill_count"]


def test_dependent_pairs_fewer(stats):
    new, old = stats
    print(new["fp64_adjacent_dependent_pairs"], "against", old["fp64_adjacent_dependent_pairs"])
    assert new["fp64_adjacent_dependent_pairs"] < old["fp64_adjacent_dependent_pairs"]


def _key(jt):
    return re.search(r"fbn_jt_([0-9a-f]{16})\.hsaco$", jt.kernel_cache_path()).group(1)


def test_sched_is_read_with_the_pool_only(monkeypatch):
    """With the pool off -- FBN_JT_REG_POOL=0, the case-major default, the exact order -- the knob
    changes no source; with the pool on it does, and unset is 1."""
    monkeypatch.delenv("FBN_JT_REG_POOL", raising=False)
    monkeypatch.delenv("FBN_JT_SCHED", raising=False)
    jt = F.JunctionTree(F.Network(prebuild.ALARM_XML), device=-1)

    def keys(**env):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            out = {}
            for layout in (0, 1):
                jt.set_output_layout(layout)
                for exact in (None, True):
                    jt.set_exact(exact)
                    out[(layout, bool(exact))] = _key(jt)
            return out

    for pool in ({"FBN_JT_REG_POOL": "0"}, {}):
        base = keys(**pool)
        for v in ("0", "1"):
            got = keys(FBN_JT_SCHED=v, **pool)
            for k in base:
                pool_on = not pool and k == (1, False)
                if not pool_on:
                    assert got[k] == base[k], (pool, v, k)
    on = keys()
    assert keys(FBN_JT_SCHED="1")[(1, False)] == on[(1, False)]
    assert keys(FBN_JT_SCHED="0")[(1, False)] != on[(1, False)]
    both = keys(FBN_JT_REG_POOL="256")
    assert keys(FBN_JT_REG_POOL="256", FBN_JT_SCHED="0")[(0, False)] != both[(0, False)]
