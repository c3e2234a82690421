#!/usr/bin/env python3
"""Digests of every source the plan-specialized JT kernel generator emits for the networks the tests
and the benchmark build kernels for (the set fastbn_amd/prebuild.py enumerates, through its own
helpers), in both output layouts and both arithmetic orders, under each environment of ENVS.  No GPU
(device=-1): the generator's output is text.

    python tools/jt_codegen_digest.py            compare with the fixture, list the differing keys
    python tools/jt_codegen_digest.py --write    regenerate the fixture after an intended change

Per entry "<network>|<layout>|<order>|<environment>": the first 16 hex digits of the source's SHA-256,
its length, and the eight place_rows_* values of refresh_info().  The code-object cache key is a hash
of the source and the compile options, so equal digests mean equal code objects; the diff of the
fixture shows which configurations a change of the generator touched.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from fastbn_amd import api, prebuild  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "jt_codegen", "sources.json")
KNOBS = ("REG_POOL", "SCHED", "LEAF_RC", "LDS_POOL", "MARG_V2", "PROFILE")
ENVS = ("", "REG_POOL=0", "REG_POOL=256", "REG_POOL=64", "SCHED=0", "REG_POOL=256,SCHED=0", "LEAF_RC=1",
        "LEAF_RC=1,REG_POOL=256", "LEAF_RC=1,REG_POOL=256,SCHED=0", "LDS_POOL=0", "LDS_POOL=0,REG_POOL=256",
        "LDS_POOL=16", "MARG_V2=0", "MARG_V2=0,REG_POOL=256", "PROFILE=1")
PLACE = ("global_collect", "global_distribute", "lds_collect", "lds_distribute", "reg_collect",
         "reg_distribute", "workspace", "lds_pool")
INELIGIBLE = ("bigdom", "wide")  # fixtures of tests/golden/synth_nets the specialized kernel does not take


def corpus(dirname):
    """[(name, plan)] of the eligible networks; the ineligible fixtures are checked to be so."""
    out = [("alarm", api.JunctionTree(api.Network(prebuild.ALARM_XML), device=-1)),
           ("synth_small", api.JunctionTree(api.Network(prebuild.synth_small_xml(dirname)), device=-1))]
    for xml in prebuild.fixture_xmls(dirname):
        name = os.path.basename(xml)[:-4]
        jt = api.JunctionTree(api.Network(xml), device=-1)
        assert bool(jt.info["specialized_eligible"]) == (name not in INELIGIBLE), name
        if jt.info["specialized_eligible"]:
            out.append((name, jt))
    for i, (net, _) in enumerate(prebuild.count_map_nets()):
        out.append(("count_map%d" % i, api.JunctionTree(api.Network.from_counts(net.dims, net.parents, net.counts), device=-1)))
    N = prebuild._load_tests_module("jt_forest_nets")
    star = N.star_net()
    path = os.path.join(dirname, "forest.xml")
    prebuild.synth.random_network(path=path, **N.RANDOM)
    for name, net in (("disconnected", api.Network.from_counts(*N.disconnected())),
                      ("star_net", api.Network.from_counts(star.dims, star.parents, star.counts)),
                      ("RANDOM", api.Network(path))):
        out.append((name, api.JunctionForest(net, device=-1)))
    for name, jt in out:
        assert jt.info["specialized_eligible"], name
    return out


def set_env(env, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """Every FBN_JT_* knob of KNOBS unset but those `env` ("A=1,B=2") names (read per call)."""
    want = dict(kv.split("=") for kv in env.split(",")) if env else {}
    for k in KNOBS:
        if k in want:
            setenv("FBN_JT_" + k, want[k])
        else:
            delenv("FBN_JT_" + k)


def digests_of(name, jt, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """The entries of one network: 2 layouts x 2 orders x ENVS."""
    out = {}
    for layout in (0, 1):
        jt.set_output_layout(layout)
        for exact in (None, True):
            jt.set_exact(exact)
            for env in ENVS:
                set_env(env, setenv, delenv)
                src = jt.kernel_source().encode()
                info = jt.refresh_info()
                key = "%s|%s|%s|%s" % (name, "vmajor" if layout else "cmajor", "exact" if exact else "fast", env)
                out[key] = [hashlib.sha256(src).hexdigest()[:16], len(src)] + [info["place_rows_" + k] for k in PLACE]
    set_env("", setenv, delenv)
    return out


def digests():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        nets = corpus(d)
    for name, jt in nets:
        out.update(digests_of(name, jt))
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def differing(have, want):
    return sorted(k for k in set(have) | set(want) if have.get(k) != want.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate the fixture")
    args = ap.parse_args()
    have = digests()
    if args.write:
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(have[k])) for k in sorted(have)) + "\n}\n")
        print("%d entries, %d distinct sources -> %s" % (len(have), len({v[0] for v in have.values()}), FIXTURE))
        return 0
    bad = differing(have, load())
    for k in bad:
        print("differs:", k)
    print("%d entries, %d differ" % (len(have), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
