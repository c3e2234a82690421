"""Prebuild plan-specialized JT kernels into the in-tree code-object cache (fastbn_amd/kcache).

The cache key is a hash of the generated source and the compile options, so a kernel built here
is found by any process that plans the same network (jt_jit.hip); a miss compiles with hiprtc at
first run instead.
"""
import os
import tempfile

from . import api, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALARM_XML = os.path.join(REPO, "tests", "golden", "alarm", "alarm.xml")
# eligible synthetic network used by the GPU parity tests (tests/test_gpu_jt.py)
SYNTH_SMALL = dict(n=60, seed=5, window=6)


def synth_small_xml(dirname):
    path = os.path.join(dirname, "synth60.xml")
    synth.random_network(SYNTH_SMALL["n"], seed=SYNTH_SMALL["seed"], window=SYNTH_SMALL["window"], path=path)
    return path


def prebuild(xml_paths, layouts=(0,)):
    out = []
    for xml in xml_paths:
        jt = api.JunctionTree(api.Network(xml), device=-1)
        if jt.info["specialized_eligible"]:
            for layout in layouts:  # output layouts (0 case-major, 1 variable-major: bench.py's ALARM)
                jt.set_output_layout(layout)
                for exact in (None, True):  # both arithmetic orders (default fast, exact on request)
                    jt.set_exact(exact)
                    out.append(jt.build_kernel())
    return out


def fixture_xmls(dirname):
    """The XMLBIF fixtures of the GPU tests (tests/golden/synth_nets/*.xml.gz), unpacked."""
    import glob
    import gzip
    out = []
    for gz in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "synth_nets", "*.xml.gz"))):
        path = os.path.join(dirname, os.path.basename(gz)[:-3])
        with gzip.open(gz, "rb") as f, open(path, "wb") as g:
            g.write(f.read())
        out.append(path)
    return out


def _load_tests_module(name):
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True  # (leave tests/ as it is)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mod


def count_map_nets():
    """The eligible count-map networks of the GPU tests (tests/test_gpu_jt_range.py,
    tests/test_gpu_jt_counts.py), from the tests' own generators (tests/jt_nets.py, plain Python):
    [(namespace with dims / parents / counts, output layouts)]."""
    J = _load_tests_module("jt_nets")
    return [(J.conflict_net(*J.CONFLICT_FORMS["xmlbif"]), (0,)), (J.conflict_net(*J.CONFLICT_FORMS["counts"]), (0, 1)),
            (J.counts_net(J.COUNTS_SEED, "small"), (0,)), (J.counts_net(J.COUNTS_SEED, "dom32"), (0,))]


def prebuild_forests(dirname):
    """The junction forests of the GPU tests (tests/test_gpu_jt_forest.py, networks from
    tests/jt_forest_nets.py): the small disconnected network in both orders and layouts, the random
    disconnected network and the 60-component network in the default order."""
    N = _load_tests_module("jt_forest_nets")
    out = []
    jf = api.JunctionForest(api.Network.from_counts(*N.disconnected()), device=-1)
    for layout in (0, 1):
        jf.set_output_layout(layout)
        for exact in (None, True):
            jf.set_exact(exact)
            out.append(jf.build_kernel())
    star = N.star_net()
    path = os.path.join(dirname, "forest.xml")
    synth.random_network(path=path, **N.RANDOM)
    for net in (api.Network.from_counts(star.dims, star.parents, star.counts), api.Network(path)):
        out.append(api.JunctionForest(net, device=-1).build_kernel())
    return out


def prebuild_count_maps():
    out = []
    for net, layouts in count_map_nets():
        jt = api.JunctionTree(api.Network.from_counts(net.dims, net.parents, net.counts), device=-1)
        assert jt.info["specialized_eligible"]
        for layout in layouts:
            jt.set_output_layout(layout)
            for exact in (None, True):
                jt.set_exact(exact)
                out.append(jt.build_kernel())
    return out


def prebuild_prob_nets():
    """The probability networks whose specialized kernel tests/test_gpu_probnet.py requests (generators in
    tests/prob_nets.py): the skewed 7-node network, the votes network, ALARM's structure with learned
    tables, and the 7-node network split into a forest -- both orders, case-major."""
    P = _load_tests_module("prob_nets")
    out = []
    for cls, net in ((api.JunctionTree, P.small("skewed")), (api.JunctionTree, P.votes("guard")),
                     (api.JunctionTree, P.learned(ALARM_XML)), (api.JunctionForest, P.small_forest("skewed"))):
        jt = cls(api.Network.from_cpts(*net), device=-1)
        assert jt.info["specialized_eligible"]
        for exact in (None, True):
            jt.set_exact(exact)
            out.append(jt.build_kernel())
    return out


# code-generation options the GPU tests run ALARM under (tests/test_gpu_jt_fast.py)
ALARM_TEST_OPTIONS = ({"FBN_JT_LEAF_RC": "1"}, {"FBN_JT_LDS_POOL": "0"}, {"FBN_JT_MARG_V2": "0"},
                      {"FBN_JT_REG_POOL": "0"}, {"FBN_JT_REG_POOL": "256"})


# by output layout: the register pool's kernel with the load pipeline (FBN_JT_SCHED unset) and
# without it (tests/test_gpu_jt_sched.py, tests/test_jt_sched_codegen.py); the pool is the default
# of the variable-major layout (1) and on request in the case-major one (0)
SCHED_TEST_OPTIONS = {0: ({"FBN_JT_REG_POOL": "256"}, {"FBN_JT_REG_POOL": "256", "FBN_JT_SCHED": "0"}),
                      1: ({}, {"FBN_JT_SCHED": "0"})}


def prebuild_options(xml, options, layout=0):
    """The fast-order kernel of `xml` under each set of generator environment options (read when
    the kernel is generated), built in a child process per set."""
    import subprocess
    import sys
    out = []
    for opt in options:
        env = dict(os.environ, **opt)
        code = ("import sys; sys.path.insert(0, %r); from fastbn_amd import api; "
                "jt = api.JunctionTree(api.Network(%r), device=-1); jt.set_output_layout(%d); "
                "print(jt.build_kernel())" % (REPO, xml, layout))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        out.append(r.stdout.strip().splitlines()[-1])
    return out


def prebuild_default(clean=True):
    """Every eligible benchmark / test network, both orders (cache hits are free), and the ALARM
    option variants the tests use; clean: then drop the code objects no current plan uses (older
    generator versions)."""
    with tempfile.TemporaryDirectory() as d:
        built = prebuild([ALARM_XML], layouts=(0, 1)) + prebuild([synth_small_xml(d)] + fixture_xmls(d))
        built += prebuild_forests(d)
        # (tests/test_gpu_jt_sched.py: the register pool's kernel of the synthetic network with and
        # without the load pipeline)
        built += prebuild_options(synth_small_xml(d), SCHED_TEST_OPTIONS[1], layout=1)
    built += prebuild_options(ALARM_XML, ALARM_TEST_OPTIONS)
    for layout in (0, 1):
        built += prebuild_options(ALARM_XML, SCHED_TEST_OPTIONS[layout], layout=layout)
    # (tests/test_gpu_jt_regpool.py compares the register pool on / off in both output layouts)
    built += prebuild_options(ALARM_XML, ({"FBN_JT_REG_POOL": "0"}, {"FBN_JT_REG_POOL": "256"}), layout=1)
    # (the exact-order kernels of the conflict networks and of the 32-state network take 5 .. 20 s each)
    built += prebuild_count_maps()
    built += prebuild_prob_nets()
    if clean:
        keep = {os.path.basename(p) for p in built}
        kdir = os.path.join(REPO, "fastbn_amd", "kcache")
        for f in os.listdir(kdir) if os.path.isdir(kdir) else []:
            if f.endswith(".hsaco") and f not in keep:
                os.remove(os.path.join(kdir, f))
    return built
