"""Every source the plan-specialized JT kernel generator emits for the networks the tests and the
benchmark build kernels for, pinned by digest (tools/jt_codegen_digest.py; the fixture
tests/golden/jt_codegen/sources.json was written by the generator before its split into schedule,
placement and emission).  Host only: the generator's output is text, and the code-object cache key
is a hash of it, so equal sources are equal kernels.  After an intended change of the generator:
python tools/jt_codegen_digest.py --write, and the fixture's diff names the configurations touched."""
import importlib.util
import os
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETWORKS = ("alarm", "synth_small", "tie", "count_map0", "count_map1", "count_map2", "count_map3",
            "disconnected", "star_net", "RANDOM")
_seen = {}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("jt_codegen_digest", os.path.join(REPO, "tools", "jt_codegen_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def corpus(tool):
    with tempfile.TemporaryDirectory() as d:
        nets = tool.corpus(d)  # (asserts that bigdom and wide are not eligible, and that tie is)
    assert tuple(name for name, _ in nets) == NETWORKS
    return dict(nets)


@pytest.mark.parametrize("name", NETWORKS)
def test_sources_pinned(tool, corpus, name, monkeypatch):
    have = tool.digests_of(name, corpus[name], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert len(have) == 2 * 2 * len(tool.ENVS) == 60
    _seen.update(have)
    want = {k: v for k, v in tool.load().items() if k.split("|")[0] == name}
    bad = tool.differing(have, want)
    assert not bad, "generated source or placement differs from the fixture: %s" % ", ".join(bad)


def test_corpus_complete_and_knobs_matter(tool, corpus, monkeypatch):
    """All 600 fixture entries are generated (those of the networks' tests above; run alone, it
    generates them itself), and the knobs reach the generator (at least 250 distinct sources)."""
    for name in NETWORKS:
        if not any(k.split("|")[0] == name for k in _seen):
            _seen.update(tool.digests_of(name, corpus[name], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False)))
    want = tool.load()
    assert len(want) == 600 and set(_seen) == set(want)
    assert len({v[0] for v in _seen.values()}) >= 250
