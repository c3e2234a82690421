"""The environment variables of libfastbn are one table (fastbn_amd/csrc/knobs.h): the library reads
its environment nowhere else, and every variable a test, the benchmark or the Python package names
is a row of it -- so a test that sets a variable the library no longer reads fails here instead of
passing vacuously.  Reads text only."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "fastbn_amd", "csrc")
PREFIXES = ("FBN_JT_", "FBN_CI_", "FBN_PC_", "FBN_PLAN_", "FBN_KERNEL_")


def _table():
    text = open(os.path.join(CSRC, "knobs.h")).read()
    body = text[text.index("kKnobs[] = {"):]
    return re.findall(r'^\s*\{"([A-Z0-9_]+)",', body[:body.index("};")], re.M)


def test_environment_is_read_in_the_knob_file_only():
    """(the CLI under csrc/cli keeps its own single read)"""
    readers = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(CSRC, "*")))
               if os.path.isfile(f) and "getenv(" in open(f, errors="replace").read()]
    assert readers == ["knobs.h"]


def test_every_named_variable_is_a_knob():
    names = _table()
    assert names and len(names) == len(set(names)), "a knob is listed once"
    files = (glob.glob(os.path.join(REPO, "tests", "*.py")) + [os.path.join(REPO, "bench.py")] +
             glob.glob(os.path.join(REPO, "fastbn_amd", "*.py")))
    token = re.compile(r"\b(?:%s)\w+" % "|".join(PREFIXES))
    seen = {}
    for f in files:
        for t in token.findall(open(f).read()):
            seen.setdefault(t, os.path.relpath(f, REPO))
    assert len(seen) > 20, "the scan found the tests' variables"
    unknown = {t: f for t, f in seen.items() if t not in names}
    assert not unknown, "not in fastbn_amd/csrc/knobs.h: %s" % unknown
