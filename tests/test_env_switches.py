"""CPU tests that read the sources: the library asks the environment in one place, INTEGRATION.md's table lists
exactly the switches that place reads, and the retired A/B macros and switches stay retired."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gs-livm_amd")
CSRC = os.path.join(PKG, "csrc")

RETIRED = ("GSR_FWD_ASM_VISIT", "GSR_FWD_EXEC_MASK", "GSR_FWD_SCALAR", "GSR_BWD_EXEC_MASK", "GSR_BWD_STRIP_BRANCH",
           "GSR_BWD_MIN_WAVES", "GSR_ASYNC_FAR_MT", "GSR_PRE_WG_PER_CU", "GSR_PRE_BLOCK_ROWS")


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _sources(top):
    for d, _, names in os.walk(top):
        for n in names:
            if n.endswith((".hip", ".hpp", ".h", ".cpp", ".py")):
                yield os.path.join(d, n)


def test_one_file_reads_the_environment():
    readers = sorted(os.path.relpath(p, CSRC) for p in _sources(CSRC) if "getenv(" in _read(p))
    assert readers == ["api.hip"], readers


def test_integration_table_lists_the_switches_that_are_read():
    src = _read(os.path.join(CSRC, "api.hip"))
    read = re.findall(r'getenv\("(GSR_[A-Z0-9_]+)"\)', src)
    assert len(read) == src.count("getenv("), "a getenv whose name this test cannot see"
    assert len(read) == len(set(read)), "a switch is read twice: %s" % sorted(read)
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    table = re.findall(r"^\s*\| `(GSR_[A-Z0-9_]+)` \|", doc, re.M)
    assert len(table) == len(set(table)), sorted(table)
    assert set(table) == set(read), sorted(set(table) ^ set(read))
    # every member of struct Env names its switch, and nothing else does
    env = re.search(r"struct Env \{(.*?)\n\};", _read(os.path.join(CSRC, "gsr_internal.hpp")), re.S).group(1)
    assert sorted(re.findall(r"// (GSR_[A-Z0-9_]+)", env)) == sorted(read)


def test_retired_names_are_gone():
    left = [(os.path.relpath(p, ROOT), n) for p in _sources(PKG) for n in RETIRED if n in _read(p)]
    assert not left, left
