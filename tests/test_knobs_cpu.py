"""The FW_* tuning / test knobs have ONE table (csrc/fw_knobs.h).  Plain text scans: no GPU, no build.

* nothing under csrc/ reads the environment, or names a knob by string, outside fw_knobs.h;
* every knob is listed once there and documented in DESIGN.md;
* every FW_* key that the tests, bench.py and profiles/tools put into an environment is a knob the library reads.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")
NAME = r"FW_[A-Z0-9_]+"

# FW_* names that are environment variables of the tests / the Python package, not library knobs ...
NOT_KNOBS = {"FW_KNOBS", "FW_LIB_PATH", "FW_SKIP_LONG_ORACLE", "FW_CFG3_ORACLE_TARGETS", "FW_CFG4_ORACLE_TARGETS"}
# ... and the ABI's enum / error constants, which the same files name in quotes
ABI_CONSTANTS = re.compile(r"FW_(FZ|FZ_NZ|MI|MI_NZ|OK|ERR_[A-Z]+|MAX_K)$")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _table():
    return re.findall(r"^\s*X\((%s)," % NAME, _read(os.path.join(CSRC, "fw_knobs.h")), re.M)


def _other_sources():
    srcs = [p for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if p.endswith((".hip", ".cpp", ".h")) and os.path.basename(p) != "fw_knobs.h"]
    assert len(srcs) >= 14
    return srcs


def test_table_lists_every_knob_once():
    names = _table()
    assert len(names) >= 73
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)


def test_environment_is_read_in_one_place():
    assert "getenv(" in _read(os.path.join(CSRC, "fw_knobs.h"))
    for p in _other_sources():
        assert "getenv(" not in _read(p), p


def test_no_knob_named_by_string_outside_the_table():
    for p in _other_sources():
        hits = re.findall(r'\bfw_\w+\(\s*"%s"' % NAME, _read(p))
        assert not hits, (p, hits)


def test_readers_take_table_identifiers():
    # every knob::NAME under csrc/ is in the table (the compiler checks this too: the scan keeps the check where no compiler runs) ...
    names = set(_table())
    used = set()
    for p in _other_sources():
        used |= set(re.findall(r"\bknob::(%s)" % NAME, _read(p)))
    assert used <= names, sorted(used - names)
    # ... and every knob of the table is read somewhere (directly or through a named reader of fw_knobs.h)
    used |= set(re.findall(r"\bknob::(%s)" % NAME, _read(os.path.join(CSRC, "fw_knobs.h"))))
    assert names <= used, sorted(names - used)


def test_every_knob_is_documented():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    documented = set(re.findall(r"`(%s)`" % NAME, design))
    missing = [n for n in _table() if n not in documented]
    assert not missing, missing


def test_knobs_set_by_tests_and_tools_exist():
    names = set(_table())
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, "bench.py")] + \
        sorted(glob.glob(os.path.join(ROOT, "profiles", "tools", "*.py")))
    assert len(files) > 10
    unknown = {}
    for p in files:
        if os.path.abspath(p) == os.path.abspath(__file__):
            continue
        src = _read(p)
        # "FW_X" / 'FW_X' (subscripts, setenv, dict keys, tuples of keys) and FW_X=... (keyword arguments, shell-style assignments)
        keys = set(re.findall(r"[\"'](%s)[\"']" % NAME, src)) | set(re.findall(r"\b(%s)=(?!=)" % NAME, src))
        bad = sorted(k for k in keys if k not in names and k not in NOT_KNOBS and not ABI_CONSTANTS.match(k))
        if bad:
            unknown[os.path.relpath(p, ROOT)] = bad
    assert not unknown, unknown
