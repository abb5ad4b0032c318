"""csrc/fw_stage_host.h -- the capacity policy of the level-0 drivers (first capacity from pair count, limit and hint; at most two
attempts, the second with the exact count; the hint; the error of a second overflow) -- compiled natively through
tests/native/stage_check.cpp: no GPU, no build of the library.

No GPU test reaches the second attempt (it takes more than 4 Mi significant pairs), so the loop is driven here by a scripted attempt:
every attempt is handed the next (first-stage count, second-stage count) of the script, and the program reports the return code, the
hint afterwards, the capacities the attempts were given and the message."""
import os
import re
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "stage_check.cpp")
CSRC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "fw_stage_host.h")
MI = 1 << 20
FW_OK, FW_ERR_DEVICE, FW_ERR_NOMEM = 0, -2, -6  # include/flashweave_amd.h
# the messages of the five drivers as they read before the skeleton; each passes the part in front of " overflow twice"
MESSAGES = {
    "fz": "fz level-0: compaction buffer overflow twice",
    "fz64": "Float64 fz level-0: compaction buffer overflow twice",
    "fz_nz": "fz_nz level-0: compaction buffer overflow twice",
    "mi_generic": "discrete level-0 (generic form): result buffer overflow twice",
    "mi": "discrete level-0: candidate buffer overflow twice",
}
LIMITS = (4 * MI, 8 * MI)  # significant pairs (every kind; the generic discrete form per rank) / candidates of the discrete screen


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stage_check") / "stage_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", out, SRC], check=True)
    return out


def _run(exe, tokens):
    r = subprocess.run([exe], input=" ".join(map(str, tokens)), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.split("\n")


def test_header_compiles_without_hip(tmp_path):
    # plain g++, nothing on the include path: the header and everything it includes is host C++, and none of it is a HIP header
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "%s"\nint main() { return 0; }\n' % HEADER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-H", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    included = [ln for ln in r.stderr.splitlines() if ln.startswith(".")]  # -H: one line per header, dots for the depth
    assert included and not [ln for ln in included if "hip" in ln.lower()]


def test_the_drivers_pass_the_messages_checked_here():
    # each driver names its buffer once, and "overflow twice" is spelled in the header alone
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp", ".h"))}
    for msg in MESSAGES.values():
        what = '"%s"' % msg[: -len(" overflow twice")]
        assert sum(t.count(what) for t in text.values()) == 1, what
    assert [f for f, t in text.items() if '"overflow twice"' in t or ' overflow twice"' in t] == ["fw_stage_host.h"]


# ---- 1. first capacity ----
def _cap(exe, pairs, limit, hint):
    return int(_run(exe, ["cap", pairs, limit, hint])[0])


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("pairs", [0, 1, 4 * MI + 1])
def test_first_capacity(exe, pairs, limit):
    base = max(min(pairs, limit), 1)  # never 0, never above the limit
    assert base == {0: 1, 1: 1, 4 * MI + 1: 4 * MI if limit == 4 * MI else 4 * MI + 1}[pairs]
    assert _cap(exe, pairs, limit, 0) == base
    for hint in (base - 1, base, base + 1, 3 * limit):  # below, equal, above: the hint only ever raises it
        assert _cap(exe, pairs, limit, hint) == max(base, hint), hint


def test_first_capacity_of_an_empty_rank_range(exe):
    # generic discrete form, more ranks than pairs: q1 - q0 = 0 pairs against the 4 Mi limit still reserves one entry
    assert _cap(exe, 0, 4 * MI, 0) == 1
    assert _cap(exe, 0, 4 * MI, 17) == 17


# ---- 2. attempts ----
def _attempts(exe, cap, hint, script, what="fz level-0: compaction buffer"):
    tok = ["attempts", cap, hint, what.replace(" ", "~"), len(script)]
    for first, second in script:
        tok += [first, second]
    out = _run(exe, tok)
    rc, hint_after, n = (int(x) for x in out[0].split())
    caps = [int(x) for x in out[1].split()]
    assert n == len(caps)
    assert hint_after >= hint  # the hint never falls
    return rc, hint_after, caps, out[2]


@pytest.mark.parametrize("count", [0, 7, 10])
def test_a_count_that_fits_takes_one_attempt(exe, count):
    assert _attempts(exe, 10, 0, [(count, 0)]) == (FW_OK, count, [10], "")


def test_the_hint_never_falls(exe):
    assert _attempts(exe, 100, 100, [(5, 0)]) == (FW_OK, 100, [100], "")
    assert _attempts(exe, 10, 100, [(50, 0), (50, 0)]) == (FW_OK, 100, [10, 50], "")


def test_one_overflow_retries_with_exactly_that_count(exe):
    assert _attempts(exe, 10, 0, [(11, 0), (11, 0)]) == (FW_OK, 11, [10, 11], "")
    # more than 4 Mi significant pairs, the case no GPU test reaches
    cap = _cap(exe, 4 * MI + 1, 4 * MI, 0)
    assert _attempts(exe, cap, 0, [(4 * MI + 1, 0), (4 * MI + 1, 0)]) == (FW_OK, 4 * MI + 1, [4 * MI, 4 * MI + 1], "")
    # ... and the next call starts from the hint: no overflow
    cap = _cap(exe, 4 * MI + 1, 4 * MI, 4 * MI + 1)
    assert _attempts(exe, cap, 4 * MI + 1, [(4 * MI + 1, 0)]) == (FW_OK, 4 * MI + 1, [4 * MI + 1], "")


@pytest.mark.parametrize("kind", sorted(MESSAGES))
def test_two_overflows_are_an_error_with_the_kinds_message(exe, kind):
    msg = MESSAGES[kind]
    what = msg[: -len(" overflow twice")]
    assert _attempts(exe, 10, 0, [(25, 0), (40, 0)], what) == (FW_ERR_DEVICE, 40, [10, 25], msg)
    assert _attempts(exe, 10, 30, [(25, 0), (26, 0)], what) == (FW_ERR_DEVICE, 30, [10, 25], msg)


def test_two_stages_screen_fits_and_exact_exceeds(exe):
    # fz: the screen's count raises the hint, a larger count of the exact stage asks for the second attempt as well
    assert _attempts(exe, 10, 0, [(8, 12), (8, 12)]) == (FW_OK, 8, [10, 12], "")
    assert _attempts(exe, 10, 0, [(8, 12), (8, 13)]) == (FW_ERR_DEVICE, 8, [10, 12], MESSAGES["fz"])
    # the screen overflows (its second stage did not run), then both fit
    assert _attempts(exe, 10, 0, [(15, 0), (15, 14)]) == (FW_OK, 15, [10, 15], "")


def test_an_error_of_the_attempt_ends_the_loop(exe):
    # (stage_check.cpp turns a first count of 99999 into FW_ERR_NOMEM: a failed reservation) no second attempt, no message, hint as it was
    assert _attempts(exe, 10, 3, [(99999, 0)]) == (FW_ERR_NOMEM, 3, [10], "")
    assert _attempts(exe, 10, 3, [(20, 0), (99999, 0)]) == (FW_ERR_NOMEM, 20, [10, 20], "")


def test_error_codes_are_the_abi_headers():
    h = open(os.path.join(ROOT, "include", "flashweave_amd.h")).read()
    for name, val in (("FW_OK", FW_OK), ("FW_ERR_DEVICE", FW_ERR_DEVICE), ("FW_ERR_NOMEM", FW_ERR_NOMEM)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, h).group(1)) == val
