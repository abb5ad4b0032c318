"""learn_network / normalize_data against the call traces recorded on the parent commit of the last change to api.py
(tests/golden/api_trace.json; tests/api_trace.py says what a trace holds and how the file is written): the whole hand-off to the
engine and the front-end, every result, every refusal with its full message, which of two refusals fires first, and the frame a
warning is attributed to.  No device: the engine and the device front-end are the recording stand-ins of the helper."""
import pytest

from tests import api_trace

GOLDEN = api_trace.load_golden()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return api_trace._files(str(tmp_path_factory.mktemp("api_trace")))


@pytest.mark.parametrize("name", sorted(set(api_trace.CASES) | set(GOLDEN)))
def test_the_trace_is_the_parents(name, files):
    assert name in GOLDEN, "case %s has no golden trace: record it on the parent commit" % name
    assert name in api_trace.CASES, "the golden trace %s has no case" % name
    got = api_trace.run_case(name, files)
    assert list(got) == list(GOLDEN[name]), (list(got), list(GOLDEN[name]))
    for part in got:  # raised / result, warnings, calls
        d = api_trace.difference(got[part], GOLDEN[name][part], part)
        assert d is None, d
