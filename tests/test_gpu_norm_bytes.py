"""The device normalisation front-end against the digests recorded on the parent commit of the change that split its host half into
stages (tests/golden/norm_bytes.json; tests/norm_bytes.py says what a digest holds, which tables it covers and how the file is
written): all six kinds, Int32 and Float64 tables, dense and CSC, byte for byte, with both masks."""
import pytest

from tests import norm_bytes

pytestmark = pytest.mark.gpu

GOLDEN = norm_bytes.load_golden()


@pytest.mark.parametrize("name", sorted(set(norm_bytes.CASES) | set(GOLDEN)))
def test_the_bytes_are_the_parents(name):
    assert name in GOLDEN, "case %s has no golden digest: record it on the parent commit" % name
    assert name in norm_bytes.CASES, "the golden digest %s has no case" % name
    digest, shape = norm_bytes.run_case(name)
    if name.startswith("t80000"):
        assert shape[1] > 65535, shape  # (or the output kernels' loop beyond the limit on grid.y is not visited)
    assert digest == GOLDEN[name]
