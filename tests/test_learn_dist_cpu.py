"""learn_network(distributed=True) without a GPU: the refusals that come before any device call, and the declarations of the
rejection-log gather (fw_rejections_allgather_dev / _comm)."""
import json
import os
import re
import tempfile

import numpy as np
import pytest

from tests.learn_dist_worker import launch
from tests.util import ROOT


def test_distributed_needs_a_process_group():
    """No torch.distributed group in this process: ValueError naming `distributed`, before any device call (this host has no GPU:
    a device call would raise FlashWeaveError instead).  This is the test that fails without the feature: before it, the keyword
    ended in TypeError: learn_network: unsupported options ['distributed']."""
    import flashweave_jl_amd as fw
    with pytest.raises(ValueError, match="distributed"):
        fw.learn_network(np.ones((8, 4), np.int32), distributed=True)


def test_prec64_refused_in_a_distributed_run():
    """prec=64 with the plain fz test inside a world-2 gloo group of CPU processes: both ranks raise the ValueError that names both
    options, and no engine was created."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res")
        assert launch("cpu", 2, out, limit_s=90.0) == [0, 0]
        for r in range(2):
            got = json.load(open("%s.%d" % (out, r)))
            assert got["engines"] == 0 and got["message"] is not None
            assert "prec=64" in got["message"] and "distributed" in got["message"]


def test_gather_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "flashweave_amd.h")).read()
    assert re.search(r"int fw_rejections_allgather_dev\(fw_ctx \*ctx, const fw_dev_exchange \*exchange\);", header)
    assert re.search(r"int fw_rejections_allgather_comm\(fw_ctx \*ctx\);", header)
    assert re.search(r"#define FW_ABI_VERSION 6\b", header)
    engine = open(os.path.join(ROOT, "flashweave.jl_amd", "engine.py")).read()
    assert 'hasattr(L, "fw_rejections_allgather_dev")' in engine
    assert "L.fw_rejections_allgather_dev.argtypes" in engine and "L.fw_rejections_allgather_comm.argtypes" in engine
