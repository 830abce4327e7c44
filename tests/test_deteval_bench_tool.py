"""tools/deteval_bench.py: the synthetic set it builds (CPU) and one tiny run of the tool itself (GPU) -- the JSON line that
FINDINGS 69 is filled from has to carry the four timed parts, the single numpy time and the two equality checks."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "deteval_bench.py")


def test_wider_like_set_has_the_stated_shape():
    spec = importlib.util.spec_from_file_location("deteval_bench", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gt, gi, dt, sc, di = mod.wider_like(3226, 100)
    n_gt = np.bincount(gi, minlength=3226)
    assert n_gt.min() >= 1 and n_gt.max() == 1500 and np.median(n_gt) == 2 and (n_gt > 100).sum() > 10      # heavy tail
    assert gt.shape == (len(gi), 4) and dt.shape == (3226 * 100, 4) and sc.shape == di.shape == (3226 * 100,)
    assert (np.bincount(di, minlength=3226) == 100).all() and (np.diff(gi) >= 0).all()
    assert np.isfinite(gt).all() and np.isfinite(dt).all() and (gt[:, 2:] > 0).all() and (dt[:, 2:] > 0).all()
    gt2 = mod.wider_like(3226, 100)[0]
    assert np.array_equal(gt, gt2)                                                                          # seeded


@pytest.mark.gpu
def test_tool_runs_and_reports(dev):
    """60 images (one of them with 1 500 GTs), one short round: the tool's own comparison with the numpy path must hold."""
    r = subprocess.run([sys.executable, TOOL, "--images", "60", "--dets", "100", "--rounds", "1", "--round-s", "0.005"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bench"] == "deteval" and rec["images"] == 60 and rec["detections"] == 6000 and rec["curves"] == 120
    assert rec["max_gts_per_image"] == 1500
    for part in ("plumbing", "match", "accumulate", "total"):
        assert 0 < rec[part]["min_ms"] <= rec[part]["ms"] <= rec[part]["max_ms"] and rec[part]["calls_per_round"] >= 1
    assert rec["numpy_once_s"] >= 0 and rec["flags_equal"] is True and rec["precision_bit_equal"] is True
    assert len(rec["stats_device"]) == 12 and "not pycocotools" in rec["compared_against"]
