"""tools/cluster_bench.py: one tiny run of the tool itself -- the JSON line FINDINGS 72 is filled from has to carry the yardstick,
both walk variants, the ratios and the graph's counts for both operands."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "cluster_bench.py")


@pytest.mark.gpu
def test_tool_runs_and_reports(dev):
    r = subprocess.run([sys.executable, TOOL, "--n", "1500", "--d", "64", "--rounds", "1", "--round-s", "0.005"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bench"] == "cluster_dbscan" and [c["operand"] for c in rec["configs"]] == ["iid", "faces"]
    iid, faces = rec["configs"]
    for c in rec["configs"]:
        assert c["N"] == 1500 and c["D"] == 64 and c["tau"] == 0.5
        for part in ("topk_k1_full_square", "walk1", "walk2"):
            assert 0 < c[part]["min_ms"] <= c[part]["ms"] <= c[part]["max_ms"] and c[part]["calls_per_round"] >= 1
            assert c[part]["tflops_fp32_equiv"] > 0
        assert c["walk2"]["per_pass_ms"] == pytest.approx(c["walk2"]["ms"] / 2, abs=1e-3)
        assert c["walk1_over_yardstick"] > 0 and c["per_pass_over_yardstick"] > 0
    # 64 features: the cosine of two i.i.d. rows has sigma 1 / 8, 0.5 is four sigma -- a few edges at most, no big cluster
    assert iid["edges"] < 100 and iid["clusters_min_samples_1"] > 1400
    assert faces["largest_identity"] == 150 and faces["edges"] > 150 * 100 / 2
    assert faces["largest_cluster_min_samples_3"] >= 100 and faces["clusters_min_samples_3"] >= 1
    assert faces["summary"]["ms"] > 0
