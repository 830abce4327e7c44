"""tools/verify_bench.py: one tiny run of the tool itself -- the JSON line FINDINGS 73 is filled from has to carry the yardstick
walk, the histogram walk at both occupancies, the ratios and the pair totals for every operand."""
import json
import os
import subprocess
import sys
from math import comb

import pytest

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "verify_bench.py")


@pytest.mark.gpu
def test_tool_runs_and_reports(dev):
    r = subprocess.run([sys.executable, TOOL, "--n", "1500", "--d", "64", "--rounds", "1", "--round-s", "0.005"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bench"] == "pair_histogram" and [c["operand"] for c in rec["configs"]] == ["iid", "faces", "one"]
    iid, faces, one = rec["configs"]
    for c in rec["configs"]:
        assert c["N"] == 1500 and c["D"] == 64
        for part in ("walk", "hist1024", "hist512"):
            assert 0 < c[part]["min_ms"] <= c[part]["ms"] <= c[part]["max_ms"] and c[part]["calls_per_round"] >= 1
            assert c[part]["tflops_fp32_equiv"] > 0
        for part in ("hist1024", "hist512"):
            assert c[part + "_over_walk"] == pytest.approx(c[part]["ms"] / c["walk"]["ms"], abs=2e-3)
        assert c["n_genuine"] + c["n_impostor"] == comb(1500, 2)        # every row is live
        assert c["hist512_is_hist1024_folded"] is True
    assert iid["n_genuine"] == 500 and iid["bins_hit_genuine"] >= 1     # labels i mod 1000: rows i and i + 1000
    assert one["n_impostor"] == 0 and one["bins_hit_impostor"] == 0
    assert faces["largest_identity"] == 150 and faces["n_genuine"] > comb(150, 2) * 0.6
