"""tools/coarse_bench.py: one tiny run of the tool itself -- the JSON line FINDINGS 78 is filled from has to carry the exact
search, the coarse pass, the rerank, both two-stage forms, the recalls and the footprints."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "coarse_bench.py")


@pytest.mark.gpu
def test_tool_runs_and_reports(dev):
    r = subprocess.run([sys.executable, TOOL, "--shapes", "40x3000x128", "300x200x128", "--k", "1", "5", "--small-k", "5",
                        "--rounds", "1", "--round-s", "0.005", "--host-limit-mb", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bench"] == "coarse_gallery" and [(s["M"], s["N"], s["D"]) for s in rec["shapes"]] == [(40, 3000, 128), (300, 200, 128)]
    big, small = rec["shapes"]
    assert sorted(big["k"]) == ["1", "5"] and sorted(small["k"]) == ["5"]
    for s in rec["shapes"]:
        b = s["device_bytes"]
        Npad = (s["N"] + 127) // 128 * 128
        assert b["compressed_rows_host_or_none"] <= Npad * (128 + 12) + 4 * s["N"]
        assert b["compressed_rows_device"] == b["compressed_rows_host_or_none"] + s["N"] * 128 * 4
        assert b["face_gallery"] >= s["N"] * 128 * 10
        for k, c in s["k"].items():
            assert c["pool"] == min(64, 4 * int(k))
            for part in ("exact", "quantize_q", "coarse", "rerank", "two_stage_device"):
                assert 0 < c[part]["min_ms"] <= c[part]["ms"] <= c[part]["max_ms"] and c[part]["calls_per_round"] >= 1
            assert c["two_stage_device_over_exact"] > 0 and c["coarse_over_exact"] > 0
            # noise 0.5: the planted neighbour scores 0.89, far above the crowd -- both stages find it
            assert c["planted_found_at_1"] == 1.0 and c["recall_coarse_at_1"] == 1.0 and c["recall_two_stage_at_1"] == 1.0
            assert 0 < c["recall_two_stage_at_k"] <= c["recall_coarse_at_k"] <= 1.0
            assert c["max_score_diff_where_same_row"] < 1e-4
    # 40 x 20 x 128 x 4 B = 0.4 MB of gathered rows fits the limit of 1 MB, 300 x 20 rows do not
    assert big["k"]["5"]["host_equals_device"] is True and big["k"]["5"]["two_stage_host"]["ms"] > 0
    assert isinstance(small["k"]["5"]["two_stage_host"], str)
