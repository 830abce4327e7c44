"""tools/moteval_bench.py: the synthetic generator's stated shape (CPU), and one tiny run of the tool on the GPU -- its equality
flags and the JSON fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import moteval_bench as MB  # noqa: E402

from face_detection_and_recognition_amd import tracking_eval as TE  # noqa: E402


def test_generator_shape():
    S, F, T = 5, 30, 4
    d = MB.synthetic(S, F, T, seed=3)
    again = MB.synthetic(S, F, T, seed=3)
    assert all(np.array_equal(d[k], again[k]) for k in d)                   # seeded
    assert not np.array_equal(d["hy_boxes"], MB.synthetic(S, F, T, seed=4)["hy_boxes"])
    assert list(d["n_frames"]) == [F] * S
    for side, cap in (("gt", T), ("hy", T + 1)):
        seq, frame, ids, boxes = (d[f"{side}_{k}"] for k in ("seq", "frame", "id", "boxes"))
        assert boxes.shape == (len(seq), 4) and boxes.dtype == np.float64 and np.isfinite(boxes).all() and (boxes[:, 2:] > 0).all()
        assert seq.min() >= 0 and seq.max() < S and frame.min() >= 0 and frame.max() < F and ids.min() > 0
        key = seq * F + frame
        assert (np.diff(key) >= 0).all()                                    # rows in (sequence, frame) order
        assert np.bincount(key).max() <= cap
        assert len(np.unique(np.stack([key, ids]), axis=1).T) == len(key)   # no id twice in a frame
    assert set(d["gt_id"].tolist()) == set(range(1, T + 1))
    assert len(d["hy_seq"]) < len(d["gt_seq"]) + S * F                      # misses, plus at most one spurious box per frame
    res = TE.mot_eval(**d)                                                  # every ingredient shows in the score
    assert res.TP > 0 and res.FN > 0 and res.FP > 0 and res.IDSW > 0 and res.Frag > 0 and 0 < res.IDF1 < 1
    with pytest.raises(ValueError):
        MB.synthetic(1, 2, 64)


@pytest.mark.gpu
def test_tiny_run_of_the_tool(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "moteval_bench.py"), "--seqs", "6", "--frames", "8", "--targets", "3",
                        "--long-frames", "24", "--rounds", "1", "--round-s", "0.002"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["bench"] == "moteval" and out["targets"] == 3 and "numpy restatement" in out["compared_against"]
    for layout, seqs, longest in (("many_short", 6, 8), ("one_long", 1, 24)):
        o = out[layout]
        assert o["sequences"] == seqs and o["frames_longest"] == longest and o["frames"] == seqs * longest
        assert o["integers_equal"] and o["rows_equal"] and o["sum_iou_bit_equal"]
        for name in ("plumbing", "launch"):
            assert o[name]["ms"] > 0 and o[name]["min_ms"] <= o[name]["ms"] <= o[name]["max_ms"]
        for key in ("readback_ms", "host_id_assignment_ms", "numpy_once_s", "launch_us_per_frame_of_longest",
                    "launch_us_per_frame_overall", "numpy_over_device_total", "MOTA", "IDF1"):
            assert key in o, key
        assert o["combined_device"]["TP"] > 0 and o["gt_rows"] > 0 and o["hy_rows"] > 0
