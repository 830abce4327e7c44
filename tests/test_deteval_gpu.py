"""fp_det_match / fp_pr_accumulate against the numpy path of evaluation.py on seeded synthetic sets (deteval_cases.py).

Exactness: match flags and the counts of ground truth are integers and must be equal; precision and recall are quotients of
those integers by the same fp64 operations and must be equal bit for bit; the twelve statistics are means of at most 1 010
such values taken by the same host code: 1e-12 leaves room for nothing but a different summation."""
import numpy as np
import pytest
import torch

from deteval_cases import synthetic_set
from face_detection_and_recognition_amd.evaluation import DetectionEvaluator, coco_eval_bbox

pytestmark = pytest.mark.gpu
KEYS = ("gt_boxes", "gt_image", "dt_boxes", "dt_scores", "dt_image", "n_images")


def evaluate(s, device=None):
    return coco_eval_bbox(*(s[k] for k in KEYS), gt_area=s["gt_area"], device=device)


def assert_same(got, want, s_got=None, s_want=None):
    assert got.matched.shape == want.matched.shape
    assert np.array_equal(got.matched, want.matched) and np.array_equal(got.ignored, want.ignored)
    assert np.array_equal(got.npig, want.npig)
    assert np.array_equal(got.dt_rank, want.dt_rank)
    if s_got is None:
        assert np.array_equal(got.dt_order, want.dt_order)
    else:                                    # differently ordered inputs: the same detections, not the same indices
        for k in ("dt_boxes", "dt_scores", "dt_image"):
            assert np.array_equal(s_got[k][got.dt_order], s_want[k][want.dt_order])
    assert got.precision.dtype == np.float64 and got.recall.dtype == np.float64
    assert np.array_equal(got.precision.view(np.int64), want.precision.view(np.int64))
    assert np.array_equal(got.recall.view(np.int64), want.recall.view(np.int64))
    assert np.abs(got.stats - want.stats).max() <= 1e-12


@pytest.fixture(scope="module")
def main_set():
    s = synthetic_set(seed=0)
    # what the set is meant to contain
    n_gt = np.bincount(s["gt_image"], minlength=s["n_images"])
    n_dt = np.bincount(s["dt_image"], minlength=s["n_images"])
    assert n_gt[0] == 0 and n_dt[0] > 0 and n_gt[1] > 0 and n_dt[1] == 0 and n_gt[2] == 0 and n_dt[2] == 0
    assert n_gt[3] == 300 and n_gt[4] == 1100 and n_dt[5] == 130 and 3500 <= len(s["dt_scores"]) <= 4500
    assert len(np.unique(s["dt_scores"])) == 16
    return s, evaluate(s)


def test_device_equals_numpy(dev, main_set):
    s, want = main_set
    got = evaluate(s, dev)
    n_dt = np.bincount(s["dt_image"], minlength=s["n_images"])
    assert n_dt[5] == 130 and want.matched.shape[2] == np.minimum(n_dt, 100).sum() < n_dt.sum()      # cut to 100 per image
    assert 0 < want.matched.mean() < 1 and 0 < want.ignored.mean() < 1 and (want.npig > 0).all()
    assert_same(got, want)


def test_single_image(dev):
    s = synthetic_set(seed=5, n_images=4, big=False)
    keep_g, keep_d = s["gt_image"] == 3, s["dt_image"] == 3
    one = dict(gt_boxes=s["gt_boxes"][keep_g], gt_image=np.zeros(keep_g.sum(), np.int64), gt_area=s["gt_area"][keep_g],
               dt_boxes=s["dt_boxes"][keep_d], dt_scores=s["dt_scores"][keep_d], dt_image=np.zeros(keep_d.sum(), np.int64),
               n_images=1)
    assert len(one["gt_boxes"]) and len(one["dt_boxes"])
    assert_same(evaluate(one, dev), evaluate(one))


def test_area_range_without_ground_truth(dev):
    s = synthetic_set(seed=6, n_images=8, big=False)
    keep = s["gt_area"] > 32.0 ** 2                                    # nothing left for `small`
    for k in ("gt_boxes", "gt_image", "gt_area"):
        s[k] = s[k][keep]
    want = evaluate(s)
    assert want.npig[1] == 0 and (want.precision[:, :, 1, :] == -1).all() and want.stats[3] == -1
    assert_same(evaluate(s, dev), want)


def test_deterministic_and_independent_of_input_order(dev, main_set):
    s, want = main_set
    a, b = evaluate(s, dev), evaluate(s, dev)
    assert_same(a, b)
    # the images' blocks of rows in another order, image ids unchanged
    rng = np.random.default_rng(1)
    order = rng.permutation(s["n_images"])
    gsel = np.concatenate([np.nonzero(s["gt_image"] == i)[0] for i in order])
    dsel = np.concatenate([np.nonzero(s["dt_image"] == i)[0] for i in order])
    p = dict(s)
    for k in ("gt_boxes", "gt_image", "gt_area"):
        p[k] = s[k][gsel]
    for k in ("dt_boxes", "dt_scores", "dt_image"):
        p[k] = s[k][dsel]
    assert not np.array_equal(p["dt_image"], s["dt_image"])
    assert_same(evaluate(p, dev), a, p, s)
    assert_same(a, want)


def test_evaluator_in_three_batches(dev, main_set):
    s, want = main_set
    ev = DetectionEvaluator(s["n_images"], dev).set_ground_truth(s["gt_boxes"], s["gt_image"], s["gt_area"])
    n = len(s["dt_scores"])
    for lo, hi in ((0, 17), (17, n // 2 + 3), (n // 2 + 3, n)):
        ev.add(torch.from_numpy(s["dt_image"][lo:hi]).to(dev), torch.from_numpy(s["dt_boxes"][lo:hi]).to(dev),
               torch.from_numpy(s["dt_scores"][lo:hi]).to(dev))
    assert_same(ev.evaluate(), want)


def test_tie_goes_to_the_later_gt_on_the_device(dev):
    """Both GTs have IoU exactly 0.5 with the first detection; it must take the later one, the only GT the second
    detection could have matched (IoU 1; with the earlier GT it has 1 / 3).  Then the same with the GTs swapped."""
    gts = np.array([[0, 0, 10, 20], [0, 0, 20, 10]], float)
    dts = np.array([[0, 0, 10, 10], [0, 0, 20, 10]], float)
    z2 = np.zeros(2, np.int64)
    r = coco_eval_bbox(gts, z2, dts, np.array([0.9, 0.8]), z2, 1, device=dev)
    assert r.matched[0, 0].tolist() == [1, 0] and r.ignored[0, 0].tolist() == [0, 0]
    r = coco_eval_bbox(gts[::-1].copy(), z2, dts, np.array([0.9, 0.8]), z2, 1, device=dev)
    assert r.matched[0, 0].tolist() == [1, 1] and r.matched[0, 1:].sum() == 9          # the second keeps its IoU-1 match at every t
    assert_same(r, coco_eval_bbox(gts[::-1].copy(), z2, dts, np.array([0.9, 0.8]), z2, 1))
