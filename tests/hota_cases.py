"""Shared inputs of the HOTA tests (test_hota_cpu.py: numpy against the host emulator, scipy and hand cases; test_hota_gpu.py:
the device against numpy; test_hota_drivers.py).  The generators are those of moteval_cases.py; a data set is a dict of the
positional arguments of tracking_eval.hota_eval.  Hand cases use B = [0, 0, 100, 100] and the default alphas; their expected
values are the ones DESIGN section 7 "Tracker evaluation: HOTA" lists.
"""
import numpy as np

from moteval_cases import B, KEYS, combine, emulator_inputs, hand_cases, make, many_sequences, seeded_set, shifted  # noqa: F401

INT_KEYS = ("TP", "FN", "FP", "levels", "n_gt", "n_hy")
BIT_KEYS = ("loc_sum", "ass_num", "re_num", "pr_num")


def case_L():
    """Localisation: one frame, the hypothesis at IoU 70 / 130 = 0.538."""
    return make([(0, 0, 1, B)], [(0, 0, 1, shifted(30))], [1])


def case_G():
    """Alignment beats IoU: hypothesis 5 at IoU 0.538 in all four frames, hypothesis 6 at IoU 0.961 in frame 3 only (listed
    before hypothesis 5 there, so hypothesis 5's rows are 0, 1, 2 and 4)."""
    hy = [(0, f, 5, shifted(30)) for f in range(3)] + [(0, 3, 6, shifted(2)), (0, 3, 5, shifted(30))]
    return make([(0, f, 1, B) for f in range(4)], hy, [4])


def wide_set(seed, n_frames=24, n_targets=5):
    """seeded_set with the hypothesis boxes jittered further (sigma 25 % of the size on top of seeded_set's 9 % / 6 %), so that
    the matched pairs spread over the localisation levels."""
    data = seeded_set(seed, n_frames=n_frames, n_targets=n_targets)
    rng = np.random.default_rng(seed + 1000)
    boxes = data["hy_boxes"].copy()
    boxes[:, :2] += rng.normal(0.0, 0.25, boxes[:, :2].shape) * boxes[:, 2:]
    return {**data, "hy_boxes": boxes}


def named_inputs():
    """name -> data: what the emulator and the device are compared on against numpy."""
    cases = emulator_inputs()
    cases["wide10"] = wide_set(10)
    cases["handG"], cases["handL"] = case_G(), case_L()
    cases["32seqs"] = many_sequences()
    cases["merged"] = combine([cases["seed1"], cases["64x64"], cases["seed4"]], merge_seed=3)
    return cases


def assert_same_result(a, b, what=""):
    """Two HotaResults: equal integers per sequence and combined (TP / FN / FP per alpha, levels, counts), gt_match, gtc, hyc,
    and gt_sim, gas and the numerators bit for bit."""
    assert len(a.sequences) == len(b.sequences), what
    assert a.alphas.tobytes() == b.alphas.tobytes(), what
    for s, (x, y) in enumerate(zip(a.sequences + [a.combined], b.sequences + [b.combined])):
        for key in INT_KEYS:
            assert np.array_equal(x[key], y[key]), (what, s, key, x[key], y[key])
        for key in BIT_KEYS:
            assert x[key].dtype == np.float64 and x[key].tobytes() == y[key].tobytes(), (what, s, key, x[key], y[key])
    assert np.array_equal(a.gt_match, b.gt_match), (what, "gt_match", np.nonzero(a.gt_match != b.gt_match)[0][:8])
    assert np.array_equal(a.levels, b.levels), (what, "levels")
    assert a.gt_sim.dtype == np.float64 and a.gt_sim.tobytes() == b.gt_sim.tobytes(), (what, "gt_sim")
    for name in ("gtc", "hyc"):
        for s, (p, q) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert np.array_equal(p, q), (what, name, s)
    for s, (p, q) in enumerate(zip(a.gas, b.gas)):
        assert p.shape == q.shape and p.tobytes() == q.tobytes(), (what, "gas", s)
