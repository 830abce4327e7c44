"""What fp_plan_validate answers does not move (CPU).

tools/validate_digest.py's procedure on a smaller corpus: every distinct fp_op of the networks of test_plan_digests._networks()
at N = 2 with PlanBuilder.X6 on and off, plus the one-op plans of generic_op_cases.  Every op is validated as it is (status 0,
kernel name), with the tightest weight and arena limits it still passes, with every single-field mutation and with 100 seeded
compound mutations, one fp_plan_validate call each.  tests/golden/validate_statuses.json holds, per (op kind, SPLIT3 or fp32),
a SHA-256 over all of those statuses in order, their histogram, and a SHA-256 and the maxima of the tight limits.  It was
recorded before validate_op (csrc/capi.cpp) became a table of op kinds, so a check that moves, changes its status or changes
its place among the others fails here; tools/validate_digest.py --compare names the op and the mutation.

Regenerate (only when a change of the validator's answers is intended): python tests/test_validate_statuses.py --write
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "validate_statuses.json")


def compute_summary():
    from face_detection_and_recognition_amd import _lib as L
    from face_detection_and_recognition_amd.plan import PlanBuilder
    from test_plan_digests import _networks
    from tools import validate_digest as V
    corpus = {}
    saved = PlanBuilder.X6
    try:
        for emit in _networks().values():
            for x6 in (True, False):
                PlanBuilder.X6 = x6
                V.add_plan(corpus, emit(2))
    finally:
        PlanBuilder.X6 = saved
    V.generic_corpus(corpus)
    return V.summary(V.table(L.load(), corpus))


def test_validate_statuses_unchanged():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = compute_summary()
    assert sorted(got) == sorted(want)
    assert all(sum(g["histogram"].values()) == g["calls"] and g["histogram"].get("0", 0) > 0 for g in got.values())
    moved = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not moved, f"fp_plan_validate answers differently: {moved}"


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python tests/test_validate_statuses.py --write")
    with open(FIXTURE, "w") as f:
        json.dump(compute_summary(), f, indent=1, sort_keys=True)
        f.write("\n")
