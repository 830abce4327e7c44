"""The plans of the existing networks do not move (CPU).

tests/golden/plan_digests.json holds, for BlazeFace front / back (fp32 canvas and u8 frames), YOLOv5n / s / n-0.5 (fp32 canvas
and u8 frames) Mobile-FaceNet and FaceNet (128-d and 512-d heads) at three batch sizes with the split-MFMA kernels on and off, a SHA-256
over every field of every fp_op the network emits plus the kernel family fp_op_kernel_name reports for it, a SHA-256 of the
packed weight blob and the arena size (floats) builder.finish() returns.  The op digests were recorded before the split conv
kernel learnt rectangular windows (csrc/pwx6.hip), so any change of op, field, kernel choice, weight packing or arena layout
in those networks fails here.

Regenerate (only when a plan change is intended): python tests/test_plan_digests.py --write
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
BATCHES = (2, 16, 256)
FRAME_HW = (576, 1024)


def _networks():
    import torch
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace
    from face_detection_and_recognition_amd.modules.facenet.inception_resnet_v1 import InceptionResnetV1
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    from face_detection_and_recognition_amd.modules.yolov5_face.yolo import Model

    torch.manual_seed(0)
    nets = {}
    for back in (False, True):
        name = "blazeface_back" if back else "blazeface_front"
        net = BlazeFace(back)
        nets[name] = lambda n, net=net: net._emit(n)[0]
        nets[name + "_u8"] = lambda n, net=net: net._emit(n, frame_hw=FRAME_HW)[0]
    for cfg in ("yolov5n", "yolov5s", "yolov5n-0.5"):
        net = Model(cfg)
        nets[cfg] = lambda n, net=net: net._emit(n, 640, 640)[0]
        nets[cfg + "_u8"] = lambda n, net=net: net._emit(n, 640, 640, frame_hw=FRAME_HW)[0]
    mfn = MobileFaceNet(512)
    nets["mobile_facenet"] = lambda n: mfn._emit(n)[0]
    for d in (128, 512):
        fn = InceptionResnetV1(d)
        nets[f"facenet{d}"] = lambda n, fn=fn: fn._emit(n)[0]
    return nets


def plan_digest(builder):
    """{n_ops, sha256 over every fp_op field and the kernel name of every op, weights_sha256, arena_floats}"""
    from face_detection_and_recognition_amd import _lib as L
    lib = L.load()
    ops, weights, arena_floats = builder.finish()
    h = hashlib.sha256()
    for op in ops:
        fields = [str(getattr(op, f)) for f, _ in L.FpOp._fields_]
        name = lib.fp_op_kernel_name(ctypes.byref(op)).decode()
        h.update((",".join(fields) + "|" + name + "\n").encode())
    return {"n_ops": len(ops), "sha256": h.hexdigest(), "weights_sha256": hashlib.sha256(weights.tobytes()).hexdigest(),
            "arena_floats": int(arena_floats)}


def compute_digests():
    from face_detection_and_recognition_amd.plan import PlanBuilder
    out = {}
    saved = PlanBuilder.X6
    try:
        for name, emit in _networks().items():
            for n in BATCHES:
                for x6 in (True, False):
                    PlanBuilder.X6 = x6
                    out[f"{name}/N={n}/X6={int(x6)}"] = plan_digest(emit(n))
    finally:
        PlanBuilder.X6 = saved
    return out


@pytest.fixture(scope="module")
def lib():
    from face_detection_and_recognition_amd import _lib as L
    return L.load()


def test_existing_plans_unchanged(lib):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = compute_digests()
    assert sorted(got) == sorted(want)
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, f"plans changed: {moved}"


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python tests/test_plan_digests.py --write")
    with open(FIXTURE, "w") as f:
        json.dump(compute_digests(), f, indent=1, sort_keys=True)
        f.write("\n")
