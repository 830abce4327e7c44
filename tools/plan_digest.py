"""Digest of every network's plan, host only (no GPU): a plan is bytes -- the fp_op array, the weight blob, the arena size --
so two versions of the plan builder that print the same digests hand the kernels the same work.

One line per case: SHA-256 over the raw bytes of every fp_op, the weight blob, the arena size, alg_bytes and the row windows;
then the op count, the weight count and validate_on_host's status.  Every case runs at the default switches, with
PlanBuilder.X6 off, and with every other boolean class-wide switch of its plan-cache key (switch_key) flipped alone; a few
combinations that single flips do not reach follow.  The tool ends with the (op kind, SPLIT3, OUT_DW / IN_UP2 ...)
combinations it saw.

usage: python tools/plan_digest.py [--out FILE] [--compare FILE] [--only SUBSTRING]
  --out FILE      write the digests as JSON
  --compare FILE  compare with digests written earlier ON THE SAME MACHINE (the .fuse() cases go through torch.mm on the
                  host); names the differing cases and exits 1 if there are any
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from face_detection_and_recognition_amd import _lib as L  # noqa: E402
from face_detection_and_recognition_amd.modules.age_gender.age_gender_net import AgeGenderNet  # noqa: E402
from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeBlock, BlazeFace  # noqa: E402
from face_detection_and_recognition_amd.modules.facenet.inception_resnet_v1 import InceptionResnetV1  # noqa: E402
from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import Depth_Wise, MobileFaceNet  # noqa: E402
from face_detection_and_recognition_amd.modules.mtcnn.mtcnn import MTCNN  # noqa: E402
from face_detection_and_recognition_amd.modules.yolov5_face import yolo as Y  # noqa: E402
from face_detection_and_recognition_amd.plan import PlanBuilder, switch_key, validate_on_host  # noqa: E402
from face_detection_and_recognition_amd.synth import synth_state_dict  # noqa: E402

FRAME_HW = (576, 1024)
KIND = {v: k[3:] for k, v in vars(L).items() if k.startswith("OP_")}
SEEN = set()


def synth(net, seed):
    net.load_state_dict(synth_state_dict(net.state_dict(), seed))
    return net


def digest(pb):
    """(sha256, op count, weight count, validate status) of an emitted plan; notes the op forms in SEEN."""
    ops, weights, arena = pb.finish()
    h = hashlib.sha256()
    for op in ops:
        h.update(bytes(op))
        tags = [name for name, bit in (("OUT_DW", L.OPF_OUT_DW), ("IN_UP2", L.OPF_IN_UP2)) if op.flags & bit]
        # forms the two flags do not tell apart: the flat-K split conv, the stride-2 pair, the ops reading u8 frames with /
        # without a scale, the dw -> 1x1 op's second PReLU and its shuffle epilogue
        if op.kind == L.OP_CONV and op.flags & L.OPF_SPLIT3 and not op.flags & L.OPF_OUT_DW and op.Cin < 32:
            tags.append("flatK")
        if op.kind == L.OP_BLAZEPAIR and op.stride == 2:
            tags.append("s2")
        if op.kind == L.OP_DWPW and op.bias_off >= 0:
            tags.append("out_slope")
        if op.kind == L.OP_DWPW and op.res_mode == L.RES_SHUFFLE2:
            tags.append("shuffle")
        SEEN.add((KIND[op.kind], "SPLIT3" if op.flags & L.OPF_SPLIT3 else "fp32", "+".join(tags)))
    h.update(np.ascontiguousarray(weights).tobytes())
    h.update(repr((int(arena), [int(b) for b in pb.alg_bytes], [tuple(map(int, w)) for w in pb.windows])).encode())
    return h.hexdigest(), len(ops), int(weights.size), int(validate_on_host(pb))


@contextlib.contextmanager
def switched(settings):
    """settings: [(class, attribute, value)], restored on exit."""
    old = [(cls, name, getattr(cls, name)) for cls, name, _ in settings]
    try:
        for cls, name, v in settings:
            setattr(cls, name, v)
        yield
    finally:
        for cls, name, v in old:
            setattr(cls, name, v)


def variants(classes, extra=()):
    """[(label, settings)]: defaults, X6 off, every other boolean switch of switch_key(*classes) flipped alone, then `extra`."""
    out = [("default", []), ("X6=0", [(PlanBuilder, "X6", False)])]
    by_name = {c.__name__: c for c in classes}
    for cname, name, v in switch_key(*classes):
        if isinstance(v, bool) and (cname, name) != ("PlanBuilder", "X6"):
            out.append((f"{cname}.{name}={int(not v)}", [(by_name[cname], name, not v)]))
    return out + list(extra)


def cases():
    """[(name, switch classes, extra variants, emit() -> PlanBuilder)]"""
    out = []
    blaze = (PlanBuilder, BlazeBlock, BlazeFace)
    for back in (False, True):
        net = synth(BlazeFace(back), 11)
        for n in (3, 16, 256):
            for fhw in (None, FRAME_HW):
                out.append((f"blazeface-{'back' if back else 'front'} N={n} frame_hw={fhw}", blaze, (),
                            lambda net=net, n=n, fhw=fhw: net._emit(n, frame_hw=fhw)[0]))
    mfn_cls = (PlanBuilder, Depth_Wise, MobileFaceNet)
    x6off = (PlanBuilder, "X6", False)
    mfn_extra = [("X6=0 BLOCK_SHAPES=(7,14)", [x6off, (Depth_Wise, "BLOCK_SHAPES", (7, 14))])]
    mfn = synth(MobileFaceNet(512), 12)
    for n in (4, 528):
        out.append((f"mobilefacenet N={n}", mfn_cls, mfn_extra, lambda n=n: mfn._emit(n)[0]))
    yolo = (PlanBuilder, Y.Conv, Y.StemBlock, Y.C3, Y.ShuffleV2Block, Y.SPP, Y.Concat, Y.Model)
    yolo_extra = [("X6=0 FUSE=0", [x6off, (Y.ShuffleV2Block, "FUSE", False), (Y.StemBlock, "FUSE", False)]),
                  ("FUSE_DOWN=0 FUSE_UNIT=0", [(Y.ShuffleV2Block, "FUSE_DOWN", False), (Y.ShuffleV2Block, "FUSE_UNIT", False)])]
    for name in ("yolov5n", "yolov5n-0.5", "yolov5s"):
        for fused in (False, True):
            net = synth(Y.Model(name), 13)
            if fused:
                net.fuse()
            for fhw in (None, FRAME_HW):
                out.append((f"{name}{' fused' if fused else ''} N=4 frame_hw={fhw}", yolo, yolo_extra,
                            lambda net=net, fhw=fhw: net._emit(4, 640, 640, frame_hw=fhw)[0]))
    one = (PlanBuilder,)
    facenet = synth(InceptionResnetV1(512), 14)
    out.append(("inception-resnet-v1 N=2", one, (), lambda: facenet._emit(2)[0]))
    ag = synth(AgeGenderNet(), 15)
    out.append(("agegender N=2", one, (), lambda: ag._emit(2)[0]))
    mt = synth(MTCNN(), 16)
    for sub in ("rnet", "onet"):
        out.append((f"mtcnn-{sub} N=8", one, (), lambda sub=sub: mt._emit(sub, 8)[0]))
    out.append(("mtcnn-pnet N=2 40x56", one, (), lambda: mt._emit_pnet(2, 40, 56)[0]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare")
    ap.add_argument("--only", default="", help="run only the cases whose name contains this")
    args = ap.parse_args()
    result = {}
    for name, classes, extra, emit in cases():
        if args.only not in name:
            continue
        for label, settings in variants(classes, extra):
            with switched(settings):
                sha, n_ops, n_w, status = digest(emit())
            key = f"{name} [{label}]"
            result[key] = dict(sha256=sha, ops=n_ops, weights=n_w, status=status)
            print(f"{sha[:16]}  ops={n_ops:4d}  weights={n_w:9d}  validate={status}  {key}")
    print(f"{len(result)} cases, {sum(r['status'] != 0 for r in result.values())} failed validation")
    print("op forms seen (kind, arithmetic, flags):")
    for form in sorted(SEEN):
        print("  " + "  ".join(f for f in form if f))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
    rc = 1 if any(r["status"] != 0 for r in result.values()) else 0
    if args.compare:
        with open(args.compare) as f:
            want = json.load(f)
        if args.only:
            want = {k: v for k, v in want.items() if k in result}
        diff = sorted(k for k in set(want) | set(result) if want.get(k) != result.get(k))
        for k in diff:
            print(f"DIFFERS: {k}: {want.get(k)} -> {result.get(k)}")
        print(f"{len(diff)} of {len(result)} cases differ from {args.compare}")
        rc = rc or (1 if diff else 0)
    return rc


if __name__ == "__main__":
    sys.exit(main())
