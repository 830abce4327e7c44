"""Shared cases of the augmented-inference tests (test_tta_cpu.py, test_tta_gpu.py): the reference's three views restated
with torch on the CPU -- torch.flip, F.interpolate, F.pad (scale_img, y5/utils/torch_utils.py:230-240), oracle.yolo_ref.forward
per view, the un-mapping of y5/models/yolo.py:166-170 -- and a seeded YOLOv5n-face whose Detect biases are conditioned on the
CPU so that a few hundred of the 2583 concatenated rows of a 128 x 128 input pass conf 0.4."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from face_detection_and_recognition_amd.modules.yolov5_face.yolo import SPECS, Model
from face_detection_and_recognition_amd.synth import synth_state_dict
from oracle import yolo_ref

SCALES = (1, 0.83, 0.67)          # yolo.py:159
FLIPS = (None, 3, None)           # yolo.py:160
SHAPES = ((128, 128), (96, 160))  # padded size equal to / different from the input per axis; height and width differ
NAMES = ("yolov5n-0.5", "yolov5n")
B = 2
# the table of the issue, worked out by hand from scale_img's formulas: content, padded per view, decoded rows per view
TABLE = {
    (128, 128): (((128, 128), (128, 128)), ((106, 106), (128, 128)), ((85, 85), (96, 96)), (1008, 1008, 567)),
    (96, 160): (((96, 160), (96, 160)), ((79, 132), (96, 160)), ((64, 107), (96, 128)), (945, 945, 756)),
    (640, 640): (((640, 640), (640, 640)), ((531, 531), (544, 544)), ((428, 428), (448, 448)), (25200, 18207, 12348)),
}


def scale_img(img, ratio, gs=32):
    """torch_utils.py:230-240 with same_shape = False."""
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    h, w = [math.ceil(x * ratio / gs) * gs for x in (h, w)]
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=0.447)


def views_torch(x):
    """x (b, 3, H, W) -> the three network inputs, yolo.py:162-163."""
    return [scale_img(x.flip(fi) if fi else x, si) for si, fi in zip(SCALES, FLIPS)]


def restate(name, sd, x):
    """Model.forward(x, augment=True) of the reference on the CPU -> (z (b, R1 + R2 + R3, 16), rows per view)."""
    ys = []
    with torch.no_grad():
        for xi, si, fi in zip(views_torch(x), SCALES, FLIPS):
            yi = yolo_ref.forward(SPECS[name], sd, xi)[0].clone()
            yi[..., :4] /= si
            if fi == 3:
                yi[..., 0] = x.shape[-1] - yi[..., 0]
            ys.append(yi)
    return torch.cat(ys, 1), [y.shape[1] for y in ys]


def canvas(h, w, seed=0, b=B):
    """(b, 3, h, w) fp32 in [0, 1], seeded."""
    return torch.from_numpy(np.random.default_rng(seed).random((b, 3, h, w), dtype=np.float32))


def column_canvas(h, w, b=B):
    """A canvas whose value encodes its column (and, faintly, row, channel and image): a view that is not mirrored, or is
    mirrored about the wrong axis, is off by far more than any tolerance."""
    col = torch.arange(w, dtype=torch.float32) / w
    row = torch.arange(h, dtype=torch.float32) / (64.0 * h)
    x = col[None, None, None, :] * 0.9 + row[None, None, :, None]
    return (x + torch.arange(3)[None, :, None, None] * 0.01 + torch.arange(b)[:, None, None, None] * 0.02).contiguous()


def state_dict(name, seed, fuse):
    m = Model(name)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed))
    if fuse:
        m.fuse()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def frames_u8(sizes, seed):
    """Frames with structure (a low-contrast background and two patches each), seeded."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        f = (112 + rng.integers(-6, 7, size=(h, w, 3))).astype(np.uint8)
        for _ in range(2):
            p = int(rng.integers(h // 4, h // 2))
            y0, x0 = int(rng.integers(0, h - p)), int(rng.integers(0, w - p))
            f[y0:y0 + p, x0:x0 + p] = rng.integers(0, 256, size=(p, p, 3), dtype=np.uint8)
        out.append(f)
    return out


NMS_HW = (128, 128)
NMS_SEED, NMS_PASS = 11, 300


def frame_canvas(frames):
    """u8 BGR frames of the network's input size -> (b, 3, h, w) fp32 RGB / 255 (the letterbox is the identity there)."""
    lut = np.arange(256).astype(np.float32)
    lut /= 255.0
    return torch.from_numpy(np.stack([lut[f[..., ::-1]] for f in frames])).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def nms_case():
    """-> (fused state_dict of a YOLOv5n-face, the dense frames): workload.build_yolo_detector's conditioning done on the CPU
    with the oracle, over the rows of all three views -- the class score saturates, the boxes are a few anchors wide, the landmarks stay near their cell, every
    (level, anchor) group's objectness logit gets a spread of 2, and the shift lets about NMS_PASS of the 2583 rows of an
    image pass conf 0.4."""
    name = "yolov5n"
    sd = state_dict(name, NMS_SEED, True)
    frames = frames_u8([NMS_HW] * B, 5)
    xs = views_torch(frame_canvas(frames))
    last = len(SPECS[name]["backbone"]) + len(SPECS[name]["head"]) - 1
    na, no = 3, 16
    for lvl in range(3):
        bias = sd[f"model.{last}.m.{lvl}.bias"].view(na, no)
        bias[:, 15] += 8.0
        bias[:, 2:4] += 2.0
        # random heads throw the landmarks up to 1.7 anchors from their cell (-164 .. 214 px on this 128 px input, in view 1
        # already); a face's landmarks lie inside its box, within half an anchor of the cell: a quarter of the random offsets
        sd[f"model.{last}.m.{lvl}.weight"].view(na, no, -1)[:, 5:15] *= 0.25
        bias[:, 5:15] *= 0.25

    def logits():
        with torch.no_grad():
            per_view = [yolo_ref.forward(SPECS[name], sd, xi)[1] for xi in xs]
        return [[heads[lvl][..., 4] for heads in per_view] for lvl in range(3)]        # [lvl][view] (b, na, ny, nx)

    lg = logits()
    for lvl in range(3):
        wgt = sd[f"model.{last}.m.{lvl}.weight"].view(na, no, -1)
        bias = sd[f"model.{last}.m.{lvl}.bias"].view(na, no)
        for a in range(na):
            grp = torch.cat([v[:, a].flatten() for v in lg[lvl]])
            g = 2.0 / max(float(grp.std()), 1e-6)
            wgt[a, 4] *= g
            bias[a, 4] = g * (bias[a, 4] - float(grp.mean()))
    flat = torch.cat([v.flatten() for per in logits() for v in per])
    kth = torch.topk(flat, NMS_PASS * B + 1).values[-1]
    delta = math.log(0.4 / 0.6) - float(kth) + 1e-3
    for lvl in range(3):
        sd[f"model.{last}.m.{lvl}.bias"].view(na, no)[:, 4] += delta
    return sd, frames
