"""Shared cases of the face-quality tests (test_quality_cpu.py, test_quality_gpu.py): the rectangles at which the decimation
step, the block grid or the clamping changes, on frames whose contents reach the extreme sums, and the landmark sets of the pose
record.  A case is (name, frames, dense, items): frames a list of (h, w, 3) u8 arrays, dense True when they share a size (the GPU
test then runs them as a (B, H, W, 3) tensor AND as a RaggedFrames), items (n, 9) int32 fp_resize_item rows."""
import numpy as np

from face_detection_and_recognition_amd import quality as Q


def item(src, sx, sy, sw, sh):
    return [src, sx, sy, sw, sh, -3, 9, 112, 0]          # the destination fields are ignored: anything


def checker(h, w, cell=1):
    """0 / 255 checkerboard of cell x cell squares, all three channels."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y // cell + x // cell) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


def box_blur(img, r):
    """Mean over (2r + 1)^2 neighbours, edges replicated; u8 in, u8 out."""
    p = np.pad(img.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="edge")
    k = 2 * r + 1
    acc = sum(p[dy:dy + img.shape[0], dx:dx + img.shape[1]] for dy in range(k) for dx in range(k))
    return np.round(acc / (k * k)).astype(np.uint8)


def _contents(h, w, seed):
    rng = np.random.default_rng(seed)
    return [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), checker(h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]


def _dense2():
    """Two 40 x 64 frames: the smallest rectangles, one hanging over each edge, the empty and the bad rows."""
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (40, 64, 3), dtype=np.uint8), checker(40, 64)]
    rows = []
    for f in (0, 1):
        rows += [item(f, 5, 6, 1, 1), item(f, 62, 38, 2, 2), item(f, 30, 20, 3, 3), item(f, 0, 0, 64, 40),
                 item(f, -7, 4, 20, 20), item(f, 50, 4, 30, 20), item(f, 10, -5, 20, 20), item(f, 10, 30, 20, 20),     # left, right, top, bottom
                 item(f, -10, -10, 100, 100), item(f, 7, 7, 0, 5), item(f, 7, 7, 5, -1), item(f, 64, 3, 5, 5), item(f, -9, 3, 5, 5)]
    rows += [item(-1, 0, 0, 10, 10), item(2, 0, 0, 10, 10), item(0, 2**31 - 20, 2, 2**31 - 1, 5)]
    return frames, True, rows


def _sizes():
    """112 x 112 (the largest s = 1), 113 x 112 (s = 2, a trailing column), 224 x 113 (a trailing row) and 3 x 3 on all-0, all-255,
    1-px checkerboard and random frames; 300 x 40 (s = 3, more columns than threads); frames 3 and 7 pixels wide."""
    rng = np.random.default_rng(12)
    frames = _contents(130, 240, 13) + [rng.integers(0, 256, (50, 320, 3), dtype=np.uint8), rng.integers(0, 256, (5, 3, 3), dtype=np.uint8),
                                        rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)]
    rows = []
    for f in range(4):
        rows += [item(f, 3, 5, 112, 112), item(f, 100, 17, 113, 112), item(f, 11, 13, 224, 113), item(f, 236, 126, 3, 3), item(f, 1, 1, 111, 37)]
    rows += [item(4, 7, 3, 300, 40), item(4, 0, 0, 320, 50), item(5, 0, 0, 3, 5), item(5, 1, 1, 2, 3), item(6, 0, 0, 7, 9), item(6, 2, 3, 5, 5)]
    return frames, False, rows


def _largest():
    """7168 x 192 of 0 / 255 blocks of 64 px inside a 200 x 7200 frame: s = 64 and the largest sums; 7169 x 4: too large."""
    frames = [checker(200, 7200, 64)]
    return frames, True, [item(0, 0, 0, 7168, 192), item(0, 17, 3, 7168, 192), item(0, 0, 0, 7169, 4), item(0, 5, 1, 7105, 190)]


def _empty_batch():
    return [np.zeros((8, 8, 3), np.uint8)], True, []


def _many():
    """300 faces, more than a workgroup has lanes, of every size up to 150 px in three frames."""
    rng = np.random.default_rng(14)
    frames = [rng.integers(0, 256, (160, 200, 3), dtype=np.uint8) for _ in range(3)]
    frames[1][40:120, 30:150] = 250        # a blown-out and a dark patch
    frames[2][:, 100:] //= 20
    rows = [item(int(rng.integers(0, 3)), int(rng.integers(-10, 190)), int(rng.integers(-10, 150)), int(rng.integers(1, 151)),
                 int(rng.integers(1, 151))) for _ in range(300)]
    return frames, True, rows


CASES = []
for _name, _make in [("dense2", _dense2), ("sizes", _sizes), ("largest", _largest), ("n0", _empty_batch), ("n300", _many)]:
    _frames, _dense, _rows = _make()
    CASES.append((_name, _frames, _dense, np.array(_rows, np.int32).reshape(-1, 9)))
IDS = [c[0] for c in CASES]

_EXPECTED = {}


def expected(case):
    """face_quality_numpy of the case, computed once and shared (do not modify)."""
    if case[0] not in _EXPECTED:
        _EXPECTED[case[0]] = Q.face_quality_numpy(case[1], case[3])
    return _EXPECTED[case[0]]


# ------------------------------------------------------------------------------------------------ pose

FRONTAL = np.array([100, 100, 160, 100, 130, 135, 105, 165, 155, 165], np.float64)     # eyes 60 px apart, nose midway


def _rot(lm, deg):
    p = lm.reshape(5, 2) - lm[:2]
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return (p @ np.array([[c, s], [-s, c]]) + lm[:2]).reshape(10)


def _edit(lm, **kw):
    out = lm.copy()
    for k, v in kw.items():
        out[int(k[1:])] = v
    return out


def pose_landmarks(fmt):
    """(names, (n, 10) fp32 landmarks in the layout of `fmt`, degenerate (n,) bool).  fmt 0: point 3 is the mouth centre and slots
    8, 9 are 0.  In the non-degenerate rows every landmark lies within 4 iod of the left eye."""
    rows = [("frontal", FRONTAL, False)]
    rows += [(f"yaw{dx:+d}", _edit(FRONTAL, _4=130 + dx), False) for dx in (-30, -12, 7, 30, 45)]
    rows += [(f"roll{d:+d}", _rot(FRONTAL, d), False) for d in (-35, -10, 5, 20, 80)]
    rows += [(f"pitch{dy:+d}", _edit(FRONTAL, _5=135 + dy), False) for dy in (-40, -20, 10, 28)]
    rows += [("small", (FRONTAL - 100) / 40 + 3.25, False),                                # iod 1.5
             ("iod_half", _edit(FRONTAL, _2=100.5), True),                                 # eyes 0.5 px apart
             ("iod_zero", _edit(FRONTAL, _2=100), True),
             ("mouth_above", _edit(FRONTAL, _7=40, _9=40), True),
             ("mouth_on_axis", _edit(FRONTAL, _7=100, _9=100), True),                      # the denominator is 0
             ("far", FRONTAL * 0.5 + np.tile([32640.25, 32600.5], 5), False),              # coordinates near 32767
             ("far_rolled", _rot(FRONTAL * 0.25 + np.tile([32700.125, 32690.75], 5), 33), False),
             ("subpixel", FRONTAL + np.linspace(0.013, 0.977, 10), False)]
    lm = np.array([r[1] for r in rows], np.float64)
    if fmt == 0:
        lm[:, 6:8] = (lm[:, 6:8] + lm[:, 8:10]) / 2
        lm[:, 8:10] = 0
    return [r[0] for r in rows], lm.astype(np.float32), np.array([r[2] for r in rows])


POSE_FMTS = (0, 1, 2)
