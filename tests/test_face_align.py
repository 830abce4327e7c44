"""Five-point face alignment (csrc/align.hip, modules/utils/align.py, FacePipeline(align=True)).

The contract, restated in fp64 numpy below: landmarks in frame pixels from the same kernel pass as the box (BlazeFace:
bbox_lmarks of the reference's get_dets_bboxes_confs_lmarks_areas; YOLOv5-face: scale_coords_landmarks), a least-squares
similarity onto the ArcFace 112 x 112 template (Umeyama's estimate in closed form), and a bilinear warp with cv2.warpAffine's
pixel convention and a constant 0 border.  CPU: the host emulator against the oracle.  GPU: the device against the
emulator bit for bit, the unchanged crop records, and the pipeline / driver with align=True."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.utils import align as A

FMT_BLAZE, FMT_YOLO = 0, 1


# ---------------------------------------------------------------------------------------------- fp64 oracle

def oracle_estimate(p, q):
    """Least-squares similarity p -> q (2-D Umeyama, no reflection) in fp64 -> (M (2, 3), S)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    mp, mq = p.mean(0), q.mean(0)
    dp, dq = p - mp, q - mq
    S = float((dp ** 2).sum())
    a = float((dp * dq).sum()) / S
    b = float((dp[:, 0] * dq[:, 1] - dp[:, 1] * dq[:, 0]).sum()) / S
    R = np.array([[a, -b], [b, a]])
    t = mq - R @ mp
    return np.concatenate([R, t[:, None]], 1), S


def oracle_warp(frame, M):
    """fp64 bilinear warp: out[y, x] = frame sampled at M^-1 (x, y), taps outside the frame 0, round half-to-even."""
    M = np.asarray(M, np.float64).reshape(2, 3)
    h, w = frame.shape[:2]
    Ri = np.linalg.inv(M[:, :2])
    ys, xs = np.mgrid[0:A.SIZE, 0:A.SIZE].astype(np.float64)
    u, v = xs - M[0, 2], ys - M[1, 2]
    sx = Ri[0, 0] * u + Ri[0, 1] * v
    sy = Ri[1, 0] * u + Ri[1, 1] * v
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    f = frame.astype(np.float64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok[..., None], f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0.0)
    val = ((tap(y0, x0) * (1 - fx)[..., None] + tap(y0, x0 + 1) * fx[..., None]) * (1 - fy)[..., None]
           + (tap(y0 + 1, x0) * (1 - fx)[..., None] + tap(y0 + 1, x0 + 1) * fx[..., None]) * fy[..., None])
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def similarity(angle, scale, tx, ty):
    a, b = scale * np.cos(angle), scale * np.sin(angle)
    return np.array([[a, -b, tx], [b, a, ty]])


def lmarks_for(M, fmt):
    """Landmarks (10,) float32 that M maps exactly onto the template targets (up to their float32 rounding)."""
    q = A.targets(fmt)
    Ri = np.linalg.inv(M[:, :2])
    p = (q - M[:, 2]) @ Ri.T
    out = np.zeros(10, np.float32)
    out[:2 * len(p)] = p.reshape(-1)
    return out


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


# ---------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("fmt", [FMT_BLAZE, FMT_YOLO])
def test_estimate_recovers_a_known_similarity(lib, fmt):
    """Rotations over +-180 degrees, scales 0.05 .. 20, arbitrary translations: the emulated estimate equals the fp64 oracle
    on the same (float32) landmarks to 1e-9 relative, and the known similarity to the landmarks' float32 rounding."""
    rng = np.random.default_rng(1)
    Ms, lms = [], []
    for angle in np.linspace(-np.pi, np.pi, 13):
        for scale in (0.05, 0.3, 1.0, 4.0, 20.0):
            Ms.append(similarity(angle, scale, *rng.uniform(-3000, 3000, 2)))
            lms.append(lmarks_for(Ms[-1], fmt))
    M, fl = A.emulate_estimate(np.stack(lms), fmt)
    assert (fl == 0).all()
    n = 4 if fmt == FMT_BLAZE else 5
    for k, (want, lm) in enumerate(zip(Ms, lms)):
        ref, _ = oracle_estimate(lm[:2 * n].reshape(n, 2), A.targets(fmt))
        got = M[k].reshape(2, 3)
        assert _rel(got[:, :2], ref[:, :2]) <= 1e-9 and _rel(got[:, 2], ref[:, 2]) <= 1e-9 * max(1.0, np.abs(ref[:, 2]).max()
                                                                                                   / np.abs(ref[:, :2]).max()), k
        assert _rel(got[:, :2], want[:, :2]) < 1e-4, k
        assert got[0, 0] == got[1, 1] and got[0, 1] == -got[1, 0]


def test_estimate_on_noisy_landmarks_is_the_least_squares_solution(lib):
    rng = np.random.default_rng(2)
    for fmt in (FMT_BLAZE, FMT_YOLO):
        q = A.targets(fmt)
        for _ in range(40):
            M0 = similarity(rng.uniform(-np.pi, np.pi), rng.uniform(0.1, 5), *rng.uniform(-500, 500, 2))
            lm = lmarks_for(M0, fmt)
            n = len(q)
            lm[:2 * n] += rng.normal(0, 3.0 / np.hypot(M0[0, 0], M0[1, 0]), 2 * n).astype(np.float32)
            M, fl = A.emulate_estimate(lm[None], fmt)
            assert fl[0] == 0
            p = lm[:2 * n].reshape(n, 2).astype(np.float64)
            Amat = np.zeros((2 * n, 4))
            Amat[0::2] = np.stack([p[:, 0], -p[:, 1], np.ones(n), np.zeros(n)], 1)
            Amat[1::2] = np.stack([p[:, 1], p[:, 0], np.zeros(n), np.ones(n)], 1)
            a, b, tx, ty = np.linalg.lstsq(Amat, q.reshape(-1), rcond=None)[0]
            want = np.array([a, -b, tx, b, a, ty])
            assert np.abs(M[0] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (fmt, M[0], want)


def test_degenerate_landmarks_are_flagged(lib):
    lm = np.zeros((4, 10), np.float32)
    lm[0, :] = 100.0                                    # every landmark on one point
    lm[1, :] = 7.0
    lm[1, 0::2] += np.float32(0.1) * np.arange(5)       # spread S = 0.1 px^2 < 1
    lm[2, 0::2] = [10, 40, 25, 12, 38]                  # a normal face
    lm[2, 1::2] = [10, 10, 25, 40, 40]
    lm[3, :] = np.nan
    for fmt in (FMT_BLAZE, FMT_YOLO):
        M, fl = A.emulate_estimate(lm, fmt)
        assert fl.tolist() == [A.DEGENERATE, A.DEGENERATE, 0, A.DEGENERATE], fmt
        assert (M[[0, 1, 3]] == 0).all() and (M[2] != 0).any()


def _blaze_rows(dets_ref):
    """Reference-order rows (xmin, ymin, xmax, ymax, 12 keypoint values, conf) -> the device's (ymin, xmin, ymax, xmax, ...)."""
    d = np.asarray(dets_ref, np.float32)
    return np.concatenate([d[:, [1, 0, 3, 2]], d[:, 4:]], 1)


def test_blazeface_landmarks_equal_the_reference_golden(lib):
    """bbox_lmarks of the reference's get_dets_bboxes_confs_lmarks_areas (tests/golden/utils_postprocess.npz), keypoints 0..3;
    boxes and the crop records as fp_dets_to_crops' arithmetic gives them."""
    g = golden("utils_postprocess")
    rows = _blaze_rows(g["blaze_dets"])
    out = A.emulate_crops(rows[None], [len(rows)], [(576, 1024)], (256, 256), FMT_BLAZE, 0.7, 0.12)
    n = len(g["blaze_lmarks"])
    assert len(out["info"]) == n
    np.testing.assert_array_equal(out["info"][:, 1:5], g["blaze_boxes"])
    np.testing.assert_array_equal(out["lmarks"][:, :8], g["blaze_lmarks"][:, :8])
    assert (out["lmarks"][:, 8:] == 0).all()
    assert (out["flags"] == 0).all()
    for k in range(n):
        ref, _ = oracle_estimate(out["lmarks"][k, :8].reshape(4, 2), A.BLAZE_TARGETS)
        assert np.abs(out["M"][k] - ref.reshape(-1)).max() <= 1e-9 * np.abs(ref).max()


def _yolo_rows(rng, n, in_size=640):
    x1y1 = rng.uniform(-40, in_size * 0.8, (n, 2))
    wh = rng.uniform(60, 260, (n, 2))
    lm = x1y1[:, None, :] + wh[:, None, :] * rng.uniform(-0.3, 1.3, (n, 5, 2))     # some outside the frame: clamped
    rows = np.zeros((n, 16), np.float32)
    rows[:, 0:2], rows[:, 2:4] = x1y1, x1y1 + wh
    rows[:, 4] = rng.uniform(0.3, 1.0, n)
    rows[:, 5:15] = lm.reshape(n, 10)
    rows[:, 15] = 1.0
    return rows


def numpy_scale_coords_landmarks(rows, in_size, frame_hw):
    """scale_coords_landmarks (y5/detect_face_pytorch.py:20-46) on float32 rows: - pad, / gain, clamp to the frame."""
    from face_detection_and_recognition_amd.pipeline import scale_coords_params
    h, w = frame_hw
    gain, px, py = scale_coords_params(in_size, (w, h))
    lm = rows[:, 5:15].astype(np.float32).copy()
    lm[:, 0::2] -= px
    lm[:, 1::2] -= py
    lm /= gain
    lm[:, 0::2] = np.clip(lm[:, 0::2], np.float32(0), np.float32(w))
    lm[:, 1::2] = np.clip(lm[:, 1::2], np.float32(0), np.float32(h))
    return lm


def test_yolo_landmarks_equal_numpy_scale_coords_landmarks(lib):
    rng = np.random.default_rng(3)
    for frame_hw in [(576, 1024), (1650, 1275), (480, 640)]:
        rows = _yolo_rows(rng, 24)
        out = A.emulate_crops(rows[None], [len(rows)], [frame_hw], (640, 640), FMT_YOLO, 0.4, 0.12)
        keep = (rows[:, 4] > np.float32(0.4)) & ((np.float32(100) * (rows[:, 2] - rows[:, 0]) * (rows[:, 3] - rows[:, 1]))
                                                 / np.float32(640 * 640) > np.float32(0.12))
        want = numpy_scale_coords_landmarks(rows[keep], (640, 640), frame_hw)
        assert len(out["lmarks"]) == keep.sum() > 0
        np.testing.assert_array_equal(out["lmarks"], want)
        assert (out["lmarks"] >= 0).all() and (out["lmarks"][:, 0::2] <= frame_hw[1]).all()


def _faces(M, frame_idx):
    n = len(M)
    info = np.zeros((n, 7), np.float32)
    info[:, 0] = frame_idx
    items = np.zeros((n, 9), np.int32)
    items[:, 0] = frame_idx
    return info, np.zeros(n, np.int32), items


def test_emulated_warp_matches_the_fp64_oracle(lib):
    """Random similarities (faces partly outside the frame included): u8 within 1 level everywhere, exact on >= 99.9 %."""
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (2, 150, 200, 3), dtype=np.uint8)
    frames = np.clip(frames.astype(np.int32) // 4 + np.linspace(0, 180, 200)[None, None, :, None], 0, 255).astype(np.uint8)
    Ms, idx = [], []
    for k in range(24):
        Ms.append(similarity(rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 3.0), *rng.uniform(-150, 250, 2)).reshape(-1))
        idx.append(k % 2)
    M = np.stack(Ms)
    info, fl, items = _faces(M, np.array(idx))
    got = A.emulate_warp(frames, M, info, fl, items)
    want = np.stack([oracle_warp(frames[i], m) for m, i in zip(M, idx)])
    d = np.abs(got.astype(np.int32) - want)
    assert d.max() <= 1 and (d == 0).mean() >= 0.999, (d.max(), (d == 0).mean())


def test_emulated_warp_exact_cases(lib):
    """Integer translation at scale 1 copies frame pixels, 90 / 180 degree rotations permute them, taps outside are 0."""
    rng = np.random.default_rng(5)
    H, W = 90, 130
    f = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    ys, xs = np.mgrid[0:A.SIZE, 0:A.SIZE]
    cases = []
    for tx, ty in [(-10, -5), (20, 30), (-100, 0), (0, -60)]:
        cases.append((np.array([1, 0, tx, 0, 1, ty], np.float64), ys - ty, xs - tx))
    for tx, ty in [(100, -7), (50, 40)]:               # (x', y') = (-y + tx, x + ty): x = y' - ty, y = tx - x'
        cases.append((np.array([0, -1, tx, 1, 0, ty], np.float64), tx - xs, ys - ty))
    for tx, ty in [(120, 80), (60, 130)]:              # (x', y') = (tx - x, ty - y)
        cases.append((np.array([-1, 0, tx, 0, -1, ty], np.float64), ty - ys, tx - xs))
    M = np.stack([c[0] for c in cases])
    info, fl, items = _faces(M, np.zeros(len(M), np.int64))
    got = A.emulate_warp(f, M, info, fl, items)
    outside = 0
    for k, (_, sy, sx) in enumerate(cases):
        ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        want = np.where(ok[..., None], f[0][np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0)
        np.testing.assert_array_equal(got[k], want, err_msg=str(k))
        outside += int((~ok).sum())
    assert outside > 0


def test_new_entry_points_refuse_bad_arguments(lib):
    """Refusals on the host before any launch (never the launch status -4); the pointers are never dereferenced."""
    P = ctypes.c_void_p
    fake, fake8 = P(0x10000), P(0x20000)

    def warp(**kw):
        a = dict(frames=fake, B=2, H=64, W=64, M=fake8, info=fake, flags=fake, items=fake, n=3, u8=fake, f32=None, c=0, lut=None)
        a.update(kw)
        return lib.fp_align_warp(a["frames"], a["B"], a["H"], a["W"], a["M"], a["info"], a["flags"], a["items"], a["n"], a["u8"],
                                 a["f32"], a["c"], a["lut"], None)
    for kw in [dict(frames=None), dict(M=None), dict(info=None), dict(flags=None), dict(items=None), dict(n=-1), dict(B=0),
               dict(H=0), dict(W=0), dict(W=32768), dict(H=65536), dict(u8=None), dict(f32=fake, c=4, lut=None),
               dict(f32=fake, c=2, lut=fake), dict(f32=fake, c=5, lut=fake)]:
        assert warp(**kw) == -1, kw
    assert warp(M=P(0x20004)) == -5
    assert warp(f32=P(0x10004), c=4, lut=fake) == -5
    assert warp(n=0) == 0
    assert lib.fp_align_warp_ragged(fake, 8, fake, 1, fake8, fake, fake, fake, 1, fake, None, 0, None, None) == -1
    assert lib.fp_align_warp_ragged(fake, 1 << 20, None, 1, fake8, fake, fake, fake, 1, fake, None, 0, None, None) == -1

    def cr(**kw):
        a = dict(dets=fake, counts=fake, row=17, fmt=0, lm=fake, M=fake8, fl=fake, ow=1024, oh=576, gain=0.25)
        a.update(kw)
        return lib.fp_dets_to_crops_aligned(a["dets"], a["counts"], 2, 16, a["row"], a["fmt"], 256, 256, a["ow"], a["oh"], 0.7,
                                            0.12, a["gain"], 0.0, 56.0, -6, -1, 4, 5, 112, 112, 32, fake, fake, fake, a["lm"],
                                            a["M"], a["fl"], None)
    for kw in [dict(dets=None), dict(lm=None), dict(M=None), dict(fl=None), dict(row=16), dict(fmt=1, row=14), dict(fmt=2),
               dict(ow=0), dict(gain=0.0)]:
        assert cr(**kw) == -1, kw
    assert cr(M=P(0x20004)) == -5
    assert lib.fp_dets_to_crops_aligned_ragged(fake, fake, 2, 16, 17, 0, 256, 256, None, fake, 0.7, 0.12, -6, -1, 4, 5, 112,
                                               112, 32, fake, fake, fake, fake, fake8, fake, None) == -1


def test_header_prototypes_match_the_bindings(lib, tmp_path):
    """The new declarations compile as C99 against the argument types _lib.py binds."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "align.c"
    src.write_text("""#include "facepath.h"
int main(void) {
  int (*a)(const float*, const int32_t*, int, int, int, int, int, int, int, int, float, float, float, float, float, int, int,
           int, int, int, int, int, fp_resize_item*, float*, int32_t*, float*, double*, int32_t*, void*) = fp_dets_to_crops_aligned;
  int (*b)(const float*, const int32_t*, int, int, int, int, int, int, const fp_frame_desc*, const float*, float, float, int,
           int, int, int, int, int, int, fp_resize_item*, float*, int32_t*, float*, double*, int32_t*, void*)
      = fp_dets_to_crops_aligned_ragged;
  int (*c)(const float*, const int32_t*, int, int, int, int, int, int, const fp_frame_desc*, const float*, float, float, int,
           int, int, int, int, int, int, fp_resize_item*, float*, int32_t*, float*, double*, int32_t*)
      = fp_dets_to_crops_aligned_emulate;
  int (*d)(const uint8_t*, int, int, int, const double*, const float*, const int32_t*, const fp_resize_item*, int, uint8_t*,
           float*, int, const float*, void*) = fp_align_warp;
  int (*e)(const uint8_t*, size_t, const fp_frame_desc*, int, const double*, const float*, const int32_t*,
           const fp_resize_item*, int, uint8_t*, float*, int, const float*, void*) = fp_align_warp_ragged;
  int (*f)(const uint8_t*, size_t, const fp_frame_desc*, int, const float*, int, double*, const float*, int32_t*,
           const fp_resize_item*, int, uint8_t*) = fp_align_emulate;
  return (a == 0) + (b == 0) + (c == 0) + (d == 0) + (e == 0) + (f == 0) + (FP_ALIGN_SIZE != 112) + (FP_ALIGN_DEGENERATE != 1);
}
""")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(tmp_path / "align.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for name, nargs in [("fp_dets_to_crops_aligned", 29), ("fp_dets_to_crops_aligned_ragged", 26),
                        ("fp_dets_to_crops_aligned_emulate", 25), ("fp_align_warp", 14), ("fp_align_warp_ragged", 14),
                        ("fp_align_emulate", 12)]:
        assert len(L.SIGNATURES[name][1]) == nargs, name
    assert L.ABI_VERSION == 15


# ---------------------------------------------------------------------------------------------- GPU

def _synth_dets(rng, fmt, B, max_dets, sizes, in_size):
    """Random detector rows for B frames (with landmarks inside / around each box, one degenerate face, faces at the edges)."""
    iw, ih = in_size
    row = 17 if fmt == FMT_BLAZE else 16
    dets = np.zeros((B, max_dets, row), np.float32)
    counts = rng.integers(1, max_dets + 1, B).astype(np.int32)
    for f in range(B):
        for i in range(max_dets):
            x1, y1 = rng.uniform(-0.1, 0.85), rng.uniform(-0.1, 0.85)
            w, h = rng.uniform(0.08, 0.4), rng.uniform(0.08, 0.4)
            lm = np.stack([x1 + w * rng.uniform(-0.2, 1.2, 6), y1 + h * rng.uniform(-0.2, 1.2, 6)], 1)
            if i == 1:
                lm[:] = lm[0]                           # degenerate: every landmark on one point
            if fmt == FMT_BLAZE:
                dets[f, i, :4] = [y1, x1, y1 + h, x1 + w]
                dets[f, i, 4:16] = lm.reshape(-1)
                dets[f, i, 16] = rng.uniform(0.6, 1.0)
            else:
                dets[f, i, :4] = [x1 * iw, y1 * ih, (x1 + w) * iw, (y1 + h) * ih]
                dets[f, i, 4] = rng.uniform(0.3, 1.0)
                dets[f, i, 5:15] = (lm[:5] * [iw, ih]).reshape(-1)
                dets[f, i, 15] = 1.0
    return dets, counts


def _device_crops(lib, dev, dets, counts, frames, in_size, fmt, thr, aligned, cap=None):
    from face_detection_and_recognition_amd.frames import RaggedFrames
    from face_detection_and_recognition_amd.pipeline import ragged_scale_coords_params, scale_coords_params
    B, max_dets, row = dets.shape
    cap = cap or B * max_dets
    d, c = torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev)
    items = torch.full((cap, 9), -7, dtype=torch.int32, device=dev)
    info = torch.full((cap, 7), -7.0, dtype=torch.float32, device=dev)
    nf = torch.zeros((1,), dtype=torch.int32, device=dev)
    al = A.alloc(cap, dev)
    extra = [L.ptr(al["lmarks"]), L.ptr(al["M"]), L.ptr(al["flags"])] if aligned else []
    s = L.current_stream(dev)
    if isinstance(frames, RaggedFrames):
        geom = torch.from_numpy(ragged_scale_coords_params(in_size, frames.sizes)).to(dev)
        fn = lib.fp_dets_to_crops_aligned_ragged if aligned else lib.fp_dets_to_crops_ragged
        L.check(fn(L.ptr(d), L.ptr(c), B, max_dets, row, fmt, in_size[0], in_size[1], L.ptr(frames.descs), L.ptr(geom), thr, 0.12,
                   -6, -1, 4, 5, 112, 112, cap, L.ptr(items), L.ptr(info), L.ptr(nf), *extra, s), "crops")
    else:
        _, H, W, _ = frames.shape
        gain, px, py = scale_coords_params(in_size, (W, H))
        fn = lib.fp_dets_to_crops_aligned if aligned else lib.fp_dets_to_crops
        L.check(fn(L.ptr(d), L.ptr(c), B, max_dets, row, fmt, in_size[0], in_size[1], W, H, thr, 0.12, float(gain), float(px),
                   float(py), -6, -1, 4, 5, 112, 112, cap, L.ptr(items), L.ptr(info), L.ptr(nf), *extra, s), "crops")
    n = int(nf.item())
    out = dict(n=n, items=items[:n].cpu().numpy(), info=info[:n].cpu().numpy())
    if aligned:
        out.update(lmarks=al["lmarks"][:n].cpu().numpy(), M=al["M"][:n].cpu().numpy(), flags=al["flags"][:n].cpu().numpy())
        out["dev"] = dict(items=items, info=info, M=al["M"], flags=al["flags"])
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [FMT_BLAZE, FMT_YOLO])
def test_device_equals_emulator_and_crop_records_are_unchanged(lib, dev, fmt):
    """Uniform and ragged batches: items / info / n_faces equal fp_dets_to_crops'; M, lmarks, flags and the u8 faces equal
    the emulator's bit for bit; the fp32 canvas is lut[u8] for C = 3 and 4; degenerate faces get the box crop of
    fp_resize_ragged / fp_resize_normalize; a ragged batch of one size equals the uniform batch."""
    from face_detection_and_recognition_amd.frames import RaggedFrames, resize_ragged
    from face_detection_and_recognition_amd.modules.mobile_facenet.utils import crops_to_input, mfn_lut
    rng = np.random.default_rng(10 + fmt)
    in_size = (256, 256) if fmt == FMT_BLAZE else (640, 640)
    thr = 0.7 if fmt == FMT_BLAZE else 0.4
    sizes = [(576, 1024), (1080, 1920), (1650, 1275), (540, 720), (17, 29)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    lut = mfn_lut(dev)
    lut_h = lut.cpu().numpy()
    dets, counts = _synth_dets(rng, fmt, len(sizes), 6, sizes, in_size)
    uni = torch.from_numpy(np.stack([host[0]] * len(sizes))).to(dev)
    rag = RaggedFrames.from_list(host, dev)
    rag_same = RaggedFrames.from_list([host[0]] * len(sizes), dev)
    results = {}
    for tag, frames, fsizes, fhost in [("uniform", uni, [sizes[0]] * len(sizes), [host[0]] * len(sizes)),
                                       ("ragged", rag, sizes, host), ("ragged_same", rag_same, [sizes[0]] * len(sizes),
                                                                       [host[0]] * len(sizes))]:
        plain = _device_crops(lib, dev, dets, counts, frames, in_size, fmt, thr, False)
        got = _device_crops(lib, dev, dets, counts, frames, in_size, fmt, thr, True)
        n = got["n"]
        assert n == plain["n"] > 0, tag
        assert _bits(got["items"]).tobytes() == _bits(plain["items"]).tobytes(), tag
        assert _bits(got["info"]).tobytes() == _bits(plain["info"]).tobytes(), tag
        emu = A.emulate_crops(dets, counts, fsizes, in_size, fmt, thr, 0.12)
        for k in ("items", "info", "lmarks", "M", "flags"):
            assert _bits(got[k]).tobytes() == _bits(emu[k]).tobytes(), (tag, k)
        deg = got["flags"] == A.DEGENERATE
        assert deg.any() and (~deg).any(), tag
        D = got["dev"]
        u8 = A.warp_u8(frames, D["M"], D["info"], D["flags"], D["items"], n)
        u8h = u8.cpu().numpy()
        want = A.emulate_warp(fhost, got["M"], got["info"], got["flags"], got["items"])
        assert np.array_equal(u8h, want), tag
        for C in (3, 4):
            f32 = torch.full((n, 112, 112, C), 7.0, dtype=torch.float32, device=dev)
            A.warp(frames, D["M"], D["info"], D["flags"], D["items"], n, out_f32=f32, lut=lut)
            f = f32.cpu().numpy()
            assert _bits(f[..., :3]).tobytes() == _bits(lut_h[u8h]).tobytes(), (tag, C)
            if C == 4:
                assert (f[..., 3] == 0).all()
        # degenerate faces: the box crop the resize kernels make of the same item
        box = torch.zeros((n, 112, 112, 4), dtype=torch.float32, device=dev)
        crops_to_input(frames, D["items"], n, box, lut)
        f32 = torch.zeros((n, 112, 112, 4), dtype=torch.float32, device=dev)
        A.warp(frames, D["M"], D["info"], D["flags"], D["items"], n, out_f32=f32, lut=lut)
        idx = torch.from_numpy(np.nonzero(deg)[0]).to(dev)
        assert torch.equal(f32[idx].view(torch.int32), box[idx].view(torch.int32)), tag
        if tag != "uniform":
            boxu8 = torch.zeros((n, 112, 112, 3), dtype=torch.uint8, device=dev)
            resize_ragged(frames, D["items"], n, boxu8, None, pad_value=0)
            assert torch.equal(u8[idx], boxu8[idx]), tag
        results[tag] = (got, u8h)
    a, b = results["uniform"], results["ragged_same"]
    for k in ("items", "info", "lmarks", "M", "flags"):
        assert _bits(a[0][k]).tobytes() == _bits(b[0][k]).tobytes(), k
    assert np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [FMT_BLAZE, FMT_YOLO])
def test_crops_carry_the_slot_across_chunks_of_256_frames(lib, dev, fmt):
    """300 ragged frames: the kernel walks them in two chunks of 256 and carries the face count from one to the next.  items /
    info (plain and aligned), lmarks / M / flags and n_faces equal the host emulator's bit for bit; with max_faces below the
    count n_faces still reports every face and the rows up to the cap are the same."""
    from face_detection_and_recognition_amd.frames import RaggedFrames
    rng = np.random.default_rng(40 + fmt)
    in_size = (256, 256) if fmt == FMT_BLAZE else (640, 640)
    thr = 0.7 if fmt == FMT_BLAZE else 0.4
    B, cap = 300, 512
    sizes = [[(40, 64), (33, 47), (64, 40)][i % 3] for i in range(B)]
    frames = RaggedFrames.from_list([np.zeros((h, w, 3), np.uint8) for h, w in sizes], dev)
    dets, counts = _synth_dets(rng, fmt, B, 2, sizes, in_size)
    emu = A.emulate_crops(dets, counts, sizes, in_size, fmt, thr, 0.12, max_faces=cap)
    n = emu["info"].shape[0]
    first = int((emu["info"][:, 0] < 256).sum())
    assert 0 < first < n < cap, (first, n)                       # faces on both sides of the chunk boundary, none cut
    for k, want in [(cap, emu), (first + (n - first) // 2, None)]:
        want = want or A.emulate_crops(dets, counts, sizes, in_size, fmt, thr, 0.12, max_faces=k)
        assert want["info"].shape[0] == min(n, k)
        plain = _device_crops(lib, dev, dets, counts, frames, in_size, fmt, thr, False, cap=k)
        got = _device_crops(lib, dev, dets, counts, frames, in_size, fmt, thr, True, cap=k)
        assert plain["n"] == got["n"] == n, k                    # the true count, above the cap too
        for key in ("items", "info"):
            assert _bits(plain[key]).tobytes() == _bits(want[key]).tobytes(), (k, key)
        for key in ("items", "info", "lmarks", "M", "flags"):
            assert _bits(got[key]).tobytes() == _bits(want[key]).tobytes(), (k, key)


@pytest.mark.gpu
def test_warp_commutes_with_a_90_degree_rotation_of_the_frame(lib, dev):
    """warp(rot90(frame), rot90(landmarks)) equals warp(frame, landmarks) within 1 level, faces partly outside included."""
    rng = np.random.default_rng(21)
    H, W = 300, 420
    base = rng.integers(0, 256, (H // 10 + 1, W // 10 + 1, 3)).astype(np.float64)
    frame = np.clip(np.kron(base, np.ones((10, 10, 1)))[:H, :W] + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    rot = np.ascontiguousarray(np.rot90(frame))        # rot[i, j] = frame[j, W - 1 - i]: (x, y) -> (y, W - 1 - x)
    lms, lms_r = [], []
    for k in range(16):
        M0 = similarity(rng.uniform(-0.6, 0.6), rng.uniform(0.4, 1.6), *rng.uniform(-150, 60, 2))
        lm = np.round(lmarks_for(M0, FMT_YOLO) * 4) / 4               # quarter pixels: exact after the rotation
        lr = lm.copy()
        lr[0::2], lr[1::2] = lm[1::2], (W - 1) - lm[0::2]
        lms.append(lm)
        lms_r.append(lr)
    M, fl = A.emulate_estimate(np.stack(lms), FMT_YOLO)
    Mr, flr = A.emulate_estimate(np.stack(lms_r), FMT_YOLO)
    assert (fl == 0).all() and (flr == 0).all()
    info, _, items = _faces(M, np.zeros(len(M), np.int64))

    def dwarp(fr, MM):
        t = torch.from_numpy(fr[None]).to(dev)
        return A.warp_u8(t, torch.from_numpy(MM).to(dev), torch.from_numpy(info).to(dev), torch.from_numpy(fl).to(dev),
                         torch.from_numpy(items).to(dev), len(MM)).cpu().numpy()
    a, b = dwarp(frame, M), dwarp(rot, Mr)
    d = np.abs(a.astype(np.int32) - b)
    assert d.max() <= 1, d.max()
    assert (a == 0).any()                               # some faces reach outside the frame


def _pipelines(dev, kind):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    if kind == "blazeface":
        det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    else:
        det = W.build_yolo_detector(dev, W.make_frames(4, dev, seed=32), "yolov5n", cand_per_frame=80)
    emb = W.build_embedder(dev)
    return det, emb


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["blazeface", "yolov5n"])
def test_pipeline_align_embeddings_match_the_oracle_on_the_aligned_faces(dev, kind):
    """FacePipeline(align=True): step, step_overlapped and a ragged batch give the same faces; the embeddings are within
    1e-4 of oracle/mobilefacenet_ref.py run on the device's own u8 aligned faces; align=False is bit-identical to a
    pipeline built without the argument."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.frames import RaggedFrames
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    from oracle import image_ref, mobilefacenet_ref
    det, emb = _pipelines(dev, kind)
    frames = W.make_frames(4, dev, seed=7)
    cap = dict(max_faces_per_frame=256 if kind == "yolov5n" else 8)
    pa = FacePipeline(det, emb, None, tau=0.0, align=True, **cap)
    res = pa.step(frames)
    n = res["n_faces"]
    assert n > 0 and res["lmarks"].shape == (n, 10) and res["align_M"].shape == (n, 6) and res["align_flags"].shape == (n,)
    faces = A.warp_u8(frames, res["align_M"], res["info"], res["align_flags"], res["items"], n).cpu().numpy()
    sd = {k: v.detach().cpu() for k, v in emb.state_dict().items()}
    x = image_ref.mfn_lut()[faces]
    with torch.no_grad():
        want = mobilefacenet_ref.forward(sd, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))).numpy()
    err = float(np.abs(res["emb"].cpu().numpy() - want).max())
    assert err < 1e-4, err
    # the box-crop pipeline finds the same faces; its embeddings differ (the inputs do)
    base = FacePipeline(det, emb, None, tau=0.0, **cap).step(frames)
    assert base["n_faces"] == n and torch.equal(base["info"], res["info"]) and torch.equal(base["items"], res["items"])
    assert not torch.equal(base["emb"], res["emb"])
    # step_overlapped
    first = pa.step_overlapped(frames)
    assert first is None
    ov = pa.flush()
    assert ov["n_faces"] == n and torch.equal(ov["emb"], res["emb"]) and torch.equal(ov["align_M"], res["align_M"])
    # ragged: the same frames packed
    rg = pa.step(RaggedFrames.from_list(list(frames), dev))
    assert rg["n_faces"] == n and torch.equal(rg["align_M"], res["align_M"]) and torch.equal(rg["lmarks"], res["lmarks"])
    assert float((rg["emb"] - res["emb"]).abs().max()) == 0.0
    # align=False: bit-identical to a pipeline built without the argument
    off = FacePipeline(det, emb, None, tau=0.0, align=False, **cap).step(frames)
    assert set(off) == set(base) and "lmarks" not in off
    for k in ("info", "items", "emb"):
        assert torch.equal(off[k].view(torch.int32), base[k].view(torch.int32)), k


@pytest.mark.gpu
def test_driver_saves_aligned_faces(dev, tmp_path):
    """extract_face_feat_conf_area_list(align=True, save_face=True): 112 x 112 JPEGs that Pillow decodes, under the same
    names; the features are those of FacePipeline(align=True)."""
    from PIL import Image
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.face_extraction import extract_faces_from_dataset as X
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    det, emb = _pipelines(dev, "blazeface")
    pipe = FacePipeline(det, emb, None, tau=0.0)
    frames = W.make_frames(4, dev, seed=7)
    recs = X.extract_face_feat_conf_area_list(pipe, frames, save_face=True, align=True)
    assert not pipe.align
    ref = FacePipeline(det, emb, None, tau=0.0, align=True).step(frames)
    feats = [f for r in recs for f in r.feats]
    assert len(feats) == ref["n_faces"] > 0
    assert np.array_equal(np.stack(feats), ref["emb"].cpu().numpy())
    n = 0
    for r in recs:
        assert len(r.face_jpegs) == len(r.confs)
        for data in r.face_jpegs:
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.size == (112, 112)
            n += 1
    assert n == ref["n_faces"]
    total = X.save_extracted_faces(recs, "vid0", "person_a", str(tmp_path / "feats"), 512, {"person_a": 0}, save_face=True,
                                   faces_save_dir=str(tmp_path / "faces"))
    assert total == n and len(os.listdir(tmp_path / "faces")) >= 1
