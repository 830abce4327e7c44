"""Baseline JPEG encoding of crop batches (csrc/jpegenc.hip, ABI 13; modules/utils/jpeg.py encode_jpeg_batch / encode_crops /
imwrite; the driver's save_face).

Pin: Pillow's save(quality=q, subsampling=s), which is libjpeg-turbo's default compressor -- the stream cv2.imwrite writes.
  CPU:  fp_jpeg_encode_emulate (the device's phases run serially) + fp_jpeg_encode_headers byte-identical to Pillow over sizes
        1 x 1 .. 250 x 17, seven qualities, three subsamplings and six kinds of content; the quality -> DQT mapping for every
        quality; the round trip through the repo's host decoder; the refusals.
  GPU:  encode_jpeg_batch on one mixed batch of the CPU cases; the worst-case output bound on saturated noise at q=100;
        encode_crops on planted rectangles that touch and cross every frame edge; the driver end to end with save_face=True."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.utils import jpeg as J
from oracle import image_ref, jpeg_ref
from test_jpeg import _host_decode

SIZES = [(1, 1), (7, 9), (8, 8), (9, 8), (15, 17), (16, 16), (17, 16), (37, 53), (63, 65), (112, 112), (250, 17),  # (h, w)
         (16, 1), (16, 2), (16, 3), (16, 4), (3, 3), (2, 5)]      # narrow crops: chroma planes 1-3 samples wide
NARROW_SIZES = SIZES[-6:]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
SUBSAMPLINGS = [0, 1, 2]      # Pillow's numbering: 4:4:4, 4:2:2, 4:2:0
KINDS = ["noise", "grey", "zero", "full", "checker", "gradient"]


def _content(kind, h, w, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "grey":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "zero":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, np.uint8)
    y, x = np.indices((h, w))
    if kind == "checker":     # hard black / white: long AC codes and many 0xFF bytes to stuff
        return (((y + x) % 2) * 255).astype(np.uint8)[..., None].repeat(3, 2)
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 7) % 256], -1).astype(np.uint8)


def _pil(rgb, quality=95, subsampling=2):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(b, "JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


def _cases():
    k = 0
    for h, w in SIZES:
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                for kind in KINDS:
                    yield h, w, q, s, kind, k
                    k += 1


def _segments(data):
    """marker -> list of segment payloads, up to the SOS header."""
    out, i = {}, 2
    while True:
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.setdefault(m, []).append(data[i + 4:i + 2 + n])
        if m == 0xDA:
            return out
        i += 2 + n


def test_emulator_and_headers_are_byte_identical_to_pillow():
    """Every (size, quality, subsampling, content) case: headers + emulated scan data + EOI == Pillow's file.  One emulator call
    per (quality, subsampling) batch, so images of every size share a batch as on the device."""
    groups = {}
    for h, w, q, s, kind, k in _cases():
        groups.setdefault((q, s), []).append(_content(kind, h, w, k))
    n = 0
    for (q, s), imgs in groups.items():
        got = J.encode_jpeg_batch_emulate(imgs, quality=q, subsampling=s, bgr=False)
        for img, data in zip(imgs, got):
            assert data == _pil(img, q, s), (img.shape, q, s)
            n += 1
    assert n == len(SIZES) * len(QUALITIES) * len(SUBSAMPLINGS) * len(KINDS)
    # bgr=True reads the pixels as B, G, R (cv2's order)
    img = _content("gradient", 37, 53, 1)
    assert J.encode_jpeg_batch_emulate([img[..., ::-1]], bgr=True)[0] == _pil(img)


def test_quality_to_dqt_matches_pillow_for_every_quality():
    img = np.zeros((8, 8, 3), np.uint8)
    for q in range(1, 101):
        ours = _segments(J.encode_headers(8, 8, q, "4:2:0"))[0xDB]
        assert ours == _segments(_pil(img, q))[0xDB], q
    for s, name in zip(SUBSAMPLINGS, ("4:4:4", "4:2:2", "4:2:0")):
        assert J.encode_headers(17, 9, 95, name) == _pil(np.zeros((9, 17, 3), np.uint8), 95, s)[:L.JPEG_ENC_HEADER_BYTES]


def test_round_trip_through_the_host_decoder(lib):
    """Each encoded file decodes, through fp_jpeg_parse + fp_jpeg_entropy_decode and the oracle's reconstruction, to the pixels
    Pillow decodes from the SAME bytes (which are Pillow's own file of the image too): five mixed cases and every narrow size at
    every subsampling, noise content."""
    cases = [((37, 53), 95, 2, "noise"), ((63, 65), 75, 1, "gradient"), ((250, 17), 50, 0, "checker"), ((1, 1), 100, 2, "full"),
             ((17, 16), 10, 2, "gradient")] + [(hw, 90, s, "noise") for hw in NARROW_SIZES for s in SUBSAMPLINGS]
    for (h, w), q, s, kind in cases:
        img = _content(kind, h, w, 3)
        data = J.encode_jpeg_batch_emulate([img], quality=q, subsampling=s, bgr=False)[0]
        assert data == _pil(img, q, s), (h, w, q, s)
        rc, info, coefs = _host_decode(lib, data)
        assert rc == 0
        np.testing.assert_array_equal(jpeg_ref.reconstruct(info, coefs), jpeg_ref.decode_pil(data), err_msg=str((h, w, q, s)))


def test_refusals(lib):
    src = np.zeros((16 * 16 * 3,), np.uint8)

    def rc(items, q=95, s=2, bgr=0):
        arr = (L.FpJpegEncItem * len(items))(*items)
        ws, ob = ctypes.c_size_t(), ctypes.c_size_t()
        r1 = lib.fp_jpeg_encode_workspace_bytes(arr, len(items), s, ctypes.byref(ws), ctypes.byref(ob))
        out = np.zeros((max(ob.value, 1),), np.uint8)
        offs = (ctypes.c_int64 * (len(items) + 1))()
        r2 = lib.fp_jpeg_encode_emulate(src.ctypes.data, arr, len(items), q, s, bgr, out.ctypes.data, out.size, offs)
        return r1 if r1 else r2

    ok = L.FpJpegEncItem(0, 16, 16, 0, 0, 16, 16)
    assert rc([ok]) == 0
    for x0, y0, x1, y1 in [(3, 3, 3, 9), (3, 3, 9, 3), (9, 3, 3, 9), (3, 9, 9, 3),      # zero-size and inverted
                           (16, 0, 20, 16), (0, 16, 16, 20), (-9, 0, 0, 16), (0, -5, 16, 0)]:   # outside after the clamp
        assert rc([ok, L.FpJpegEncItem(0, 16, 16, x0, y0, x1, y1)]) == -1, (x0, y0, x1, y1)
    assert rc([ok], s=3) == -3 and rc([ok], s=-1) == -3                       # subsampling other than 4:4:4 / 4:2:2 / 4:2:0
    assert rc([ok], q=0) == -1 and rc([ok], q=101) == -1 and rc([ok], bgr=2) == -1
    assert rc([L.FpJpegEncItem(0, 0, 16, 0, 0, 16, 16)]) == -1 and rc([L.FpJpegEncItem(-1, 16, 16, 0, 0, 16, 16)]) == -1
    assert rc([L.FpJpegEncItem(0, 70000, 16, 0, 0, 16, 70000)]) == -3          # a side over 65535
    # a rectangle that crosses the edges is clamped the way the reference slices it
    frame = _content("noise", 16, 16, 5)
    arr = (L.FpJpegEncItem * 1)(L.FpJpegEncItem(0, 16, 16, -4, 10, 9, 40))
    got = J._encode_items(np.ascontiguousarray(frame).reshape(-1), list(arr), 95, 2, False, emulate=True)[0]
    assert got == _pil(frame[10:16, 0:9])
    with pytest.raises(J.JpegUnsupported):
        J.encode_jpeg_batch_emulate([frame], subsampling="4:1:1")
    hdr = (ctypes.c_uint8 * L.JPEG_ENC_HEADER_BYTES)()
    assert lib.fp_jpeg_encode_headers(0, 8, 95, 2, hdr, len(hdr)) == -1
    assert lib.fp_jpeg_encode_headers(8, 8, 95, 2, hdr, len(hdr) - 1) == -2


def test_worst_case_bound_holds_for_the_emulator():
    """Saturated black / white noise at q=100, 4:4:4 (the largest AC coefficients there are): the scan data stays inside
    n_blocks * FP_JPEG_ENC_BYTES_PER_BLOCK."""
    img = np.random.default_rng(9).integers(0, 2, (64, 64, 3), dtype=np.uint8) * 255
    data = J.encode_jpeg_batch_emulate([img], quality=100, subsampling=0, bgr=False)[0]
    assert data == _pil(img, 100, 0)
    blocks = 3 * 8 * 8
    assert len(data) - L.JPEG_ENC_HEADER_BYTES - 2 <= blocks * L.JPEG_ENC_BYTES_PER_BLOCK


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_encode_jpeg_batch_is_byte_identical_to_pillow(dev):
    """All CPU cases of one subsampling and quality in ONE device call each (mixed sizes and contents), RGB and BGR input."""
    groups = {}
    for h, w, q, s, kind, k in _cases():
        groups.setdefault((q, s), []).append(_content(kind, h, w, k))
    for (q, s), imgs in groups.items():
        got = J.encode_jpeg_batch([torch.from_numpy(i).to(dev) for i in imgs], quality=q, subsampling=s, bgr=False)
        for img, data in zip(imgs, got):
            assert data == _pil(img, q, s), (img.shape, q, s)
    imgs = [_content("noise", h, w, 7) for h, w in SIZES]
    got = J.encode_jpeg_batch([torch.from_numpy(np.ascontiguousarray(i[..., ::-1])).to(dev) for i in imgs])
    assert got == [_pil(i) for i in imgs]


@pytest.mark.gpu
def test_encode_worst_case_bound_on_saturated_noise(dev):
    rng = np.random.default_rng(10)
    imgs = [rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255 for h, w in [(64, 64), (112, 112), (37, 53), (8, 8)]]
    imgs.append(rng.integers(0, 256, (96, 80, 3), dtype=np.uint8))
    for s in SUBSAMPLINGS:
        got = J.encode_jpeg_batch([torch.from_numpy(i).to(dev) for i in imgs], quality=100, subsampling=s, bgr=False)
        assert got == [_pil(i, 100, s) for i in imgs]
        mh, mw = (2 if s == 2 else 1), (1 if s == 0 else 2)       # luma blocks per MCU down / across
        blocks = sum(-(-h // (8 * mh)) * -(-w // (8 * mw)) * (mh * mw + 2) for h, w in [i.shape[:2] for i in imgs])
        scan = sum(len(d) - L.JPEG_ENC_HEADER_BYTES - 2 for d in got)
        assert scan <= blocks * L.JPEG_ENC_BYTES_PER_BLOCK


@pytest.mark.gpu
def test_encode_crops_planted_rectangles(dev):
    """fp_resize_item records over a seeded frame batch, rectangles inside, touching and crossing every edge (clamped as the
    reference slices), plus an empty one: each file equals Pillow on frame[y:yh, x:xw][..., ::-1]."""
    B, H, W = 3, 72, 96
    frames = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    rects = [(0, 10, 12, 40, 30), (0, 0, 0, 96, 72), (1, -6, -1, 20, 17), (1, 80, 60, 120, 90), (2, -3, 20, 5, 40),
             (2, 50, -2, 70, 4), (2, 95, 71, 200, 200), (0, 0, 33, 96, 34), (1, 17, 0, 18, 72), (2, 40, 40, 40, 60)]
    items = torch.tensor([[f, x, y, xw - x, yh - y, 0, 0, 112, 112] for f, x, y, xw, yh in rects], dtype=torch.int32, device=dev)
    got = J.encode_crops(frames, items, len(rects))
    fr = frames.cpu().numpy()
    for (f, x, y, xw, yh), data in zip(rects, got):
        x, y, xw, yh = max(x, 0), max(y, 0), min(xw, W), min(yh, H)
        crop = fr[f, y:yh, x:xw]
        if crop.size == 0:
            assert data is None
        else:
            assert data == _pil(crop[..., ::-1]), (f, x, y, xw, yh)
    assert J.encode_crops(frames, items, 0) == []


@pytest.mark.gpu
def test_driver_save_face_end_to_end(dev, tmp_path):
    """FacePipeline.step on the synthetic workload + the driver with save_face=True: the reference's file names under
    faces/<class>/, each file Pillow's encoding of the oracle crop, read back by imread_batch."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.face_extraction import extract_faces_from_dataset as X
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    frames = W.make_frames(6, dev, seed=11)
    det = W.build_detector(dev, W.make_frames(8, dev, seed=12), cand_per_frame=48)
    pipe = FacePipeline(det, W.build_embedder(dev), None)
    recs = X.extract_face_feat_conf_area_list(pipe, frames, frame_nums=list(range(1, 7)), times_sec=[0, 0, 1, 1, 2, 2],
                                              save_face=True)
    plain = X.extract_face_feat_conf_area_list(pipe, frames, frame_nums=list(range(1, 7)))
    assert all(r.face_jpegs == [] for r in plain)                 # the default leaves the records as they were
    faces_dir = os.path.join(str(tmp_path), "faces", "person_a")
    total = X.save_extracted_faces(recs, "img0", "person_a", str(tmp_path / "feats"), 512, {"person_a": 0}, save_face=True,
                                   faces_save_dir=faces_dir)
    assert total > 0
    fr = frames.cpu().numpy()
    expected = {}
    for i, r in enumerate(recs):
        for box, conf, area in zip(r.boxes, r.confs, r.areas):
            crop, _ = image_ref.crop_face(fr[i], box)
            name = f"frame_{r.frame_num}_sec_{r.time_sec}_conf_{str(round(conf, 3)).replace('.', '_')}_area_{area}.jpg"
            expected[name] = _pil(crop[..., ::-1])             # a later face of the same name overwrites, as cv2.imwrite does
    assert sorted(os.listdir(faces_dir)) == sorted(expected)
    for name, data in expected.items():
        assert open(os.path.join(faces_dir, name), "rb").read() == data, name
    paths = [os.path.join(faces_dir, nm) for nm in sorted(expected)]
    back = J.imread_batch(paths, dev)
    for p, img in zip(paths, back if isinstance(back, list) else list(back)):
        pil = np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
        np.testing.assert_array_equal(img.cpu().numpy(), pil)
    # imwrite: cv2.imwrite's argument order and defaults
    J.imwrite(str(tmp_path / "one.jpg"), frames[0, 5:50, 7:70].contiguous())
    assert open(tmp_path / "one.jpg", "rb").read() == _pil(fr[0, 5:50, 7:70][..., ::-1])
