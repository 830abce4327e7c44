"""Drawing on the device (csrc/draw.hip through annotate.draw) against the numpy restatement, byte for byte: every shared case
with guard bytes around the packed buffer, run twice; annotate_step on a real FacePipeline.step result, dense and ragged;
draw_bbox_on_image; the BlazeFace program's -o; the bench tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import draw_cases as DC
from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import annotate as A
from face_detection_and_recognition_amd.frames import RaggedFrames, frame_descs

pytestmark = pytest.mark.gpu
GUARD = 64


def _guarded(host_frames, dense, dev):
    """(buffer with GUARD bytes of 0xA5 before and after the packed frames, the batch as a view into it)."""
    sizes = [f.shape[:2] for f in host_frames]
    offs = np.cumsum([0] + [3 * h * w for h, w in sizes])
    flat = np.concatenate([np.full(GUARD, 0xA5, np.uint8)] + [f.reshape(-1) for f in host_frames] + [np.full(GUARD, 0xA5, np.uint8)])
    buf = torch.from_numpy(flat).to(dev)
    body = buf[GUARD:GUARD + int(offs[-1])]
    if dense:
        return buf, body.view(len(sizes), sizes[0][0], sizes[0][1], 3)
    descs = torch.from_numpy(frame_descs(offs[:-1], sizes).view(np.uint8)).to(dev)
    return buf, RaggedFrames(body, sizes, offs[:-1], descs)


def _unpack(buf, sizes):
    flat = buf.cpu().numpy()
    out, o = [], GUARD
    for h, w in sizes:
        out.append(flat[o:o + 3 * h * w].reshape(h, w, 3))
        o += 3 * h * w
    return flat[:GUARD], out, flat[o:]


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_draw_equals_numpy_guards_hold_and_two_runs_agree(case, dev):
    name, sizes, dense, dl = case
    src, want = DC.frames(case), DC.expected(case)
    runs = []
    for _ in range(2):
        buf, batch = _guarded(src, dense, dev)
        assert A.draw(batch, dl) is batch
        torch.cuda.synchronize()
        runs.append(buf.cpu().numpy())
        before, got, after = _unpack(buf, sizes)
        assert (before == 0xA5).all() and (after == 0xA5).all(), name
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (name, k, np.argwhere((g != w).any(-1))[:5])
        ranges = dl.host()[1]
        for k in np.nonzero(np.diff(ranges) == 0)[0]:
            assert np.array_equal(got[k], src[k]), (name, k)          # a frame without commands
    assert np.array_equal(runs[0], runs[1])


def test_draw_refuses_other_sizes_and_layouts(dev):
    dl = A.DrawList([(20, 20)])
    dl.fill(0, 0, 0, 5, 5)
    with pytest.raises(ValueError):
        A.draw(torch.zeros((1, 20, 21, 3), dtype=torch.uint8, device=dev), dl)
    with pytest.raises(ValueError):
        A.draw(torch.zeros((1, 20, 40, 3), dtype=torch.uint8, device=dev)[:, :, ::2], dl)
    with pytest.raises(ValueError):
        A.draw(torch.zeros((1, 20, 20, 3), dtype=torch.float32, device=dev), dl)


# ---------------------------------------------------------------------------------------------------- a real step result

@pytest.fixture(scope="module")
def stepped(dev):
    """4 frames of 144 x 256, BlazeFace-back and Mobile-FaceNet with synthetic weights, align=True (the result carries
    lmarks), a gallery enrolled from the step's own embeddings (it carries identity)."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.gallery import FaceGallery
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    frames = W.make_frames(4, dev, seed=7, h=144, w=256)
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8, h=144, w=256), cand_per_frame=48, box_px=60.0)
    emb = W.build_embedder(dev)
    first = FacePipeline(det, emb, None, tau=0.0, align=True).step(frames)
    n = first["n_faces"]
    assert n > 0
    gal = FaceGallery(first["emb"][:max(1, n // 2)], torch.arange(max(1, n // 2), dtype=torch.int32), {0: "Ann", 1: "Bo_2"}, dev)
    pipe = FacePipeline(det, emb, None, tau=0.0, align=True, gallery=gal, identify_tau=0.9)
    return pipe, frames


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_annotate_step_equals_numpy(stepped, dev, ragged):
    pipe, frames = stepped
    batch = RaggedFrames.from_list(list(frames), dev) if ragged else frames
    res = pipe.step(batch)
    n = res["n_faces"]
    assert n > 0 and "lmarks" in res and (res["identity"] >= 0).any()
    host = [f.copy() for f in frames.cpu().numpy()]
    sizes = [(144, 256)] * 4
    for cell in (0, 8):
        out = pipe.annotate(batch, res, anonymize=cell)
        dl = A.step_draw_list(res, sizes, pipe.gallery.names, cell)
        assert any("Ann" in c for c in dl.captions) and (dl.host()[0]["kind"] == L.DRAW_RING).sum() >= 4 * n
        want = A.draw_numpy([f.copy() for f in host], dl)
        got = [t.cpu().numpy() for t in (out.to_list() if ragged else out)]
        for k in range(4):
            assert np.array_equal(got[k], want[k]), (cell, k)
        assert any((g != h).any() for g, h in zip(got, host))
        # inplace=False: the input batch is as it was
        now = [t.cpu().numpy() for t in (batch.to_list() if ragged else batch)]
        assert all(np.array_equal(a, b) for a, b in zip(now, host))
        if cell:
            _check_pixelated(res, dl, host, got, cell)
    # inplace=True draws on the batch itself and returns it
    work = RaggedFrames.from_list(list(frames), dev) if ragged else frames.clone()
    assert A.annotate_step(work, res, names=pipe.gallery.names, inplace=True) is work
    got = [t.cpu().numpy() for t in (work.to_list() if ragged else work)]
    want = A.draw_numpy([f.copy() for f in host], A.step_draw_list(res, sizes, pipe.gallery.names, 0))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def _check_pixelated(res, dl, host, got, cell):
    """With anonymize, every pixel of a box that the face's own outline, rings, bar and glyphs do not cover holds its cell's
    mean of the INPUT.  Checked on the cells that meet nothing of another face: neither its box (a second mosaic averages
    again) nor anything drawn for it (an earlier face's caption inside this box is averaged as part of the frame)."""
    cmds = dl.host()[0]
    faces, cover = [], []                                 # per face: (frame, clamped box), mask of what is drawn for it
    for c, (x0, y0, x1, y1) in zip(cmds, A.DrawList.boxes_of(cmds).tolist()):
        f = int(c["frame"])
        if c["kind"] == L.DRAW_MOSAIC:
            faces.append((f, x0, y0, x1, y1))
            cover.append(np.zeros(host[f].shape[:2], bool))
            continue
        mask = np.zeros(host[f].shape[:2], bool)
        mask[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        if c["kind"] == L.DRAW_RECT:                     # the outline only: the rectangle shrunk by (t + 1) / 2 stays free
            s_ = (int(c["arg"]) + 1) // 2
            mask[max(int(c["y0"]) + s_, 0):max(int(c["y1"]) - s_, 0), max(int(c["x0"]) + s_, 0):max(int(c["x1"]) - s_, 0)] = False
        cover[-1] |= mask
    assert len(faces) == res["n_faces"]
    checked = 0
    for i, (f, x0, y0, x1, y1) in enumerate(faces):
        others = [j for j, b in enumerate(faces) if j != i and b[0] == f]
        for cy in range(y0 // cell * cell, y1, cell):
            for cx in range(x0 // cell * cell, x1, cell):
                ax, ay, bx, by = max(cx, x0), max(cy, y0), min(cx + cell, x1), min(cy + cell, y1)
                here = (slice(ay, by), slice(ax, bx))
                if any((ax < faces[j][3] and bx > faces[j][1] and ay < faces[j][4] and by > faces[j][2]) or cover[j][here].any()
                       for j in others):
                    continue
                px = host[f][here].reshape(-1, 3).astype(np.int64)
                mean = (px.sum(0) + len(px) // 2) // len(px)
                free = ~cover[i][here]
                assert (got[f][here][free] == mean).all(), (i, cx, cy)
                checked += int(free.sum())
    assert checked > 0


# ---------------------------------------------------------------------------------------------------- the reference's entry points

def _post(h, w, areas=True, labels=None):
    from face_detection_and_recognition_amd.modules.models.base import PostProcessedDetection
    return PostProcessedDetection(boxes=np.array([[10.0, 30.0, 90.0, 100.0], [60.0, 0.0, w + 5.0, 50.0]]), bbox_confs=np.array([0.91, 0.705], np.float32),
                                  bbox_areas=np.array([0.125, 0.2], np.float32) if areas else None,
                                  bbox_lmarks=np.array([[20.0, 40, 70, 45, 64, 64], [80, 10, 100, 12, 90, 30]]), bbox_labels=labels)


def test_draw_bbox_on_image_numpy_and_tensor_agree(dev):
    from face_detection_and_recognition_amd.modules.utils.image import draw_bbox_on_image
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (120, 150, 3), dtype=np.uint8)
    post = _post(120, 150)
    a = img.copy()
    assert draw_bbox_on_image(a, post) is a                                   # in place, the same array
    t = torch.from_numpy(img).to(dev)
    assert draw_bbox_on_image(t, post) is t
    want = A.draw_numpy([img.copy()], A.post_dets_draw_list(post, 120, 150))[0]
    assert np.array_equal(a, want) and np.array_equal(t.cpu().numpy(), want) and not np.array_equal(want, img)
    b = img.copy()
    draw_bbox_on_image(b, post, line_thickness=3, text_bg_alpha=0.0)
    assert np.array_equal(b, A.draw_numpy([img.copy()], A.post_dets_draw_list(post, 120, 150, 3, 0.0))[0]) and not np.array_equal(a, b)
    assert A.post_dets_draw_list(post, 120, 150).captions == ["0.91_0.12", "0.70_0.20"]
    assert A.post_dets_draw_list(_post(120, 150, False, ["a", "b"]), 120, 150).captions == ["0.91a", "0.70b"]


def test_blazeface_program_writes_the_annotated_image(dev, tmp_path):
    from PIL import Image
    from face_detection_and_recognition_amd import detect_face_blazeface
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import generate_anchors
    from face_detection_and_recognition_amd.modules.utils.inference import load_image
    from face_detection_and_recognition_amd.modules.utils.jpeg import imread
    frames = W.make_frames(8, dev, seed=3)
    det = W.build_detector(dev, frames, cand_per_frame=48)
    wpath = str(tmp_path / "blazefaceback.pth")
    torch.save({k: v.cpu() for k, v in det.net.state_dict().items()}, wpath)
    np.save(str(tmp_path / "anchors.npy"), generate_anchors(True))
    ipath, opath, apath = (str(tmp_path / n) for n in ("frame.jpg", "out.jpg", "anon.jpg"))
    Image.fromarray(frames[0].cpu().numpy()[..., ::-1]).save(ipath, quality=95)
    argv = ["-i", ipath, "--md", wpath, "--mt", "back", "--dt", "0.7", "--at", "0.12", "-d", "hip:0"]
    plain = detect_face_blazeface.main(argv)
    assert not os.path.exists(opath)
    post = detect_face_blazeface.main(argv + ["-o", opath])
    assert len(post.boxes) > 0 and np.array_equal(post.boxes, plain.boxes) and np.array_equal(post.bbox_confs, plain.bbox_confs)
    inp = load_image(ipath)
    out = imread(opath, dev).cpu().numpy()
    assert out.shape == inp.shape == (576, 1024, 3)
    x0, y0, x1, y1 = (int(v) for v in post.boxes[0])
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, 1024), min(y1, 576)
    ring = np.zeros((576, 1024), bool)
    ring[y0:y1, x0:x1] = True
    ring[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False                 # the outline's inner pixel row (thickness 2 here)
    assert (out[ring] != inp[ring]).any()
    red = out[ring].astype(int)
    assert np.median(red[:, 2] - red[:, 0]) > 40               # a red line through 4:2:0 JPEG: half-red chroma is R - B of about 128
    detect_face_blazeface.main(argv + ["-o", apath, "--anonymize", "16"])
    anon = imread(apath, dev).cpu().numpy()
    inner = (slice(y0 + 8, y1 - 8), slice(x0 + 8, x1 - 8))
    assert anon.shape == inp.shape and (anon[inner] != out[inner]).any()


def test_mtcnn_program_writes_the_annotated_image(dev, tmp_path):
    """The program that does not go through inference_img: rows and JSON as before, and the drawn frame in the file."""
    from conftest import GOLDEN
    from face_detection_and_recognition_amd import detect_face_mtcnn
    from face_detection_and_recognition_amd.modules.utils.inference import load_image
    from face_detection_and_recognition_amd.modules.utils.jpeg import imread
    img = os.path.join(GOLDEN, "jpeg", "ref_test2_faces_3.jpg")
    opath = str(tmp_path / "mtcnn.jpg")
    dets = detect_face_mtcnn.main(["-i", img, "--mt", "fast", "--md", "synthetic", "--dt", "0.0", "--at", "0.0", "-o", opath, "--anonymize", "8"])
    assert len(dets) > 0
    inp, out = load_image(img), imread(opath, dev).cpu().numpy()
    assert out.shape == inp.shape
    assert (np.abs(out.astype(int) - inp.astype(int)).max(-1) > 64).sum() > 20      # outline, rings and caption; JPEG noise is a few levels


def test_bench_tool_runs_and_reports(dev):
    tool = os.path.join(ROOT, "tools", "annotate_bench.py")
    r = subprocess.run([sys.executable, tool, "--frames", "8", "--iters", "2", "--rounds", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bench"] == "annotate" and rec["frames"] == 8 and rec["faces"] == 16 and [c["anonymize"] for c in rec["configs"]] == [0, 16]
    for c in rec["configs"]:
        assert 0 < c["draw_us"]["min"] <= c["draw_us"]["median"] <= c["draw_us"]["max"]
        assert 0 < c["tiles"] and 0 < c["tile_bytes"] <= rec["frame_bytes"] and c["draw_over_encode"] > 0 and c["commands"] > 16
    assert rec["configs"][1]["commands"] == rec["configs"][0]["commands"] + 16
    assert 0 < rec["encode_jpeg_batch_ms"]["min"] <= rec["encode_jpeg_batch_ms"]["median"] and rec["jpeg_bytes"] > 0
