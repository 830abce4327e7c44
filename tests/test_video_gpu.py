"""Motion-JPEG video on the device: decode_video_batch (fp_jpeg_reconstruct_batch, csrc/jpegbatch.hip) against the per-frame
decode and Pillow, byte for byte; frames without Huffman tables on both entropy paths; VideoWriter -> VideoReader; inference_vid;
the tracker driver's --video."""
import json

import numpy as np
import pytest
import torch

import video_cases as V
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.utils import jpeg as J
from face_detection_and_recognition_amd.modules.utils.video import VideoReader, VideoWriter

pytestmark = pytest.mark.gpu


def _batch(seed, n, w, h, make=V.smooth, qualities=(85,), **kw):
    rng = np.random.default_rng(seed)
    return [V.encode(make(rng, w, h), quality=qualities[i % len(qualities)], **kw) for i in range(n)]


# the shapes where the batching can go wrong (name -> the frames of one video)
CASES = {
    "one-frame": _batch(1, 1, 50, 38, subsampling=2),
    "three-67x45-420": _batch(2, 3, 67, 45, subsampling=2),                # pixels no multiple of 256, frames split workgroups
    "50x38-420": _batch(3, 2, 50, 38, subsampling=2),                      # no multiple of the MCU
    "50x38-422": _batch(4, 2, 50, 38, subsampling=1),
    "50x38-444-noise": _batch(5, 2, 50, 38, make=V.noise, qualities=(100,), subsampling=0),     # the clamps
    "3-wide-420": _batch(6, 3, 3, 9, subsampling=2),                       # chroma plane 2 wide: chroma_sample's replication
    "3-wide-422": _batch(7, 2, 3, 9, subsampling=1),
    "2x5-420": _batch(8, 3, 2, 5, subsampling=2),
    "2x5-444": _batch(9, 2, 2, 5, subsampling=0),
    "gray": _batch(10, 3, 50, 38, gray=True),
    "mixed-quality": _batch(11, 3, 67, 45, qualities=(30, 75, 100), subsampling=2),            # quant tables per frame
    "250x131-420": _batch(12, 2, 250, 131, subsampling=2),
    "restart-420": _batch(13, 2, 50, 38, subsampling=2, restart_marker_blocks=3),
}


def _check(got, datas, dev, bgr):
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.device == dev and got.shape[0] == len(datas)
    got = got.cpu().numpy()
    for i, d in enumerate(datas):
        rgb = V.pil_rgb(d)
        assert np.array_equal(got[i], rgb[..., ::-1] if bgr else rgb), i                       # Pillow
        one = J.decode_jpeg(d, dev, bgr=bgr, orientation=False)
        assert np.array_equal(got[i], one.cpu().numpy()), i                                    # fp_jpeg_reconstruct


@pytest.mark.parametrize("name", sorted(CASES))
def test_batched_kernel_equals_per_frame_and_pillow(dev, name):
    datas = CASES[name]
    for entropy in ("host", "device"):
        for bgr in (True, False):
            _check(J.decode_video_batch(datas, dev, bgr=bgr, entropy=entropy), datas, dev, bgr)


def test_chunks_under_the_workspace_cap(dev):
    datas = _batch(20, 5, 50, 38, qualities=(60, 90), subsampling=2)
    info, _ = J.parse(datas[0])
    per = int(L.load().fp_jpeg_workspace_bytes(info))
    assert per == 64 * 48 + 2 * 32 * 24
    calls = []
    real = J.reconstruct_batch

    def spy(info, coefs, offs, *a, **kw):
        calls.append(len(offs))
        return real(info, coefs, offs, *a, **kw)
    J.reconstruct_batch = spy
    try:
        for entropy in ("host", "device"):
            del calls[:]
            _check(J.decode_video_batch(datas, dev, entropy=entropy, max_ws_bytes=2 * per + 100), datas, dev, True)
            assert calls == [2, 2, 1]
            del calls[:]
            _check(J.decode_video_batch(datas, dev, entropy=entropy, max_ws_bytes=1), datas, dev, True)     # a frame over the cap goes alone
            assert calls == [1] * 5
            del calls[:]
            _check(J.decode_video_batch(datas, dev, entropy=entropy), datas, dev, True)
            assert calls == [5]
    finally:
        J.reconstruct_batch = real
    assert J.VIDEO_WS_BYTES == 64 << 20
    out = torch.zeros((5, 38, 50, 3), dtype=torch.uint8, device=dev)
    assert J.decode_video_batch(datas, dev, out=out) is out
    _check(out, datas, dev, True)
    with pytest.raises(ValueError):
        J.decode_video_batch(datas, dev, out=out[:4])


def test_device_entropy_with_frames_left_to_the_host(dev):
    """Progressive frames are not taken by the device Huffman stage: their coefficients come from the host path's arena, the
    others from the device decoder's, and the reconstruction is cut where the arena changes."""
    rng = np.random.default_rng(22)
    imgs = [V.smooth(rng, 50, 38) for _ in range(5)]
    datas = [V.encode(im, quality=85, subsampling=2, progressive=i in (1, 2)) for i, im in enumerate(imgs)]
    calls = []
    real = J.reconstruct_batch

    def spy(info, coefs, offs, *a, **kw):
        calls.append(len(offs))
        return real(info, coefs, offs, *a, **kw)
    J.reconstruct_batch = spy
    try:
        _check(J.decode_video_batch(datas, dev, entropy="device"), datas, dev, True)
        assert calls == [1, 2, 2]
        del calls[:]
        _check(J.decode_video_batch(datas[1:3], dev, entropy="device"), datas[1:3], dev, True)     # every frame from the host
        assert calls == [2]
    finally:
        J.reconstruct_batch = real
    _check(J.decode_video_batch(datas, dev, entropy="host"), datas, dev, True)


def test_frames_must_share_one_geometry(dev):
    rng = np.random.default_rng(21)
    a, b = V.encode(V.smooth(rng, 48, 40), subsampling=2), V.encode(V.smooth(rng, 40, 48), subsampling=2)
    for entropy in ("host", "device"):
        with pytest.raises(ValueError, match="the frames of a video share one size"):
            J.decode_video_batch([a, b], dev, entropy=entropy)
    with pytest.raises(ValueError, match="the frames of a video share one size"):             # the same size, another sampling
        J.decode_video_batch([a, V.encode(V.smooth(rng, 48, 40), subsampling=1)], dev)
    with pytest.raises(ValueError):
        J.decode_video_batch([], dev)


def test_a_damaged_frame_raises_what_decode_jpeg_batch_raises(dev):
    good = CASES["50x38-420"]
    for bad in (good[1][:300], good[1][:2] + b"\x00" + good[1][3:]):
        for entropy in ("host", "device"):
            with pytest.raises(L.FacepathError) as a:
                J.decode_jpeg_batch([good[0], bad], dev, entropy=entropy)
            with pytest.raises(L.FacepathError) as b:
                J.decode_video_batch([good[0], bad], dev, entropy=entropy)
            assert type(a.value) is type(b.value) and str(a.value) == str(b.value)


def test_frames_without_huffman_tables(dev):
    for name in ("three-67x45-420", "50x38-422", "50x38-444-noise", "gray", "restart-420"):
        full = CASES[name]
        stripped = [V.strip_dht(d)[0] for d in full]
        assert all(len(s) < len(d) and not V.dht_tables(s) for s, d in zip(stripped, full))
        mixed = [stripped[0]] + full[1:]                                   # a stream may carry its tables in some frames only
        for datas in (stripped, mixed):
            for entropy in ("host", "device"):
                got = J.decode_video_batch(datas, dev, bgr=False, entropy=entropy).cpu().numpy()
                for i, d in enumerate(full):
                    assert np.array_equal(got[i], V.pil_rgb(d)) and np.array_equal(got[i], V.pil_rgb(datas[i])), (name, entropy, i)
        one = J.decode_jpeg(stripped[0], dev, bgr=False, entropy="device")
        assert np.array_equal(one.cpu().numpy(), V.pil_rgb(full[0]))


def _clip(dev, n=7, w=64, h=48):
    """n frames with a bright patch that moves two pixels a frame."""
    rng = np.random.default_rng(30)
    base = V.smooth(rng, w, h) // 2 + 40
    frames = np.stack([base] * n)
    for i in range(n):
        frames[i, 10:26, 4 + 2 * i:20 + 2 * i] = 230 - 3 * i
    return torch.from_numpy(np.ascontiguousarray(frames)).to(dev)


def test_file_to_frames(dev, tmp_path):
    frames = _clip(dev)
    path = str(tmp_path / "clip.avi")
    with VideoWriter(path, 25) as w:
        w.write(frames[:3])
        w.write(list(frames[3:]))
    with VideoReader(path) as r:
        assert (r.width, r.height, r.n_frames, r.fps) == (64, 48, 7, 25)
        files = [r.frame_bytes(i) for i in range(7)]
        assert files == J.encode_jpeg_batch(list(frames))                  # the encoder's byte strings
        want = torch.stack([J.decode_jpeg(f, dev) for f in files])
        assert torch.equal(r.read(0, 7, dev), want)
        assert torch.equal(r.read(2, 5, dev, entropy="device"), want[2:5])
        assert torch.equal(r.read(0, None, dev, bgr=False), want.flip(-1))
        half = torch.stack([J.decode_jpeg(f, dev, reduce=2) for f in files])
        assert tuple(half.shape) == (7, 24, 32, 3) and torch.equal(r.read(0, 7, dev, reduce=2), half)
        seen = list(r.batches(3, dev))
        assert [s for s, _ in seen] == [0, 3, 6] and torch.equal(torch.cat([f for _, f in seen]), want)
        for i, f in enumerate(files):
            assert np.array_equal(want[i].cpu().numpy(), V.pil_rgb(f)[..., ::-1])


def _front_detector(dev, calib):
    """BlazeFace-front on the seeded synthetic weights of the entry-point tests, its scores calibrated on the clip."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace, generate_anchors
    from face_detection_and_recognition_amd.modules.blazeface.model import BlazeFaceModel
    from face_detection_and_recognition_amd.synth import synth_state_dict
    net = BlazeFace(back_model=False)
    sd = synth_state_dict(net.state_dict(), 111, residual_gain=0.5)
    for name in ("regressor_8", "regressor_16"):
        sd[name + ".weight"] = sd[name + ".weight"] * 0.05
        b = sd[name + ".bias"] * 0.0
        b.view(-1, 16)[:, 2:4] = 40.0
        sd[name + ".bias"] = b
    for name in ("classifier_8", "classifier_16"):
        sd[name + ".weight"] = sd[name + ".weight"].abs() * 0.5
        sd[name + ".bias"] = sd[name + ".bias"] * 0.0
    net.load_state_dict(sd)
    net = net.to(dev)
    net.set_anchors(generate_anchors(False))
    model = BlazeFaceModel("", 0.7, 0.12, "front", device=str(dev), net=net)
    W.calibrate_scores(model, calib, 24)
    return model


def test_inference_vid(dev, tmp_path):
    from face_detection_and_recognition_amd.modules.utils.inference import inference_img, inference_vid, save_annotated
    frames = _clip(dev, n=5, w=96, h=72)
    src = str(tmp_path / "in.avi")
    with VideoWriter(src, 30) as w:
        w.write(frames)
    det = _front_detector(dev, frames)
    with VideoReader(src) as r:
        decoded = [J.decode_jpeg(r.frame_bytes(i), dev) for i in range(5)]
    want = [inference_img(det, f) for f in decoded]
    assert sum(len(p.boxes) for p in want) > 0
    for batch, entropy in ((2, "host"), (64, "device")):
        got = inference_vid(det, src, batch=batch, entropy=entropy)
        assert len(got) == 5
        for g, p in zip(got, want):
            assert np.array_equal(g.boxes, p.boxes) and np.array_equal(g.bbox_confs, p.bbox_confs)
            assert np.array_equal(g.bbox_lmarks, p.bbox_lmarks) and np.array_equal(g.bbox_areas, p.bbox_areas)
    out = str(tmp_path / "out.avi")
    got = inference_vid(det, src, save=out, batch=3, anonymize=8)
    assert all(np.array_equal(g.boxes, p.boxes) for g, p in zip(got, want))
    with VideoReader(out) as r:
        assert (r.n_frames, r.fps, r.width, r.height) == (5, 30, 96, 72)
        for i in range(5):
            jpg = str(tmp_path / f"drawn_{i}.jpg")
            save_annotated(jpg, decoded[i], want[i], anonymize=8)
            assert r.frame_bytes(i) == open(jpg, "rb").read()
            assert torch.equal(r.read(i, i + 1, dev)[0], J.imread(jpg, dev))
    raw = str(tmp_path / "cam.mjpeg")
    with VideoReader(src) as r, open(raw, "wb") as f:
        f.write(b"".join(r.frame_bytes(i) for i in range(5)))
    assert all(np.array_equal(g.boxes, p.boxes) for g, p in zip(inference_vid(det, raw), want))
    with pytest.raises(ValueError, match="fps"):
        inference_vid(det, raw, save=str(tmp_path / "no_rate.avi"))


def _same_posts(got, want):
    assert len(got) == len(want)
    for g, p in zip(got, want):
        assert np.array_equal(g.boxes, p.boxes) and np.array_equal(g.bbox_confs, p.bbox_confs)
        assert np.array_equal(g.bbox_lmarks, p.bbox_lmarks) and np.array_equal(g.bbox_areas, p.bbox_areas)


def test_inference_vid_yolov5_takes_host_frames(dev, tmp_path):
    """YOLOV5FaceModel.__call__ takes numpy frames only: inference_vid decodes on the net's device and hands it host copies."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.utils.inference import inference_img, inference_vid, save_annotated
    frames = _clip(dev, n=4, w=96, h=72)
    src = str(tmp_path / "in.avi")
    with VideoWriter(src, 30) as w:
        w.write(frames)
    with VideoReader(src) as r:
        decoded = [J.decode_jpeg(r.frame_bytes(i), dev).cpu().numpy() for i in range(4)]
    det = W.build_yolo_detector(dev, torch.from_numpy(np.stack(decoded)).to(dev), "yolov5n-0.5", cand_per_frame=20)
    assert not getattr(det, "accepts_device_frames", False) and not hasattr(det, "predict_batch")
    want = [inference_img(det, f) for f in decoded]
    assert sum(len(p.boxes) for p in want) > 0
    out = str(tmp_path / "out.avi")
    _same_posts(inference_vid(det, src, save=out, batch=3), want)
    with VideoReader(out) as r:
        for i in range(4):
            jpg = str(tmp_path / f"drawn_{i}.jpg")
            save_annotated(jpg, decoded[i], want[i], device=dev)
            assert r.frame_bytes(i) == open(jpg, "rb").read()
    half = [J.decode_jpeg(f, dev, reduce=2).cpu().numpy() for f in _frame_files(src)]       # 48 x 36
    _same_posts(inference_vid(det, src, reduce=2), [inference_img(det, f) for f in half])


def test_inference_vid_tiled_detector(dev, tmp_path):
    """The tiled detector normalises its rows by the frame: inference_vid must post-process them with the frame's size, as
    inference_img does through the wrapper's __call__, not with the inner net's input size."""
    from face_detection_and_recognition_amd.modules.utils.inference import inference_img, inference_vid
    from face_detection_and_recognition_amd.tiling import TiledDetector
    frames = _clip(dev, n=4, w=96, h=72)
    src = str(tmp_path / "in.avi")
    with VideoWriter(src, 30) as w:
        w.write(frames)
    with VideoReader(src) as r:
        decoded = [J.decode_jpeg(r.frame_bytes(i), dev) for i in range(4)]
    det = TiledDetector(_front_detector(dev, frames), (64, 48), (16, 16), 0.5)
    want = [inference_img(det, f) for f in decoded]
    assert sum(len(p.boxes) for p in want) > 0
    for p in want:
        assert (p.boxes[:, [0, 2]] <= 96 + 1).all() and (p.boxes[:, [1, 3]] <= 72 + 1).all()
    det.input_size = det.inner.input_size                                  # as a freshly wrapped detector
    _same_posts(inference_vid(det, src, batch=3), want)


def _frame_files(path):
    with VideoReader(path) as r:
        return [r.frame_bytes(i) for i in range(len(r))]


def test_track_faces_in_a_video_file(dev, tmp_path):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    frames = W.make_frames(6, dev, seed=7, h=131, w=250)
    clip = str(tmp_path / "clip.avi")
    with VideoWriter(clip, 25) as w:
        w.write(frames)
    folder = tmp_path / "frames"
    folder.mkdir()
    with VideoReader(clip) as r:
        for i in range(len(r)):
            (folder / f"frame_{i:06d}.jpg").write_bytes(r.frame_bytes(i))
    common = ["--max_age", "3", "-b", "4", "-d", str(dev)]
    a = TF.main(["--frames", str(folder), "--td", str(tmp_path / "a"), "--mot_out", str(tmp_path / "a.txt")] + common)
    b = TF.main(["--video", clip, "--td", str(tmp_path / "b"), "--mot_out", str(tmp_path / "b.txt"),
                 "--video_out", str(tmp_path / "tracked.avi")] + common)
    assert a == b
    ja, jb = (json.load(open(tmp_path / d / "tracks.json")) for d in "ab")
    assert ja == jb and ja["frames"] == 6
    assert open(tmp_path / "a.txt").read() == open(tmp_path / "b.txt").read()
    for t in ja["tracks"]:
        if t["best_jpg"]:
            assert (tmp_path / "a" / t["best_jpg"]).read_bytes() == (tmp_path / "b" / t["best_jpg"]).read_bytes()
    with VideoReader(str(tmp_path / "tracked.avi")) as r:
        assert (r.n_frames, r.width, r.height, r.fps) == (6, 250, 131, 25)
        drawn = r.read(0, 6, dev)
    assert tuple(drawn.shape) == tuple(frames.shape)
    if ja["tracks"]:                                                       # boxes and captions were drawn on
        with VideoReader(clip) as r:
            assert not torch.equal(drawn, r.read(0, 6, dev))
