"""The evaluation driver on the GPU: detector rows -> boxes in frame pixels for the three row formats against the host path
(modules/utils/inference.py / image.py scale_coords), and eval_face_detector.main end to end on synthetic JPEGs.

Tolerance of the boxes: 1e-3 px -- the host path keeps fp32 rows (coordinates up to ~1 024, ulp 1.2e-4) through a handful of
operations, the device path works in fp64."""
import argparse
import copy
import json

import numpy as np
import pytest
import torch

import mtcnn_cases as C
from face_detection_and_recognition_amd import workload as W
from face_detection_and_recognition_amd.eval import eval_face_detector as drv
from face_detection_and_recognition_amd.evaluation import dets_to_frame_boxes
from face_detection_and_recognition_amd.frames import RaggedFrames
from face_detection_and_recognition_amd.modules.blazeface.model import _REORDER
from face_detection_and_recognition_amd.modules.mtcnn.model import MTCNNFastModel
from face_detection_and_recognition_amd.modules.utils.image import scale_coords
from face_detection_and_recognition_amd.modules.utils.inference import get_dets_bboxes_confs_lmarks_areas
from face_detection_and_recognition_amd.modules.utils.jpeg import imwrite

pytestmark = pytest.mark.gpu
BOX_TOL = 1e-3


@pytest.fixture(scope="module")
def yolo(dev):
    """YOLOv5n-face with the project's synthetic weights, built by the driver's own loader."""
    args = argparse.Namespace(model="synthetic", model_type="yolov5_face", variant="yolov5n", input_size=None)
    return drv.load_detector(args, dev)


def mixed_frames(dev, seed=1234):
    """Four frames, two sizes; the larger two are among the frames the synthetic detector's scores were calibrated on."""
    a, b = W.make_frames(2, dev, seed=seed), W.make_frames(2, dev, seed=22, h=480, w=640)
    return [a[0], b[0], a[1], b[1]]


def normalised_rows(det, rows, hw):
    """A frame's raw rows as the detector's __call__ returns them: (x1, y1, x2, y2, ..., conf) normalised by the input size."""
    fmt = getattr(det, "dets_fmt", 0)
    if fmt == 0:
        return rows[:, _REORDER].copy(), det.input_size
    if fmt == 1:
        iw, ih = det.input_size
        out = rows[:, :5].copy()
        out[:, :4] = out[:, :4] / np.array([iw, ih, iw, ih])
        return out, det.input_size
    h, w = hw
    out = rows.copy()
    out[:, :14] /= np.asarray([w, h] * 7, np.float32)
    return out, (w, h)


def check_against_host(det, frames, dev):
    rf = RaggedFrames.from_list(frames, dev)
    out = det.raw_batch(rf)
    dets, counts = out[0], out[1]
    boxes, scores, valid = dets_to_frame_boxes(det, dets, counts, rf.sizes)
    assert boxes.dtype == torch.float64 and boxes.device == dets.device and boxes.shape == dets.shape[:2] + (4,)
    boxes, scores, valid = boxes.cpu().numpy(), scores.cpu().numpy(), valid.cpu().numpy()
    raw, cnt = dets.cpu().numpy(), counts.cpu().numpy()
    assert cnt.sum() > 0, "the synthetic detector found nothing"
    for i, (h, w) in enumerate(rf.sizes):
        n = int(cnt[i])
        assert valid[i].sum() == n and valid[i, :n].all()
        rows, in_size = normalised_rows(det, raw[i, :n], (h, w))
        iw, ih = in_size
        post = get_dets_bboxes_confs_lmarks_areas(rows.copy(), (w, h), in_size, -1e9, -1e9)
        assert len(post.bbox_confs) == n and np.array_equal(post.bbox_confs.astype(np.float64), scores[i, :n])
        coords = rows[:, :4] * np.array([iw, ih, iw, ih])                    # the host path before its .round()
        want = scale_coords((ih, iw), coords, (h, w)) if n else coords
        err = np.abs(boxes[i, :n] - want).max() if n else 0.0
        assert err <= BOX_TOL, (i, err)
    return int(cnt.sum())


def test_frame_boxes_blazeface_back(dev):
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    assert getattr(det, "dets_fmt", 0) == 0
    check_against_host(det, mixed_frames(dev, seed=8), dev)


def test_frame_boxes_yolov5n_face(dev, yolo):
    assert yolo.dets_fmt == 1
    check_against_host(yolo, mixed_frames(dev), dev)


def test_frame_boxes_mtcnn_fast(dev):
    fr, net, kw = C.ragged_mix()
    det = MTCNNFastModel("unused", 0.7, 0.12, min_size=kw["min_face_size"], factor=kw["factor"], thresholds=kw["thresholds"],
                         net=copy.deepcopy(net).to(dev))
    assert det.dets_fmt == 2 and len({f.shape for f in fr}) == 2
    check_against_host(det, [torch.from_numpy(f).to(dev) for f in fr], dev)


def test_driver_end_to_end(dev, yolo, tmp_path, capsys, monkeypatch):
    frames = mixed_frames(dev) + [W.make_frames(1, dev, seed=23, h=300, w=420)[0]]
    pics = tmp_path / "pics" / "0--Synth"
    pics.mkdir(parents=True)
    lines = []
    for k, f in enumerate(frames):
        imwrite(str(pics / f"f{k}.jpg"), f)
        h, w = f.shape[:2]
        lines.append(f"0--Synth/f{k}.jpg")
        if k == 2:
            lines += ["0", "0 0 0 0 0 0 0 0 0 0"]
            continue
        gt = [(w // 8, h // 8, w // 4, h // 3), (w // 2, h // 2, w // 5, h // 5), (5, 7, 20, 24)]
        lines.append(str(len(gt)))
        lines += [" ".join(map(str, g)) + " 0 0 0 0 0 0" for g in gt]
    ann = tmp_path / "gt.txt"
    ann.write_text("\n".join(lines) + "\n")
    out = tmp_path / "out"
    monkeypatch.setattr(drv, "load_detector", lambda args, device: yolo)      # the fixture went through the real loader
    argv = [str(ann), str(tmp_path / "pics"), "--model_type", "yolov5_face", "--mt", "yolov5n", "--model", "synthetic",
            "--batch", "3", "--out", str(out)]
    res = drv.main(argv)
    block = res.summary()
    assert block in capsys.readouterr().out and len(block.split("\n")) == 12
    anns = json.loads((out / "annotations.json").read_text())
    assert len(anns["images"]) == 5 and len(anns["annotations"]) == 12
    rows = json.loads((out / "detections.json").read_text())
    assert rows and 0 < res.matched.shape[2] <= len(rows)

    # every written row = the reference script's clamp arithmetic on the detector's boxes, here in Python integers
    from face_detection_and_recognition_amd.modules.utils.jpeg import imread
    want = []
    for k0 in (0, 3):                                                         # the driver's batches of three
        rf = RaggedFrames.from_list([imread(str(pics / f"f{k}.jpg"), dev) for k in range(k0, min(k0 + 3, len(frames)))], dev)
        o = yolo.raw_batch(rf)
        boxes, scores, valid = dets_to_frame_boxes(yolo, o[0], o[1], rf.sizes)
        for j, (H, Wd) in enumerate(rf.sizes):
            for b, s in zip(boxes[j][valid[j]].cpu().tolist(), scores[j][valid[j]].cpu().tolist()):
                left, top, right, bottom = (int(v) for v in b)
                x, y = max(0, min(left, Wd - 1)), max(0, min(top, H - 1))
                w, h = max(0, min(right - x + 1, Wd - x)), max(0, min(bottom - y + 1, H - y))
                want.append({"image_id": k0 + j, "category_id": 0, "bbox": [x, y, w, h], "score": float(s)})
    assert rows == want

    # scoring the written file reproduces the printed block
    res2 = drv.main([str(ann), str(tmp_path / "pics"), "--dets", str(out / "detections.json"), "--out", str(tmp_path / "out2")])
    assert res2.summary() == block and res2.summary() in capsys.readouterr().out
    assert np.array_equal(res2.precision, res.precision)
