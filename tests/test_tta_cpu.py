"""Augmented inference of YOLOv5-face on the host (no GPU): the view geometry against the table worked out from the
reference's formulas, the numpy restatement of the view fill against torch (flip, F.interpolate, F.pad), torch's `/= si` as
the fp32 division the kernel makes, the "mapped" landmarks on constructed rows, the exports and refusals of the two new entry
points, the conditioned NMS case, and the command lines."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import tta_cases as TC
from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.yolov5_face import tta
from oracle import yolo_ref


@pytest.mark.parametrize("hw", sorted(TC.TABLE))
def test_view_geometry_is_the_table(hw):
    from face_detection_and_recognition_amd.modules.yolov5_face import tta_views
    views = tta_views(*hw)
    assert [(v[0], v[1]) for v in views] == [(1.0, False), (0.83, True), (0.67, False)]
    assert tuple((v[2], v[3]) for v in views) == TC.TABLE[hw][:3]
    assert tuple(tta.tta_rows(*hw)) == TC.TABLE[hw][3]
    assert tta_views(*hw, gs=32) == views
    # the torch restatement pads to the same sizes
    if hw != (640, 640):
        assert [tuple(x.shape[2:]) for x in TC.views_torch(torch.zeros(1, 3, *hw))] == [v[3] for v in views]


@pytest.mark.parametrize("hw", TC.SHAPES)
def test_numpy_view_fill_agrees_with_torch(hw):
    """Inputs in [0, 1]: two evaluation orders of a convex four-tap blend of values <= 1 differ by fewer than ten fp32
    roundings (6e-7) once the taps' weights agree -- which needs the source coordinate as ONE fma, as torch's CPU kernel
    computes it (a separately rounded product moves the weight by an ulp of the coordinate, 1e-5 at 640 columns)."""
    for x in (TC.canvas(*hw, seed=3), TC.column_canvas(*hw)):
        want = TC.views_torch(x)[1:]
        for c in (3, 4):
            nhwc = np.zeros((TC.B,) + hw + (c,), np.float32)
            nhwc[..., :3] = x.permute(0, 2, 3, 1).numpy()
            if c == 4:
                nhwc[..., 3] = 7.0                                       # whatever channel 3 holds, the views carry 0 there
            got = tta.tta_views_numpy(nhwc)
            for g, w_, v in zip(got, want, tta.tta_views(*hw)[1:]):
                (ch, cw), (ph, pw) = v[2], v[3]
                w_ = w_.permute(0, 2, 3, 1).numpy()
                assert g.shape == (TC.B, ph, pw, c) and g.dtype == np.float32
                assert np.abs(g[:, :ch, :cw, :3] - w_[:, :ch, :cw]).max() <= 1e-6
                pad = np.ones((ph, pw), bool)
                pad[:ch, :cw] = False
                assert (g[:, pad][..., :3] == np.float32(0.447)).all() and (w_[:, pad] == np.float32(0.447)).all()
                if c == 4:
                    assert (g[..., 3] == 0).all()
    # the mirrored view of the column canvas really is mirrored: its first content column shows the canvas's last columns
    h, w = hw
    v2 = tta.tta_views_numpy(TC.column_canvas(*hw).permute(0, 2, 3, 1).numpy())[0]
    cw = tta.tta_views(*hw)[1][2][1]
    assert v2[0, 0, 0, 0] > 0.8 and v2[0, 0, cw - 1, 0] < 0.1


def test_torch_division_by_the_ratio_is_the_fp32_division():
    """yi[..., :4] /= si on a float32 tensor divides by the float nearest si -- what the kernel and the numpy restatement do."""
    x = torch.from_numpy(np.random.default_rng(1).normal(0, 200, 4096).astype(np.float32))
    for si in (0.83, 0.67, 1):
        y = x.clone()
        y /= si
        assert np.array_equal(y.numpy(), x.numpy() / np.float32(si))
        assert np.array_equal(tta.unmap_rows_numpy(x.numpy().reshape(-1, 16), si, False, 128, "reference")[:, :4],
                              y.numpy().reshape(-1, 16)[:, :4])


def test_mapped_landmarks_on_constructed_rows():
    rows = np.arange(32, dtype=np.float32).reshape(2, 16) + 1
    W, si = 160, np.float32(0.83)
    ref = tta.unmap_rows_numpy(rows, 0.83, True, W, "reference")
    assert np.array_equal(ref[:, 4:], rows[:, 4:])                                  # the reference leaves the landmarks alone
    assert np.array_equal(ref[:, 0], np.float32(W) - rows[:, 0] / si) and np.array_equal(ref[:, 1:4], rows[:, 1:4] / si)
    got = tta.unmap_rows_numpy(rows, 0.83, True, W, "mapped")
    assert np.array_equal(got[:, :5], ref[:, :5]) and np.array_equal(got[:, 15], rows[:, 15])
    x = lambda k: np.float32(W) - rows[:, 5 + 2 * k] / si       # noqa: E731
    y = lambda k: rows[:, 6 + 2 * k] / si                       # noqa: E731
    for dst, src in ((0, 1), (1, 0), (2, 2), (3, 4), (4, 3)):                       # eyes and mouth corners swap, the nose stays
        assert np.array_equal(got[:, 5 + 2 * dst], x(src)) and np.array_equal(got[:, 6 + 2 * dst], y(src))
    plain = tta.unmap_rows_numpy(rows, 0.67, False, W, "mapped")                    # no flip: divided only
    assert np.array_equal(plain[:, 5:15], rows[:, 5:15] / np.float32(0.67)) and np.array_equal(plain[:, :4], rows[:, :4] / np.float32(0.67))
    one = tta.unmap_rows_numpy(rows, 1.0, False, W, "mapped")
    assert np.array_equal(one, rows)


def test_view_of_rows():
    from face_detection_and_recognition_amd.modules.yolov5_face import tta_view_of_rows
    idx = np.array([0, 1007, 1008, 2015, 2016, 2582])
    assert tta_view_of_rows(idx, 128, 128).tolist() == [0, 0, 1, 1, 2, 2]
    assert tta_view_of_rows(torch.from_numpy(idx).int(), 128, 128).tolist() == [0, 0, 1, 1, 2, 2]


def test_exports_and_abi(lib):
    assert lib.fp_abi_version() == 15 == L.ABI_VERSION
    for name in ("fp_tta_views", "fp_yolo_decode_view"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    with open(os.path.join(ROOT, "include", "facepath.h")) as f:
        hdr = f.read()
    assert "int fp_tta_views(" in hdr and "int fp_yolo_decode_view(" in hdr and "#define FP_ABI_VERSION 15" in hdr


def test_refusals_before_any_launch(lib):
    """NULL pointers, na != 3 and bad geometry are refused on the host: no device is touched (the pointers are fakes)."""
    p = ctypes.c_void_p(4096)
    views = (L.FpTtaView * 2)(L.FpTtaView(106, 106, 128, 128, 1, 0), L.FpTtaView(85, 85, 96, 96, 0, 0))
    ok = [p, 2, 128, 128, views, p, p, 0.447, None]
    for k in (0, 4, 5, 6):
        a = list(ok)
        a[k] = None
        assert lib.fp_tta_views(*a) == L.FP_ERR_INVALID_ARG, k
    for k, v in ((1, -1), (2, 0), (3, 0)):
        a = list(ok)
        a[k] = v
        assert lib.fp_tta_views(*a) == L.FP_ERR_INVALID_ARG, k
    for bad in (L.FpTtaView(129, 106, 128, 128, 1, 0), L.FpTtaView(0, 106, 128, 128, 1, 0), L.FpTtaView(106, 106, 128, 128, 2, 0),
                L.FpTtaView(106, 106, 96, 128, 1, 0)):
        a = list(ok)
        a[4] = (L.FpTtaView * 2)(bad, views[1])
        assert lib.fp_tta_views(*a) == L.FP_ERR_INVALID_ARG
    a = list(ok)
    a[5] = ctypes.c_void_p(4100)
    assert lib.fp_tta_views(*a) == -5                                                  # FP_ERR_ALIGNMENT
    a = list(ok)
    a[1] = 0
    assert lib.fp_tta_views(*a) == L.FP_OK                                             # nothing to do, nothing launched

    anc = (ctypes.c_float * 6)(4, 5, 8, 10, 13, 16)
    ok = [p, 2, 16, 16, 3, 8.0, anc, p, 2583 * 16, 0, 0.83, 1, 128, 1, None]
    for k in (0, 6, 7):
        a = list(ok)
        a[k] = None
        assert lib.fp_yolo_decode_view(*a) == L.FP_ERR_INVALID_ARG, k
    for k, v in ((4, 2), (4, 4), (2, 0), (3, 0), (10, 0.0), (10, float("nan")), (11, 2), (12, 0), (13, 2), (9, -1)):
        a = list(ok)
        a[k] = v
        assert lib.fp_yolo_decode_view(*a) == L.FP_ERR_INVALID_ARG, (k, v)
    a = list(ok)
    a[1] = 0
    assert lib.fp_yolo_decode_view(*a) == L.FP_OK
    assert lib.fp_yolo_decode(None, 2, 16, 16, 3, 8.0, anc, p, 16, 0, None) == L.FP_ERR_INVALID_ARG      # the old entry is as it was


def test_conditioned_case_splits_the_candidates():
    """The seed of the NMS test: on the restated rows a few hundred of the 2583 rows of each image are candidates, the
    oracle keeps some and suppresses some, and every view contributes candidates."""
    sd, frames = TC.nms_case()
    z, rows = TC.restate("yolov5n", sd, TC.frame_canvas(frames))
    assert rows == [1008, 1008, 567] and z.shape == (TC.B, 2583, 16)
    kept, idxs = yolo_ref.non_max_suppression_face(z.numpy(), 0.4, 0.5)
    for i in range(TC.B):
        cand = int(((z[i, :, 4] > 0.4) & (z[i, :, 4] * z[i, :, 15] > 0.4)).sum())
        assert 100 <= cand <= 600, cand
        assert 0 < len(idxs[i]) < cand, (len(idxs[i]), cand)
        views = tta.tta_view_of_rows(idxs[i].numpy(), *TC.NMS_HW)
        assert set(tta.tta_view_of_rows(np.nonzero((z[i, :, 4] > 0.4).numpy())[0], *TC.NMS_HW).tolist()) == {0, 1, 2}
        assert len(set(views.tolist())) >= 2


def test_model_validates_its_arguments():
    from face_detection_and_recognition_amd.modules.yolov5_face.yolo import Model
    m = Model("yolov5n-0.5")
    with pytest.raises(L.FacepathError):
        m(torch.zeros(1, 3, 128, 128), augment=True)                                   # parameters on the CPU: no fall-back


def test_command_lines_take_augment(capsys):
    from face_detection_and_recognition_amd import detect_face_blazeface, detect_face_mtcnn, detect_face_yolov5_face
    from face_detection_and_recognition_amd.eval import eval_face_detector
    p = detect_face_yolov5_face.build_parser()
    assert p.parse_args(["-i", "x.jpg", "--augment"]).augment is True and "augment" not in vars(p.parse_args(["-i", "x.jpg"]))
    for other in (detect_face_blazeface, detect_face_mtcnn):
        with pytest.raises(SystemExit):
            other.build_parser().parse_args(["-i", "x.jpg", "--augment"])
    capsys.readouterr()
    for mt in ("blazeface", "mtcnn"):
        with pytest.raises(SystemExit) as e:
            eval_face_detector.main(["no_such_ann.txt", "pics", "--model_type", mt, "--model", "synthetic", "--augment"])
        assert e.value.code == 2
        assert "--augment applies to yolov5_face only" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):                                             # yolov5_face: accepted, goes on to the file
        eval_face_detector.main(["no_such_ann.txt", "pics", "--model", "synthetic", "--augment"])


def test_bench_tool_parses_and_counts_bytes():
    spec = importlib.util.spec_from_file_location("tta_bench", os.path.join(ROOT, "tools", "tta_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--small"])
    assert a.small is True and mod.build_parser().parse_args([]).small is False
    # canvas read once + both views written once, 16 bytes per pixel
    assert mod.views_floor_bytes(1, 640, 640) == 16 * (640 * 640 + 544 * 544 + 448 * 448)
    assert mod.views_floor_bytes(2, 128, 128) == 2 * 16 * (128 * 128 + 128 * 128 + 96 * 96)
    assert abs(mod.forward_ratio(640, 640) - 2.2125) < 1e-3
