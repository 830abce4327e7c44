"""Augmented inference of YOLOv5-face on the device: fp_tta_views against torch on the CPU (content, pad, channel 3, the mirror,
guard regions), fp_yolo_decode_view against fp_yolo_decode un-mapped on the host with torch and against the numpy restatement,
Model.forward(x, augment=True) against the restatement of the reference's three views (tta_cases.restate), the augmented
detector's raw_batch (dense and ragged) against nms_face_device and the oracle's keep set on the 2583 concatenated rows, and
a TiledDetector and a FacePipeline over the augmented detector."""
import numpy as np
import pytest
import torch

import tta_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.frames import RaggedFrames
from face_detection_and_recognition_amd.modules.yolov5_face import (inference_pytorch_model_yolov5_face, nms_face_device, tta)
from face_detection_and_recognition_amd.modules.yolov5_face.model import YOLOV5FaceModel
from face_detection_and_recognition_amd.modules.yolov5_face.yolo import Model
from oracle import yolo_ref

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
GUARD = 1024          # floats in front of, between and behind the view buffers


def _nhwc4(x, dev, fourth=0.0):
    b, _, h, w = x.shape
    c = torch.full((b, h, w, 4), fourth, dtype=torch.float32)
    c[..., :3] = x.permute(0, 2, 3, 1)
    return c.to(dev)


@pytest.mark.parametrize("hw", TC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_kernel_equals_torch_and_stays_in_its_buffers(hw, dev):
    views = tta.tta_views(*hw)[1:]
    n = [TC.B * v[3][0] * v[3][1] * 4 for v in views]
    for x, fourth in ((TC.canvas(*hw, seed=3), 0.0), (TC.column_canvas(*hw), 5.0)):
        canvas = _nhwc4(x, dev, fourth)
        before = canvas.clone()
        buf = torch.full((3 * GUARD + n[0] + n[1],), SENTINEL, dtype=torch.float32, device=dev)
        o0, o1 = GUARD, 2 * GUARD + n[0]
        out = [buf[o0:o0 + n[0]].view(TC.B, *views[0][3], 4), buf[o1:o1 + n[1]].view(TC.B, *views[1][3], 4)]
        tta.fill_views(canvas, out[0], out[1])
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert torch.equal(canvas, before)
        for lo, hi in ((0, o0), (o0 + n[0], o1), (o1 + n[1], len(host))):                  # the guards are untouched
            assert (host[lo:hi] == SENTINEL).all(), (lo, hi)
        want = [t.permute(0, 2, 3, 1).numpy() for t in TC.views_torch(x)[1:]]
        restated = tta.tta_views_numpy(before.cpu().numpy())
        for g, w_, r, v in zip(out, want, restated, views):
            g = g.cpu().numpy()
            (ch, cw), (ph, pw) = v[2], v[3]
            err = float(np.abs(g[:, :ch, :cw, :3] - w_[:, :ch, :cw]).max())
            print(f"views {hw} ratio {v[0]}: max |device - torch| on the content = {err:.3e}")
            assert err <= 1e-6
            pad = np.ones((ph, pw), bool)
            pad[:ch, :cw] = False
            assert (g[:, pad][..., :3] == np.float32(0.447)).all() and (g[..., 3] == 0).all()
            assert np.array_equal(g, r)                                                    # the numpy restatement, bit for bit
        if fourth:      # the column canvas: the mirrored view starts at the canvas's right edge, the other at its left
            g2, g3 = out[0].cpu().numpy(), out[1].cpu().numpy()
            cw2, cw3 = views[0][2][1], views[1][2][1]
            assert g2[0, 0, 0, 0] > 0.8 and g2[0, 0, cw2 - 1, 0] < 0.1 and g3[0, 0, 0, 0] < 0.1 and g3[0, 0, cw3 - 1, 0] > 0.8
            assert (np.diff(g2[0, 0, :cw2, 0]) < 0).all() and (np.diff(g3[0, 0, :cw3, 0]) > 0).all()


@pytest.mark.parametrize("si,flip", [(1.0, False), (0.83, True), (0.67, False)], ids=["1.0", "0.83flip", "0.67"])
def test_decode_view_equals_decode_then_unmap(si, flip, dev, lib):
    det = Model("yolov5n-0.5").model[-1]
    H, W = 96, 160                                        # the input; the heads are those of a 96 x 128 view
    rng = np.random.default_rng(17)
    heads = [torch.from_numpy(rng.normal(0, 2, (TC.B, 96 // s, 128 // s, 48)).astype(np.float32)).to(dev) for s in (8, 16, 32)]
    R = tta.view_rows((96, 128))
    assert R == 756
    ag = det.anchor_grid.view(det.nl, det.na, 2).numpy()
    plain = torch.empty((TC.B, R, 16), dtype=torch.float32, device=dev)
    row = 0
    for lvl, h in enumerate(heads):
        _, ny, nx, _ = h.shape
        anc = (L.C.c_float * 6)(*[float(v) for v in ag[lvl].reshape(-1)])
        L.check(lib.fp_yolo_decode(L.ptr(h), TC.B, ny, nx, 3, float(det.stride[lvl]), anc, L.ptr(plain), R * 16, row,
                                   L.current_stream(dev)), "fp_yolo_decode")
        row += 3 * ny * nx
    want = plain.cpu().clone()
    want[..., :4] /= si                                   # yolo.py:166-170 on the host
    if flip:
        want[..., 0] = W - want[..., 0]
    off, tail = 7, 5
    for mode, ref in (("reference", want.numpy()), ("mapped", tta.unmap_rows_numpy(plain.cpu().numpy(), si, flip, W, "mapped"))):
        z = torch.full((TC.B, off + R + tail, 16), SENTINEL, dtype=torch.float32, device=dev)
        assert tta.decode_view(det.to("cpu"), heads, z, off, si, flip, W, mode) == off + R
        torch.cuda.synchronize()
        got = z.cpu().numpy()
        assert (got[:, :off] == SENTINEL).all() and (got[:, off + R:] == SENTINEL).all()
        assert np.array_equal(got[:, off:off + R].view(np.uint32), ref.view(np.uint32)), (mode, si)
    if si == 1.0:
        assert np.array_equal(want.numpy(), plain.cpu().numpy())


def _model(name, sd, dev):
    m = Model(name)
    m.load_state_dict(sd)
    return m.to(dev)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("hw", TC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", TC.NAMES)
def test_forward_augment_equals_the_restated_reference(name, hw, fuse, dev):
    """Fails on a Model whose forward ignores augment: that returns R1 rows and the heads."""
    sd = TC.state_dict(name, 23, fuse)
    m = _model(name, sd, dev)
    x = TC.canvas(*hw, seed=9)
    z, second = m(x, augment=True)
    torch.cuda.synchronize()
    want, rows = TC.restate(name, sd, x)
    assert rows == tta.tta_rows(*hw) and second is None
    assert z.shape == (TC.B, sum(rows), 16) == tuple(want.shape)
    zz, zr = z.cpu().numpy(), want.numpy()
    e_conf = float(np.abs(zz[..., [4, 15]] - zr[..., [4, 15]]).max())
    print(f"{name} {hw} fused={fuse}: columns 4, 15 max err {e_conf:.3e}")
    assert e_conf < 1e-4
    lo = 0
    for r, si in zip(rows, TC.SCALES):
        a, b = np.delete(zz[:, lo:lo + r], [4, 15], axis=-1), np.delete(zr[:, lo:lo + r], [4, 15], axis=-1)
        err, bound = float(np.abs(a - b).max()), 1e-4 * max(hw) / si
        print(f"{name} {hw} fused={fuse} view {si}: max err {err:.3e} px, bound {bound:.3e}")
        assert err < bound
        lo += r
    # "mapped" changes the landmark columns of views 2 and 3 only, as the numpy restatement says
    zm = m(x, augment=True, landmarks="mapped")[0].cpu().numpy()
    assert np.array_equal(zm[:, :rows[0]], zz[:, :rows[0]]) and np.array_equal(zm[..., [0, 1, 2, 3, 4, 15]], zz[..., [0, 1, 2, 3, 4, 15]])
    lo = rows[0]
    for r, si, fi in zip(rows[1:], TC.SCALES[1:], TC.FLIPS[1:]):
        ref_lm = zz[:, lo:lo + r].copy()
        ref_lm[..., :4] = 0                                                  # only the landmark columns of the restatement are used
        mapped = tta.unmap_rows_numpy(ref_lm, si, fi == 3, hw[1], "mapped")
        assert np.array_equal(zm[:, lo:lo + r, 5:15], mapped[..., 5:15])
        lo += r
    with pytest.raises(ValueError):
        m(x, augment=True, landmarks="fixed")
    # augment=False is the path it was
    z0, h0 = m(x)
    z1, h1 = m(x, augment=False)
    assert torch.equal(z0, z1) and all(torch.equal(a, b) for a, b in zip(h0, h1)) and z0.shape == (TC.B, rows[0], 16)
    assert np.array_equal(z0.cpu().numpy(), zz[:, :rows[0]])                 # and view 1 of the augmented rows is that path's z


@pytest.fixture(scope="module")
def augmented(dev):
    sd, frames = TC.nms_case()
    net = _model("yolov5n", sd, dev)
    return YOLOV5FaceModel(net, 0.4, 0.0, inference_pytorch_model_yolov5_face, TC.NMS_HW[::-1], augment=True), frames


@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_augmented_raw_batch_is_nms_of_the_views_and_the_oracles_keep_set(augmented, kind, dev):
    det, dense = augmented
    if kind == "dense":
        frames = torch.from_numpy(np.stack(dense)).to(dev)
    else:
        frames = RaggedFrames.from_list([torch.from_numpy(f).to(dev) for f in TC.frames_u8([TC.NMS_HW, (96, 160)], 6)], dev)
    out, cnt, over = det.raw_batch(frames)
    assert out.shape == (TC.B, 2048, 16) and cnt.dtype == torch.int32 and over.shape == (TC.B,)
    plan = det.net.last_plan
    assert plan.input is not None and plan.frame_hw is None                  # the fp32 canvas, not the stem that reads u8 frames
    z = det.net.run_views(plan, "mapped").clone()
    assert z.shape == (TC.B, 2583, 16)
    out2, cnt2, keep, over2 = nms_face_device(z, conf_thres=0.4, iou_thres=0.5, max_det=2048)
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert np.array_equal(c, cnt2.cpu().numpy()) and not over.any() and not over2.any() and (c > 0).all()
    zh = z.cpu().numpy()
    kept, idxs = yolo_ref.non_max_suppression_face(zh, 0.4, 0.5)
    for i in range(TC.B):
        assert torch.equal(out[i, :c[i]], out2[i, :c[i]])
        cand = int(((zh[i, :, 4] > 0.4) & (zh[i, :, 4] * zh[i, :, 15] > 0.4)).sum())
        print(f"{kind} image {i}: {cand} candidates, {c[i]} kept, views of the kept rows "
              f"{np.bincount(tta.tta_view_of_rows(idxs[i].numpy(), *TC.NMS_HW), minlength=3).tolist()}")
        assert np.array_equal(keep[i, :c[i]].cpu().numpy(), idxs[i].numpy()) and 0 < c[i] < cand
    if kind == "dense":     # the conditioning was done on the CPU for these frames: the device's rows are the restated rows
        want, _ = TC.restate("yolov5n", TC.nms_case()[0], TC.frame_canvas(dense))
        assert np.abs(zh[..., [4, 15]] - want.numpy()[..., [4, 15]]).max() < 1e-4
    # the same frames without augment: the plan that reads u8 frames, 1008 rows
    plain = YOLOV5FaceModel(det.net, 0.4, 0.0, inference_pytorch_model_yolov5_face, det.input_size)
    p_out, p_cnt, _ = plain.raw_batch(frames)
    assert det.net.last_plan.n_rows == 1008 and p_out.shape == out.shape and plain.augment is False
    # one image through __call__: the reference's landmarks, normalised boxes
    one = det(dense[0])
    assert one.shape[1] == 5 and len(one) == int(c[0]) if kind == "dense" else len(one) > 0


def test_tiled_detector_and_pipeline_over_the_augmented_detector(augmented, dev):
    from face_detection_and_recognition_amd import tiling as T
    from face_detection_and_recognition_amd import workload as Wk
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    det, _ = augmented
    H, W = 96, 160
    frames = Wk.make_frames(TC.B, dev, seed=21, h=H, w=W)
    raw = det.raw_batch(frames)
    d, c = raw[0].clone(), raw[1].clone()
    assert int(c.sum()) > 0
    # tile = the frame, no whole-frame view, no suppression: every row of the augmented detector, mapped to the frame's pixels
    td = T.TiledDetector(det, (W, H), (0, 0), float("inf"), edge_px=0.0, full_frame=False, max_det=2048)
    out, cnt, over = (x.cpu().numpy() for x in td.raw_batch(frames))
    views, start, _ = T.build_views([(H, W)] * TC.B, (W, H), (0, 0), det.input_size, full_frame=False)
    want = T.merge_views_numpy(d.cpu().numpy(), c.cpu().numpy(), views, start, [(H, W)] * TC.B, det.input_size, det.dets_fmt, np.inf,
                               0.0, 2048)
    assert np.array_equal(cnt, want[1]) and cnt.sum() > 0 and (cnt <= c.cpu().numpy()).all()
    for f in range(TC.B):
        lm = out[f, :cnt[f], 4:14]
        assert np.isfinite(lm).all() and (lm >= -W).all() and (lm <= 2 * W).all()
    # and a real tiling runs
    t_out, t_cnt, _ = T.TiledDetector(det, (64, 64), (32, 32), 0.5, edge_px=1.0, max_det=512).raw_batch(frames)
    assert t_out.shape == (TC.B, 512, 16) and int(t_cnt.sum()) > 0
    emb = Wk.build_embedder(dev)
    pipe = FacePipeline(det, emb, None, tau=0.0, max_faces_per_frame=2048, align=True)
    res = pipe.step(frames)
    n = res["n_faces"]
    dets, counts, _ = det.raw_batch(frames)
    assert torch.equal(counts, c) and 0 < n <= int(counts.sum())
    assert int(pipe.crops(frames, dets, counts)[2]) == n
    assert res["lmarks"].shape == (n, 10) and res["emb"].shape == (n, 512)
    lm = res["lmarks"].cpu().numpy()
    assert np.isfinite(lm).all() and (lm >= -W).all() and (lm <= 2 * W).all()
    # the dataset driver's augment=: a plain detector augmented for the call, and left as it was
    from face_detection_and_recognition_amd.face_extraction.extract_faces_from_dataset import extract_face_feat_conf_area_list
    plain = YOLOV5FaceModel(det.net, 0.4, 0.0, inference_pytorch_model_yolov5_face, det.input_size)
    p_pipe = FacePipeline(plain, emb, None, tau=0.0, max_faces_per_frame=2048)
    recs = extract_face_feat_conf_area_list(p_pipe, frames, augment=True)
    assert plain.augment is False and sum(len(r.confs) for r in recs) == n
    assert sum(len(r.confs) for r in extract_face_feat_conf_area_list(p_pipe, frames)) == p_pipe.step(frames)["n_faces"]
    with pytest.raises(ValueError):
        extract_face_feat_conf_area_list(FacePipeline(T.TiledDetector(plain, (64, 64), (32, 32), 0.5), emb, None, tau=0.0), frames, augment=True)
