"""Ragged batches (ABI 14): frames of different sizes through letterbox, detect, crop, embed and the dataset driver.

CPU: the C layout and prototypes, RaggedFrames packing and refusals, per-frame geometry, argument refusals of the new
entry points.  GPU: the ragged resize against the oracle and fp_resize_normalize, the detectors, the pipeline and the
driver against the same frames run by size (uniform batches of the same batch size) and one by one."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.frames import RaggedFrames, resize_ragged
from face_detection_and_recognition_amd.pipeline import ragged_scale_coords_params, scale_coords_params
from face_detection_and_recognition_amd.modules.utils.image import letterbox_geometry, letterbox_items

SIZES = [(576, 1024), (1080, 1920), (1650, 1275), (540, 720), (17, 29), (3, 3)]   # H x W; 1650 x 1275: portrait
JPEGS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jp*g")))


# ---------------------------------------------------------------------------------------------- CPU

def test_frame_desc_layout_and_prototypes_match_a_c_compiler(lib, tmp_path):
    """fp_frame_desc as a C99 compiler lays it out equals the ctypes mirror; the new prototypes have the argument types
    _lib.py binds (a C file assigns each symbol to a pointer of the expected type with -Werror)."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['printf("fp_frame_desc %zu\\n", sizeof(fp_frame_desc));']
    for fname, _ in L.FpFrameDesc._fields_:
        lines.append('printf("fp_frame_desc.%s %%zu\\n", offsetof(fp_frame_desc, %s));' % (fname, fname))
    src = tmp_path / "ragged.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "facepath.h"
int main(void) {
  int (*resize)(const uint8_t*, size_t, const fp_frame_desc*, int, const fp_resize_item*, int, void*, int, int, int, int,
                const float*, int, int, void*) = fp_resize_ragged;
  int (*crops)(const float*, const int32_t*, int, int, int, int, int, int, const fp_frame_desc*, const float*, float, float,
               int, int, int, int, int, int, int, fp_resize_item*, float*, int32_t*, void*) = fp_dets_to_crops_ragged;
  /*PRINTS*/
  printf("consts %d %d %d %d %d\\n", FP_FRAME_MIN_W, FP_FRAME_MAX_W, FP_FRAME_MAX_H, FP_RAGGED_U8, FP_RAGGED_F32_LUT);
  printf("abi %d %d\\n", FP_ABI_VERSION, fp_abi_version());
  return (resize == NULL) + (crops == NULL);
}
""".replace("/*PRINTS*/", "\n  ".join(lines)))
    libdir = os.path.dirname(L.LIB_PATH)
    exe = tmp_path / "ragged"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-L", libdir, "-lfacepath", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert int(got["fp_frame_desc"][0]) == ctypes.sizeof(L.FpFrameDesc) == 16
    for fname, _ in L.FpFrameDesc._fields_:
        assert int(got[f"fp_frame_desc.{fname}"][0]) == getattr(L.FpFrameDesc, fname).offset
    assert [int(v) for v in got["consts"]] == [L.FRAME_MIN_W, L.FRAME_MAX_W, L.FRAME_MAX_H, L.RAGGED_U8, L.RAGGED_F32_LUT]
    assert [int(v) for v in got["abi"]] == [L.ABI_VERSION, L.ABI_VERSION] == [15, 15]
    assert len(L.SIGNATURES["fp_resize_ragged"][1]) == 15 and len(L.SIGNATURES["fp_dets_to_crops_ragged"][1]) == 23


def _host_frames(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def test_ragged_frames_pack_and_round_trip():
    fr = _host_frames(SIZES)
    rf = RaggedFrames.from_list(fr[:3] + [torch.from_numpy(f) for f in fr[3:]], "cpu")
    assert len(rf) == len(SIZES) and rf.sizes == SIZES
    want_off = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in SIZES])[:-1]]).tolist()
    assert rf.offsets == want_off and rf.data.numel() == sum(h * w * 3 for h, w in SIZES)
    d = (L.FpFrameDesc * len(rf)).from_buffer_copy(rf.descs.numpy().tobytes())
    assert [(x.off, x.h, x.w) for x in d] == [(o, h, w) for o, (h, w) in zip(want_off, SIZES)]
    for f, g in zip(fr, rf.to_list()):
        np.testing.assert_array_equal(g.numpy(), f)


@pytest.mark.parametrize("bad,err", [([], "empty"), ([np.zeros((4, 4, 3), np.float32)], "dtype"),
                                     ([torch.zeros((4, 4, 3), dtype=torch.int16)], "dtype"),
                                     ([np.zeros((4, 4), np.uint8)], "shape"), ([np.zeros((4, 4, 4), np.uint8)], "shape"),
                                     ([np.zeros((4, 4, 1), np.uint8)], "shape"), ([np.zeros((4, 2, 3), np.uint8)], "2"),
                                     ([np.zeros((0, 8, 3), np.uint8)], "0 x 8"), ([np.zeros((1, 32768, 3), np.uint8)], "32768"),
                                     ([np.zeros((65536, 3, 3), np.uint8)], "65536"), ([[[1, 2, 3]]], "list")])
def test_ragged_frames_refusals(bad, err):
    with pytest.raises(ValueError, match=err):
        RaggedFrames.from_list(bad, "cpu")


def test_per_frame_geometry_equals_each_frame_alone():
    """The letterbox items and scale_coords values of a mixed batch are, row by row, those of each frame alone."""
    rf = RaggedFrames.from_list(_host_frames(SIZES), "cpu")
    for in_size in [(256, 256), (128, 128), (640, 640), (640, 480)]:
        items = letterbox_items(rf, in_size).numpy()
        geo = ragged_scale_coords_params(in_size, rf.sizes)
        assert geo.dtype == np.float32 and geo.shape == (len(SIZES), 3)
        for i, (h, w) in enumerate(SIZES):
            sw, sh, left, top = letterbox_geometry(w, h, *in_size)
            assert items[i].tolist() == [i, 0, 0, w, h, left, top, sw, sh]
            assert geo[i].tobytes() == np.array(scale_coords_params(in_size, (w, h)), np.float32).tobytes()


def test_ragged_entry_points_refuse_bad_arguments(lib):
    """Every refusal happens on the host before a launch (status -1 / -5, never the launch status -4); no GPU needed.
    The pointers are never dereferenced: each call below is refused."""
    P = ctypes.c_void_p
    fake, lut = P(0x10000), P(0x20000)

    def rs(**kw):
        a = dict(frames=fake, nbytes=1 << 20, descs=fake, n_frames=2, items=fake, n_items=3, canvas=fake, ch=256, cw=256,
                 cc=3, mode=L.RAGGED_U8, lut=None, pad=125, swap=0)
        a.update(kw)
        return lib.fp_resize_ragged(a["frames"], a["nbytes"], a["descs"], a["n_frames"], a["items"], a["n_items"], a["canvas"],
                                    a["ch"], a["cw"], a["cc"], a["mode"], a["lut"], a["pad"], a["swap"], None)
    bad = [dict(frames=None), dict(descs=None), dict(items=None), dict(canvas=None), dict(nbytes=8), dict(n_frames=0),
           dict(n_items=-1), dict(ch=0), dict(ch=65536), dict(cw=0), dict(cw=4097), dict(pad=-1), dict(pad=256), dict(swap=2),
           dict(cc=4), dict(cc=1), dict(swap=1), dict(mode=2), dict(mode=-1),
           dict(mode=L.RAGGED_F32_LUT, cc=3, lut=lut), dict(mode=L.RAGGED_F32_LUT, cc=4, lut=None)]
    for kw in bad:
        assert rs(**kw) == -1, kw
    assert rs(mode=L.RAGGED_F32_LUT, cc=4, lut=lut, canvas=P(0x10004)) == -5        # fp32 canvas not 16-byte aligned
    assert rs(n_items=0) == 0                                                      # nothing to do: no launch

    def cr(**kw):
        a = dict(dets=fake, counts=fake, B=4, max_dets=16, row=17, fmt=0, in_w=256, in_h=256, descs=fake, geom=fake,
                 items=fake, info=fake, nf=fake, dst_w=112, dst_h=112, max_faces=32)
        a.update(kw)
        return lib.fp_dets_to_crops_ragged(a["dets"], a["counts"], a["B"], a["max_dets"], a["row"], a["fmt"], a["in_w"],
                                           a["in_h"], a["descs"], a["geom"], 0.7, 0.12, -6, -1, 4, 5, a["dst_w"], a["dst_h"],
                                           a["max_faces"], a["items"], a["info"], a["nf"], None)
    bad = [dict(dets=None), dict(counts=None), dict(descs=None), dict(geom=None), dict(items=None), dict(info=None),
           dict(nf=None), dict(B=-1), dict(max_dets=0), dict(max_faces=0), dict(in_w=0), dict(in_h=-3), dict(dst_w=0),
           dict(dst_h=0), dict(row=16), dict(fmt=1, row=4), dict(fmt=2), dict(fmt=-1)]
    for kw in bad:
        assert cr(**kw) == -1, kw


# ---------------------------------------------------------------------------------------------- GPU

def _frames(sizes, dev, seed=5):
    """Synthetic frames of the bench's kind (textured patches on a flat background) for sizes a detector sees, noise for tiny ones."""
    from face_detection_and_recognition_amd import workload as W
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(sizes):
        if h >= 64 and w >= 64:
            out.append(W.make_frames(1, dev, seed=seed * 100 + k, h=h, w=w)[0])
        else:
            out.append(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.gpu
@pytest.mark.parametrize("canvas", [(256, 256), (128, 128), (640, 640), (97, 130)])   # (h, w); 130: rows not dword-aligned
def test_ragged_u8_canvas_matches_oracle_and_fp32_mode_matches_resize_normalize(dev, lib, canvas):
    from oracle import image_ref
    ch, cw = canvas
    fr = _frames(SIZES, dev)
    rf = RaggedFrames.from_list(fr, dev)
    u8 = torch.full((len(fr), ch, cw, 3), 7, dtype=torch.uint8, device=dev)
    resize_ragged(rf, letterbox_items(rf, (cw, ch)), len(fr), u8)
    torch.cuda.synchronize()
    for i, f in enumerate(fr):
        want = image_ref.pad_resize_image(f.cpu().numpy(), (cw, ch))
        np.testing.assert_array_equal(u8[i].cpu().numpy(), want, err_msg=str(SIZES[i]))
    # fp32 + LUT: letterbox items and crop items (edge-crossing and out-of-frame rectangles are clamped in the kernel)
    rng = np.random.default_rng(ch)
    lut = torch.from_numpy(rng.standard_normal(256).astype(np.float32)).to(dev)
    rows = letterbox_items(rf, (cw, ch)).cpu().tolist()
    for i, (h, w) in enumerate(SIZES):
        for _ in range(3):
            sx, sy = int(rng.integers(-w // 4, w)), int(rng.integers(-h // 4, h))
            rows.append([i, sx, sy, int(rng.integers(1, w + 4)), int(rng.integers(1, h + 4)),
                         int(rng.integers(0, cw // 4)), int(rng.integers(0, ch // 4)), int(rng.integers(1, cw)), int(rng.integers(1, ch))])
    rows.append([len(fr), 0, 0, 5, 5, 0, 0, 9, 9])      # src_image outside the batch: pad colour
    items = torch.tensor(rows, dtype=torch.int32, device=dev)
    for swap in (0, 1):
        got = torch.empty((len(rows), ch, cw, 4), dtype=torch.float32, device=dev)
        resize_ragged(rf, items, len(rows), got, lut, pad_value=33, swap_rb=swap)
        for k, row in enumerate(rows):
            src = min(row[0], len(fr) - 1)
            one = torch.tensor([[0] + row[1:]], dtype=torch.int32, device=dev)
            want = torch.empty((1, ch, cw, 4), dtype=torch.float32, device=dev)
            h, w = SIZES[src]
            n_frames = 1 if row[0] < len(fr) else 0
            if n_frames:
                L.check(lib.fp_resize_normalize(L.ptr(fr[src]), 1, h, w, L.ptr(one), 1, L.ptr(want), ch, cw, 4, L.ptr(lut), 33,
                                                swap, L.current_stream(dev)), "fp_resize_normalize")
            else:
                want[..., :3] = lut[33]
                want[..., 3] = 0
            assert torch.equal(_bits(got[k:k + 1]), _bits(want)), (k, row, swap)


def _blazeface(dev, back):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace, generate_anchors
    from face_detection_and_recognition_amd.modules.blazeface.model import BlazeFaceModel
    from face_detection_and_recognition_amd.synth import synth_state_dict
    if back:
        return W.build_detector(dev, W.make_frames(8, dev, seed=12), cand_per_frame=48)
    net = BlazeFace(False)
    net.load_state_dict(synth_state_dict(net.state_dict(), 100, residual_gain=0.5))
    net = net.to(dev)
    net.set_anchors(generate_anchors(False))
    model = BlazeFaceModel("", 0.7, 0.12, "front", device=str(dev), net=net)
    W.calibrate_scores(model, W.make_frames(8, dev, seed=12), 48)
    return model


def _grouped(fr):
    """frame index -> (group tensor padded to len(fr) with copies, position in it): uniform batches of the SAME batch size
    (the plan form depends on N: the split stem from 16 frames on)."""
    B = len(fr)
    groups = {}
    for i, f in enumerate(fr):
        groups.setdefault(tuple(f.shape), []).append(i)
    out = {}
    for shape, idx in groups.items():
        pick = [idx[k % len(idx)] for k in range(B)]
        t = torch.stack([fr[j] for j in pick])
        for pos, j in enumerate(idx):
            out[j] = (t, pos)
    return groups, out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["back", "front", "yolov5n"])
def test_detectors_on_ragged_batches_equal_uniform_batches_of_the_same_size(dev, kind):
    from face_detection_and_recognition_amd import workload as W
    sizes = [s for s in SIZES]
    if kind == "yolov5n":
        det = W.build_yolo_detector(dev, W.make_frames(4, dev, seed=32), "yolov5n", cand_per_frame=80)
        fr = _frames(sizes, dev, seed=7)
    else:
        det = _blazeface(dev, kind == "back")
        fr = _frames(sizes * 3, dev, seed=7)            # 18 frames: the band / split stems (N >= 16)
    net = det.net
    raw = (lambda p: (p.z.clone(),)) if kind == "yolov5n" else (lambda p: (p.r.clone(), p.c.clone()))
    out = det.raw_batch(RaggedFrames.from_list(fr, dev))
    got_raw = raw(net.last_plan)
    got = [t.clone() for t in out]
    groups, where = _grouped(fr)
    for idx in groups.values():
        t, _ = where[idx[0]]
        o = det.raw_batch(t)
        r = raw(net.last_plan)
        for pos, j in enumerate(idx):
            for a, b in zip(got_raw, r):
                assert torch.equal(_bits(a[j]), _bits(b[pos])), (kind, j, fr[j].shape)
            # dets: the first counts[j] rows (the rows after them are scratch), counts and YOLO's overflow flags exactly
            n = int(got[1][j])
            assert n == int(o[1][pos]), (kind, j, fr[j].shape)
            assert torch.equal(_bits(got[0][j, :n]), _bits(o[0][pos, :n])), (kind, j, fr[j].shape)
            for a, b in zip(got[2:], o[2:]):
                assert torch.equal(a[j], b[pos]), (kind, j, fr[j].shape)
    counts = got[1]
    assert int(counts.sum()) > 0


def _pipe(dev, max_faces_per_frame=8):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    det = _blazeface(dev, True)
    return FacePipeline(det, W.build_embedder(dev), W.make_reference(64, dev), tau=0.0, max_faces_per_frame=max_faces_per_frame)


def _per_frame(res, B):
    info, items, emb = res["info"].cpu(), res["items"].cpu(), res["emb"].cpu()
    out = [[] for _ in range(B)]
    for k in range(res["n_faces"]):
        out[int(info[k, 0])].append((info[k, 1:].numpy(), items[k, 1:].numpy(), emb[k].numpy()))
    return out


def _same_faces(a, b):
    assert len(a) == len(b)
    for (ia, ta, ea), (ib, tb, eb) in zip(a, b):
        assert ia.tobytes() == ib.tobytes() and np.array_equal(ta, tb) and ea.tobytes() == eb.tobytes()


@pytest.mark.gpu
def test_pipeline_step_on_a_ragged_batch(dev):
    """step(RaggedFrames) equals the grouped uniform steps of the same batch size (info, items, embeddings bit for bit)
    and the oracle flow frame by frame; step_overlapped over ragged batches equals step."""
    from oracle import blazeface_ref, image_ref, mobilefacenet_ref
    pipe = _pipe(dev)
    fr = _frames(SIZES * 3, dev, seed=9)
    B = len(fr)
    rf = RaggedFrames.from_list(fr, dev)
    res = pipe.step(rf)
    got = _per_frame(res, B)
    assert res["n_faces"] > 0
    groups, where = _grouped(fr)
    for idx in groups.values():
        t, _ = where[idx[0]]
        ref = _per_frame(pipe.step(t), B)
        for pos, j in enumerate(idx):
            _same_faces(got[j], ref[pos])
    # oracle flow (tests/test_gpu_entry_points.py test_extract_faces_batched_matches_oracle_and_format) on one frame per size
    det, emb = pipe.det, pipe.emb
    sd_det = {k: v.cpu() for k, v in det.net.state_dict().items()}
    sd_emb = {k: v.cpu() for k, v in emb.state_dict().items()}
    for i in range(len(SIZES)):
        f = fr[i].cpu().numpy()
        lb = image_ref.pad_resize_image(f, (256, 256))[..., ::-1].copy()
        faces, _ = blazeface_ref.predict_on_batch(sd_det, torch.from_numpy(lb).permute(2, 0, 1).unsqueeze(0), det.net.anchors.cpu(), True)
        d = faces[0].numpy()
        if len(d) == 0:
            assert len(got[i]) == 0
            continue
        d = d[:, [1, 0, 3, 2] + list(range(4, 17))]
        post = image_ref.dets_to_boxes(d.copy(), (f.shape[1], f.shape[0]), (256, 256), det.det_thres, det.bbox_area_thres)
        assert len(post["boxes"]) == len(got[i])
        for k, box in enumerate(post["boxes"]):
            np.testing.assert_array_equal(got[i][k][0][:4], np.asarray(box, np.float32))
            crop, _ = image_ref.crop_face(f, box)
            face = image_ref.mfn_lut()[image_ref.resize_bilinear_u8(crop, (112, 112))]
            with torch.no_grad():
                e = mobilefacenet_ref.forward(sd_emb, torch.from_numpy(np.ascontiguousarray(face.transpose(2, 0, 1))).unsqueeze(0))[0].numpy()
            assert np.abs(got[i][k][2] - e).max() < 1e-4
    # software-pipelined form over two ragged batches
    rf2 = RaggedFrames.from_list(_frames(SIZES[::-1] * 2, dev, seed=10), dev)
    want = [_per_frame(pipe.step(x), len(x)) for x in (rf, rf2)]
    outs = [pipe.step_overlapped(rf), pipe.step_overlapped(rf2), pipe.flush()]
    assert outs[0] is None
    for o, w, x in zip(outs[1:], want, (rf, rf2)):
        g = _per_frame(o, len(x))
        for a, b in zip(g, w):
            _same_faces(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [None, 2])      # 2: every frame with more than two survivors overflows the capped pass
def test_pipeline_ragged_yolo_and_overflow_rerun_match_uniform(dev, monkeypatch, cap):
    """YOLOv5n through the pipeline on a ragged batch, including the un-capped re-run after an overflow, equals the grouped
    uniform steps."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    from face_detection_and_recognition_amd.modules.yolov5_face.model import YOLOV5FaceModel
    if cap is not None:
        orig = YOLOV5FaceModel.raw_batch
        monkeypatch.setattr(YOLOV5FaceModel, "raw_batch", lambda self, frames, max_det=cap: orig(self, frames, max_det=max_det))
    det = W.build_yolo_detector(dev, W.make_frames(4, dev, seed=32), "yolov5n", cand_per_frame=80)
    pipe = FacePipeline(det, W.build_embedder(dev), None, max_faces_per_frame=256)
    fr = _frames(SIZES[:4] * 2, dev, seed=13)
    res = pipe.step(RaggedFrames.from_list(fr, dev))
    assert res["n_faces"] > 0
    got = _per_frame(res, len(fr))
    groups, where = _grouped(fr)
    for idx in groups.values():
        t, _ = where[idx[0]]
        ref = _per_frame(pipe.step(t), len(fr))
        for pos, j in enumerate(idx):
            _same_faces(got[j], ref[pos])


@pytest.mark.gpu
def test_extract_faces_from_images_equals_one_call_per_image(dev, tmp_path):
    """The four reference JPEGs (four sizes, one progressive) in one ragged step equal one call per image; with save_face the
    JPEG bytes equal encode_crops on each frame alone."""
    from face_detection_and_recognition_amd.face_extraction import extract_faces_from_dataset as X
    from face_detection_and_recognition_amd.modules.utils.jpeg import imread_batch
    assert len(JPEGS) == 4
    pipe = _pipe(dev)
    recs = X.extract_faces_from_images(pipe, JPEGS, batch_size=256, save_face=True)
    assert len(recs) == 4 and all(r.frame_num == 1 and r.time_sec == 1 for r in recs)
    frames = imread_batch(JPEGS, dev)
    assert isinstance(frames, list) and len({tuple(f.shape) for f in frames}) == 4
    for rec, f in zip(recs, frames):
        one = X.extract_face_feat_conf_area_list(pipe, f[None], save_face=True)[0]
        assert rec.confs == one.confs and rec.areas == one.areas
        np.testing.assert_array_equal(rec.boxes, one.boxes)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rec.feats, one.feats)) and len(rec.feats) == len(one.feats)
        assert rec.face_jpegs == one.face_jpegs
    # smaller batches give the same records
    again = X.extract_faces_from_images(pipe, JPEGS, batch_size=3)
    for a, b in zip(recs, again):
        assert a.confs == b.confs and np.array_equal(a.boxes, b.boxes)
    total = X.save_extracted_faces(recs[:1], "img0", "person_a", str(tmp_path / "feats"), 512, {"person_a": 0}, save_face=True,
                                   faces_save_dir=str(tmp_path / "faces"))
    assert total == len(recs[0].confs)


@pytest.mark.gpu
def test_embed_images_mixed_sizes_bit_identical_to_the_per_image_loop(dev):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.mobile_facenet.utils import crops_to_input, mfn_lut
    from face_detection_and_recognition_amd.modules.utils.jpeg import imread_batch
    from face_detection_and_recognition_amd.similar_face_filtering.filter_faces_using_reference import embed_images
    model = W.build_embedder(dev)
    paths = JPEGS + JPEGS[:2]
    got = embed_images(model, paths, batch_size=4)
    lut = mfn_lut(dev)
    want = []
    for i in range(0, len(paths), 4):        # the loop embed_images ran before: one resize launch per image
        chunk = paths[i:i + 4]
        plan = model.plan_for(len(chunk))
        decoded = imread_batch(chunk, dev)
        for j in range(len(chunk)):
            img = decoded[j].unsqueeze(0)
            h, w = img.shape[1:3]
            item = torch.tensor([[0, 0, 0, w, h, 0, 0, 112, 112]], dtype=torch.int32, device=dev)
            crops_to_input(img, item, 1, plan.input[j:j + 1], lut)
        plan.run()
        want.append(plan.out.clone())
    assert torch.equal(_bits(got), _bits(torch.cat(want)))
