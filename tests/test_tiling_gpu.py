"""Tiled detection on the device: fp_merge_views against its host emulator on every scene of tile_cases.py (both formats, guard
rows, two runs), fp_gather_tiles against the numpy restatement (dense and ragged, a frame smaller than the tile, odd widths),
TiledDetector end to end over BlazeFace-front and YOLOv5n-face with synthetic weights, and FacePipeline over a
TiledDetector."""
import numpy as np
import pytest
import torch

import tile_cases as TC
from face_detection_and_recognition_amd import tiling as T
from face_detection_and_recognition_amd.frames import RaggedFrames

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
H, W_ = 96, 160


def _dev_tables(scene, dev):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    descs = T._descs_host(scene.sizes)
    return (to(np.ascontiguousarray(scene.views).view(np.uint8).reshape(-1, 32)), to(scene.view_start), to(descs.view(np.uint8).reshape(-1, 16)))


@pytest.mark.parametrize("fmt", TC.FMTS)
@pytest.mark.parametrize("scene", TC.ALL, ids=TC.IDS)
def test_device_merge_equals_the_emulator_and_two_runs_agree(scene, fmt, dev):
    args = scene.args(fmt)
    want = T.merge_views_emulate(*args)
    dets, counts = torch.from_numpy(args[0]).to(dev), torch.from_numpy(args[1]).to(dev)
    views, start, descs = _dev_tables(scene, dev)
    B = len(scene.sizes)
    runs = []
    for _ in range(2):
        out, cnt, over = T.merge_views(dets, counts, views, start, descs, B, TC.IN_SIZE, fmt, scene.merge_thr, scene.edge_px, scene.max_out)
        torch.cuda.synchronize()
        runs.append((out.cpu().numpy(), cnt.cpu().numpy(), over.cpu().numpy()))
    assert TC.rows_equal(runs[0], want), (scene.name, runs[0][1], want[1], runs[0][2], want[2])
    assert TC.rows_equal(runs[1], runs[0])
    # nothing behind a frame's count is written, and a preset flag stays
    lib = T.L.load()
    out = torch.full((B, scene.max_out, 16), SENTINEL, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    over = torch.ones((B,), dtype=torch.int32, device=dev)
    L = T.L
    assert lib.fp_merge_views(L.ptr(dets), L.ptr(counts), dets.shape[0], dets.shape[1], dets.shape[2], fmt, *TC.IN_SIZE, L.ptr(views),
                              L.ptr(start), L.ptr(descs), B, scene.merge_thr, scene.edge_px, scene.max_out, L.ptr(out), L.ptr(cnt),
                              L.ptr(over), L.current_stream(dev)) == 0
    torch.cuda.synchronize()
    o, c = out.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(c, want[1]) and np.array_equal(over.cpu().numpy(), want[2] | 1)
    for f in range(B):
        assert (o[f, c[f]:] == SENTINEL).all(), (scene.name, f)


def _frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


@pytest.mark.parametrize("kind,sizes,tile", [("dense", [(H, W_)] * 2, (64, 64)), ("ragged", [(H, W_), (30, 40), (64, 100)], (64, 64)),
                                             ("ragged", [(H, W_), (30, 40), (64, 100)], (50, 48)), ("dense", [(64, 100)] * 2, (37, 29))],
                         ids=["dense64", "ragged64", "ragged50x48", "dense37x29"])
def test_gather_tiles_equals_numpy_and_torch_slicing(kind, sizes, tile, dev):
    """The tile's row pitch picks the chunk size: 64-wide tiles take 16-byte chunks, 37 x 3 = 111 bytes single bytes, 50 x 3 = 150
    neither 16 nor 4.  Frames 100 and 40 pixels wide and tile starts at odd offsets make the source rows unaligned."""
    host = _frames(sizes, 3)
    views, _, is_tile = T.build_views(sizes, tile, (tile[0] // 2, tile[1] // 4), TC.IN_SIZE, full_frame=True)
    tv = np.ascontiguousarray(views[is_tile])
    want = T.gather_tiles_numpy(host, tv, tile)
    batch = torch.from_numpy(np.stack(host)).to(dev) if kind == "dense" else RaggedFrames.from_list(host, dev)
    tv_dev = torch.from_numpy(tv.view(np.uint8).reshape(-1, 32)).to(dev)
    got = T.gather_tiles(batch, tv_dev, len(tv), tile)
    sliced = T.gather_tiles_torch(batch, tv, tile)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(sliced.cpu().numpy(), want)
    if (30, 40) in sizes and tile == (64, 64):
        s = int(np.nonzero(tv["frame"] == 1)[0][0])
        assert (want[s, 30:] == 125).all() and (want[s, :, 40:] == 125).all() and np.array_equal(want[s, :30, :40], host[1])


# ---------------------------------------------------------------------------------------------------- the detector

def _front(dev):
    from face_detection_and_recognition_amd import workload as Wk
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace, generate_anchors
    from face_detection_and_recognition_amd.modules.blazeface.model import BlazeFaceModel
    from face_detection_and_recognition_amd.synth import synth_state_dict
    net = BlazeFace(False)
    net.load_state_dict(synth_state_dict(net.state_dict(), 100, residual_gain=0.5))
    net = net.to(dev)
    net.set_anchors(generate_anchors(False))
    model = BlazeFaceModel("", 0.7, 0.0, "front", device=str(dev), net=net)
    Wk.calibrate_scores(model, Wk.make_frames(8, dev, seed=12, h=H, w=W_), 48)
    return model


@pytest.fixture(scope="module")
def inner(dev):
    from face_detection_and_recognition_amd import workload as Wk
    frames = Wk.make_frames(2, dev, seed=21, h=H, w=W_)
    # 32 x 32 is YOLOv5-face's smallest input (one multiple of its largest stride): 63 rows per image
    yolo = Wk.build_yolo_detector(dev, Wk.make_frames(4, dev, seed=32, h=H, w=W_), "yolov5n", cand_per_frame=24, input_size=(32, 32))
    return {"front": _front(dev), "yolov5n": yolo}, frames


def _view_order(t, parts, dev):
    """The rows of inner on the tiles and on the frames, put into the table's view order on the host."""
    S = len(t.views)
    d0 = parts[0][1][0]
    dets = np.zeros((S,) + tuple(d0.shape[1:]), np.float32)
    counts = np.zeros((S,), np.int32)
    over = np.zeros((S,), np.int32)
    for pos, out in parts:
        pos = pos.cpu().numpy()
        dets[pos], counts[pos] = out[0].cpu().numpy(), out[1].cpu().numpy()
        if len(out) > 2:
            over[pos] = out[2].cpu().numpy()
    return dets, counts, over


@pytest.mark.parametrize("kind", ["front", "yolov5n"])
def test_tiled_detector_equals_numpy_merge_of_inner_rows(inner, kind, dev):
    dets_by, frames = inner
    det = dets_by[kind]
    td = T.TiledDetector(det, (64, 64), (32, 32), 0.5, edge_px=1.0, max_det=64)
    out, cnt, over = td.raw_batch(frames)
    assert out.shape == (2, 64, 16) and out.dtype == torch.float32 and cnt.dtype == torch.int32 and over.shape == (2,)
    t = td.view_table(frames)
    assert t is td.view_table(frames) and t.n_tiles == 16 and len(t.views) == 18
    tiles = T.gather_tiles(frames, t.tile_views_dev, t.n_tiles, td.tile)
    parts = [(t.tile_pos, det.raw_batch(tiles)), (t.full_pos, det.raw_batch(frames))]
    dets, counts, over_v = _view_order(t, parts, dev)
    assert counts.sum() > 0
    preset = np.array([int(over_v[t.view_start[f]:t.view_start[f + 1]].any()) for f in range(2)], np.int32)
    want = T.merge_views_numpy(dets, counts, t.views, t.view_start, [(H, W_)] * 2, det.input_size, det.dets_fmt, 0.5, 1.0, 64, preset)
    got = (out.cpu().numpy(), cnt.cpu().numpy(), over.cpu().numpy())
    assert TC.rows_equal(got, want), (kind, got[1], want[1], got[2], want[2])
    assert want[1].sum() > 0
    # the same frames as a RaggedFrames: the table rides on the batch, the rows are the same
    rag = RaggedFrames.from_list(list(frames), dev)
    r_out = td.raw_batch(rag)
    assert td.view_table(rag) is td.view_table(rag)
    assert TC.rows_equal(tuple(x.cpu().numpy() for x in r_out), want), kind


@pytest.mark.parametrize("kind", ["front", "yolov5n"])
def test_tile_of_the_frame_alone_gives_inner_rows_in_pixels(inner, kind, dev):
    """tile = the frame, no whole-frame view, merge_thr = +inf: every row of inner, mapped to pixels, in score order."""
    dets_by, frames = inner
    det = dets_by[kind]
    td = T.TiledDetector(det, (W_, H), (0, 0), float("inf"), edge_px=0.0, full_frame=False, max_det=256)
    out, cnt, over = (x.cpu().numpy() for x in td.raw_batch(frames))
    raw = det.raw_batch(frames)
    d, c = raw[0].cpu().numpy(), raw[1].cpu().numpy()
    views, start, _ = T.build_views([(H, W_)] * 2, (W_, H), (0, 0), det.input_size, full_frame=False)
    want = T.merge_views_numpy(d, c, views, start, [(H, W_)] * 2, det.input_size, det.dets_fmt, np.inf, 0.0, 256)
    assert TC.rows_equal((out, cnt, over & ~1), want) and cnt.sum() > 0
    iw, ih = det.input_size
    g, px, py = (float(v) for v in (views["gain"][0], views["pad_x"][0], views["pad_y"][0]))
    for f in range(2):
        n = min(int(c[f]), d.shape[1])
        r = d[f, :n]
        box = r[:, [1, 0, 3, 2]] * [iw, ih, iw, ih] if det.dets_fmt == 0 else r[:, :4]
        sc = r[:, 16] if det.dets_fmt == 0 else r[:, 4]
        box = np.clip((box - [px, py, px, py]) / g, 0, [W_, H, W_, H])
        ok = (box[:, 2] > box[:, 0]) & (box[:, 3] > box[:, 1])
        order = np.argsort(-sc[ok], kind="stable")
        assert cnt[f] == ok.sum()
        assert np.allclose(out[f, :cnt[f], :4], box[ok][order], atol=1e-3) and np.array_equal(out[f, :cnt[f], 14], sc[ok][order])


@pytest.mark.parametrize("kind", ["front", "yolov5n"])
def test_pipeline_over_a_tiled_detector(inner, kind, dev):
    from face_detection_and_recognition_amd import workload as Wk
    from face_detection_and_recognition_amd.annotate import annotate_step
    from face_detection_and_recognition_amd.evaluation import dets_to_frame_boxes
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    dets_by, frames = inner
    td = T.TiledDetector(dets_by[kind], (64, 64), (32, 32), 0.5, edge_px=1.0, max_det=512)
    emb = Wk.build_embedder(dev)
    pipe = FacePipeline(td, emb, None, tau=0.0, max_faces_per_frame=512)
    res = pipe.step(frames)
    n = res["n_faces"]
    dets, counts, _ = td.raw_batch(frames)
    assert 0 < n <= int(counts.sum()) and res["emb"].shape == (n, 512) and res["info"].shape == (n, 7) and res["items"].shape == (n, 9)
    items, info, nf = pipe.crops(frames, dets, counts)
    assert int(nf) == n
    by_hand = pipe.embed(frames, items, n).clone()
    assert torch.equal(res["emb"], by_hand) and torch.equal(res["info"], info[:n])
    boxes, scores, valid = dets_to_frame_boxes(td, dets, counts, [(H, W_)] * 2)          # the evaluator takes the rows as they stand
    assert int(valid.sum()) == int(counts.sum()) and torch.equal(boxes[valid].float(), dets[..., :4][valid])
    full = FacePipeline(td, emb, None, tau=0.0, max_faces_per_frame=512, align=True, quality=True).step(frames)
    assert full["n_faces"] == n and full["lmarks"].shape == (n, 10) and full["align_M"].shape == (n, 6) and full["emb"].shape == (n, 512)
    assert all(v.shape[0] == n for v in full["quality"].values()) and "yaw" in full["quality"]
    assert torch.equal(full["info"], res["info"])
    over = FacePipeline(td, emb, None, tau=0.0, max_faces_per_frame=512)
    assert over.step_overlapped(frames) is None
    late = over.flush()
    assert late["n_faces"] == n and torch.equal(late["emb"], res["emb"])
    # a cap the merge overflows (flag 4): the step re-runs the detector uncapped and finds the same faces
    tight = T.TiledDetector(dets_by[kind], (64, 64), (32, 32), 0.5, edge_px=1.0, max_det=4)
    assert (tight.raw_batch(frames)[2] & 4).any()
    again = FacePipeline(tight, emb, None, tau=0.0, max_faces_per_frame=512).step(frames)
    assert again["n_faces"] == n and torch.equal(again["info"], res["info"])
    # the dataset driver's tiled=: the plain pipeline wrapped for the call, and left as it was
    from face_detection_and_recognition_amd.face_extraction.extract_faces_from_dataset import extract_face_feat_conf_area_list
    plain = FacePipeline(dets_by[kind], emb, None, tau=0.0, max_faces_per_frame=512)
    recs = extract_face_feat_conf_area_list(plain, frames, tiled=dict(tile=(64, 64), overlap=(32, 32), merge_thr=0.5, edge_px=1.0, max_det=512))
    assert plain.det is dets_by[kind] and [c for r in recs for c in r.confs] == [float(c) for c in res["info"][:, 5].cpu()]
    drawn = annotate_step(frames, res)
    torch.cuda.synchronize()
    assert drawn.shape == frames.shape and not torch.equal(drawn, frames)
