"""Tiled detection on the host (no GPU): tile_grid and its coverage property, fp_merge_views_emulate against the float32 numpy
restatement on every crafted and random scene of tile_cases.py (all 16 columns, counts and flags, bit for bit), the crafted
scenes' stated outcomes, a single whole-frame view as the identity of the crop path, and the refusals."""
import ctypes

import numpy as np
import pytest

import tile_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import tiling as T
from face_detection_and_recognition_amd.frames import ragged_scale_coords_params


# ------------------------------------------------------------------------------------------------ tile_grid

@pytest.mark.parametrize("wh,tile,overlap,want", TC.GRIDS, ids=[str(g[0]) for g in TC.GRIDS])
def test_tile_grid_exact_lists_cover_and_stay_inside(wh, tile, overlap, want):
    w, h = wh
    got = T.tile_grid(w, h, tile, overlap)
    assert got == want
    covered = np.zeros((h, w), bool)
    for x0, y0, vw, vh in got:
        assert 0 <= x0 and 0 <= y0 and x0 + vw <= w and y0 + vh <= h and vw >= 1 and vh >= 1
        covered[y0:y0 + vh, x0:x0 + vw] = True
    assert covered.all()
    if w >= tile[0] and h >= tile[1]:
        assert {(vw, vh) for _, _, vw, vh in got} == {tuple(tile)}


def test_tile_grid_refuses_bad_overlap():
    for tile, overlap in (((64, 64), (64, 0)), ((64, 64), (0, 70)), ((64, 64), (-1, 0)), ((0, 64), (0, 0))):
        with pytest.raises(ValueError):
            T.tile_grid(160, 96, tile, overlap)
    assert T.tile_grid(160, 96, (64, 64), (63, 63))[0] == (0, 0, 64, 64)


def _uncut_1d(a, b, size, starts, span, edge):
    """Is the interval [a, b] uncut along one axis in some tile: the cut rule of fp_merge_views with integer coordinates."""
    return [(x0 == 0 or a - x0 > edge) and (x0 + span == size or b - x0 < span - edge) for x0 in starts]


@pytest.mark.parametrize("wh,tile,overlap,want", TC.GRIDS, ids=[str(g[0]) for g in TC.GRIDS])
@pytest.mark.parametrize("edge", [0, 2])
def test_every_small_box_is_whole_in_some_tile(wh, tile, overlap, want, edge):
    """Brute force: every integer box with both sides <= overlap - 2 (edge_px + 1) is uncut in at least one tile.  The cut rule
    is separable, so a box is uncut in tile (x0, y0) exactly when its x interval is uncut at x0 and its y interval at y0, and
    the grid is the product of its axis starts."""
    w, h = wh
    grid = T.tile_grid(w, h, tile, overlap)
    xs, ys = sorted({g[0] for g in grid}), sorted({g[1] for g in grid})
    assert len(grid) == len(xs) * len(ys)
    vw, vh = grid[0][2], grid[0][3]
    lim_x = w if len(xs) == 1 else overlap[0] - 2 * (edge + 1)       # a single tile along an axis has no interior edge there
    lim_y = h if len(ys) == 1 else overlap[1] - 2 * (edge + 1)
    ok_x = {(a, b): any(_uncut_1d(a, b, w, xs, vw, edge)) for a in range(w) for b in range(a + 1, min(a + lim_x, w) + 1)}
    ok_y = {(a, b): any(_uncut_1d(a, b, h, ys, vh, edge)) for a in range(h) for b in range(a + 1, min(a + lim_y, h) + 1)}
    assert all(ok_x.values()), [k for k, v in ok_x.items() if not v][:5]
    assert all(ok_y.values()), [k for k, v in ok_y.items() if not v][:5]
    assert len(ok_x) > 0 and len(ok_y) > 0


# ------------------------------------------------------------------------------------------------ the merge

@pytest.mark.parametrize("fmt", TC.FMTS)
@pytest.mark.parametrize("scene", TC.ALL, ids=TC.IDS)
def test_emulator_equals_numpy_bit_for_bit(scene, fmt):
    args = scene.args(fmt)
    want = T.merge_views_numpy(*args)
    got = T.merge_views_emulate(*args)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (scene.name, got[1], want[1], got[2], want[2])
    assert TC.rows_equal(got, want), scene.name
    assert want[1].sum() > 0 or scene.expect is not None
    if scene.expect is not None:
        assert want[1].tolist() == scene.expect, scene.name
    # the flags are OR-ed into what the caller presets
    preset = np.full((len(scene.sizes),), 1, np.int32)
    again = T.merge_views_emulate(*args, overflow=preset)
    assert np.array_equal(again[2], want[2] | 1) and np.array_equal(again[0], got[0])


@pytest.mark.parametrize("fmt", TC.FMTS)
def test_crafted_outcomes(fmt):
    by = {s.name: T.merge_views_emulate(*s.args(fmt)) for s in TC.SCENES}
    out, cnt, over = by["two_tiles"]
    assert cnt[0] == 1 and out[0, 0, 14] == np.float32(0.9) and over[0] == 0
    assert np.allclose(out[0, 0, :4], [40.25, 10, 56, 26.5], atol=1e-3)
    assert by["cut_interior"][1][0] == 0 and by["no_cut"][1][0] == 1
    out, cnt, _ = by["frame_edge"]
    assert cnt[0] == 1 and out[0, 0, 2] == 160.0                       # clamped to the view, which ends at the frame
    out, cnt, _ = by["partial_in_whole"]
    assert cnt[0] == 1 and out[0, 0, 14] == np.float32(0.9) and np.allclose(out[0, 0, :4], [40, 40, 80, 80], atol=1e-3)
    out, cnt, _ = by["equal_scores"]
    assert cnt[0] == 1 and np.allclose(out[0, 0, 4:14], [43, 13] * 5, atol=1e-3)     # view 0's row, not view 1's
    out, cnt, _ = by["counts"]
    assert cnt[0] == 4 and np.allclose(out[0, :4, 14], [0.8, 0.7, 0.6, 0.5])
    out, cnt, _ = by["invalid"]
    assert cnt[0] == 2 and (out[0, :2, 14] == 0).all() and not np.signbit(out[0, :2, 14]).any()
    assert np.allclose(out[0, :2, 0], [5, 70], atol=1e-3)              # equal scores (-0 is +0): view order
    out, cnt, over = by["thr_inf"]
    assert cnt[0] == 3 and over[0] == 0 and np.allclose(out[0, :3, 14], [0.9, 0.8, 0.7])
    out, cnt, over = by["cap"]
    assert over[0] == 2 and cnt[0] > 0 and out[0, 0, 14] < np.float32(0.999)
    out, cnt, over = by["max_out"]
    assert cnt[0] == 2 and over[0] == 4 and np.allclose(out[0, :2, 14], [0.9, 0.8])
    # landmarks: fmt 0 puts the mouth centre into both mouth slots, fmt 1 keeps five landmarks
    row = by["two_tiles"][0][0, 0]
    assert (row[10:12] == row[12:14]).all() == (fmt == 0) and row[15] == 0


def _crop_px_numpy(rows, n, W, H, det_thres, offsets, dst):
    """crop_one / crop_emit_box of csrc/align.hip for fmt-2 rows of one frame, area threshold 0, in float32 numpy: -> (items
    (k, 8) = sx, sy, sw, sh, dx, dy, dw, dh; info (k, 5) = x1, y1, x2, y2, conf)."""
    items, info = [], []
    tx, ty, bx, by = offsets
    for d in rows[:n]:
        conf = d[14]
        if not conf > np.float32(det_thres):
            continue
        x1, y1, x2, y2 = d[0], d[1], d[2], d[3]
        perc = ((x2 - x1) * (y2 - y1)) / np.float32(W * H)
        if not np.float32(100) * perc > 0:
            continue
        x1, x2 = [np.rint(np.minimum(np.maximum((v - np.float32(0)) / np.float32(1), 0), np.float32(W))) for v in (x1, x2)]
        y1, y2 = [np.rint(np.minimum(np.maximum((v - np.float32(0)) / np.float32(1), 0), np.float32(H))) for v in (y1, y2)]
        x, y, xw, yh = max(int(x1) + tx, 0), max(int(y1) + ty, 0), min(int(x2) + bx, W), min(int(y2) + by, H)
        it = [x, y, xw - x, yh - y, 0, 0, dst[0], dst[1]]
        if it[2] <= 0 or it[3] <= 0:
            it[6] = it[7] = 0
        items.append(it)
        info.append([x1, y1, x2, y2, conf])
    return np.asarray(items, np.int32).reshape(-1, 8), np.asarray(info, np.float32).reshape(-1, 5)


@pytest.mark.parametrize("fmt", TC.FMTS)
def test_single_whole_frame_view_is_the_identity_of_the_crop_path(fmt, lib):
    """One whole-frame view per frame, merge_thr = +inf, bbox_area_thres = 0: the crops of the merged rows are the crops of the
    detector's own rows.  The original rows go through fp_dets_to_crops_aligned_emulate (the only crop emulator the library
    exports).  That emulator refuses fmt 2, so the merged half is derived from crop_one's written arithmetic for fmt 2 in
    numpy (_crop_px_numpy).  Per frame both sides are sorted by confidence (all distinct here)."""
    sizes = [(96, 160), (120, 90)]
    sc = TC.Scene("identity", sizes=sizes, tile=(512, 512), overlap=(0, 0), full_frame=False, max_dets=12, merge_thr=np.inf, max_out=12)
    assert len(sc.views) == 2 and [tuple(v)[1:5] for v in sc.views] == [(0, 0, 160, 96), (0, 0, 90, 120)]
    sc.views["gain"], sc.views["pad_x"], sc.views["pad_y"] = ragged_scale_coords_params(TC.IN_SIZE, sizes).T   # whole-frame views
    rng = np.random.default_rng(3)
    for s, (h, w) in enumerate(sizes):
        for k in range(10):
            x, y = rng.uniform(-8, w - 20), rng.uniform(-8, h - 20)
            sc.add(s, (x, y, x + rng.uniform(12, 50), y + rng.uniform(12, 50)), 0.3 + 0.06 * k + 0.01 * s)
    dets, counts = sc.arrays(fmt)
    out, cnt, over = T.merge_views_emulate(*sc.args(fmt))
    assert cnt.tolist() == [10, 10] and not over.any()
    det_thres, offsets, dst, cap = 0.45, (-6, -1, 4, 5), (112, 112), 32
    descs, geom = T._descs_host(sizes), ragged_scale_coords_params(TC.IN_SIZE, sizes)
    items = np.zeros((cap, 9), np.int32)
    info = np.zeros((cap, 7), np.float32)
    nf = np.zeros((1,), np.int32)
    lm, M, flags = np.zeros((cap, 10), np.float32), np.zeros((cap, 6), np.float64), np.zeros((cap,), np.int32)
    p = lambda a: a.ctypes.data      # noqa: E731
    rc = lib.fp_dets_to_crops_aligned_emulate(p(dets), p(counts), 2, dets.shape[1], dets.shape[2], fmt, *TC.IN_SIZE, p(descs), p(geom),
                                              det_thres, 0.0, *offsets, *dst, cap, p(items), p(info), p(nf), p(lm), p(M), p(flags))
    assert rc == 0 and 0 < nf[0] < 20
    # fmt 2 through the exported emulator is refused: the merged half is the numpy restatement
    assert lib.fp_dets_to_crops_aligned_emulate(p(out), p(cnt), 2, out.shape[1], 16, 2, *TC.IN_SIZE, p(descs), p(geom), det_thres, 0.0,
                                                *offsets, *dst, cap, p(items.copy()), p(info.copy()), p(nf.copy()), p(lm), p(M),
                                                p(flags)) == L.FP_ERR_INVALID_ARG
    for f, (h, w) in enumerate(sizes):
        mine = info[:nf[0], 0] == f
        a_items, a_info = items[:nf[0]][mine][:, 1:], info[:nf[0]][mine][:, 1:6]
        b_items, b_info = _crop_px_numpy(out[f], cnt[f], w, h, det_thres, offsets, dst)
        oa, ob = np.argsort(-a_info[:, 4], kind="stable"), np.argsort(-b_info[:, 4], kind="stable")
        assert len(oa) == len(ob) > 0
        assert np.array_equal(a_items[oa], b_items[ob]), f
        assert np.array_equal(a_info[oa].view(np.int32), b_info[ob].view(np.int32)), f


def test_refusals(lib):
    sc = TC.SCENES[0]
    dets, counts = sc.arrays(1)
    views, vs, descs = np.ascontiguousarray(sc.views), sc.view_start, T._descs_host(sc.sizes)
    out, oc, ov = np.zeros((1, 4, 16), np.float32), np.zeros((1,), np.int32), np.zeros((1,), np.int32)
    p = lambda a: a.ctypes.data      # noqa: E731
    good = [p(dets), p(counts), len(views), dets.shape[1], 16, 1, 128, 128, p(views), p(vs), p(descs), 1, 0.5, 0.0, 4, p(out), p(oc), p(ov)]
    for fn, tail in ((lib.fp_merge_views_emulate, []), (lib.fp_merge_views, [None])):      # the device form refuses before any launch
        if fn is lib.fp_merge_views_emulate:
            assert fn(*good) == L.FP_OK and oc[0] == 1
        bad = {k: None for k in (0, 1, 8, 9, 10, 15, 16, 17)}                              # null pointers
        bad.update({5: 2, 14: 0, 12: float("nan"), 11: -1, 2: -1, 4: 14})                  # fmt, max_out, NaN thr, B, S, short row
        for k, v in bad.items():
            a = list(good)
            a[k] = v
            assert fn(*a, *tail) == L.FP_ERR_INVALID_ARG, (fn.__name__, k)
        a = list(good)
        a[5], a[4] = 0, 16                                                                 # fmt 0 needs 17 columns
        assert fn(*a, *tail) == L.FP_ERR_INVALID_ARG
        a = list(good)
        a[11] = 0
        assert fn(*a, *tail) == L.FP_OK                                                    # B == 0: nothing to do
    assert lib.fp_gather_tiles(None, 0, None, 1, None, 0, 64, 64, None, None) == L.FP_ERR_INVALID_ARG
    assert ctypes.sizeof(ctypes.c_int32) * 8 == T.VIEW_DTYPE.itemsize == 32
    assert len(L.SIGNATURES["fp_merge_views"][1]) == 19 and len(L.SIGNATURES["fp_merge_views_emulate"][1]) == 18
    assert L.ABI_VERSION == 15 and L.MERGE_CAP == 2048


def test_tiled_detector_refusals_and_tables():
    class Inner:
        def __init__(self, fmt):
            self.dets_fmt, self.input_size, self.det_thres, self.bbox_area_thres = fmt, (128, 128), 0.5, 0.0
    with pytest.raises(ValueError):
        T.TiledDetector(Inner(2), (64, 64), (8, 8), 0.5)                # MTCNN: its own pyramid
    with pytest.raises(ValueError):
        T.TiledDetector(Inner(0), (64, 64), (64, 8), 0.5)
    with pytest.raises(TypeError):
        T.TiledDetector(Inner(0), (64, 64), (8, 8))                     # merge_thr has no default
    with pytest.raises(ValueError):
        T.TiledDetector(Inner(0), (64, 64), (8, 8), float("nan"))
    det = T.TiledDetector(Inner(1), (64, 64), (32, 32), 0.5)
    assert det.dets_fmt == 2 and det.input_size == (128, 128) and det.det_thres == 0.5 and det.bbox_area_thres == 0.0
    views, start, is_tile = T.build_views([(96, 160), (30, 40)], (64, 64), (32, 32), (128, 128))
    assert start.tolist() == [0, 9, 11] and is_tile.tolist() == [True] * 8 + [False, True, False]
    assert views["frame"].tolist() == [0] * 9 + [1, 1] and tuple(views[8])[1:5] == (0, 0, 160, 96) and tuple(views[9])[1:5] == (0, 0, 40, 30)
    assert views["gain"][0] == 2.0 and views["gain"][9] == 2.0 and np.isclose(views["gain"][8], 0.8) and np.isclose(views["gain"][10], 3.2)
    frames = [np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3) for h, w in ((96, 160), (30, 40))]
    tiles = T.gather_tiles_numpy(frames, views[is_tile], (64, 64))
    assert tiles.shape == (9, 64, 64, 3) and np.array_equal(tiles[5], frames[0][32:96, 32:96])
    assert np.array_equal(tiles[8, :30, :40], frames[1]) and (tiles[8, 30:] == 125).all() and (tiles[8, :, 40:] == 125).all()


def test_command_line_options_are_absent_by_default_and_need_merge_thr():
    import argparse
    inner = type("Inner", (), dict(dets_fmt=0, input_size=(128, 128), det_thres=0.5, bbox_area_thres=0.0))()
    parser = T.add_tile_args(argparse.ArgumentParser())
    assert vars(parser.parse_args([])) == {}
    assert T.wrap_from_args(inner, parser.parse_args([])) is inner
    with pytest.raises(ValueError):
        T.wrap_from_args(inner, parser.parse_args(["--tile", "64", "64"]))
    td = T.wrap_from_args(inner, parser.parse_args(["--tile", "64", "48", "--merge_thr", "0.4", "--overlap", "8", "4", "--edge_px", "2", "--no_full_frame"]))
    assert (td.tile, td.overlap, td.merge_thr, td.edge_px, td.full_frame) == ((64, 48), (8, 4), 0.4, 2.0, False) and td.inner is inner
    from face_detection_and_recognition_amd import detect_face_mtcnn
    with pytest.raises(SystemExit):
        detect_face_mtcnn.main(["-i", "x.jpg", "--tile", "64", "64", "--merge_thr", "0.5"])
