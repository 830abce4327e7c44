"""Drawing without a GPU: the numpy restatement (annotate.draw_numpy) against hand-written pixel sets, the library's serial
emulator (fp_draw_emulate) against the restatement on every shared case, the font table, the reference's layout
(face_draw_list), the refusals and the three programs' new flags.  Every comparison is exact equality of u8 arrays."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import draw_cases as DC
from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import annotate as A
from face_detection_and_recognition_amd.modules.utils import font6x8 as F


def art(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def changed(before, after):
    return (before != after).any(-1)


def draw12(build, value=0):
    """A 12 x 12 frame of `value`, drawn by numpy AND by the emulator (they must agree) -> the frame."""
    dl = A.DrawList([(12, 12)])
    build(dl)
    a = A.draw_numpy([np.full((12, 12, 3), value, np.uint8)], dl)[0]
    b = A.draw_emulate([np.full((12, 12, 3), value, np.uint8)], dl)[0]
    assert np.array_equal(a, b)
    return a


# ---------------------------------------------------------------------------------------------------- emulator == numpy

@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_emulator_equals_numpy(case, lib):
    want = DC.expected(case)
    got = A.draw_emulate(DC.frames(case), case[3])
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (case[0], k, np.argwhere(changed(g, w))[:5])
    if len(case[3]):
        assert any(changed(s, w).any() for s, w in zip(DC.frames(case), want)), "the case draws nothing"


def test_order_matters_in_the_order_cases():
    a, b = (DC.expected(c)[0] for c in DC.CASES if "_over_" in c[0])
    assert not np.array_equal(a, b)


def test_many_case_fills_more_than_two_chunks_of_one_tile():
    case = next(c for c in DC.CASES if c[0] == "many600")
    cmds = case[3].host()[0]
    box = A.DrawList.boxes_of(cmds)
    meets = (box[:, 0] < 64) & (box[:, 2] > 0) & (box[:, 1] < 64) & (box[:, 3] > 0)
    assert meets.sum() == 600 and len(cmds) > 600 and set(np.unique(cmds["kind"])) == {1, 2, 3, 4, 5}


# ---------------------------------------------------------------------------------------------------- predicates by hand

def test_outline_thickness_1_2_3(lib):
    want = {
        1: ["............", "............", "............", "...######...", "...#....#...", "...#....#...", "...#....#...",
            "...######...", "............", "............", "............", "............"],
        2: ["............", "............", "..########..", "..########..", "..##....##..", "..##....##..", "..##....##..",
            "..########..", "..########..", "............", "............", "............"],
        3: ["............", "............", "..########..", "..########..", "..########..", "..###..###..", "..########..",
            "..########..", "..########..", "............", "............", "............"],
    }
    for t, rows in want.items():
        img = draw12(lambda dl: dl.rect(0, 3, 3, 9, 8, (0, 0, 255), t))       # the rectangle [3, 9) x [3, 8)
        assert np.array_equal(img[..., 2] == 255, art(rows)), t
        assert (img[..., :2] == 0).all()


def test_ring_of_radius_3(lib):
    rows = ["............", "............", "....###.....", "...#...#....", "..#.....#...", "..#.....#...", "..#.....#...",
            "...#...#....", "....###.....", "............", "............", "............"]
    img = draw12(lambda dl: dl.ring(0, 5, 5, 3, (9, 8, 7)))
    assert np.array_equal((img == (9, 8, 7)).all(-1), art(rows))
    # 4 (dx^2 + dy^2) in [25, 49): (3, 1) with 40 is on the ring, (3, 2) with 52 is not
    assert img[5 + 1, 5 + 3].tolist() == [9, 8, 7] and img[5 + 2, 5 + 3].tolist() == [0, 0, 0]
    assert not changed(np.zeros((12, 12, 3), np.uint8), draw12(lambda dl: dl.ring(0, 5, 5, 0, (9, 9, 9)))).any()


def test_fill_alpha_rounding(lib):
    for a, c in ((0, 200), (128, 200), (255, 200), (128, 0), (128, 255), (1, 255), (254, 0)):
        for dst in (0, 1, 254, 255):
            img = draw12(lambda dl: dl.fill(0, 2, 2, 5, 4, (c, c, c), a), value=dst)
            want = (dst * (255 - a) + c * a + 127) // 255
            assert (img[2:4, 2:5] == want).all() and (img[4:, :] == dst).all() and (img[:, 5:] == dst).all(), (a, c, dst)
            if a == 0:
                assert want == dst
            if a == 255:
                assert want == c
    assert (0 * 127 + 200 * 128 + 127) // 255 == 100 and (1 * 127 + 200 * 128 + 127) // 255 == 101     # written out once


def test_mosaic_cell_cut_by_rectangle_and_frame_edge_rounds_half_up(lib):
    src = np.zeros((12, 12, 3), np.uint8)
    src[9, 9] = (1, 3, 255)
    src[9, 10] = (0, 0, 255)
    # cell 4 at (8 .. 12, 8 .. 12); the rectangle [9, 20) x [9, 10) leaves pixels (9, 9), (10, 9), (11, 9) of it: the frame
    # ends at x = 12.  Means of three: (1 + 1) / 3 = 0, (3 + 1) / 3 = 1, 510 / 3 = 170; the cell to the left is untouched.
    dl = A.DrawList([(12, 12)])
    dl.mosaic(0, 9, 9, 20, 10, 4)
    a, b = A.draw_numpy([src.copy()], dl)[0], A.draw_emulate([src.copy()], dl)[0]
    assert np.array_equal(a, b)
    want = src.copy()
    want[9, 9:12] = (0, 1, 170)
    assert np.array_equal(a, want)
    # two pixels, sum 1: (1 + 1) // 2 = 1, the mean .5 rounds up
    src2 = np.zeros((12, 12, 3), np.uint8)
    src2[0, 0] = (1, 255, 0)
    dl = A.DrawList([(12, 12)])
    dl.mosaic(0, -5, 0, 2, 1, 8)
    a, b = A.draw_numpy([src2.copy()], dl)[0], A.draw_emulate([src2.copy()], dl)[0]
    assert np.array_equal(a, b) and a[0, 0].tolist() == [1, 128, 0] and a[0, 1].tolist() == [1, 128, 0] and not a[1:].any() and not a[0, 2:].any()


# ---------------------------------------------------------------------------------------------------- the font

GLYPH_ART = {
    "0": [".###..", "#...#.", "#..##.", "#.#.#.", "##..#.", "#...#.", ".###..", "......"],
    "1": ["..#...", ".##...", "..#...", "..#...", "..#...", "..#...", ".###..", "......"],
    ".": ["......", "......", "......", "......", "......", ".##...", ".##...", "......"],
    "_": ["......", "......", "......", "......", "......", "......", "#####.", "......"],
}


def test_font_table(lib):
    assert len(F.FONT) == 760 == L.DRAW_FONT_BYTES and (F.FIRST, F.LAST, F.CELL_W, F.CELL_H) == (32, 126, 6, 8)
    for ch, rows in GLYPH_ART.items():
        got = np.array([[bool(b & (0x80 >> c)) for c in range(6)] for b in F.glyph_rows(ch)])
        assert np.array_equal(got, art(rows)), ch
        img = draw12(lambda dl: dl.text(0, 2, 1, ch, (255, 255, 255), 1))
        assert np.array_equal((img == 255).all(-1)[1:9, 2:8], art(rows)) and (img == 255).all(-1).sum() == art(rows).sum()
    for code in range(32, 127):
        rows = F.glyph_rows(code)
        assert rows[7] == 0 and all(b & 0x07 == 0 for b in rows), chr(code)      # inside the 5 x 7 area of the cell
        assert any(rows) or code == 32, chr(code)
    must_differ = "0123456789._-()" + "".join(chr(c) for c in range(65, 91)) + "".join(chr(c) for c in range(97, 123))
    assert len({bytes(F.glyph_rows(ch)) for ch in must_differ}) == len(must_differ)


def test_glyph_scale_3_is_the_glyph_with_3x3_pixels(lib):
    dl = A.DrawList([(30, 30)])
    dl.text(0, 4, 2, "R", (255, 255, 255), 3)
    img = A.draw_numpy([np.zeros((30, 30, 3), np.uint8)], dl)[0]
    one = np.array([[bool(b & (0x80 >> c)) for c in range(6)] for b in F.glyph_rows("R")])
    assert np.array_equal((img == 255).all(-1)[2:26, 4:22], np.kron(one, np.ones((3, 3), bool)))
    dl = A.DrawList([(12, 12)])
    dl.text(0, 0, 0, chr(7) + chr(300), (1, 1, 1))
    assert [int(a) & 255 for a in dl.host()[0]["arg"]] == [ord("?")] * 2


# ---------------------------------------------------------------------------------------------------- the reference's layout

def test_caption_formats_fp32_values_as_the_reference_does():
    for v, s in ((0.125, "0.12"), (0.375, "0.38"), (0.995, "1.00")):          # 0.995 is 0.99500000477 in fp32, 0.99499999... in fp64
        assert f"{np.float32(v):.2f}" == s                                      # what the reference's f-string gives for its float32
        assert A.caption(np.float32(v), np.float32(v)) == f"{s}_{s}" and A.caption(np.float32(v)) == s
    info = np.array([[0, 10, 40, 50, 80, 0.995, 0.125], [0, 60, 40, 90, 80, 0.375, 0.375]], np.float32)
    dl = A.face_draw_list(info, 2, [(100, 100)], labels=["", "Bo"])
    assert dl.captions == ["1.00_0.12", "0.38_0.38Bo"]
    assert A.face_draw_list(info, 2, [(100, 100)], areas=False).captions == ["1.00", "0.38"]
    glyphs = dl.host()[0]
    glyphs = glyphs[glyphs["kind"] == L.DRAW_GLYPH]
    assert "".join(chr(int(a) & 255) for a in glyphs["arg"]) == "1.00_0.120.38_0.38Bo"


def test_layout_numbers():
    assert A.layout(576, 1024) == (2, 3, 2)          # int(1600 / 600), round(1.6) + 1, tl - 1
    assert A.layout(100, 80) == (1, 1, 1)            # max(int(0.3), 1), round(0.18) + 1, max(1, 0)
    assert A.layout(576, 1024, line_thickness=5) == (2, 5, 4)


def test_face_draw_list_geometry_and_order():
    info = np.array([[0, 100.0, 200.0, 300.0, 400.0, 0.9, 0.05], [0, -5.0, 0.0, 2000.0, 50.0, 0.8, 0.01]], np.float32)
    lm = np.array([[110, 210, 120, 220], [1, 2, 3, 4]], np.float32)
    dl = A.face_draw_list(info, 2, [(576, 1024)], lmarks=lm, anonymize=16)
    c = dl.host()[0]
    kinds = c["kind"].tolist()
    per_face = [L.DRAW_MOSAIC, L.DRAW_RECT, L.DRAW_RING, L.DRAW_RING, L.DRAW_FILL] + [L.DRAW_GLYPH] * 9
    assert kinds == per_face * 2                       # the mosaic precedes the outline, the bar the caption
    row = lambda k: tuple(int(c[k][f]) for f in ("x0", "y0", "x1", "y1", "arg"))
    assert row(0) == (100, 200, 300, 400, 16) and row(1) == (100, 200, 300, 400, 2)
    assert row(2) == (110, 210, 111, 211, 3) and (c[1]["b"], c[1]["g"], c[1]["r"], c[1]["a"]) == (0, 0, 255, 255)
    s = 2                                              # bar [xmin - 1, xmin + 6 s len + 5) x [ymin - 8 s - 4, ymin), text at (xmin + 3, ymin - 8 s - 2)
    assert row(4)[:4] == (99, 200 - 20, 100 + 12 * 9 + 5, 200) and c[4]["a"] == 128 and (c[4]["b"], c[4]["g"], c[4]["r"]) == (0, 0, 0)
    assert row(5) == (103, 200 - 18, 103 + 12, 200 - 2, ord("0") | 2 << 8) and row(6)[0] == 115
    # the second box is clamped to the frame, and at ymin = 0 the bar and the caption move down by 8 s + 4, inside the box
    assert row(14)[:4] == (0, 0, 1024, 50) and row(15)[:4] == (0, 0, 1024, 50)
    assert row(18)[:4] == (-1, 0, 12 * 9 + 5, 20) and row(19)[:2] == (3, 2)
    assert A.face_draw_list(info, 2, [(576, 1024)], text_bg_alpha=0.0).host()[0][1]["a"] == 255
    no = A.face_draw_list(info, 2, [(576, 1024)]).host()[0]
    assert no["kind"].tolist() == ([L.DRAW_RECT, L.DRAW_FILL] + [L.DRAW_GLYPH] * 9) * 2
    assert A.palette(0) == (128, 0, 0) and A.palette(1) == (0, 128, 0) and A.palette(2) == (128, 128, 0) and A.palette(7) == (64, 0, 0)
    assert len({A.palette(i) for i in range(512)}) == 512


def test_tile_list_is_the_brute_force_set():
    faces = A.face_draw_list(np.array([[0, 60.0, 3.0, 130.0, 70.0, 0.9, 0.05], [0, 900.0, 500.0, 1100.0, 600.0, 0.9, 0.05]], np.float32),
                             2, [(576, 1024)], lmarks=np.array([[64, 64, 0, 0], [1023, 575, 1024, 576]], np.float32), anonymize=8)
    for case in DC.CASES + [("faces", [(576, 1024)], True, faces)]:
        cmds, ranges, tiles = case[3].host()
        want = set()
        for c, (x0, y0, x1, y1) in zip(cmds, A.DrawList.boxes_of(cmds).tolist()):
            h, w = case[1][int(c["frame"])]
            for y in range(max(y0, 0), min(y1, h)):
                for x in range(max(x0, 0), min(x1, w)):
                    want.add((int(c["frame"]), x // 64, y // 64))
        assert [tuple(t) for t in tiles.tolist()] == sorted(want), case[0]
        assert ranges[0] == 0 and ranges[-1] == len(cmds) and (np.diff(ranges) >= 0).all()
        if case[0] == "faces":
            continue
        for f, (src, out) in enumerate(zip(DC.frames(case), DC.expected(case))):     # every changed pixel lies in a listed tile
            ys, xs = np.nonzero(changed(src, out))
            assert {(f, int(x) // 64, int(y) // 64) for x, y in zip(xs, ys)} <= want


def test_step_labels_of_a_result_with_attributes():
    res = dict(n_faces=2, identity=torch.tensor([1, -1], dtype=torch.int32),
               age_probs=torch.tensor([[0, 0, 0, 0, .9, .1, 0, 0], [float("nan")] * 8]), gender_probs=torch.tensor([[.2, .8], [.5, .5]]))
    assert A.step_labels(res, {1: "Bo"}) == [" Bo Female(25-32)", ""]
    assert A.step_labels(res, ["x", "y"]) == [" y Female(25-32)", ""]
    assert A.step_labels(dict(n_faces=2)) is None


# ---------------------------------------------------------------------------------------------------- refusals

def _arrays(dl):
    cmds, ranges, tiles = (a.copy() for a in dl.host())
    sizes = dl.sizes
    offs = np.cumsum([0] + [3 * h * w for h, w in sizes])
    from face_detection_and_recognition_amd.frames import frame_descs
    return int(offs[-1]), frame_descs(offs[:-1], sizes), cmds, ranges, tiles


def _emulate_rc(lib, total, descs, cmds, ranges, tiles, frames=True, font=True):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(total, np.uint8)
    return lib.fp_draw_emulate(p(buf) if frames else None, total, p(descs), len(descs), p(cmds), p(ranges), len(cmds), p(tiles),
                               len(tiles), p(np.frombuffer(F.FONT, np.uint8)) if font else None)


def test_refusals(lib):
    dl = A.DrawList([(70, 70), (20, 20)])
    dl.mosaic(0, 1, 1, 69, 69, 8)
    dl.rect(1, 2, 2, 9, 9)
    total, descs, cmds, ranges, tiles = _arrays(dl)
    assert _emulate_rc(lib, total, descs, cmds, ranges, tiles) == L.FP_OK
    for cell in (0, 3, 5, 64, -8):
        bad = cmds.copy()
        bad["arg"][0] = cell
        assert _emulate_rc(lib, total, descs, bad, ranges, tiles) == L.FP_ERR_INVALID_ARG, cell
        with pytest.raises(ValueError):
            dl.mosaic(0, 0, 0, 5, 5, cell)
    for f in (-1, 2):
        bad = cmds.copy()
        bad["frame"][1] = f
        assert _emulate_rc(lib, total, descs, bad, ranges, tiles) == L.FP_ERR_INVALID_ARG
        bad_t = tiles.copy()
        bad_t[-1, 0] = f
        assert _emulate_rc(lib, total, descs, cmds, ranges, bad_t) == L.FP_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            dl.fill(f, 0, 0, 1, 1)
    for col, v in ((1, 2), (2, 2), (1, -1)):                          # tile (2, y) / (x, 2) of a 70 x 70 frame does not exist
        bad_t = tiles.copy()
        bad_t[0, col] = v
        assert _emulate_rc(lib, total, descs, cmds, ranges, bad_t) == L.FP_ERR_INVALID_ARG
    assert _emulate_rc(lib, total, descs, cmds, ranges, np.concatenate([tiles[:1], tiles])) == L.FP_ERR_INVALID_ARG   # a tile twice
    assert _emulate_rc(lib, total - 1, descs, cmds, ranges, tiles) == L.FP_ERR_INVALID_ARG                          # a frame past the buffer
    bad_r = ranges.copy()
    bad_r[1] = 3
    assert _emulate_rc(lib, total, descs, cmds, bad_r, tiles) == L.FP_ERR_INVALID_ARG
    assert _emulate_rc(lib, total, descs, cmds, ranges, tiles, frames=False) == L.FP_ERR_INVALID_ARG
    assert _emulate_rc(lib, total, descs, cmds, ranges, tiles, font=False) == L.FP_ERR_INVALID_ARG
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.fp_draw_check(total, None, 2, p(cmds), p(ranges), 2, p(tiles), len(tiles)) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw_check(total, p(descs), 2, None, p(ranges), 2, p(tiles), len(tiles)) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw_check(total, p(descs), 2, p(cmds), p(ranges), -1, p(tiles), len(tiles)) == L.FP_ERR_INVALID_ARG
    # fp_draw itself refuses before any launch (no device is touched): NULL pointers, negative counts
    one = ctypes.c_void_p(16)
    assert lib.fp_draw(None, 10, one, 1, one, one, 1, one, 1, one, None) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw(one, 10, one, 1, None, one, 1, one, 1, one, None) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw(one, 10, one, 1, one, one, 1, one, 1, None, None) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw(one, 10, one, 1, one, one, 1, one, -1, one, None) == L.FP_ERR_INVALID_ARG
    assert lib.fp_draw(one, 10, one, 1, None, one, 0, None, 0, one, None) == L.FP_OK       # an empty list: nothing launched


def test_bad_kind_and_glyph_code_are_skipped_not_refused(lib):
    dl = A.DrawList([(12, 12)])
    dl.fill(0, 0, 0, 12, 12, (5, 5, 5))
    dl.text(0, 1, 1, "A")
    dl.rect(0, 1, 1, 5, 5)
    total, descs, cmds, ranges, tiles = _arrays(dl)
    cmds["kind"][0] = 9
    cmds["arg"][1] = 200 | 1 << 8
    cmds["arg"][2] = 0                                   # thickness 0
    buf = np.full(total, 77, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.fp_draw_emulate(p(buf), total, p(descs), 1, p(cmds), p(ranges), 3, p(tiles), len(tiles), p(np.frombuffer(F.FONT, np.uint8))) == 0
    assert (buf == 77).all()
    fake = A.DrawList([(12, 12)])
    fake._done = (cmds, ranges, tiles)
    assert (A.draw_numpy([np.full((12, 12, 3), 77, np.uint8)], fake)[0] == 77).all()


def test_draw_cmd_layout_and_prototypes_match_a_c_compiler(lib, tmp_path):
    """fp_draw_cmd as a C99 compiler lays it out equals the ctypes mirror and the numpy record the lists are built in; the three
    prototypes have the argument types _lib.py binds; the constants agree."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['printf("fp_draw_cmd %zu\\n", sizeof(fp_draw_cmd));']
    for fname, _ in L.FpDrawCmd._fields_:
        lines.append('printf("fp_draw_cmd.%s %%zu\\n", offsetof(fp_draw_cmd, %s));' % (fname, fname))
    src = tmp_path / "draw.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "facepath.h"
int main(void) {
  int (*draw)(uint8_t*, size_t, const fp_frame_desc*, int, const fp_draw_cmd*, const int32_t*, int, const int32_t*, int,
              const uint8_t*, void*) = fp_draw;
  int (*check)(size_t, const fp_frame_desc*, int, const fp_draw_cmd*, const int32_t*, int, const int32_t*, int) = fp_draw_check;
  int (*emulate)(uint8_t*, size_t, const fp_frame_desc*, int, const fp_draw_cmd*, const int32_t*, int, const int32_t*, int,
                 const uint8_t*) = fp_draw_emulate;
  /*PRINTS*/
  printf("kinds %d %d %d %d %d\\n", FP_DRAW_RECT, FP_DRAW_FILL, FP_DRAW_RING, FP_DRAW_GLYPH, FP_DRAW_MOSAIC);
  printf("consts %d %d %d %d %d\\n", FP_DRAW_TILE, FP_DRAW_FONT_BYTES, FP_DRAW_MAX_ARG, FP_DRAW_MAX_SCALE, FP_DRAW_MAX_COORD);
  printf("abi %d %d\\n", FP_ABI_VERSION, fp_abi_version());
  return (draw == NULL) + (check == NULL) + (emulate == NULL);
}
""".replace("/*PRINTS*/", "\n  ".join(lines)))
    libdir = os.path.dirname(L.LIB_PATH)
    exe = tmp_path / "draw"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-L", libdir, "-lfacepath", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert int(got["fp_draw_cmd"][0]) == ctypes.sizeof(L.FpDrawCmd) == A.CMD_DTYPE.itemsize == 32
    for fname, _ in L.FpDrawCmd._fields_:
        assert int(got[f"fp_draw_cmd.{fname}"][0]) == getattr(L.FpDrawCmd, fname).offset == A.CMD_DTYPE.fields[fname][1], fname
    assert [int(v) for v in got["kinds"]] == [L.DRAW_RECT, L.DRAW_FILL, L.DRAW_RING, L.DRAW_GLYPH, L.DRAW_MOSAIC]
    assert [int(v) for v in got["consts"]] == [L.DRAW_TILE, L.DRAW_FONT_BYTES, L.DRAW_MAX_ARG, L.DRAW_MAX_SCALE, L.DRAW_MAX_COORD]
    assert [int(v) for v in got["abi"]] == [L.ABI_VERSION, L.ABI_VERSION] == [15, 15]


# ---------------------------------------------------------------------------------------------------- the programs' flags

def test_programs_parse_output_and_anonymize():
    from face_detection_and_recognition_amd import detect_face_blazeface, detect_face_mtcnn, detect_face_yolov5_face
    from face_detection_and_recognition_amd.modules.mtcnn.model import SLOW_WEIGHTS
    common = dict(input_src="x.jpg", det_thres=0.7, bbox_area_thres=0.12, device="hip")
    today = {
        detect_face_blazeface: dict(common, model="weights/blazeface/blazefaceback.pth", model_type="back"),
        detect_face_yolov5_face: dict(common, model="weights/yolov5s/yolov5s-face.pt", input_size=(640, 640)),
        detect_face_mtcnn: dict(common, model=SLOW_WEIGHTS, model_type="fast"),
    }
    for mod, want in today.items():
        assert vars(mod.build_parser().parse_args(["-i", "x.jpg"])) == want, mod.__name__       # without the flags: today's namespace
        got = vars(mod.build_parser().parse_args(["-i", "x.jpg", "-o", "out.jpg", "--anonymize", "16"]))
        assert got == dict(want, output="out.jpg", anonymize=16)
        assert vars(mod.build_parser().parse_args(["-i", "x.jpg", "--output", "o.jpg"])) == dict(want, output="o.jpg")
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["-i", "x.jpg", "--anonymize", "5"])
