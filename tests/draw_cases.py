"""Shared cases of the drawing tests (test_draw_cpu.py, test_draw_gpu.py): small frames whose commands sit where the tile
kernel can go wrong -- tile corners, frame edges, compaction chunks, command order -- and nowhere else.  A case is
(name, sizes, dense, DrawList); frames(case) gives its seeded random input, a list of (h, w, 3) u8 arrays."""
import numpy as np

from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.annotate import DrawList

KINDS = ("rect", "fill", "ring", "text", "mosaic")


def one_of_each(dl, f, x, y, size=20, alpha=255):
    """Every kind once, around (x, y): they overlap, so their order matters too."""
    dl.mosaic(f, x - size, y - size, x + size // 2, y + size // 2, 8)
    dl.rect(f, x - size // 2, y - size // 2, x + size, y + size, (10, 200, 30), 3, alpha)
    dl.fill(f, x - 3, y - 5, x + size, y + 4, (200, 20, 90), 128)
    dl.ring(f, x, y, 7, (0, 255, 255), alpha)
    dl.ring(f, x + 2, y - 1, 3, (0, 0, 255))
    dl.text(f, x - 11, y - 4, "a_0.9)", (255, 255, 255), 2, alpha)


def _ragged3():
    sizes = [(70, 131), (64, 64), (5, 3)]       # 5 x 3: the narrowest frame the ragged kernels take
    dl = DrawList(sizes)
    one_of_each(dl, 0, 64, 60)                  # crosses x = 64 and the tile row's lower edge (y = 64 .. 69 is a 6-row tile)
    one_of_each(dl, 0, 125, 66, alpha=77)       # the third, 3-pixel-wide tile column and the bottom rows
    one_of_each(dl, 1, 32, 32)
    dl.rect(1, 0, 0, 64, 64, (1, 2, 3), 1)      # the frame's own border
    one_of_each(dl, 2, 1, 2, size=2)
    dl.mosaic(2, 0, 0, 3, 5, 4)
    dl.text(2, 0, 0, "1", (9, 9, 9), 1, 200)
    return sizes, False, dl


def _dense2():
    sizes = [(100, 80)] * 2
    dl = DrawList(sizes)
    one_of_each(dl, 1, 70, 64)                  # appended out of frame order: finish() sorts
    one_of_each(dl, 0, 10, 90, alpha=128)
    dl.text(0, 2, 50, "conf 0.87_1.25 {~}", (0, 255, 0), 1)     # runs over the right edge
    dl.mosaic(1, 0, 0, 80, 100, 32)
    return sizes, True, dl


def _corner():
    """Each kind across the corner of four tiles, pixel (64, 64) of a 130 x 130 frame (tiles of 64, 64 and 2 pixels)."""
    sizes = [(130, 130)]
    dl = DrawList(sizes)
    dl.mosaic(0, 50, 50, 80, 80, 16)
    dl.mosaic(0, 61, 61, 67, 67, 4)
    dl.rect(0, 60, 60, 70, 70, (0, 0, 255), 1)
    dl.rect(0, 40, 40, 129, 129, (255, 0, 0), 4, 100)
    dl.fill(0, 62, 62, 66, 66, (7, 77, 177), 200)
    dl.ring(0, 64, 64, 3, (0, 0, 255))
    dl.ring(0, 64, 64, 40, (20, 30, 40), 128)
    dl.text(0, 52, 61, "0.95", (255, 255, 255), 1)
    dl.text(0, 40, 50, "Xg", (250, 250, 0), 3)
    dl.mosaic(0, 120, 120, 130, 130, 32)
    return sizes, True, dl


def _edges():
    """Each kind clipped by each of the four frame edges, and wholly outside on each side."""
    h, w = 70, 90
    sizes = [(h, w)]
    dl = DrawList(sizes)
    spots = [(-4, 30), (w - 3, 30), (40, -4), (40, h - 3),                       # cut by left, right, top, bottom
             (-60, 30), (w + 40, 30), (40, -60), (40, h + 40), (-500000, -500000)]   # outside
    for x, y in spots:
        dl.mosaic(0, x - 6, y - 6, x + 9, y + 9, 4)
        dl.rect(0, x - 5, y - 5, x + 8, y + 8, (0, 0, 255), 2)
        dl.fill(0, x - 2, y - 2, x + 6, y + 3, (0, 0, 0), 128)
        dl.ring(0, x, y, 5, (255, 0, 255))
        dl.text(0, x - 4, y - 3, "A1", (255, 255, 255), 1)
    dl.rect(0, -10, -10, w + 10, h + 10, (5, 5, 5), 3)      # the outline lies wholly outside the frame
    dl.mosaic(0, -100, -100, w + 100, h + 100, 16)          # every cell, the edge cells cut by the frame
    return sizes, True, dl


def _order(reverse):
    sizes = [(40, 70)]
    dl = DrawList(sizes)
    steps = [lambda: dl.mosaic(0, 5, 5, 66, 35, 8), lambda: dl.rect(0, 10, 8, 60, 30, (0, 0, 255), 3),
             lambda: dl.fill(0, 8, 6, 40, 20, (255, 255, 255), 128)]
    for s in (reversed(steps) if reverse else steps):
        s()
    return sizes, True, dl


def _many():
    """600 commands that all meet tile (0, 0) of the frame: three compaction chunks of 256, the last one partly filled; a few
    more that miss it lie between them in the list."""
    sizes = [(100, 100)]
    dl = DrawList(sizes)
    rng = np.random.default_rng(600)
    for k in range(600):
        x, y = int(rng.integers(0, 60)), int(rng.integers(0, 60))
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        kind = k % 5
        if kind == 0:
            dl.rect(0, x, y, x + int(rng.integers(1, 30)), y + int(rng.integers(1, 30)), col, int(rng.integers(1, 4)), int(rng.integers(0, 256)))
        elif kind == 1:
            dl.fill(0, x, y, x + int(rng.integers(1, 12)), y + int(rng.integers(1, 12)), col, int(rng.integers(0, 256)))
        elif kind == 2:
            dl.ring(0, x, y, int(rng.integers(0, 9)), col)
        elif kind == 3:
            dl.text(0, x, y, chr(int(rng.integers(32, 127))), col, int(rng.integers(1, 3)))
        else:
            dl.mosaic(0, x, y, x + int(rng.integers(1, 40)), y + int(rng.integers(1, 40)), (4, 8, 16, 32)[int(rng.integers(0, 4))])
        if k % 50 == 7:
            dl.fill(0, 70, 70, 95, 95, col, 60)             # tile (1, 1) only
    return sizes, True, dl


def _glyphs():
    sizes = [(60, 200)]
    dl = DrawList(sizes)
    dl.text(0, 1, 1, "0123456789._-()", (255, 255, 255), 1)
    dl.text(0, 1, 12, "AaBbGgQq" + chr(200) + "\n", (0, 255, 255), 3, 180)       # the last two become '?'
    dl.text(0, 58, 40, "tile", (255, 0, 0), 3)                                # crosses x = 64 and 128
    return sizes, True, dl


def _mosaics():
    sizes = [(100, 140)]
    dl = DrawList(sizes)
    for k, cell in enumerate(L.DRAW_MOSAIC_CELLS):
        dl.mosaic(0, 3 + 33 * k, 7, 3 + 33 * k + 37, 93, cell)     # unaligned rectangles, overlapping their neighbours
    return sizes, True, dl


def _gap():
    sizes = [(66, 66)] * 3
    dl = DrawList(sizes)
    one_of_each(dl, 0, 60, 60)
    one_of_each(dl, 2, 5, 5)          # frame 1 has no command
    return sizes, True, dl


def _empty():
    sizes = [(10, 12), (9, 9)]
    return sizes, False, DrawList(sizes)


CASES = [("ragged3",) + _ragged3(), ("dense2",) + _dense2(), ("corner",) + _corner(), ("edges",) + _edges(),
         ("fill_over_rect_over_mosaic",) + _order(False), ("mosaic_over_rect_over_fill",) + _order(True),
         ("many600",) + _many(), ("glyphs",) + _glyphs(), ("mosaics",) + _mosaics(), ("gap",) + _gap(), ("empty",) + _empty()]
IDS = [c[0] for c in CASES]


def frames(case):
    """The case's input: seeded random u8 frames (full range, so rounding and blending see every value)."""
    name, sizes = case[0], case[1]
    rng = np.random.default_rng(sum(name.encode()))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


_WANT = {}


def expected(case):
    """draw_numpy of the case, computed once and shared (read-only)."""
    from face_detection_and_recognition_amd.annotate import draw_numpy
    if case[0] not in _WANT:
        out = draw_numpy(frames(case), case[3])
        for f in out:
            f.setflags(write=False)
        _WANT[case[0]] = out
    return _WANT[case[0]]
