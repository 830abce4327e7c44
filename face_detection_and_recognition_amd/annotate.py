"""Drawing on device frames: boxes, landmark rings, captions and pixelated faces (build-defined; DESIGN §7 "Drawing").

The reference's detector programs end by showing the picture (modules/utils/image.py draw_bbox_on_image: the box, a ring per
landmark, a conf_area[label] caption on a half-transparent bar).  Its LAYOUT is kept here; its pixels are not (OpenCV's
anti-aliased lines and Hershey font cannot be pinned without OpenCV): every primitive is defined by an integer predicate per
pixel (include/facepath.h "Drawing on device frames"), rasterised by fp_draw (csrc/draw.hip) in place into a (B, H, W, 3)
tensor or a RaggedFrames, and restated by draw_numpy below, which the tests compare against byte for byte.

    dl = face_draw_list(res["info"], res["n_faces"], sizes, anonymize=16)    # or DrawList(sizes) and .rect / .text / ...
    draw(frames, dl)                                                          # one launch, one workgroup per touched tile
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .frames import RaggedFrames, batch_len, device_descs, frame_bytes, frame_descs, frame_layout
from .modules.utils.font6x8 import CELL_H, CELL_W, FIRST, FONT, LAST

CMD_DTYPE = np.dtype([("frame", "<i4"), ("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                      ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("arg", "<i4")])
assert CMD_DTYPE.itemsize == C.sizeof(L.FpDrawCmd) == 32

RED = (0, 0, 255)          # BGR: the reference's box and landmark colour
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
LMARK_RADIUS = 3


def palette(i):
    """A BGR colour for identity / cluster / track number i >= 0: the bits of i + 1 dealt round-robin to the three channels,
    each channel filled from its most significant bit down (1 -> blue 128, 2 -> green 128, 3 -> both, 8 -> blue 64, ...):
    neighbouring indices differ in a high bit of some channel."""
    v, c = int(i) + 1, [0, 0, 0]
    for bit in range(24):
        c[bit % 3] |= ((v >> bit) & 1) << (7 - bit // 3)
    return tuple(c)


class DrawList:
    """An ordered list of drawing commands over a batch of frames of host sizes [(h, w)].  Commands may be appended in any
    frame order; finish() sorts them by frame (stably: the commands of one frame keep their order, which is the order they
    apply in) and derives the per-frame ranges and the touched 64 x 64 tiles.  Rectangles are inclusive-exclusive and may
    lie outside the frame."""

    def __init__(self, sizes):
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self._rows = []
        self._done = None
        self._dev = {}

    def __len__(self):
        return len(self._rows)

    def _add(self, frame, kind, x0, y0, x1, y1, color, alpha, arg):
        frame, x0, y0, x1, y1, alpha, arg = (int(v) for v in (frame, x0, y0, x1, y1, alpha, arg))
        if not 0 <= frame < len(self.sizes):
            raise ValueError(f"frame {frame} outside the batch of {len(self.sizes)}")
        if max(abs(x0), abs(y0), abs(x1), abs(y1)) > L.DRAW_MAX_COORD:
            raise ValueError(f"coordinates ({x0}, {y0}, {x1}, {y1}) outside +-{L.DRAW_MAX_COORD}")
        b, g, r = (int(v) for v in color)
        if not (0 <= alpha <= 255 and all(0 <= v <= 255 for v in (b, g, r))):
            raise ValueError("colour and alpha are 8-bit values")
        self._rows.append((frame, kind, x0, y0, x1, y1, b, g, r, alpha, arg))
        self._done = None
        self._dev = {}

    def rect(self, frame, x0, y0, x1, y1, color=RED, thickness=1, alpha=255):
        """Outline of [x0, x1) x [y0, y1): the rectangle grown by thickness // 2 minus the one shrunk by (thickness + 1) // 2."""
        if not 1 <= int(thickness) <= L.DRAW_MAX_ARG:
            raise ValueError(f"thickness {thickness} outside 1 .. {L.DRAW_MAX_ARG}")
        self._add(frame, L.DRAW_RECT, x0, y0, x1, y1, color, alpha, thickness)

    def fill(self, frame, x0, y0, x1, y1, color=BLACK, alpha=255):
        self._add(frame, L.DRAW_FILL, x0, y0, x1, y1, color, alpha, 0)

    def ring(self, frame, cx, cy, radius=LMARK_RADIUS, color=RED, alpha=255):
        if not 0 <= int(radius) <= L.DRAW_MAX_ARG:
            raise ValueError(f"radius {radius} outside 0 .. {L.DRAW_MAX_ARG}")
        self._add(frame, L.DRAW_RING, cx, cy, int(cx) + 1, int(cy) + 1, color, alpha, radius)

    def text(self, frame, x, y, s, color=WHITE, scale=1, alpha=255):
        """One GLYPH per character, 6 * scale pixels apart, top-left corner (x, y); a character outside 32 .. 126 becomes '?'."""
        scale = int(scale)
        if not 1 <= scale <= L.DRAW_MAX_SCALE:
            raise ValueError(f"scale {scale} outside 1 .. {L.DRAW_MAX_SCALE}")
        for k, ch in enumerate(str(s)):
            code = ord(ch) if FIRST <= ord(ch) <= LAST else ord("?")
            gx = int(x) + k * CELL_W * scale
            self._add(frame, L.DRAW_GLYPH, gx, y, gx + CELL_W * scale, int(y) + CELL_H * scale, color, alpha, code | scale << 8)

    def mosaic(self, frame, x0, y0, x1, y1, cell=16):
        if int(cell) not in L.DRAW_MOSAIC_CELLS:
            raise ValueError(f"mosaic cell {cell} not in {L.DRAW_MOSAIC_CELLS}")
        self._add(frame, L.DRAW_MOSAIC, x0, y0, x1, y1, BLACK, 255, cell)

    # -- the finished arrays ---------------------------------------------------------------------------------------------
    @staticmethod
    def boxes_of(cmds):
        """(N, 4) int64 x0, y0, x1, y1: the bounding box of the pixels each command may set (not clipped)."""
        x0, y0, x1, y1, arg, kind = (cmds[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1", "arg", "kind"))
        grow = np.where(kind == L.DRAW_RECT, arg // 2, 0)
        box = np.stack([x0 - grow, y0 - grow, x1 + grow, y1 + grow], 1)
        ring = kind == L.DRAW_RING
        box[ring] = np.stack([x0 - arg, y0 - arg, x0 + arg + 1, y0 + arg + 1], 1)[ring]
        gl = kind == L.DRAW_GLYPH
        s = arg >> 8
        box[gl] = np.stack([x0, y0, x0 + CELL_W * s, y0 + CELL_H * s], 1)[gl]
        return box

    def host(self):
        """(cmds (N,) CMD_DTYPE sorted by frame, ranges (B + 1,) int32, tiles (T, 3) int32 of (frame, tx, ty), ascending)."""
        if self._done is None:
            cmds = np.array(self._rows, dtype=CMD_DTYPE) if self._rows else np.zeros((0,), CMD_DTYPE)
            cmds = cmds[np.argsort(cmds["frame"], kind="stable")]
            B = len(self.sizes)
            ranges = np.searchsorted(cmds["frame"], np.arange(B + 1)).astype(np.int32)
            tiles = set()
            T = L.DRAW_TILE
            for f, (x0, y0, x1, y1) in zip(cmds["frame"].tolist(), self.boxes_of(cmds).tolist()):
                h, w = self.sizes[f]
                x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
                if x0 < x1 and y0 < y1:
                    tiles.update((f, tx, ty) for tx in range(x0 // T, (x1 - 1) // T + 1) for ty in range(y0 // T, (y1 - 1) // T + 1))
            tiles = np.array(sorted(tiles), np.int32).reshape(-1, 3)
            self._done = (cmds, ranges, tiles)
        return self._done

    def finish(self, device=None):
        """The arrays fp_draw takes on `device` (cmds as (N, 32) u8, ranges, tiles), checked by fp_draw_check first; device
        None: the host arrays of host()."""
        if device is None:
            return self.host()
        device = torch.device(device)
        if device not in self._dev:
            cmds, ranges, tiles = self.host()
            offs = np.cumsum([0] + [3 * h * w for h, w in self.sizes])
            _check(offs[-1], frame_descs(offs[:-1], self.sizes), cmds, ranges, tiles)
            self._dev[device] = tuple(torch.from_numpy(a).to(device) for a in
                                      (cmds.view(np.uint8).reshape(-1, 32), ranges, tiles))
        return self._dev[device]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(total, descs, cmds, ranges, tiles):
    L.check(L.load().fp_draw_check(int(total), _p(descs), len(descs), _p(cmds), _p(ranges), len(cmds), _p(tiles), len(tiles)),
            "fp_draw_check")


_FONT_DEV = {}


def font_device(device):
    """The 760 font bytes on `device` (uploaded once per device)."""
    device = torch.device(device)
    if device not in _FONT_DEV:
        _FONT_DEV[device] = torch.from_numpy(np.frombuffer(FONT, np.uint8).copy()).to(device)
    return _FONT_DEV[device]


def draw(frames, drawlist):
    """Apply `drawlist` in place to frames: a contiguous (B, H, W, 3) u8 device tensor or a RaggedFrames whose sizes are the
    list's.  One launch on the current stream, no host sync.  Returns frames."""
    if isinstance(frames, torch.Tensor) and not (frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
                                                 and frames.is_contiguous() and frames.is_cuda):
        raise ValueError("draw: a contiguous (B, H, W, 3) uint8 device tensor or a RaggedFrames expected")
    sizes = [(h, w) for _, h, w in frame_layout(frames)]
    if sizes != drawlist.sizes:
        raise ValueError("draw: the draw list was built for frames of other sizes")
    cmds, ranges, tiles = drawlist.finish(frames.device)
    data = frame_bytes(frames)
    L.check(L.load().fp_draw(L.ptr(data), data.numel(), L.ptr(device_descs(frames)), batch_len(frames), L.ptr(cmds), L.ptr(ranges),
                             cmds.shape[0], L.ptr(tiles), tiles.shape[0], L.ptr(font_device(frames.device)),
                             L.current_stream(frames.device)), "fp_draw")
    return frames


def draw_emulate(frames_list, drawlist, tiles=None):
    """fp_draw_emulate on host frames (a list of (h, w, 3) u8 numpy arrays, drawn in place): the kernel's procedure run
    serially by the library, no GPU needed.  tiles: another tile list than the draw list's own."""
    cmds, ranges, own = drawlist.host()
    tiles = own if tiles is None else np.ascontiguousarray(tiles, np.int32).reshape(-1, 3)
    sizes = [f.shape[:2] for f in frames_list]
    offs = np.cumsum([0] + [3 * h * w for h, w in sizes])
    buf = np.concatenate([np.ascontiguousarray(f, np.uint8).reshape(-1) for f in frames_list]) if frames_list else np.zeros(0, np.uint8)
    descs = frame_descs(offs[:-1], sizes)
    font = np.frombuffer(FONT, np.uint8)
    L.check(L.load().fp_draw_emulate(_p(buf), buf.size, _p(descs), len(sizes), _p(cmds), _p(ranges), len(cmds), _p(tiles),
                                     len(tiles), _p(font)), "fp_draw_emulate")
    for f, o, (h, w) in zip(frames_list, offs, sizes):
        f[...] = buf[o:o + 3 * h * w].reshape(h, w, 3)
    return frames_list


# ------------------------------------------------------------------------------------------------ the numpy restatement

def _blend(dst, color, a):
    """dst (..., 3) u8 view, blended in place: (dst * (255 - a) + c * a + 127) // 255."""
    c = np.asarray(color, np.int64)
    dst[...] = ((dst.astype(np.int64) * (255 - a) + c * a + 127) // 255).astype(np.uint8)


def _numpy_cmd(img, c):
    """One command on one (h, w, 3) u8 image, by the definitions of include/facepath.h."""
    h, w = img.shape[:2]
    kind, x0, y0, x1, y1, arg = (int(c[k]) for k in ("kind", "x0", "y0", "x1", "y1", "arg"))
    if max(abs(x0), abs(y0)) > L.DRAW_MAX_COORD or (kind != L.DRAW_RING and kind != L.DRAW_GLYPH and max(abs(x1), abs(y1)) > L.DRAW_MAX_COORD):
        return
    color, a = (int(c["b"]), int(c["g"]), int(c["r"])), int(c["a"])
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == L.DRAW_RECT:
        if not 1 <= arg <= L.DRAW_MAX_ARG:
            return
        g, s = arg // 2, (arg + 1) // 2
        grown = (xs >= x0 - g) & (xs < x1 + g) & (ys >= y0 - g) & (ys < y1 + g)
        shrunk = (xs >= x0 + s) & (xs < x1 - s) & (ys >= y0 + s) & (ys < y1 - s)
        mask = grown & ~shrunk
    elif kind == L.DRAW_FILL:
        mask = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    elif kind == L.DRAW_RING:
        if not 0 <= arg <= L.DRAW_MAX_ARG:
            return
        d = 4 * ((xs - x0) ** 2 + (ys - y0) ** 2)
        mask = ((2 * arg - 1) ** 2 <= d) & (d < (2 * arg + 1) ** 2)
    elif kind == L.DRAW_GLYPH:
        code, s = arg & 255, arg >> 8
        if arg < 0 or not (FIRST <= code <= LAST and 1 <= s <= L.DRAW_MAX_SCALE):
            return
        bits = np.array([[(FONT[(code - FIRST) * CELL_H + r] >> (7 - col)) & 1 for col in range(CELL_W)] for r in range(CELL_H)], bool)
        gx, gy = (xs - x0) // s, (ys - y0) // s
        inside = (gx >= 0) & (gx < CELL_W) & (gy >= 0) & (gy < CELL_H)
        mask = inside & bits[np.clip(gy, 0, CELL_H - 1), np.clip(gx, 0, CELL_W - 1)]
    elif kind == L.DRAW_MOSAIC:
        if arg not in L.DRAW_MOSAIC_CELLS:
            return
        rx0, ry0, rx1, ry1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
        for cy in range(ry0 // arg * arg, ry1, arg):
            for cx in range(rx0 // arg * arg, rx1, arg):
                v = img[max(cy, ry0):min(cy + arg, ry1), max(cx, rx0):min(cx + arg, rx1)]
                cnt = v.shape[0] * v.shape[1]
                if cnt:
                    v[...] = ((v.reshape(-1, 3).astype(np.int64).sum(0) + cnt // 2) // cnt).astype(np.uint8)
        return
    else:
        return
    if mask.any():
        px = img[mask]
        _blend(px, color, a)
        img[mask] = px


def draw_numpy(frames_list, drawlist):
    """The restatement the tests compare fp_draw and fp_draw_emulate against: every command of the list, in order, applied to
    its frame (a list of (h, w, 3) u8 numpy arrays, drawn in place) by a whole-image mask per command.  Knows no tiles."""
    cmds, _, _ = drawlist.host()
    for c in cmds:
        _numpy_cmd(frames_list[int(c["frame"])], c)
    return frames_list


# ------------------------------------------------------------------------------------------------ the reference's layout

def caption(conf, area=None, label=None):
    """draw_bbox_on_image's caption: f"{conf:.2f}_{area:.2f}" (f"{conf:.2f}" without areas) + str(label).  conf and area are
    formatted as the reference formats its numpy float32 values: widened to double, not re-rounded from a decimal."""
    s = f"{float(np.float32(conf)):.2f}" if area is None else f"{float(np.float32(conf)):.2f}_{float(np.float32(area)):.2f}"
    return s + (str(label) if label else "")


def layout(h, w, line_thickness=None):
    """(box thickness, tl, caption scale) of a frame of h x w: max(int((w + h) / 600), 1), line_thickness or
    round(0.002 * (w + h) / 2) + 1, max(1, tl - 1)."""
    tl = line_thickness or round(0.002 * (w + h) / 2) + 1
    return max(int((w + h) / 600), 1), int(tl), max(1, int(tl) - 1)


def face_draw_list(info, n, sizes, lmarks=None, labels=None, areas=True, colors=None, anonymize=0, line_thickness=None,
                   text_bg_alpha=0.5):
    """The reference's draw_bbox_on_image layout for the first n rows of info (frame, x1, y1, x2, y2, conf, area), a device
    tensor or a host array; info[:n] (and lmarks[:n], (n, 2k) x, y pairs, when given) is read to the host once.  Per face, in
    this order: MOSAIC of cell `anonymize` over the clamped box (when non-zero), the outline, a ring of radius 3 per landmark
    point, the caption bar and the caption.  labels: one string per face appended to the caption; areas False: the caption
    is the confidence alone; colors: one BGR triple per face (default the reference's red).  The captions are kept in
    .captions of the returned DrawList."""
    rows = info[:n].detach().cpu().numpy() if isinstance(info, torch.Tensor) else np.asarray(info)[:n]
    lm = None
    if lmarks is not None:
        lm = lmarks[:n].detach().cpu().numpy() if isinstance(lmarks, torch.Tensor) else np.asarray(lmarks)[:n]
    dl = DrawList(sizes)
    dl.captions = []
    bar_a = 255 if text_bg_alpha == 0.0 else int((1.0 - float(text_bg_alpha)) * 255 + 0.5)
    for i, row in enumerate(rows):
        f = int(row[0])
        h, w = dl.sizes[f]
        thick, _, s = layout(h, w, line_thickness)
        xmin, ymin, xmax, ymax = (int(v) for v in row[1:5])
        xmin, ymin, xmax, ymax = max(xmin, 0), max(ymin, 0), min(xmax, w), min(ymax, h)
        color = RED if colors is None else tuple(int(v) for v in colors[i])
        if anonymize:
            dl.mosaic(f, xmin, ymin, xmax, ymax, anonymize)
        dl.rect(f, xmin, ymin, xmax, ymax, color, thick)
        if lm is not None and lm.any():
            for k in range(0, lm.shape[1] - 1, 2):
                dl.ring(f, int(lm[i][k]), int(lm[i][k + 1]), LMARK_RADIUS, color)
        text = caption(row[5], row[6] if areas else None, labels[i] if labels else None)
        dl.captions.append(text)
        top = ymin - CELL_H * s - 4
        dy = CELL_H * s + 4 if top < 0 else 0          # no room above the box: the bar and the caption move inside it
        dl.fill(f, xmin - 1, top + dy, xmin + CELL_W * s * len(text) + 5, ymin + dy, BLACK, bar_a)
        dl.text(f, xmin + 3, ymin - CELL_H * s - 2 + dy, text, WHITE, s)
    return dl


def step_labels(result, names=None):
    """One caption suffix per face of a FacePipeline.step result, or None when it carries nothing to say: the gallery name of
    `identity` (names[identity], a dict or a sequence; nothing for -1) -- of `track_identity`, the track's name, when the result
    carries it (FacePipeline(identify_tracks=True)) --, the arg-max gender / age classes and, for a step with a tracker,
    " #<track_id>" (nothing for id 0)."""
    n = result["n_faces"]
    parts = [""] * n
    said = False
    who = "track_identity" if "track_identity" in result else "identity"
    if who in result and names is not None:
        said = True
        for i, k in enumerate(result[who][:n].tolist()):
            if k >= 0:
                parts[i] += " " + str(names.get(k, k) if isinstance(names, dict) else names[k])
    if "age_probs" in result:
        from .modules.age_gender.age_gender_net import AGE_LIST, GENDER_LIST
        said = True
        age, gender = result["age_probs"][:n].cpu().numpy(), result["gender_probs"][:n].cpu().numpy()
        for i in range(n):
            if not (np.isnan(age[i]).any() or np.isnan(gender[i]).any()):
                parts[i] += f" {GENDER_LIST[int(gender[i].argmax())]}{AGE_LIST[int(age[i].argmax())]}"
    if "track_id" in result:
        said = True
        for i, k in enumerate(result["track_id"][:n].tolist()):
            if k > 0:
                parts[i] += f" #{k}"
    return parts if said else None


def step_draw_list(result, sizes, names=None, anonymize=0):
    """face_draw_list of a FacePipeline.step result over frames of `sizes`: captions from step_labels, rings from the
    result's lmarks (x, y pairs; trailing pairs that are zero for every face -- a four-keypoint detector's unused fifth slot --
    are left out)."""
    n = result["n_faces"]
    lm = result.get("lmarks")
    if lm is not None:
        lm = lm[:n].detach().cpu().numpy()
        while lm.shape[1] >= 2 and not lm[:, -2:].any():
            lm = lm[:, :-2]
    return face_draw_list(result["info"], n, sizes, lmarks=lm, labels=step_labels(result, names), anonymize=anonymize)


def annotate_step(frames, result, names=None, anonymize=0, inplace=False):
    """Draw a FacePipeline.step result on its frames ((B, H, W, 3) device tensor or RaggedFrames): box, caption (conf_area,
    the gallery name and the age / gender classes when the result carries them), landmark rings when it carries lmarks, faces
    pixelated first with anonymize = a mosaic cell.  inplace False: a clone is drawn on and returned."""
    if not inplace:
        frames = (RaggedFrames(frames.data.clone(), frames.sizes, frames.offsets, frames.descs)
                  if isinstance(frames, RaggedFrames) else frames.clone())
    sizes = [(h, w) for _, h, w in frame_layout(frames)]
    return draw(frames, step_draw_list(result, sizes, names, anonymize))


def post_dets_draw_list(post, h, w, line_thickness=None, text_bg_alpha=0.5, anonymize=0):
    """face_draw_list of a PostProcessedDetection over one h x w frame (the argument of the reference's draw_bbox_on_image)."""
    n = len(post.boxes)
    info = np.zeros((n, 7), np.float32)
    info[:, 1:5] = np.asarray(post.boxes, np.float32).reshape(n, 4)
    info[:, 5] = np.asarray(post.bbox_confs, np.float32)
    has_areas = post.bbox_areas is not None
    if has_areas:
        info[:, 6] = np.asarray(post.bbox_areas, np.float32)
    lm = None if post.bbox_lmarks is None else np.asarray(post.bbox_lmarks, np.float32)
    if lm is not None:                # (a frame without detections -- common in a video -- has nothing to infer a width from)
        lm = lm.reshape(n, -1) if n else np.zeros((0, 0), np.float32)
    return face_draw_list(info, n, [(h, w)], lmarks=lm if lm is not None and lm.shape[1] >= 2 else None,
                          labels=post.bbox_labels, areas=has_areas, anonymize=anonymize, line_thickness=line_thickness,
                          text_bg_alpha=text_bg_alpha)
