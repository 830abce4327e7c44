"""The MTCNN procedure of DESIGN.md section 7, restated once in float64 numpy / torch-CPU: the yardstick of the MTCNN tests.

Nothing here is shared with the package's kernels or plans: the nets run LITERALLY as the ports run them (the image with its
two spatial axes swapped, torch convs, the state dict's weights untouched), resizes are dense weight matrices, the NMS is the
plain greedy loop.  `dtype` switches the NETS to float32 (the reference-side measurement of how much the cascade amplifies
last-bit differences); everything around them stays float64.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ---- pyramid ----
def pyramid(h, w, min_face_size, factor):
    m = 12.0 / min_face_size
    out, k = [], 0
    while min(h, w) * m * factor ** k >= 12:
        s = m * factor ** k
        out.append((s, int(math.ceil(h * s)), int(math.ceil(w * s))))
        k += 1
    return out


# ---- resizes ----
# Exact integer arithmetic: lengths along an axis are counted in units of 1 / n_dst source cells, so every weight is an
# integer, a row of weights sums to n_src, and the resized value is S / (h w) with S an integer: rounding half-to-even is
# then exact too (a float64 mean would leave genuine ties, which do occur, to the last bit of the summation order).
def area_matrix(n_src, n_dst):
    """(n_dst, n_src) int64: row d = the length of source cell s inside [d n_src, (d + 1) n_src) (n_src >= n_dst)."""
    m = np.zeros((n_dst, n_src), np.int64)
    for d in range(n_dst):
        f1, f2 = d * n_src, (d + 1) * n_src
        for s in range(f1 // n_dst, (f2 - 1) // n_dst + 1):
            m[d, s] = min((s + 1) * n_dst, f2) - max(s * n_dst, f1)
    return m


def linear_area_matrix(n_src, n_dst):
    """cv2's linear taps in area mode (INTER_AREA when an axis grows): s = floor(d scale), f = (d + 1) - (s + 1) / scale,
    f <= 0 ? 0 : f - floor(f), scale = n_src / n_dst; weight 1 - f on s, f on s + 1 (clamped to the last cell, f = 0 there).
    (n_dst, n_src) int64 with the weights times n_src."""
    m = np.zeros((n_dst, n_src), np.int64)
    for d in range(n_dst):
        s = (d * n_src) // n_dst
        a = (d + 1) * n_src - (s + 1) * n_dst
        a = 0 if a <= 0 else a % n_src
        if s >= n_src - 1:
            s, a = n_src - 1, 0
        m[d, s] += n_src - a
        if a > 0:
            m[d, s + 1] += a
    return m


def resize_u8(img, oh, ow):
    """img (h, w, 3) u8 -> (oh, ow, 3) u8: the area mean when neither axis grows, else the linear area-mode taps on both
    axes; rounded half-to-even."""
    h, w = img.shape[:2]
    if h >= oh and w >= ow:
        my, mx = area_matrix(h, oh), area_matrix(w, ow)
    else:
        my, mx = linear_area_matrix(h, oh), linear_area_matrix(w, ow)
    rows = np.tensordot(my, img.astype(np.int64), axes=(1, 0))          # (oh, w, 3)
    s = np.tensordot(mx, rows, axes=(1, 1)).transpose(1, 0, 2)
    d = h * w
    q, r = s // d, s % d
    q = q + ((2 * r > d) | ((2 * r == d) & (q % 2 == 1)))
    return np.ascontiguousarray(q).astype(np.uint8)


def cut(img, box):
    """The zero-filled (y2 - y1 + 1) x (x2 - x1 + 1) patch of the ports' inclusive 1-based pad rule: patch pixel (py, px) is
    frame pixel (y1 - 1 + py, x1 - 1 + px) where that lies inside the frame."""
    h, w = img.shape[:2]
    x1, y1, x2, y2 = (int(v) for v in box)
    pw, ph = x2 - x1 + 1, y2 - y1 + 1
    patch = np.zeros((ph, pw, 3), np.uint8)
    sy0, sy1 = max(y1 - 1, 0), min(y2, h)
    sx0, sx1 = max(x1 - 1, 0), min(x2, w)
    if sy1 > sy0 and sx1 > sx0:
        patch[sy0 - (y1 - 1): sy1 - (y1 - 1), sx0 - (x1 - 1): sx1 - (x1 - 1)] = img[sy0:sy1, sx0:sx1]
    return patch


def normalise(u8):
    return (u8.astype(np.float64) - 127.5) * 0.0078125


# ---- nets, literally ----
def _t(sd, key, dtype):
    return sd[key].detach().cpu().to(dtype)


def _conv_prelu(sd, pre, i, x, dtype):
    x = F.conv2d(x, _t(sd, f"{pre}.conv{i}.weight", dtype), _t(sd, f"{pre}.conv{i}.bias", dtype))
    return F.prelu(x, _t(sd, f"{pre}.prelu{i}.weight", dtype))


def pnet(sd, x, dtype=torch.float64):
    """x (N, H, W, 3) normalised -> (prob of a face (N, oh, ow), reg (N, oh, ow, 4), logits (N, oh, ow, 2))."""
    x = torch.as_tensor(x).to(dtype).permute(0, 3, 2, 1)           # NCHW of the image with its axes swapped
    x = _conv_prelu(sd, "pnet", 1, x, dtype)
    x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    x = _conv_prelu(sd, "pnet", 2, x, dtype)
    x = _conv_prelu(sd, "pnet", 3, x, dtype)
    z = F.conv2d(x, _t(sd, "pnet.cls.weight", dtype), _t(sd, "pnet.cls.bias", dtype))
    r = F.conv2d(x, _t(sd, "pnet.reg.weight", dtype), _t(sd, "pnet.reg.bias", dtype))
    p = torch.softmax(z, 1)[:, 1]
    # swap the axes back
    return (p.permute(0, 2, 1).double().numpy(), r.permute(0, 3, 2, 1).double().numpy(), z.permute(0, 3, 2, 1).double().numpy())


def _refine_net(sd, pre, x, dtype):
    x = torch.as_tensor(x).to(dtype).permute(0, 3, 2, 1)
    x = _conv_prelu(sd, pre, 1, x, dtype)
    x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    x = _conv_prelu(sd, pre, 2, x, dtype)
    x = F.max_pool2d(x, 3, 2)
    x = _conv_prelu(sd, pre, 3, x, dtype)
    n_prelu = 4
    if pre == "onet":
        x = F.max_pool2d(x, 2, 2, ceil_mode=True)
        x = _conv_prelu(sd, pre, 4, x, dtype)
        n_prelu = 5
    x = x.flatten(1)
    x = F.linear(x, _t(sd, f"{pre}.fc.weight", dtype), _t(sd, f"{pre}.fc.bias", dtype))
    x = F.prelu(x, _t(sd, f"{pre}.prelu{n_prelu}.weight", dtype))
    z = F.linear(x, _t(sd, f"{pre}.cls.weight", dtype), _t(sd, f"{pre}.cls.bias", dtype))
    r = F.linear(x, _t(sd, f"{pre}.reg.weight", dtype), _t(sd, f"{pre}.reg.bias", dtype))
    if pre == "onet":
        r = torch.cat([r, F.linear(x, _t(sd, "onet.lmk.weight", dtype), _t(sd, "onet.lmk.bias", dtype))], 1)
    return torch.softmax(z, 1)[:, 1].double().numpy(), r.double().numpy(), z.double().numpy()


def rnet(sd, x, dtype=torch.float64):
    """x (N, 24, 24, 3) normalised -> (prob (N,), reg (N, 4), logits (N, 2))."""
    return _refine_net(sd, "rnet", x, dtype)


def onet(sd, x, dtype=torch.float64):
    """x (N, 48, 48, 3) normalised -> (prob (N,), reg (N, 14): box, five x, five y; logits (N, 2))."""
    return _refine_net(sd, "onet", x, dtype)


# ---- boxes ----
def iou_parts(box, boxes, mode):
    """(intersection, denominator) of the + 1 IoU of one box against many: the denominator is the union, or min(a_i, a_j)."""
    a = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
    b = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    iw = np.maximum(0.0, np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]) + 1)
    ih = np.maximum(0.0, np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]) + 1)
    inter = iw * ih
    return inter, (np.minimum(a, b) if mode == "min" else a + b - inter)


def nms(boxes, scores, thr, mode="union", margins=None):
    """Greedy NMS; returns the kept indices in visiting order (descending score, equal scores: the lower index first).
    margins: a list that receives |o - thr| of every comparison made; a comparison with o == thr is recorded as 0.0 only if it
    is an exact tie of integer boxes (inter * den == num * denominator for thr = num / den), otherwise as -1.0."""
    from fractions import Fraction
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    alive = np.ones(len(order), bool)
    keep = []
    frac = Fraction(thr).limit_denominator(1000)
    whole = bool(len(boxes)) and bool((boxes == np.rint(boxes)).all())
    for pos, i in enumerate(order):
        if not alive[pos]:
            continue
        keep.append(int(i))
        rest = np.nonzero(alive[pos + 1:])[0] + pos + 1
        if len(rest):
            inter, den = iou_parts(boxes[i], boxes[order[rest]], mode)
            o = inter / den
            if margins is not None:
                m = np.abs(o - thr)
                exact = whole & (inter * frac.denominator == frac.numerator * den)
                m[(m == 0) & ~exact] = -1.0
                margins.extend(m.tolist())
            alive[rest[o > thr]] = False
    return np.asarray(keep, np.int64)


def generate_boxes(ys, xs, scale):
    """q1 = trunc((2 (x, y) + 1) / s), q2 = trunc((2 (x, y) + 12) / s) -> (n, 4) float64 (x1, y1, x2, y2)."""
    xy = np.stack([xs, ys], 1).astype(np.float64)
    return np.concatenate([np.trunc((2 * xy + 1) / scale), np.trunc((2 * xy + 12) / scale)], 1)


def regress(boxes, reg, plus_one):
    w = boxes[:, 2] - boxes[:, 0] + plus_one
    h = boxes[:, 3] - boxes[:, 1] + plus_one
    return boxes + reg[:, :4] * np.stack([w, h, w, h], 1)


def square(b):
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    l = np.maximum(w, h)
    x1 = b[:, 0] + w * 0.5 - l * 0.5
    y1 = b[:, 1] + h * 0.5 - l * 0.5
    return np.stack([x1, y1, x1 + l, y1 + l], 1)


def positive(b):
    return (b[:, 2] - b[:, 0] + 1 > 0) & (b[:, 3] - b[:, 1] + 1 > 0)


# ---- the cascade on one frame ----
def detect(frame, sd, min_face_size=20, factor=0.709, thresholds=(0.6, 0.7, 0.7), dtype=torch.float64, trace=None):
    """frame (h, w, 3) u8 -> (n, 15) float64 rows [x1, y1, x2, y2, (x, y) x 5, score] in frame pixels, by descending score.
    trace: a dict that receives every intermediate (teacher forcing, margins)."""
    t1, t2, t3 = thresholds
    tr = trace if trace is not None else {}
    tr["nms_margins"] = {"level": [], "frame": [], "rnet": [], "onet": []}       # |o - threshold| of every comparison, per NMS
    tr["trunc_margins"], tr["nms_dropped"] = [], {"level": 0, "frame": 0, "rnet": 0, "onet": 0}
    h, w = frame.shape[:2]
    lv_i, cells, scores, regs, qs, keep_level = [], [], [], [], [], []
    base = 0
    for li, (s, lh, lw) in enumerate(pyramid(h, w, min_face_size, factor)):
        p, r, _ = pnet(sd, normalise(resize_u8(frame, lh, lw))[None], dtype)
        p, r = p[0], r[0]
        ys, xs = np.nonzero(p >= t1)                      # row-major: (y, x) ascending = cell order
        if len(ys) == 0:
            continue
        q = generate_boxes(ys, xs, s)
        k = nms(q, p[ys, xs], 0.5, "union", tr["nms_margins"]["level"])
        tr["nms_dropped"]["level"] += len(ys) - len(k)
        lv_i.append(np.full(len(ys), li)); cells.append(ys * p.shape[1] + xs); scores.append(p[ys, xs]); regs.append(r[ys, xs]); qs.append(q)
        keep_level.append(base + k)
        base += len(ys)
    cat = lambda a, shape: np.concatenate(a) if a else np.zeros(shape)
    tr["s1"] = dict(level=cat(lv_i, (0,)).astype(np.int64), cell=cat(cells, (0,)).astype(np.int64), score=cat(scores, (0,)),
                    reg=cat(regs, (0, 4)), q=cat(qs, (0, 4)))
    kl = cat(keep_level, (0,)).astype(np.int64)
    q, sc, rg = tr["s1"]["q"][kl], tr["s1"]["score"][kl], tr["s1"]["reg"][kl]
    k = nms(q, sc, 0.7, "union", tr["nms_margins"]["frame"])
    tr["nms_dropped"]["frame"] += len(kl) - len(k)
    tr["s1"].update(keep_level=kl, keep_frame=kl[k])
    pre = square(regress(q[k], rg[k], 0.0))
    tr["trunc_margins"].extend(np.abs(pre - np.rint(pre)).ravel().tolist())
    b = np.trunc(pre)
    ok = positive(b)
    boxes1, score1 = b[ok], sc[k][ok]
    tr["s1"].update(boxes=boxes1.copy(), out_score=score1.copy(), pre=pre, ok=ok)
    if len(boxes1) == 0:
        tr["s2"] = tr["s3"] = None
        return np.zeros((0, 15))

    def refine(boxes, size, net):
        x = np.stack([normalise(resize_u8(cut(frame, bx), size, size)) for bx in boxes])
        return net(sd, x, dtype)

    p2, r2, _ = refine(boxes1, 24, rnet)
    tr["s2"] = s2 = stage2_from(boxes1, p2, r2, t2, tr["nms_margins"]["rnet"])
    tr["nms_dropped"]["rnet"] += len(s2["passed"]) - len(s2["keep"])
    tr["trunc_margins"].extend(np.abs(s2["pre"] - np.rint(s2["pre"])).ravel().tolist())
    boxes2 = s2["boxes"]
    if len(boxes2) == 0:
        tr["s3"] = None
        return np.zeros((0, 15))

    p3, r3, _ = refine(boxes2, 48, onet)
    tr["s3"] = s3 = stage3_from(boxes2, p3, r3, t3, tr["nms_margins"]["onet"])
    tr["nms_dropped"]["onet"] += len(s3["passed"]) - len(s3["keep"])
    return s3["dets"].copy()


def stage2_from(boxes, p, r, t, margins=None):
    """Stage 2 behind R-Net: boxes (n, 4) integers, p (n,), r (n, 4) -> dict(prob, reg, passed, keep (candidate indices in kept
    order), pre (the kept boxes regressed and squared, before truncation), ok (which survive the positive-side rule), boxes
    (truncated survivors), out_score)."""
    boxes, p, r = np.asarray(boxes, np.float64), np.asarray(p, np.float64), np.asarray(r, np.float64)
    ps = np.nonzero(p >= t)[0]
    k = ps[nms(boxes[ps], p[ps], 0.7, "union", margins)]
    pre = square(regress(boxes[k], r[k], 1.0))
    b = np.trunc(pre)
    ok = positive(b)
    return dict(prob=p, reg=r, passed=ps, keep=k, pre=pre, ok=ok, boxes=b[ok], out_score=p[k][ok])


def stage3_rows(boxes, r):
    """(n, 14): the box regressed with w = x2 - x1 + 1 (not squared), then the five landmarks (x, y) on the input box."""
    boxes, r = np.asarray(boxes, np.float64), np.asarray(r, np.float64)
    bw = boxes[:, 2] - boxes[:, 0] + 1
    bh = boxes[:, 3] - boxes[:, 1] + 1
    rows = np.zeros((len(boxes), 14))
    rows[:, :4] = regress(boxes, r, 1.0)
    rows[:, 4:14:2] = boxes[:, 0:1] - 1 + bw[:, None] * r[:, 4:9]
    rows[:, 5:14:2] = boxes[:, 1:2] - 1 + bh[:, None] * r[:, 9:14]
    return rows


def stage3_from(boxes, p, r, t, margins=None):
    """Stage 3 behind O-Net -> dict(prob, reg, passed, keep, regressed (boxes of the passed), dets (n, 15) by descending score)."""
    p = np.asarray(p, np.float64)
    ps = np.nonzero(p >= t)[0]
    rows = stage3_rows(np.asarray(boxes, np.float64)[ps], np.asarray(r, np.float64)[ps])
    k = nms(rows[:, :4], p[ps], 0.7, "min", margins)
    dets = np.concatenate([rows[k], p[ps][k][:, None]], 1) if len(k) else np.zeros((0, 15))
    return dict(prob=p, reg=np.asarray(r, np.float64), passed=ps, keep=ps[k], regressed=rows[:, :4], dets=dets)


def match(a, b, iou=0.9):
    """One-to-one greedy matching of rows a, b (n, >= 4) at IoU >= iou (plain IoU, no + 1) -> [(i, j)], unmatched a, unmatched b."""
    pairs, used = [], set()
    for i, r in enumerate(a):
        best, bj = 0.0, -1
        for j, q in enumerate(b):
            if j in used:
                continue
            iw = max(0.0, min(r[2], q[2]) - max(r[0], q[0]))
            ih = max(0.0, min(r[3], q[3]) - max(r[1], q[1]))
            inter = iw * ih
            u = (r[2] - r[0]) * (r[3] - r[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter
            o = inter / u if u > 0 else 0.0
            if o > best:
                best, bj = o, j
        if bj >= 0 and best >= iou:
            pairs.append((i, bj))
            used.add(bj)
    ua = [i for i in range(len(a)) if i not in {p[0] for p in pairs}]
    ub = [j for j in range(len(b)) if j not in used]
    return pairs, ua, ub
