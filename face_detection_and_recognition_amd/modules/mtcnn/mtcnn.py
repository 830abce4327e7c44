"""MTCNN (Zhang et al. 2016: P-Net / R-Net / O-Net) on MI355X: the reference's third detector family
(detect_face_mtcnn.py, modules/mtcnn/model.py), as a cascade whose candidates stay on the device from the u8 frames to the
final rows.  The procedure is written down in DESIGN.md section 7 ("MTCNN").

Stage 1 runs level by level on groups of equally sized frames: fp_pnet_level_images (csrc/pnet.hip) writes the level into the
input of a P-Net plan of generic ops, fp_pnet_threshold emits the passing cells as candidate records.  fp_mtcnn_stage1 / 2 / 3
(csrc/mtcnn.hip) order the candidates, generate / regress / square / truncate boxes and run the NMS; fp_mtcnn_cut cuts the zero-padded squares and resizes them to 24 / 48; R-Net and O-Net are plans
(PlanBuilder).  The host reads one count vector per stage (to size the R-Net / O-Net batch, rounded up to `bucket`) and the
overflow flags.

State-dict layout (our own; every tensor in torch's conventions, conv weights OIHW, linear weights [out, in]):
  pnet.conv1 .. conv3 (.weight, .bias), pnet.prelu1 .. prelu3 (.weight [C]), pnet.cls (2 x 32 x 1 x 1), pnet.reg (4 x 32 x 1 x 1)
  rnet.conv1 .. conv3, prelu1 .. prelu4, rnet.fc (128 x 576), rnet.cls (2 x 128), rnet.reg (4 x 128)
  onet.conv1 .. conv4, prelu1 .. prelu5, onet.fc (256 x 1152), onet.cls, onet.reg, onet.lmk (10 x 256: five x, then five y)
The weights are those of the nets AS THE PORTS RUN THEM: on the image with its two spatial axes swapped (the weights come
from a column-major framework); `fc` flattens that swapped map in (c, row, column) order.  The plans here read
the image as it is: the swap is folded into the weights (kh / kw exchanged; for `fc`, which is run as a conv over the last
map, likewise).  tests/test_mtcnn_cpu.py shows the two agree.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from ... import _lib as L
from ...frames import as_frames, device_descs, frame_bytes, frame_layout
from ...plan import CompiledPlan, PlanBuilder, PlanCache, switch_key
from ..params import ConvParams, LinearParams, PlanCacheMixin, PReLUParams, _NoCompute, npy

MAX_CAP = 8192                 # FP_MTCNN_MAX_CAP
LANDMARKS = ("left_eye", "right_eye", "nose", "mouth_left", "mouth_right")


class PNet(_NoCompute):
    def __init__(self):
        super().__init__()
        self.conv1, self.prelu1 = ConvParams(3, 10, 3), PReLUParams(10)
        self.conv2, self.prelu2 = ConvParams(10, 16, 3), PReLUParams(16)
        self.conv3, self.prelu3 = ConvParams(16, 32, 3), PReLUParams(32)
        self.cls = ConvParams(32, 2, 1)
        self.reg = ConvParams(32, 4, 1)


class RNet(_NoCompute):
    size = 24

    def __init__(self):
        super().__init__()
        self.conv1, self.prelu1 = ConvParams(3, 28, 3), PReLUParams(28)
        self.conv2, self.prelu2 = ConvParams(28, 48, 3), PReLUParams(48)
        self.conv3, self.prelu3 = ConvParams(48, 64, 2), PReLUParams(64)
        self.fc, self.prelu4 = LinearParams(576, 128, bias=True), PReLUParams(128)
        self.cls = LinearParams(128, 2, bias=True)
        self.reg = LinearParams(128, 4, bias=True)


class ONet(_NoCompute):
    size = 48

    def __init__(self):
        super().__init__()
        self.conv1, self.prelu1 = ConvParams(3, 32, 3), PReLUParams(32)
        self.conv2, self.prelu2 = ConvParams(32, 64, 3), PReLUParams(64)
        self.conv3, self.prelu3 = ConvParams(64, 64, 3), PReLUParams(64)
        self.conv4, self.prelu4 = ConvParams(64, 128, 2), PReLUParams(128)
        self.fc, self.prelu5 = LinearParams(1152, 256, bias=True), PReLUParams(256)
        self.cls = LinearParams(256, 2, bias=True)
        self.reg = LinearParams(256, 4, bias=True)
        self.lmk = LinearParams(256, 10, bias=True)


# the classic port's weight lists: (our layer, kind) in file order
_KERAS_ORDER = {
    "pnet": [("conv1", "conv"), ("prelu1", "prelu"), ("conv2", "conv"), ("prelu2", "prelu"), ("conv3", "conv"), ("prelu3", "prelu"),
             ("cls", "conv"), ("reg", "conv")],
    "rnet": [("conv1", "conv"), ("prelu1", "prelu"), ("conv2", "conv"), ("prelu2", "prelu"), ("conv3", "conv"), ("prelu3", "prelu"),
             ("fc", "dense"), ("prelu4", "prelu"), ("cls", "dense"), ("reg", "dense")],
    "onet": [("conv1", "conv"), ("prelu1", "prelu"), ("conv2", "conv"), ("prelu2", "prelu"), ("conv3", "conv"), ("prelu3", "prelu"),
             ("conv4", "conv"), ("prelu4", "prelu"), ("fc", "dense"), ("prelu5", "prelu"), ("cls", "dense"), ("reg", "dense"),
             ("lmk", "dense")],
}
_FC_MAP = {"rnet": (64, 3, 3), "onet": (128, 3, 3)}     # (C, rows, columns) of the map `fc` flattens


def _dense_slope(name, layer):
    """The PReLU behind `fc` holds a (C,) slope in the port's lists, those behind convs (1, 1, C)."""
    return (name, layer) in (("rnet", "prelu4"), ("onet", "prelu5"))


def pyramid(h, w, min_face_size, factor):
    """[(scale, lh, lw)] of the levels of an h x w frame: s_k = 12 / min_face_size * factor^k for every k with
    min(h, w) * s_k >= 12; level size (ceil(h s), ceil(w s))."""
    m = 12.0 / min_face_size
    out, k = [], 0
    while min(h, w) * m * factor ** k >= 12:
        s = m * factor ** k
        out.append((s, int(math.ceil(h * s)), int(math.ceil(w * s))))
        k += 1
    return out


def pnet_out(n):
    """P-Net's output size on n level pixels: conv 3, pool 2 / 2 (ceil), conv 3, conv 3."""
    return -(-(n - 2) // 2) - 4


def check_params(min_face_size, factor):
    if min_face_size < 12:
        raise ValueError(f"min_face_size = {min_face_size} < 12: the pyramid would enlarge the frame")
    if not 0.0 < factor < 1.0:
        raise ValueError(f"factor = {factor} must lie in (0, 1)")


class MTCNN(PlanCacheMixin, nn.Module):
    """The three nets and the cascade.  detect_batch runs on a HIP device only."""

    def __init__(self, min_face_size=20, factor=0.709, thresholds=(0.6, 0.7, 0.7), cap=4096, bucket=256):
        super().__init__()
        check_params(min_face_size, factor)
        if not 1 <= cap <= MAX_CAP:
            raise ValueError(f"cap = {cap}: 1 .. {MAX_CAP}")
        self.pnet, self.rnet, self.onet = PNet(), RNet(), ONet()
        self.min_face_size, self.factor = min_face_size, float(factor)
        self.thresholds = tuple(float(t) for t in thresholds)
        assert len(self.thresholds) == 3
        self.cap = int(cap)          # per-frame candidate cap of every stage; a frame beyond it raises
        self.bucket = int(bucket)    # R-Net / O-Net batch sizes are multiples of it (few distinct plans)
        self._plans = PlanCache(max_plans=8)
        self._tables = {}
        self.pnet_chunk = 256        # stage 1 runs equally sized frames in groups of at most this many (bounds the plans' arenas:
                                     # 4.1 GB for level 0 of 576 x 1024 frames at min face 20) ...
        self.pnet_small = 8          # ... and groups of at most this many on plans of that capacity
        self._pnet_plans = {}
        self.last = {}               # per-stage candidate counts of the last detect_batch (host numbers it read anyway)

    # ---- loading ----
    @classmethod
    def from_state_dict(cls, sd, **kw):
        net = cls(**kw)
        net.load_state_dict(sd)
        return net

    @classmethod
    def from_npz(cls, path, **kw):
        """An ``.npz`` whose arrays are named as the state dict's keys."""
        with np.load(path) as z:
            sd = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
        return cls.from_state_dict(sd, **kw)

    def save_npz(self, path):
        np.savez(path, **{k: npy(v) for k, v in self.state_dict().items()})

    @classmethod
    def from_keras_npy(cls, weights, **kw):
        """The classic port's weight dictionary (``np.load(path, allow_pickle=True).item()`` or the path itself):
        {pnet, rnet, onet: [kernel (kh, kw, cin, cout), bias, slope (1, 1, C) | dense kernel (in, out), bias, slope (C) ...]}
        in layer order, the two / three heads last.  A dense kernel's input is the (row, column, channel) flatten of the
        net's map.  Every shape is checked; the first mismatch raises ValueError."""
        if isinstance(weights, str):
            weights = np.load(weights, allow_pickle=True).item()
        net = cls(**kw)
        sd = {}
        for name in ("pnet", "rnet", "onet"):
            if name not in weights:
                raise ValueError(f"from_keras_npy: no '{name}' entry")
            arrs = [np.asarray(a) for a in weights[name]]
            sub = getattr(net, name)
            i = 0

            def take(shape, what):
                nonlocal i
                if i >= len(arrs):
                    raise ValueError(f"from_keras_npy: {name} ends before {what}")
                a = arrs[i]
                if tuple(a.shape) != tuple(shape):
                    raise ValueError(f"from_keras_npy: {name}[{i}] ({what}) has shape {tuple(a.shape)}, expected {tuple(shape)}")
                i += 1
                return a.astype(np.float32)

            for layer, kind in _KERAS_ORDER[name]:
                p = getattr(sub, layer)
                if kind == "prelu":
                    c = p.weight.shape[0]
                    shape = (c,) if _dense_slope(name, layer) else (1, 1, c)
                    sd[f"{name}.{layer}.weight"] = torch.from_numpy(take(shape, f"{layer} slope").reshape(c).copy())
                elif kind == "conv":
                    o, ci, kh, kw_ = p.weight.shape
                    k = take((kh, kw_, ci, o), f"{layer} kernel")
                    sd[f"{name}.{layer}.weight"] = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)))
                    sd[f"{name}.{layer}.bias"] = torch.from_numpy(take((o,), f"{layer} bias").copy())
                else:
                    o, ci = p.weight.shape
                    k = take((ci, o), f"{layer} kernel")
                    if layer == "fc":     # (row, column, channel) flatten -> our (channel, row, column)
                        c, r, q = _FC_MAP[name]
                        k = k.reshape(r, q, c, o).transpose(2, 0, 1, 3).reshape(ci, o)
                    sd[f"{name}.{layer}.weight"] = torch.from_numpy(np.ascontiguousarray(k.T))
                    sd[f"{name}.{layer}.bias"] = torch.from_numpy(take((o,), f"{layer} bias").copy())
            if i != len(arrs):
                raise ValueError(f"from_keras_npy: {name} has {len(arrs)} arrays, expected {i}")
        net.load_state_dict(sd)
        return net

    def to_keras_npy(self):
        """The inverse of from_keras_npy (a dict of lists of arrays)."""
        out = {}
        for name in ("pnet", "rnet", "onet"):
            sub, arrs = getattr(self, name), []
            for layer, kind in _KERAS_ORDER[name]:
                p = getattr(sub, layer)
                w = npy(p.weight)
                if kind == "prelu":
                    arrs.append(w.copy() if _dense_slope(name, layer) else w.reshape(1, 1, -1).copy())
                elif kind == "conv":
                    arrs += [np.ascontiguousarray(w.transpose(2, 3, 1, 0)), npy(p.bias).copy()]
                else:
                    k = w.T
                    if layer == "fc":
                        c, r, q = _FC_MAP[name]
                        k = k.reshape(c, r, q, -1).transpose(1, 2, 0, 3).reshape(c * r * q, -1)
                    arrs += [np.ascontiguousarray(k), npy(p.bias).copy()]
            out[name] = arrs
        return out

    def _invalidate(self):
        super()._invalidate()
        self._tables = {}
        self._pnet_plans = {}

    def _device(self):
        return self.pnet.conv1.weight.device

    # ---- folded weights ----
    def folded_pnet(self):
        """P-Net's layers for the un-swapped image: [(weight OIHW, bias, slope)] of the three convs, then the 1x1 head
        (weight [6, 32, 1, 1], bias [6]): class logits 0, 1, box regression 2 .. 5."""
        p = self.pnet
        convs = [(npy(c.weight).transpose(0, 1, 3, 2).copy(), npy(c.bias), npy(s.weight))
                 for c, s in ((p.conv1, p.prelu1), (p.conv2, p.prelu2), (p.conv3, p.prelu3))]
        head_w = np.concatenate([npy(p.cls.weight), npy(p.reg.weight)])        # 1x1: nothing to swap
        return convs, (head_w, np.concatenate([npy(p.cls.bias), npy(p.reg.bias)]))

    def folded(self, name):
        """The layers of rnet / onet for the un-swapped image: [(weight OIHW, bias, slope)] of the convs (fc as the conv
        over the last map), then (cls weight, bias), (reg [+ lmk] weight, bias)."""
        sub = getattr(self, name)
        convs = []
        n_conv = 3 if name == "rnet" else 4
        for i in range(1, n_conv + 1):
            c = getattr(sub, f"conv{i}")
            convs.append((npy(c.weight).transpose(0, 1, 3, 2).copy(), npy(c.bias), npy(getattr(sub, f"prelu{i}").weight)))
        c, r, q = _FC_MAP[name]
        wfc = npy(sub.fc.weight).reshape(-1, c, r, q).transpose(0, 1, 3, 2).copy()
        convs.append((wfc, npy(sub.fc.bias), npy(getattr(sub, f"prelu{n_conv + 1}").weight)))
        regw = npy(sub.reg.weight) if name == "rnet" else np.concatenate([npy(sub.reg.weight), npy(sub.lmk.weight)])
        regb = npy(sub.reg.bias) if name == "rnet" else np.concatenate([npy(sub.reg.bias), npy(sub.lmk.bias)])
        return convs, (npy(sub.cls.weight), npy(sub.cls.bias)), (regw, regb)

    # ---- R-Net / O-Net plans ----
    def _emit(self, name, N):
        """The op list of rnet / onet for batch N (host only)."""
        convs, (cw, cb), (rw, rb) = self.folded(name)
        size = getattr(self, name).size
        pb = PlanBuilder(N)
        pb.x6_all = True
        A = L.ACT_PRELU
        inp = pb.new_buf(size, size, 3)
        pools = [(3, True), (3, False)] if name == "rnet" else [(3, True), (3, False), (2, True)]
        x = inp
        for i, (w, b, s) in enumerate(convs):
            k = w.shape[2]
            y = pb.new_buf(x.H - k + 1, x.W - k + 1, w.shape[0])
            pb.conv(x.view(), w, y.view(), bias=b, slope=s, act=A)
            if x is not inp:
                pb.free(x)
            x = y
            if i < len(pools):
                pk, ceil = pools[i]
                oh = (-(-(x.H - pk) // 2) if ceil else (x.H - pk) // 2) + 1
                y = pb.new_buf(oh, oh, x.C)
                pb.maxpool(x.view(), y.view(), pk, 2, 0)      # ceil mode: the last window hangs over the end, where nothing is read
                pb.free(x)
                x = y
        assert (x.H, x.W) == (1, 1)
        prob, logit = pb.new_buf(1, 1, 2), pb.new_buf(1, 1, 2)
        pb.cls_head(x.view(0, cw.shape[1]), cw, cb, prob.view(0, 2), logit.view(0, 2))
        reg = pb.new_buf(1, 1, rw.shape[0])
        pb.conv(x.view(0, rw.shape[1]), rw[:, :, None, None], reg.view(), bias=rb)
        return pb, inp, prob, logit, reg

    def _emit_pnet(self, N, lh, lw):
        """The op list of P-Net on N level images of lh x lw (host only)."""
        convs, (hw, hb) = self.folded_pnet()
        pb = PlanBuilder(N)
        pb.x6_all = True
        A = L.ACT_PRELU
        inp = pb.new_buf(lh, lw, 3)
        c1 = pb.new_buf(lh - 2, lw - 2, 10)
        pb.conv(inp.view(), convs[0][0], c1.view(), bias=convs[0][1], slope=convs[0][2], act=A)
        p1 = pb.new_buf(-(-c1.H // 2), -(-c1.W // 2), 10)
        pb.maxpool(c1.view(), p1.view(), 2, 2, 0)                        # ceil mode, as in _emit
        pb.free(c1)
        c2 = pb.new_buf(p1.H - 2, p1.W - 2, 16)
        pb.conv(p1.view(), convs[1][0], c2.view(), bias=convs[1][1], slope=convs[1][2], act=A)
        pb.free(p1)
        c3 = pb.new_buf(c2.H - 2, c2.W - 2, 32)
        pb.conv(c2.view(), convs[2][0], c3.view(), bias=convs[2][1], slope=convs[2][2], act=A)
        pb.free(c2)
        head = pb.new_buf(c3.H, c3.W, 6)
        pb.conv(c3.view(), hw, head.view(), bias=hb)
        return pb, inp, head

    def pnet_plan(self, N, lh, lw):
        """The P-Net plan of one level size at batch capacity N (input: (N, lh, lw, 4), head: (N, oh, ow, 8))."""
        key = (N, lh, lw, switch_key(PlanBuilder))
        if key not in self._pnet_plans:
            if len(self._pnet_plans) >= 64:
                self._pnet_plans.clear()
            pb, inp, head = self._emit_pnet(N, lh, lw)
            plan = CompiledPlan(pb, self._device())
            plan.input, plan.head = plan.buf_tensor(inp, N), plan.buf_tensor(head, N)
            self._pnet_plans[key] = plan
        return self._pnet_plans[key]

    def _build(self, name, N, cache=None):
        pb, inp, prob, logit, reg = self._emit(name, N)
        plan = CompiledPlan(pb, self._device(), cache)
        plan.input = plan.buf_tensor(inp, N)
        plan.prob = plan.buf_tensor(prob, N).view(N, -1)
        plan.logit = plan.buf_tensor(logit, N).view(N, -1)
        plan.reg = plan.buf_tensor(reg, N).view(N, -1)
        return plan

    def plan_for(self, name, N):
        if self._device().type != "cuda":
            raise L.FacepathError("MTCNN runs only on a HIP device (model.to('cuda')); there is no CPU path")
        key = (name, N, switch_key(PlanBuilder))
        return self._plans.get(key, lambda cache: self._build(name, N, cache))

    def run_net(self, name, x_u8):
        """rnet / onet alone on (n, size, size, 3) u8 patches -> (prob (n, 2), logits (n, 2), reg (n, 4 | 14)) clones."""
        n = x_u8.shape[0]
        plan = self.plan_for(name, n)
        x = (x_u8.to(self._device(), torch.float32) - 127.5) * 0.0078125
        plan.input[..., :3].copy_(x)
        plan.input[..., 3:].zero_()
        plan.run()
        return plan.prob.clone(), plan.logit.clone(), plan.reg.clone()

    # ---- stage 1 tables ----
    def tables(self, sizes):
        """Device tables of a batch whose frames have `sizes` [(h, w)] under the current min_face_size / factor: the levels of
        every distinct size, frame_level0, and the host-side groups of equally sized frames (built once per size list)."""
        key = (self.min_face_size, self.factor, self.pnet_chunk, tuple(sizes))
        if key not in self._tables:
            if len(self._tables) > 16:
                self._tables.clear()
            check_params(self.min_face_size, self.factor)
            lv = np.zeros(0, dtype=LEVEL_DTYPE)
            level0, per_size, groups = [], {}, {}
            for f, (h, w) in enumerate(sizes):
                if (h, w) not in per_size:
                    pyr = pyramid(h, w, self.min_face_size, self.factor)
                    if len(pyr) > 128:
                        raise ValueError(f"{len(pyr)} pyramid levels (factor {self.factor}): at most 128")
                    rows = np.zeros(len(pyr), dtype=LEVEL_DTYPE)
                    for i, (s, lh, lw) in enumerate(pyr):
                        rows[i] = (s, lh, lw, pnet_out(lh), pnet_out(lw))
                    per_size[(h, w)] = len(lv)
                    groups[(h, w)] = (pyr, [])
                    lv = np.concatenate([lv, rows])
                level0.append(per_size[(h, w)])
                groups[(h, w)][1].append(f)
            dev = self._device()
            chunks = []          # (pyramid, device int32 frame indices) per group of at most pnet_chunk equally sized frames
            for pyr, idx in groups.values():
                for i in range(0, len(idx), self.pnet_chunk):
                    chunks.append((pyr, torch.tensor(idx[i:i + self.pnet_chunk], dtype=torch.int32, device=dev)))
            # (a placeholder row keeps the pointer non-NULL when no frame has a level)
            host = lv if len(lv) else np.zeros(1, dtype=LEVEL_DTYPE)
            self._tables[key] = dict(levels=torch.from_numpy(host.view(np.uint8).copy()).to(dev), n_levels=max(len(lv), 1),
                                     level0=torch.tensor(level0, dtype=torch.int32, device=dev), chunks=chunks,
                                     any_level=len(lv) > 0)
        return self._tables[key]

    @staticmethod
    def _as_ragged(frames, dev):
        """(data u8, descs, sizes) of a (B, H, W, 3) tensor / numpy array or a RaggedFrames."""
        frames = as_frames(frames, dev)
        return frame_bytes(frames), device_descs(frames), [(h, w) for _, h, w in frame_layout(frames)]

    # ---- the stages, one call each (tests drive them alone) ----
    def propose(self, data, descs, sizes, t1=None, cap=None):
        """Stage 1's nets: per group of equally sized frames and per level, the level images (fp_pnet_level_images), the P-Net
        plan and the threshold (fp_pnet_threshold) -> (cand (B, cap, 6) float32 view of the records [reg x 4, score, key
        bits], counts, overflow)."""
        lib, dev = L.load(), self._device()
        cap = self.cap if cap is None else cap
        tb = self.tables(sizes)
        B = len(sizes)
        cand = torch.empty((B, cap, 6), dtype=torch.float32, device=dev)
        counts = torch.zeros((B,), dtype=torch.int32, device=dev)
        over = torch.zeros((B,), dtype=torch.int32, device=dev)
        t1 = self.thresholds[0] if t1 is None else t1
        st = L.current_stream(dev)
        for pyr, idx in tb["chunks"]:
            n = idx.numel()
            for li, (_, lh, lw) in enumerate(pyr):
                plan = self.pnet_plan(self.pnet_chunk if n > self.pnet_small else self.pnet_small, lh, lw)
                L.check(lib.fp_pnet_level_images(L.ptr(data), data.numel(), L.ptr(descs), B, L.ptr(idx), n, lh, lw, L.ptr(plan.input),
                                                 st), "fp_pnet_level_images")
                plan.run(n=n)
                L.check(lib.fp_pnet_threshold(L.ptr(plan.head), plan.head.shape[3], L.ptr(idx), n, B, plan.head.shape[1],
                                              plan.head.shape[2], li, float(t1), cap, L.ptr(cand), L.ptr(counts), L.ptr(over), st),
                        "fp_pnet_threshold")
        return cand, counts, over

    def _scratch(self, B, cap):
        n = L.load().fp_mtcnn_scratch_bytes(B, cap)
        return torch.empty((max(n, 8),), dtype=torch.uint8, device=self._device()), n

    def stage1(self, cand, counts, sizes):
        lib, dev = L.load(), self._device()
        B, cap = cand.shape[0], cand.shape[1]
        tb = self.tables(sizes)
        boxes = torch.empty((B, cap, 4), dtype=torch.int32, device=dev)
        scores = torch.empty((B, cap), dtype=torch.float32, device=dev)
        out_counts = torch.empty((B,), dtype=torch.int32, device=dev)
        scratch, nb = self._scratch(B, cap)
        L.check(lib.fp_mtcnn_stage1(L.ptr(cand), L.ptr(counts), B, cap, L.ptr(tb["levels"]), tb["n_levels"], L.ptr(tb["level0"]),
                                    L.ptr(boxes), L.ptr(scores), L.ptr(out_counts), L.ptr(scratch), nb, L.current_stream(dev)),
                "fp_mtcnn_stage1")
        return boxes, scores, out_counts

    def cut(self, data, descs, B, boxes, offs, n, size, out, out_u8=None):
        lib, dev = L.load(), self._device()
        L.check(lib.fp_mtcnn_cut(L.ptr(data), data.numel(), L.ptr(descs), B, L.ptr(boxes), boxes.shape[1], L.ptr(offs), int(n), size,
                                 L.ptr(out), L.ptr(out_u8) if out_u8 is not None else None, L.current_stream(dev)), "fp_mtcnn_cut")
        return out

    def stage2(self, boxes, offs, prob, reg, t2=None):
        lib, dev = L.load(), self._device()
        B, cap = boxes.shape[0], boxes.shape[1]
        ob = torch.empty((B, cap, 4), dtype=torch.int32, device=dev)
        os_ = torch.empty((B, cap), dtype=torch.float32, device=dev)
        oc = torch.empty((B,), dtype=torch.int32, device=dev)
        scratch, nb = self._scratch(B, cap)
        t2 = self.thresholds[1] if t2 is None else t2
        L.check(lib.fp_mtcnn_stage2(L.ptr(boxes), B, cap, L.ptr(offs), L.ptr(prob), prob.stride(0), L.ptr(reg), reg.stride(0),
                                    float(t2), L.ptr(ob), L.ptr(os_), L.ptr(oc), L.ptr(scratch), nb, L.current_stream(dev)),
                "fp_mtcnn_stage2")
        return ob, os_, oc

    def stage3(self, boxes, offs, prob, reg, max_det, t3=None):
        lib, dev = L.load(), self._device()
        B, cap = boxes.shape[0], boxes.shape[1]
        dets = torch.zeros((B, max_det, 15), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        over = torch.empty((B,), dtype=torch.int32, device=dev)
        scratch, nb = self._scratch(B, cap)
        t3 = self.thresholds[2] if t3 is None else t3
        L.check(lib.fp_mtcnn_stage3(L.ptr(boxes), B, cap, L.ptr(offs), L.ptr(prob), prob.stride(0), L.ptr(reg), reg.stride(0),
                                    float(t3), int(max_det), L.ptr(dets), L.ptr(counts), L.ptr(over), L.ptr(scratch), nb,
                                    L.current_stream(dev)), "fp_mtcnn_stage3")
        return dets, counts, over

    def box_arithmetic(self, boxes, reg, mode):
        """fp_mtcnn_boxes: boxes (n, 4) float32, reg (n, >= 4 | 14) float32 on the device; mode 1 / 2 -> (n, 4) int32 squares,
        mode 3 -> (n, 14) float32 rows (regressed box, five landmarks)."""
        lib, dev = L.load(), self._device()
        n = boxes.shape[0]
        ob = torch.empty((n, 4), dtype=torch.int32, device=dev) if mode != 3 else None
        rows = torch.empty((n, 14), dtype=torch.float32, device=dev) if mode == 3 else None
        L.check(lib.fp_mtcnn_boxes(L.ptr(boxes), L.ptr(reg), reg.stride(0), n, int(mode), L.ptr(ob), L.ptr(rows),
                                   L.current_stream(dev)), "fp_mtcnn_boxes")
        return rows if mode == 3 else ob

    def nms(self, boxes, scores, seg, thr, mode):
        """fp_mtcnn_nms: boxes (n, 4) float32, scores (n,), seg (n_seg + 1,) int32 on the device; mode "union" | "min"
        -> (keep_idx (n,), keep_count (n_seg,))."""
        lib, dev = L.load(), self._device()
        n, n_seg = boxes.shape[0], seg.shape[0] - 1
        keep = torch.full((n,), -1, dtype=torch.int32, device=dev)
        cnt = torch.zeros((n_seg,), dtype=torch.int32, device=dev)
        scratch, nb = self._scratch(1, n)
        L.check(lib.fp_mtcnn_nms(L.ptr(boxes), L.ptr(scores), L.ptr(seg), n_seg, n, float(thr), {"union": 0, "min": 1}[mode],
                                 L.ptr(keep), L.ptr(cnt), L.ptr(scratch), nb, L.current_stream(dev)), "fp_mtcnn_nms")
        return keep, cnt

    def _refine(self, name, data, descs, B, boxes, counts_host, counts_dev):
        """Cut the boxes, run rnet / onet on them -> (offs, plan) with the plan's prob / reg rows in candidate order."""
        dev = self._device()
        total = int(counts_host.sum())
        offs = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        offs[1:] = torch.cumsum(counts_dev, 0)
        N = max(-(-total // self.bucket) * self.bucket, self.bucket)
        plan = self.plan_for(name, N)
        self.cut(data, descs, B, boxes, offs, total, getattr(self, name).size, plan.input)
        if total < N:
            plan.input[total:].zero_()
        plan.run()
        return offs, plan

    def detect_batch(self, frames, max_det=64):
        """frames: (B, H, W, 3) u8 (numpy / tensor) or a RaggedFrames -> (dets (B, max_det, 15), counts (B,), overflow (B,))
        on the device.  A row is [x1, y1, x2, y2, (x, y) of left_eye, right_eye, nose, mouth_left, mouth_right, score] in the
        frame's own pixels, rows by descending score; overflow[b] = 1 if frame b had more than max_det faces.
        Equal scores in an NMS: the lower candidate index (level, y, x; then the previous stage's order) wins.
        Raises FacepathError if a frame has more than `cap` stage-1 candidates (never truncated silently)."""
        dev = self._device()
        if dev.type != "cuda":
            raise L.FacepathError("MTCNN runs only on a HIP device (model.to('cuda')); there is no CPU path")
        data, descs, sizes = self._as_ragged(frames, dev)
        B = len(sizes)
        if not self.tables(sizes)["any_level"]:        # every frame is smaller than the smallest face: no pyramid level
            zero = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.last = dict(pnet=np.zeros(B, np.int32), rnet_in=np.zeros(B, np.int32), onet_in=np.zeros(B, np.int32))
            return torch.zeros((B, max_det, 15), dtype=torch.float32, device=dev), zero, zero.clone()
        cand, counts0, over0 = self.propose(data, descs, sizes)
        boxes1, _, counts1 = self.stage1(cand, counts0, sizes)
        host = torch.stack([counts0, over0, counts1]).cpu().numpy()          # the one read of stage 1
        if host[1].any():
            bad = int(np.nonzero(host[1])[0][0])
            raise L.FacepathError(f"MTCNN: frame {bad} has {int(host[0][bad])} P-Net candidates, cap = {self.cap}; raise cap or "
                                  "the first threshold")
        offs2, plan2 = self._refine("rnet", data, descs, B, boxes1, host[2], counts1)
        boxes2, _, counts2 = self.stage2(boxes1, offs2, plan2.prob, plan2.reg)
        host2 = counts2.cpu().numpy()                                        # ... of stage 2
        offs3, plan3 = self._refine("onet", data, descs, B, boxes2, host2, counts2)
        dets, counts, over = self.stage3(boxes2, offs3, plan3.prob, plan3.reg, max_det)
        self.last = dict(pnet=host[0].copy(), rnet_in=host[2].copy(), onet_in=host2.copy())
        return dets, counts, over


LEVEL_DTYPE = np.dtype([("scale", "<f8"), ("lh", "<i4"), ("lw", "<i4"), ("oh", "<i4"), ("ow", "<i4")])
assert LEVEL_DTYPE.itemsize == 24
