"""Age and gender classification of face crops (Levi & Hassner 2015) on MI355X: the reference's ``age_net`` / ``gender_net``
Caffe models (modules/opencv2_dnn/model.py, OpenCVFaceAgeModel / OpenCVFaceGenderModel), both nets in ONE HIP plan.

Architecture (shared by the two nets; only the weights and fc8's width differ, 8 age or 2 gender classes):
227 x 227 BGR minus the per-channel mean -> conv1 96 7x7 /4 + ReLU -> max pool 3x3 /2 (Caffe ceil mode) -> LRN(5, 1e-4,
0.75, 1) -> conv2 256 5x5 pad 2 + ReLU -> pool -> LRN -> conv3 384 3x3 pad 1 + ReLU -> pool -> fc6 512 + ReLU -> fc7 512 +
ReLU -> fc8 -> softmax (the dropouts are the identity at inference).

The plan:
* conv1 of both nets reads the same image: ONE op with 192 output channels (age 0 .. 95, gender 96 .. 191).  The mean
  subtraction is folded into its bias (conv1 has no padding, so conv1(x - mean) = conv1(x) - sum w * mean exactly in
  real arithmetic): the plan's input is the crop's pixel values as floats, the pipeline's resize writes them directly.
* pool + LRN are one FP_OP_POOL_LRN per stage over both nets' channels, with the LRN group = one net's channels.
* conv2 / conv3 / fc6 / fc7 are split-MFMA convs (FP_OPF_SPLIT3, csrc/pwx6.hip) in the x6 plan, each net writing its half
  of a shared buffer; fc6 is a 7x7 valid conv on the 7x7 map (Caffe's (c, y, x) flatten is the OIHW weight), fc7 a 1x1.
* fc8 + softmax is one FP_OP_CLS_HEAD per net (csrc/clshead.hip), which also writes the logits.
With PlanBuilder.X6 = False every conv runs on the fp32-MFMA kernels instead (the comparison build).
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib as L
from ...plan import CompiledPlan, PlanBuilder, PlanCache, switch_key
from ..params import ConvParams, LinearParams, PlanCacheMixin, _NoCompute, npy

MEAN_BGR = (78.4263377603, 87.7689143744, 114.895847746)   # the reference's AGE_MEAN_VALUES = GENDER_MEAN_VALUES
AGE_LIST = ['(0-2)', '(4-6)', '(8-12)', '(15-20)', '(25-32)', '(38-43)', '(48-53)', '(60-100)']
GENDER_LIST = ['Male', 'Female']
LRN_SIZE, LRN_ALPHA, LRN_BETA, LRN_K = 5, 1e-4, 0.75, 1.0
LAYERS = ("conv1", "conv2", "conv3", "fc6", "fc7", "fc8")


def pool_out(n, k=3, s=2):
    """Caffe's pooled size (ceil mode, no padding)."""
    return -(-(n - k) // s) + 1


class LeviHassnerNet(_NoCompute):
    """The parameters of one net, Caffe layer names as attributes: conv1 .. conv3 (OIHW + bias), fc6 .. fc8 ([out, in] + bias)."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = int(n_classes)
        self.conv1 = ConvParams(3, 96, 7, stride=4)
        self.conv2 = ConvParams(96, 256, 5, padding=2)
        self.conv3 = ConvParams(256, 384, 3, padding=1)
        self.fc6 = LinearParams(384 * 7 * 7, 512, bias=True)
        self.fc7 = LinearParams(512, 512, bias=True)
        self.fc8 = LinearParams(512, self.n_classes, bias=True)

    def blob_shapes(self):
        """Caffe layer name -> (weight shape, bias shape) this net expects."""
        return {name: (tuple(getattr(self, name).weight.shape), tuple(getattr(self, name).bias.shape)) for name in LAYERS}


class AgeGenderNet(PlanCacheMixin, nn.Module):
    """Both nets.  ``forward(x)``: (N, 3, 227, 227) float BGR pixel values (0 .. 255, the resized crop, mean NOT subtracted:
    the plan subtracts it) -> (age_probs (N, 8), gender_probs (N, 2)); with ``return_logits`` also the two logit tensors.
    HIP only: on a CPU device plan_for / forward raise."""

    input_size = (227, 227)
    swap_rb = False      # crops in BGR, as cv2.dnn.blobFromImage(swapRB=False) feeds them
    n_age, n_gender = len(AGE_LIST), len(GENDER_LIST)

    def __init__(self):
        super().__init__()
        self.age = LeviHassnerNet(self.n_age)
        self.gender = LeviHassnerNet(self.n_gender)
        self._plans = PlanCache()

    @classmethod
    def from_caffemodels(cls, age_path, gender_path):
        """The reference's two ``.caffemodel`` files (age_net / gender_net); layers conv1 .. fc8 are read, shapes checked."""
        from ..utils.caffemodel import read_caffemodel_blobs
        net = cls()
        for sub, path in ((net.age, age_path), (net.gender, gender_path)):
            blobs = read_caffemodel_blobs(path, sub.blob_shapes())
            with torch.no_grad():
                for name, (w, b) in blobs.items():
                    getattr(sub, name).weight.copy_(torch.from_numpy(w))
                    getattr(sub, name).bias.copy_(torch.from_numpy(b))
        net._invalidate()
        return net

    def _device(self):
        return self.age.conv1.weight.device

    # ---- plan ----
    def _conv1(self):
        """conv1 of both nets as one [192, 3, 7, 7] weight, the mean folded into the bias (float64, then fp32)."""
        w = np.concatenate([npy(self.age.conv1.weight), npy(self.gender.conv1.weight)])
        b = np.concatenate([npy(self.age.conv1.bias), npy(self.gender.conv1.bias)]).astype(np.float64)
        b -= np.einsum("ochw,c->o", w.astype(np.float64), np.asarray(MEAN_BGR, np.float64))
        return w, b.astype(np.float32)

    def _emit(self, N):
        """Emit the op list for batch N (host only, no GPU needed)."""
        pb = PlanBuilder(N)
        pb.x6_all = True
        H, W = self.input_size
        nets = (self.age, self.gender)
        R = L.ACT_RELU
        inp = pb.new_buf(H, W, 3)                                          # 4-float pixels, the fourth channel zero
        h1 = (H - 7) // 4 + 1
        c1 = pb.new_buf(h1, h1, 192)
        w1, b1 = self._conv1()
        pb.conv(inp.view(), w1, c1.view(), stride=4, bias=b1, act=R)
        lrn = dict(size=LRN_SIZE, alpha=LRN_ALPHA, beta=LRN_BETA, lrn_k=LRN_K)
        p1 = pb.new_buf(pool_out(h1), pool_out(h1), 192)
        pb.pool_lrn(c1.view(), p1.view(), 3, 2, group=96, **lrn)
        pb.free(c1)
        c2 = pb.new_buf(p1.H, p1.W, 512)
        for i, net in enumerate(nets):
            pb.conv(p1.view(96 * i, 96), npy(net.conv2.weight), c2.view(256 * i, 256), pad=(2, 2), bias=npy(net.conv2.bias), act=R)
        pb.free(p1)
        p2 = pb.new_buf(pool_out(c2.H), pool_out(c2.W), 512)
        pb.pool_lrn(c2.view(), p2.view(), 3, 2, group=256, **lrn)
        pb.free(c2)
        c3 = pb.new_buf(p2.H, p2.W, 768)
        for i, net in enumerate(nets):
            pb.conv(p2.view(256 * i, 256), npy(net.conv3.weight), c3.view(384 * i, 384), pad=(1, 1), bias=npy(net.conv3.bias), act=R)
        pb.free(p2)
        p5 = pb.new_buf(pool_out(c3.H), pool_out(c3.W), 768)
        pb.maxpool(c3.view(), p5.view(), 3, 2, 0)                        # pool5: OH / OW in ceil mode
        pb.free(c3)
        f6 = pb.new_buf(1, 1, 1024)
        for i, net in enumerate(nets):
            w6 = npy(net.fc6.weight).reshape(512, 384, p5.H, p5.W)        # Caffe's (c, y, x) flatten order
            pb.conv(p5.view(384 * i, 384), w6, f6.view(512 * i, 512), bias=npy(net.fc6.bias), act=R)
        pb.free(p5)
        f7 = pb.new_buf(1, 1, 1024)
        for i, net in enumerate(nets):
            pb.conv(f6.view(512 * i, 512), npy(net.fc7.weight)[:, :, None, None], f7.view(512 * i, 512), bias=npy(net.fc7.bias),
                    act=R)
        pb.free(f6)
        na, ng = self.n_age, self.n_gender
        prob = pb.new_buf(1, 1, na + ng)
        logit = pb.new_buf(1, 1, na + ng)
        for i, (net, c0, d) in enumerate(((self.age, 0, na), (self.gender, na, ng))):
            pb.cls_head(f7.view(512 * i, 512), npy(net.fc8.weight), npy(net.fc8.bias), prob.view(c0, d), logit.view(c0, d))
        pb.free(f7)
        return pb, inp, prob, logit

    def _build(self, N, cache=None):
        pb, inp, prob, logit = self._emit(N)
        plan = CompiledPlan(pb, self._device(), cache)
        plan.input = plan.buf_tensor(inp, N)
        na, ng = self.n_age, self.n_gender
        p = plan.buf_tensor(prob, N).view(N, -1)
        z = plan.buf_tensor(logit, N).view(N, -1)
        plan.out = p[:, :na + ng]
        plan.age, plan.gender = p[:, :na], p[:, na:na + ng]
        plan.age_logits, plan.gender_logits = z[:, :na], z[:, na:na + ng]
        return plan

    def plan_for(self, N, n_run=None):
        """The plan with batch capacity N (n_run: accepted for the embedder-style interface; the op list does not depend on it)."""
        if self._device().type != "cuda":
            raise L.FacepathError("AgeGenderNet runs only on a HIP device (model.to('cuda')); there is no CPU path")
        key = (N, switch_key(PlanBuilder))
        return self._plans.get(key, lambda cache: self._build(N, cache))

    def forward(self, x, return_logits=False):
        b = x.shape[0]
        plan = self.plan_for(b)
        plan.input[..., :3].copy_(x.to(self._device(), torch.float32).permute(0, 2, 3, 1))
        plan.input[..., 3:].zero_()
        plan.run()
        out = (plan.age.clone(), plan.gender.clone())        # arena views the next call overwrites
        if return_logits:
            out += (plan.age_logits.clone(), plan.gender_logits.clone())
        return out

    def input_lut(self, device):
        """Per-value input LUT of the pipeline's crops: the u8 value itself (the mean lives in conv1's bias)."""
        return torch.arange(256, dtype=torch.float32).to(device)


def labels(age_probs, gender_probs):
    """The reference's label strings (OpenCVFaceDetAgeGenderModel): f"{gender}:{p:.2f},{age}:{p:.2f}" per row, from host
    arrays (N, 8) / (N, 2).  A row with NaN probabilities (an empty crop) gives "?:nan,?:nan"."""
    out = []
    for a, g in zip(np.asarray(age_probs), np.asarray(gender_probs)):
        if np.isnan(a).any() or np.isnan(g).any():
            out.append("?:nan,?:nan")
            continue
        out.append(f"{GENDER_LIST[int(g.argmax())]}:{g.max():.2f}," + f"{AGE_LIST[int(a.argmax())]}:{a.max():.2f}")
    return out


# ---- crop rectangles of the reference's age / gender path (fp_attr_crop_items) ----
ATTR_PAD = 5    # OpenCVFaceDetAgeGenderModel's padding around the rounded box


def attr_crop_items(info, n, frames, dst=(227, 227), pad=ATTR_PAD, out=None):
    """Device: fp_resize_item rows (n, 9) int32 of the age / gender crops of face rows info (n, >= 5: frame, x1, y1, x2, y2)
    of `frames` ((B, H, W, 3) or a RaggedFrames).  An empty crop has dw = dh = 0."""
    import torch
    from ...frames import frame_call_args
    lib = L.load()
    dev = info.device
    items = out if out is not None else torch.empty((max(n, 1), 9), dtype=torch.int32, device=dev)
    if n == 0:
        return items[:0]
    ragged, fa = frame_call_args(frames)     # ragged: (data, bytes, descs, B); dense: (frames, B, H, W)
    descs, nf, fh, fw = (fa[2], fa[3], 0, 0) if ragged else (None,) + fa[1:]
    L.check(lib.fp_attr_crop_items(L.ptr(info), int(n), info.shape[1], descs, nf, fw, fh, int(pad), dst[0], dst[1], L.ptr(items),
                                   L.current_stream(dev)), "fp_attr_crop_items")
    return items[:n]


def attr_crop_items_host(info, frame_sizes, dst=(227, 227), pad=ATTR_PAD):
    """Host emulation (the same C function): info (n, >= 5) float32, frame_sizes [(h, w)] per frame -> (n, 9) int32."""
    info = np.ascontiguousarray(info, np.float32)
    n = info.shape[0]
    descs = (L.FpFrameDesc * max(len(frame_sizes), 1))(*[L.FpFrameDesc(0, int(h), int(w)) for h, w in frame_sizes])
    items = np.zeros((max(n, 1), 9), np.int32)
    L.check(L.load().fp_attr_crop_items_emulate(info.ctypes.data if n else None, n, info.shape[1] if info.ndim == 2 else 5,
                                                descs, len(frame_sizes), 0, 0, int(pad), dst[0], dst[1], items.ctypes.data),
            "fp_attr_crop_items_emulate")
    return items[:n]


def run_on_items(net, frames, items, n, n_pad=None, plan=None):
    """Resize the n crops of `items` into the plan's input (cv2 INTER_LINEAR u8 arithmetic, BGR) and run both nets on it.
    -> (age (n, 8), gender (n, 2)) arena views of the plan (valid until its next run), rows of empty crops NaN-free:
    the caller masks them (nan_empty)."""
    from ..mobile_facenet.utils import crops_to_input
    n_pad = n if n_pad is None else n_pad
    plan = plan if plan is not None else net.plan_for(n_pad)
    crops_to_input(frames, items, n, plan.input, net.input_lut(plan.input.device), swap_rb=False)
    if n_pad > n:
        plan.input[n:n_pad].zero_()
    plan.run(n=n_pad)
    return plan.age[:n], plan.gender[:n]


def nan_empty(probs, items):
    """probs with the rows of empty crops (items' dw == 0) set to NaN (a new tensor; no host sync)."""
    import torch
    empty = (items[:, 7] == 0).unsqueeze(1)
    return torch.where(empty, torch.full_like(probs, float("nan")), probs)
