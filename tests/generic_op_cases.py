"""Case table, float64 references, write footprints and the product census for the generic fp32 plan ops of csrc/conv.hip
(conv_igemm_kernel, dwconv_kernel, dwconv3_row_kernel, maxpool_kernel, maxpool_generic_kernel, upsample2x_kernel, copy_kernel,
copy4_kernel, l2norm_kernel).  tests/test_generic_ops.py runs every case as a one-op plan.  The kernels that take an FP_OP_CONV
away from conv_igemm_kernel have tables of their own: the split-bf16 convs tests/split_conv_cases.py, the stems (stem_conv_kernel,
stemdw_kernel) and pws_kernel tests/stem_mfn_op_cases.py, which also holds the Mobile-FaceNet DWPW forms and the fp32 dwblock_kernel.

* A Case says how to build the op with PlanBuilder (shapes, channel slices, image strides, flags), the kernel instance the
  launcher must pick for it and what the data look like.  build() emits the plan, inputs() draws the seeded data, reference()
  computes the op in torch on the CPU in the requested dtype (float64 for the truth, float32 for the yardstick) from the op
  semantics of include/facepath.h -- never from the kernels.
* footprint() is the exact set of arena floats an op may write, from its output view.
* census() emits the plans of the shipped networks on the host and returns the feature keys with which they reach the
  generic kernels; CENSUS_KEYS is the copy of that set every key of which has a case (case_from_key).  A network that sends a
  new combination to a generic kernel makes census() grow past CENSUS_KEYS: add the key (and, where the combination has an
  edge of its own, a hand-written case) here.
"""
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import Buf, PlanBuilder

ACTS = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "prelu": L.ACT_PRELU, "silu": L.ACT_SILU}
RES = {"": L.RES_NONE, "before": L.RES_ADD_BEFORE_ACT, "after": L.RES_ADD_AFTER_ACT, "pool2": L.RES_POOL2_BEFORE_ACT,
       "shuffle": L.RES_SHUFFLE2}
KINDS = ("conv", "dwconv", "maxpool", "upsample", "copy", "l2norm")
GENERIC = ("conv_igemm_kernel", "dwconv_kernel", "dwconv3_row_kernel", "maxpool_kernel", "maxpool_generic_kernel",
           "upsample2x_kernel", "copy_kernel", "copy4_kernel", "l2norm_kernel")
EXACT_KINDS = ("maxpool", "upsample", "copy")      # compared bit for bit


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    kernel: str              # the instance fp_op_kernel_name must report
    N: int
    H: int
    W: int
    C: int                   # channels of the input view (conv: the physical Cin the op sees)
    cin: int = 0             # conv: logical input channels of the weight (<= C; 0: C); channels cin .. C-1 meet zero weights
    cout: int = 0            # conv: logical output channels of the weight (<= out_C)
    out_C: int = 0           # conv: channels of the output view = fp_op.Cout (0: cout rounded up to 4)
    k: tuple = (1, 1)        # window (KH, KW); dwconv / maxpool: square
    stride: int = 1
    pad: tuple = (0, 0)      # (pad_t, pad_l)
    OH: int = 0              # output map; 0: floor((H + 2 pad_t - KH) / stride) + 1 (symmetric padding)
    OW: int = 0
    act: str = "none"
    scale: bool = True
    bias: bool = True
    res: str = ""            # "", "before", "after", "pool2", "shuffle"
    res_C: int = 0           # channels of the residual view (0: out_C)
    res_buf_C: int = 0       # width of the residual buffer (0: res_C)
    res_coff: int = 0
    in_buf_C: int = 0        # width of the input buffer (0: C): the view is channels [in_coff, in_coff + C)
    in_coff: int = 0
    in_ns_extra: int = 0     # floats between the images of the input buffer beyond H * W * in_buf_C
    out_buf_C: int = 0       # width of the output buffer (0: what the op writes)
    out_coff: int = 0
    out_cmul: int = 1
    out_ns_extra: int = 0
    out_rowpad: bool = False
    partial: int = 0         # > 0: also run(partial) on the plan of capacity N
    special: str = ""        # "inf": +-inf among the inputs; "zero_row": one all-zero input row; "neg": bias pushes every channel negative
                             # "inf_pair": one +inf and one -inf among the inputs
    up_C: int = 0            # conv, FP_OPF_IN_UP2 (tests/split_conv_cases.py): channels [0, up_C) of the input view are the
    up_buf_C: int = 0        # nearest-neighbour 2x of an (H/2, W/2, up_C) view at up_coff of a buffer up_buf_C wide (0: up_C)
    up_coff: int = 0


def _out_hw(c):
    if c.kind in ("copy", "l2norm"):
        return c.H, c.W
    if c.kind == "upsample":
        return 2 * c.H, 2 * c.W
    oh = c.OH or (c.H + 2 * c.pad[0] - c.k[0]) // c.stride + 1
    ow = c.OW or (c.W + 2 * c.pad[1] - c.k[1]) // c.stride + 1
    return oh, ow


def _out_view_C(c):
    if c.kind == "conv":
        return c.out_C or (c.cout + 3) // 4 * 4
    return c.C


def _written_C(c):
    return 2 * _out_view_C(c) if c.res == "shuffle" else _out_view_C(c)


def _raw_buf(pb, H, W, C, ns_extra=0):
    """A hand-made Buf of exactly C channels per pixel (no rounding to 4) and, with ns_extra, a foreign image stride."""
    ns = H * W * C + ns_extra
    off, size = pb.new_raw(ns)
    return Buf(H, W, C, off, size, ns_=ns if ns_extra else -1)


def weights(c):
    """Seeded parameters of a case (float32 numpy), logical shapes."""
    rng = np.random.default_rng(abs(hash_name(c.name)) % (2 ** 31))
    p = {}
    if c.kind == "conv":
        cin = c.cin or c.C
        kdim = cin * c.k[0] * c.k[1]
        p["w"] = rng.normal(0, (2.0 / kdim) ** 0.5, (c.cout, cin, *c.k)).astype(np.float32)
        n = c.cout
    elif c.kind == "dwconv":
        p["w"] = rng.normal(0, (2.0 / (c.k[0] * c.k[1])) ** 0.5, (c.C, 1, *c.k)).astype(np.float32)
        n = c.C
    else:
        return p
    if c.scale:
        p["scale"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    if c.bias:
        p["bias"] = (rng.normal(0, 0.2, n) - (4.0 if c.special == "neg" else 0.0)).astype(np.float32)
    if c.act == "prelu":
        p["slope"] = rng.uniform(0.1, 0.3, n).astype(np.float32)
    return p


def hash_name(s):
    h = 0
    for ch in s.encode():
        h = (h * 131 + ch) % (2 ** 61 - 1)
    return h


def inputs(c):
    """Seeded inputs of a case: {"x": (N, H, W, C) float32, "res": (N, rH, rW, res_C)}; every value finite unless `special`."""
    rng = np.random.default_rng((hash_name(c.name) + 1) % (2 ** 31))
    x = rng.normal(0, 1, (c.N, c.H, c.W, c.C)).astype(np.float32)
    if c.special == "inf":
        flat = x.reshape(-1)
        pos = rng.choice(flat.size, size=max(2, flat.size // 9), replace=False)
        flat[pos[::2]] = -np.inf
        flat[pos[1::2]] = np.inf
    if c.special == "inf_pair":        # one +inf and one -inf: the outputs whose windows miss both stay finite
        x[0, 0, 0, 0], x[-1, -1, -1, -1] = np.inf, -np.inf
    if c.special == "zero_row":
        x[c.N // 2, c.H // 2, c.W // 2, :] = 0.0
    d = {"x": x}
    if c.res:
        oh, ow = _out_hw(c)
        rh, rw = (2 * oh, 2 * ow) if c.res == "pool2" else (oh, ow)
        d["res"] = rng.normal(0, 1, (c.N, rh, rw, c.res_C or _out_view_C(c))).astype(np.float32)
    if c.up_C:
        d["up"] = rng.normal(0, 1, (c.N, c.H // 2, c.W // 2, c.up_C)).astype(np.float32)
    return d


def build(c, N=None):
    """Emit the one-op plan of a case -> (builder, {"x": Buf, "out": Buf, "res": Buf or None}).  The fp32 kernels only
    (PlanBuilder.X6 off on this builder: the split-MFMA conv kernels have a table of their own, tests/split_conv_cases.py)."""
    pb = PlanBuilder(N or c.N)
    pb.X6 = False
    oh, ow = _out_hw(c)
    xb = _raw_buf(pb, c.H, c.W, c.in_buf_C or c.C, c.in_ns_extra)
    rb = None
    if c.res:
        rh, rw = (2 * oh, 2 * ow) if c.res == "pool2" else (oh, ow)
        rb = _raw_buf(pb, rh, rw, c.res_buf_C or c.res_C or _out_view_C(c))
    wc = _written_C(c)
    if c.out_rowpad:
        ob = pb.new_buf_rowpad(oh, ow, wc)
    else:
        ob = _raw_buf(pb, oh, ow, c.out_buf_C or wc * c.out_cmul, c.out_ns_extra)
    xv = xb.view(c.in_coff, c.C)
    ov = ob.view(c.out_coff, _out_view_C(c), c.out_cmul)
    p = weights(c)
    if c.kind == "conv":
        rv = rb.view(c.res_coff, c.res_C or _out_view_C(c)) if rb is not None else None
        pb.conv(xv, p["w"], ov, stride=c.stride, pad=c.pad, scale=p.get("scale"), bias=p.get("bias"), slope=p.get("slope"),
                act=ACTS[c.act], res=rv, res_mode=RES[c.res])
    elif c.kind == "dwconv":
        pb.dwconv(xv, p["w"], ov, stride=c.stride, pad=c.pad, scale=p.get("scale"), bias=p.get("bias"), slope=p.get("slope"),
                  act=ACTS[c.act])
    elif c.kind == "maxpool":
        assert c.pad[0] == c.pad[1]
        pb.maxpool(xv, ov, c.k[0], c.stride, c.pad[0])
    elif c.kind == "upsample":
        pb.upsample2x(xv, ov)
    elif c.kind == "copy":
        pb.copy(xv, ov)
    elif c.kind == "l2norm":
        pb.l2norm(xv, ov)
    else:
        raise ValueError(c.kind)
    assert len(pb.ops) == 1
    return pb, {"x": xb, "out": ob, "res": rb}


def kernel_name(op):
    return L.load().fp_op_kernel_name(ctypes.byref(op)).decode()


# ---------------------------------------------------------------------------------------------------------------------------
# references (torch on the CPU, dtype dt)
# ---------------------------------------------------------------------------------------------------------------------------
def _pad_window(x, fill, k, stride, pad, oh, ow):
    """NCHW x padded explicitly so that an unpadded window op yields at least oh x ow outputs: pad_t / pad_l in front, whatever
    the last window needs behind (a window that hangs over the bottom / right edge reads `fill` there)."""
    H, W = x.shape[2:]
    pb = max(0, (oh - 1) * stride + k[0] - pad[0] - H)
    pr = max(0, (ow - 1) * stride + k[1] - pad[1] - W)
    return F.pad(x, (pad[1], pr, pad[0], pb), value=fill)


def _act(v, act, slope):
    if act == "relu":
        return torch.relu(v)
    if act == "prelu":
        return torch.where(v > 0, v, v * slope.view(1, -1, 1, 1))
    if act == "silu":
        return v * torch.sigmoid(v)
    return v


def _vec(p, key, n, dt, fill):
    """A per-channel parameter padded to the n physical channels with what PlanBuilder packs there (zeros)."""
    out = torch.full((n,), fill, dtype=dt)
    if key in p:
        out[:p[key].shape[0]] = torch.from_numpy(p[key]).to(dt)
    return out


def reference(c, data, dt, pre=False, p=None, conv=None):
    """The op of case c on data (inputs()) -> (N, OH, OW, written channels) numpy array of dtype dt.  pre: the conv / dwconv
    value in front of the activation instead.  p: parameters other than weights(c) (a mutant); conv: what computes the dense
    conv of the padded NCHW input in place of F.conv2d(xp, w, stride=...) (another summation order)."""
    x = torch.from_numpy(data["x"]).to(dt).permute(0, 3, 1, 2)
    oh, ow = _out_hw(c)
    p = weights(c) if p is None else p
    if c.up_C:      # the folded nn.Upsample(2, "nearest") + Concat: the small map's 2x in front of the direct channels
        u = torch.from_numpy(data["up"]).to(dt).permute(0, 3, 1, 2)
        iy, ix = torch.arange(c.H) // 2, torch.arange(c.W) // 2
        x = torch.cat([u[:, :, iy][:, :, :, ix], x[:, c.up_C:]], dim=1)
    if c.kind in ("conv", "dwconv"):
        oc = _out_view_C(c)
        xp = _pad_window(x, 0.0, c.k, c.stride, c.pad, oh, ow)
        if c.kind == "conv":
            w = torch.zeros((oc, c.C, *c.k), dtype=dt)
            w[:c.cout, :c.cin or c.C] = torch.from_numpy(p["w"]).to(dt)
            v = F.conv2d(xp, w, stride=c.stride) if conv is None else conv(xp, w, c.stride)
        else:
            v = F.conv2d(xp, torch.from_numpy(p["w"]).to(dt), stride=c.stride, groups=c.C)
        v = v[:, :, :oh, :ow]
        scale = _vec(p, "scale", oc, dt, 0.0) if "scale" in p else torch.ones(oc, dtype=dt)      # absent: 1
        v = v * scale.view(1, -1, 1, 1) + _vec(p, "bias", oc, dt, 0.0).view(1, -1, 1, 1)
        slope = _vec(p, "slope", oc, dt, 0.0)
        r = None
        if c.res:
            r = torch.from_numpy(data["res"]).to(dt).permute(0, 3, 1, 2)
            if c.res == "pool2":
                r = F.max_pool2d(r, 2)[:, :, :oh, :ow]
            rc = min(r.shape[1], oc)                       # fp_op.res_C: channels beyond it add 0
            r = F.pad(r[:, :rc], (0, 0, 0, 0, 0, oc - rc))
        if c.res in ("before", "pool2"):
            v = v + r
        if pre:
            return v.permute(0, 2, 3, 1).numpy()
        v = _act(v, c.act, slope)
        if c.res == "after":
            v = v + r
        if c.res == "shuffle":                             # out[2c] = res[c], out[2c + 1] = act(conv)[c]
            v = torch.stack([r, v], dim=2).reshape(v.shape[0], 2 * oc, oh, ow)
    elif c.kind == "maxpool":
        xp = _pad_window(x, float("-inf"), c.k, c.stride, c.pad, oh, ow)
        v = F.max_pool2d(xp, c.k, c.stride)[:, :, :oh, :ow]
    elif c.kind == "upsample":
        iy, ix = torch.arange(oh) // 2, torch.arange(ow) // 2
        v = x[:, :, iy][:, :, :, ix]
    elif c.kind == "copy":
        v = x
    elif c.kind == "l2norm":
        v = x / torch.sqrt((x * x).sum(dim=1, keepdim=True))      # no epsilon (mobile_facenet.py l2_norm)
    else:
        raise ValueError(c.kind)
    return np.ascontiguousarray(v.permute(0, 2, 3, 1).numpy())


def tolerance(c):
    """The relative term of the fp64 bound: 2e-7, or 2e-6 where fp_silu's hardware exp2 / rcp take part."""
    return 2e-6 if c.act == "silu" else 2e-7


# ---------------------------------------------------------------------------------------------------------------------------
# footprint
# ---------------------------------------------------------------------------------------------------------------------------
def footprint(op, n_run=None):
    """Arena indices (int64 array [n, OH, OW, Cw]) of every float the op may write when it runs on n_run images (default
    op.N), from its output view: out_off + n*out_ns + pix*out_ld + c*out_cmul; pix = y*(OW + 1) + x in a row-padded output;
    FP_RES_SHUFFLE2 writes both interleaved halves (2*Cout dense channels); a conv's Cout is its output view's channel count,
    zero-weight pad channels included."""
    n = op.N if n_run is None else n_run
    spatial = op.kind not in (L.OP_COPY, L.OP_L2NORM)
    oh, ow = (op.OH, op.OW) if spatial else (op.H, op.W)
    cw = op.Cout if op.kind == L.OP_CONV else op.Cin
    if op.kind == L.OP_CONV and op.res_mode == L.RES_SHUFFLE2:
        cw = 2 * op.Cout
    pitch = ow + 1 if op.flags & L.OPF_OUT_ROWPAD else ow
    ni = np.arange(n, dtype=np.int64).reshape(-1, 1, 1, 1)
    yi = np.arange(oh, dtype=np.int64).reshape(1, -1, 1, 1)
    xi = np.arange(ow, dtype=np.int64).reshape(1, 1, -1, 1)
    ci = np.arange(cw, dtype=np.int64).reshape(1, 1, 1, -1)
    return op.out_off + ni * op.out_ns + (yi * pitch + xi) * op.out_ld + ci * op.out_cmul


def input_index(c, buf, view_coff, view_C, N, H, W):
    """Arena indices [N, H, W, view_C] of a dense channel slice of an input buffer."""
    ni = np.arange(N, dtype=np.int64).reshape(-1, 1, 1, 1)
    pi = np.arange(H * W, dtype=np.int64).reshape(1, H, W, 1)
    ci = np.arange(view_C, dtype=np.int64).reshape(1, 1, 1, -1)
    return buf.off + view_coff + ni * buf.ns + pi * buf.ld + ci


# ---------------------------------------------------------------------------------------------------------------------------
# census of the shipped plans
# ---------------------------------------------------------------------------------------------------------------------------
def _hang(op):
    """The last window reaches beyond the symmetric padding: past row H - 1 + pad_t or column W - 1 + pad_l."""
    return bool((op.OH - 1) * op.stride - op.pad_t + op.KH - 1 > op.H - 1 + op.pad_t or
                (op.OW - 1) * op.stride - op.pad_l + op.KW - 1 > op.W - 1 + op.pad_l)


def feature_key(op, name=None):
    """The feature key of an op that runs on a generic kernel, or None for any other op.
      conv    : (instance, KH, KW, stride, pad_t, pad_l, hanging, act, res_mode, out_cmul, small map (OH*OW < 32), scale,
                 FP_OPF_IN_C3, sliced in, sliced out, foreign image stride in, out)
      dwconv  : (instance, K, stride, pad, hanging, act, scale, bias, OW % 4 != 0, sliced in, sliced out)
      maxpool : (instance, K, stride, pad, hanging, sliced in, sliced out)
      upsample: (instance, sliced in, sliced out)
      copy    : (instance, out_cmul, sliced in, sliced out, row-padded out)
      l2norm  : (instance, H*W > 1, foreign image stride in, out, in_ld != D, out_ld != D)"""
    name = name or kernel_name(op)
    if name.split("<")[0] not in GENERIC:
        return None
    spatial = op.kind not in (L.OP_COPY, L.OP_L2NORM)
    ohw = op.OH * op.OW if spatial else op.H * op.W
    sl_in = op.in_ld != op.Cin
    wc = 2 * op.Cout if op.res_mode == L.RES_SHUFFLE2 else (op.Cout if op.kind == L.OP_CONV else op.Cin)
    rowpad = bool(op.flags & L.OPF_OUT_ROWPAD)
    sl_out = op.out_ld != wc * op.out_cmul
    fns_in = op.in_ns != op.H * op.W * op.in_ld
    fns_out = (not rowpad) and op.out_ns != ohw * op.out_ld
    if op.kind == L.OP_CONV:
        return (name, op.KH, op.KW, op.stride, op.pad_t, op.pad_l, _hang(op), op.act, op.res_mode, op.out_cmul, ohw < 32,
                op.scale_off >= 0, bool(op.flags & L.OPF_IN_C3), sl_in, sl_out, fns_in, fns_out)
    if op.kind == L.OP_DWCONV:
        return (name, op.KH, op.stride, op.pad_t, _hang(op), op.act, op.scale_off >= 0, op.bias_off >= 0, op.OW % 4 != 0,
                sl_in, sl_out)
    if op.kind == L.OP_MAXPOOL:
        return (name, op.KH, op.stride, op.pad_t, _hang(op), sl_in, sl_out)
    if op.kind == L.OP_UPSAMPLE2X:
        return (name, sl_in, sl_out)
    if op.kind == L.OP_COPY:
        return (name, op.out_cmul, sl_in, sl_out, rowpad)
    if op.kind == L.OP_L2NORM:
        return (name, ohw > 1, fns_in, fns_out, op.in_ld != op.Cin, op.out_ld != op.Cin)
    return None


def product_plans():
    """(label, builder) of the plans the shipped networks emit, on the host: every network, several batch sizes, u8 and fp32
    frames, the split-MFMA kernels on and off (PlanBuilder.X6)."""
    from face_detection_and_recognition_amd.modules.age_gender.age_gender_net import AgeGenderNet
    from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace
    from face_detection_and_recognition_amd.modules.facenet.inception_resnet_v1 import InceptionResnetV1
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    from face_detection_and_recognition_amd.modules.mtcnn.mtcnn import MTCNN
    from face_detection_and_recognition_amd.modules.yolov5_face.yolo import Model

    torch.manual_seed(0)
    emit = {}
    for back in (False, True):
        net = BlazeFace(back)
        emit[f"blazeface{int(back)}"] = lambda n, net=net: net._emit(n)[0]
        emit[f"blazeface{int(back)}_u8"] = lambda n, net=net: net._emit(n, frame_hw=(576, 1024))[0]
    for cfg in ("yolov5n", "yolov5s", "yolov5n-0.5"):
        net = Model(cfg)
        emit[cfg] = lambda n, net=net: net._emit(n, 640, 640)[0]
        emit[cfg + "_u8"] = lambda n, net=net: net._emit(n, 640, 640, frame_hw=(576, 1024))[0]
    mfn = MobileFaceNet(512)
    emit["mobile_facenet"] = lambda n: mfn._emit(n)[0]
    for d in (128, 512):
        fn = InceptionResnetV1(d)
        emit[f"facenet{d}"] = lambda n, fn=fn: fn._emit(n)[0]
    mt = MTCNN()
    for name in ("rnet", "onet"):
        emit[name] = lambda n, name=name: mt._emit(name, n)[0]
    for lh, lw in ((12, 12), (17, 23), (58, 81), (96, 135)):
        emit[f"pnet{lh}x{lw}"] = lambda n, lh=lh, lw=lw: mt._emit_pnet(n, lh, lw)[0]
    ag = AgeGenderNet()
    emit["age_gender"] = lambda n: ag._emit(n)[0]
    saved = PlanBuilder.X6
    try:
        for label, fn in emit.items():
            for n in (1, 16, 256):
                for x6 in (True, False):
                    PlanBuilder.X6 = x6
                    yield f"{label}/N={n}/X6={int(x6)}", fn(n)
    finally:
        PlanBuilder.X6 = saved


@functools.lru_cache(maxsize=None)
def census():
    """{feature key: label of the first plan that reaches a generic kernel with it} over product_plans()."""
    found = {}
    for label, pb in product_plans():
        for op in pb.finish()[0]:
            key = feature_key(op)
            if key is not None:
                found.setdefault(key, label)
    return found


# ---------------------------------------------------------------------------------------------------------------------------
# one case per census key
# ---------------------------------------------------------------------------------------------------------------------------
_ACT_NAMES = {v: k for k, v in ACTS.items()}
_RES_NAMES = {v: k for k, v in RES.items()}
_NB_COUT = {1: 24, 2: 64, 3: 96, 4: 128}


def _in_size(o, k, stride, pad, hang):
    """Input extent for o outputs: the window just fits the symmetric padding, or (hang) overshoots it by one."""
    return (o - 1) * stride + k - 2 * pad - (1 if hang else 0)


def case_from_key(key, i):
    """A small case with exactly this feature key (feature_key of its op gives `key` back; test_generic_ops checks that)."""
    name = key[0]
    fam = name.split("<")[0]
    tag = f"census{i:02d}"
    if fam == "conv_igemm_kernel":
        (_, kh, kw, stride, pt, pl, hang, act, res_mode, cmul, small, scale, c3, sl_in, sl_out, fns_in, fns_out) = key
        nb = int(name.split("<")[1].split(",")[0])
        res = _RES_NAMES[res_mode]
        cout = _NB_COUT[nb]
        oh, ow = (2, 3) if small else (7, 9)
        if small and kh == 7 and kw == 7 and stride == 1:      # a window as large as the map (a Linear over a 7 x 7 map)
            oh = ow = 1
        H, W = _in_size(oh, kh, stride, pt, hang), _in_size(ow, kw, stride, pl, hang)
        C = 4 if c3 else 8
        wc = 2 * cout if res == "shuffle" else cout
        return Case(f"{tag}_conv", "conv", name, 3, H, W, C, cin=3 if c3 else 0, cout=cout, k=(kh, kw), stride=stride, pad=(pt, pl),
                    OH=oh, OW=ow, act=_ACT_NAMES[act], scale=scale, res=res,
                    in_buf_C=C + 8 if sl_in else 0, in_coff=4 if sl_in else 0, in_ns_extra=20 if fns_in else 0,
                    out_buf_C=(wc * cmul + 8 if sl_out else 0), out_coff=4 if sl_out else 0, out_cmul=cmul,
                    out_ns_extra=24 if fns_out else 0, partial=1 if i % 2 == 0 else 0)
    if fam in ("dwconv_kernel", "dwconv3_row_kernel"):
        (_, k, stride, pad, hang, act, scale, bias, ragged, sl_in, sl_out) = key
        oh, ow = (1, 1) if (k == 7 and pad == 0) else (5, 6 if ragged else 8)
        H, W = _in_size(oh, k, stride, pad, hang), _in_size(ow, k, stride, pad, hang)
        return Case(f"{tag}_dw", "dwconv", name, 3, H, W, 8, k=(k, k), stride=stride, pad=(pad, pad), OH=oh, OW=ow,
                    act=_ACT_NAMES[act], scale=scale, bias=bias, in_buf_C=16 if sl_in else 0, in_coff=4 if sl_in else 0,
                    out_buf_C=16 if sl_out else 0, out_coff=4 if sl_out else 0, partial=1 if i % 2 == 0 else 0)
    if fam in ("maxpool_kernel", "maxpool_generic_kernel"):
        (_, k, stride, pad, hang, sl_in, sl_out) = key
        oh, ow = 5, 6
        H, W = _in_size(oh, k, stride, pad, hang), _in_size(ow, k, stride, pad, hang)
        return Case(f"{tag}_pool", "maxpool", name, 3, H, W, 8, k=(k, k), stride=stride, pad=(pad, pad), OH=oh, OW=ow,
                    in_buf_C=16 if sl_in else 0, in_coff=4 if sl_in else 0, out_buf_C=16 if sl_out else 0,
                    out_coff=8 if sl_out else 0, special="inf", partial=1 if i % 2 == 0 else 0)
    if fam == "upsample2x_kernel":
        (_, sl_in, sl_out) = key
        return Case(f"{tag}_up", "upsample", name, 3, 3, 5, 8, in_buf_C=16 if sl_in else 0, in_coff=4 if sl_in else 0,
                    out_buf_C=20 if sl_out else 0, out_coff=8 if sl_out else 0)
    if fam in ("copy_kernel", "copy4_kernel"):
        (_, cmul, sl_in, sl_out, rowpad) = key
        return Case(f"{tag}_copy", "copy", name, 3, 4, 5, 8, in_buf_C=16 if sl_in else 0, in_coff=4 if sl_in else 0,
                    out_buf_C=(8 * cmul + 8 if sl_out else 0), out_coff=4 if sl_out else 0, out_cmul=cmul, out_rowpad=rowpad)
    if fam == "l2norm_kernel":
        (_, hw, fns_in, fns_out, ld_in, ld_out) = key
        return Case(f"{tag}_l2", "l2norm", name, 5, 2 if hw else 1, 3 if hw else 1, 512, in_buf_C=520 if ld_in else 0,
                    in_coff=4 if ld_in else 0, out_buf_C=516 if ld_out else 0, in_ns_extra=12 if fns_in else 0,
                    out_ns_extra=8 if fns_out else 0)
    raise ValueError(key)


# The feature keys census() found in the shipped plans when this table was last brought up to date (tests/test_generic_ops.py
# test_census_is_covered fails, printing the missing keys, as soon as census() finds one that is not here).
CENSUS_KEYS = [
    ('conv_igemm_kernel<1, true, false>', 1, 1, 1, 0, 0, False, 0, 0, 1, False, False, False, False, False, False, True),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 0, 0, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 0, 0, False, 2, 0, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 0, 0, False, 2, 0, 1, False, False, True, False, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 0, 0, False, 2, 0, 1, True, False, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, True, True, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 1, 1, 1, False, 3, 2, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 2, 0, 0, False, 1, 0, 1, False, True, True, False, False, False, False),
    ('conv_igemm_kernel<1, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 0, 0, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 0, 0, 1, True, False, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 3, 4, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<1, true, true>', 1, 1, 1, 0, 0, False, 3, 4, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<2, true, false>', 2, 2, 1, 0, 0, False, 2, 0, 1, True, False, False, False, False, False, False),
    ('conv_igemm_kernel<2, true, false>', 3, 3, 1, 0, 0, False, 2, 0, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<2, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<2, true, false>', 3, 3, 1, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<2, true, false>', 3, 3, 1, 1, 1, False, 3, 2, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<2, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<2, true, true>', 1, 1, 1, 0, 0, False, 0, 0, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<2, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<2, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<2, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 1, 1, 1, 0, 0, False, 0, 0, 1, False, False, False, False, False, False, True),
    ('conv_igemm_kernel<3, true, false>', 1, 1, 1, 0, 0, False, 1, 3, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 1, 3, 1, 0, 1, False, 1, 0, 1, True, True, False, True, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 1, 1, 1, 0, False, 1, 0, 1, True, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 1, 0, 0, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 1, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 1, 1, 1, False, 3, 2, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<3, true, false>', 7, 7, 4, 0, 0, False, 1, 0, 1, False, False, True, False, False, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 1, 1, 1, False, False, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<3, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 1, 7, 1, 0, 3, False, 1, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 2, 2, 1, 0, 0, False, 2, 0, 1, True, False, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 1, 0, 0, False, 2, 0, 1, True, False, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, False, False, True, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 1, 1, 1, False, 1, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 0, 0, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 0, 0, False, 1, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 0, 0, False, 1, 0, 1, True, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 0, 0, False, 1, 0, 1, True, True, False, True, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 3, 3, 2, 1, 1, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, false>', 5, 5, 1, 2, 2, False, 1, 0, 1, False, False, False, True, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 7, 1, 1, 3, 0, False, 1, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, false>', 7, 7, 1, 0, 0, False, 1, 0, 1, True, False, False, True, True, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 0, 0, 1, True, True, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 0, 1, 1, True, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, True, False, False, True, True, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 0, 1, True, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 1, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 1, 1, 1, True, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 2, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, False, True, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 3, 0, 1, False, True, False, True, False, False, False),
    ('conv_igemm_kernel<4, true, true>', 1, 1, 1, 0, 0, False, 3, 4, 1, False, True, False, False, False, False, False),
    ('copy4_kernel', 1, False, False, True),
    ('dwconv3_row_kernel<1>', 3, 1, 1, False, 0, False, True, False, False, False),
    ('dwconv3_row_kernel<1>', 3, 1, 1, False, 0, True, True, False, False, False),
    ('dwconv3_row_kernel<2>', 3, 2, 0, True, 0, False, True, False, False, False),
    ('dwconv3_row_kernel<2>', 3, 2, 1, False, 0, True, True, False, False, False),
    ('dwconv3_row_kernel<2>', 3, 2, 1, False, 0, True, True, False, True, False),
    ('dwconv_kernel<7>', 7, 1, 0, False, 0, True, True, True, False, False),
    ('l2norm_kernel', False, False, False, False, False),
    ('maxpool_kernel', 2, 2, 0, False, False, False),
    ('maxpool_kernel', 2, 2, 0, True, False, False),
    ('maxpool_kernel', 3, 1, 1, False, True, True),
    ('maxpool_kernel', 3, 2, 0, False, False, False),
    ('maxpool_kernel', 3, 2, 0, False, False, True),
    ('maxpool_kernel', 3, 2, 0, True, False, False),
    ('upsample2x_kernel', True, True),
]


def _c(name, **kw):
    return Case(name=name, **kw)


_V = "conv_igemm_kernel<%d, %s, %s>"


def _conv(name, nb, vec, pwd, **kw):
    kw.setdefault("N", 2)
    return Case(name=name, kind="conv", kernel=_V % (nb, "true" if vec else "false", "true" if pwd else "false"), **kw)


HAND = [
    # ---- conv: every instance, channel-count edges ----------------------------------------------------------------------
    _conv("pw_c24_dense", 1, 1, 1, H=9, W=7, C=16, cout=24, act="relu"),
    _conv("pw_c64_dense", 2, 1, 1, H=9, W=7, C=16, cout=64, act="prelu", partial=1),
    _conv("pw_c96_dense", 3, 1, 1, H=9, W=7, C=16, cout=96, act="silu"),
    _conv("pw_c128_dense", 4, 1, 1, H=9, W=7, C=16, cout=128, res="after", act="relu"),
    _conv("pw_c192_nb3", 3, 1, 1, H=5, W=5, C=24, cout=192),
    _conv("pw_c256_nb4", 4, 1, 1, H=5, W=5, C=24, cout=256, act="relu", res="before"),
    _conv("pw_c100_nb4", 4, 1, 1, H=6, W=5, C=12, cout=100, act="prelu"),
    _conv("pw_c136_partial_tile", 4, 1, 1, H=12, W=12, C=20, cout=136, act="relu", res="after", partial=1),
    _conv("pw_c160_partial_tile", 4, 1, 1, H=6, W=6, C=20, cout=160, act="silu"),
    _conv("c3x3_c136_partial_tile", 4, 1, 0, H=9, W=9, C=8, cout=136, k=(3, 3), pad=(1, 1), act="prelu"),
    _conv("c3x3_c40", 2, 1, 0, H=8, W=8, C=8, cout=40, k=(3, 3), pad=(1, 1), stride=2, act="relu"),
    _conv("c3x3_c10_in_c3", 1, 1, 0, H=10, W=9, C=4, cin=3, cout=10, k=(3, 3), act="prelu"),
    # Cout % 4 != 0 through out.view(0, 6): scalar epilogue; the same op with the 4-aligned view: vector epilogue
    _conv("pw_c6_scalar_epi", 1, 1, 0, H=9, W=7, C=32, cout=6, out_C=6, out_buf_C=8),
    _conv("pw_c6_vector_epi", 1, 1, 1, H=9, W=7, C=32, cout=6, out_C=8),
    _conv("c3x3_c6_scalar_epi_res", 1, 1, 0, H=6, W=6, C=8, cout=6, out_C=6, out_buf_C=8, k=(3, 3), pad=(1, 1), act="relu",
          res="before", res_C=6, res_buf_C=8),
    # out_cmul = 2 (scalar epilogue): the other parity of the interleaved buffer is not written
    _conv("pw_cmul2_even", 1, 1, 0, H=5, W=6, C=16, cout=16, out_cmul=2, act="silu", partial=1),
    _conv("pw_cmul2_odd", 2, 1, 0, H=5, W=6, C=16, cout=64, out_cmul=2, out_coff=1, act="relu"),
    _conv("c3x3_cmul2_nb3", 3, 1, 0, H=5, W=6, C=8, cout=96, k=(3, 3), pad=(1, 1), out_cmul=2, act="prelu", res="after"),
    _conv("pw_cmul2_nb4", 4, 1, 0, H=5, W=6, C=8, cout=128, out_cmul=2, out_coff=1, bias=False),
    # K % 8 != 0 (K = 12, 36, 100)
    _conv("pw_k12", 1, 1, 1, H=7, W=7, C=12, cout=24),
    _conv("c3x3_k36", 1, 1, 0, H=7, W=7, C=4, cout=24, k=(3, 3), pad=(1, 1), act="relu"),
    _conv("c5x5_k100", 1, 1, 0, H=9, W=9, C=4, cout=16, k=(5, 5), pad=(2, 2), act="relu"),
    # rows: M not a multiple of the tile, M = 1, tiny maps at N = 70 (a 32-row tile spans many images)
    _conv("pw_m1", 1, 1, 1, N=1, H=1, W=1, C=16, cout=24, act="relu"),
    _conv("pw_1x1_n70", 2, 1, 1, N=70, H=1, W=1, C=32, cout=64, act="prelu", partial=33),
    _conv("pw_3x3map_n70_slice", 1, 1, 1, N=70, H=3, W=3, C=8, cout=24, in_buf_C=16, in_coff=8, act="relu"),
    _conv("c3x3_3x3map_n70", 2, 1, 0, N=70, H=3, W=3, C=8, cout=40, k=(3, 3), pad=(1, 1), act="relu", res="after", partial=7),
    _conv("c3x3_1x1map_n70_scalar", 1, 1, 0, N=70, H=3, W=3, C=8, cout=6, out_C=6, out_buf_C=8, k=(3, 3), act="prelu"),
    _conv("pw_m130", 4, 1, 1, N=1, H=10, W=13, C=16, cout=128, act="silu"),
    # the same pointwise op dense (PWD) and through views that leave the dense path
    _conv("pw_dense_ref", 2, 1, 1, H=6, W=7, C=24, cout=64, act="relu", res="after"),
    _conv("pw_in_slice", 2, 1, 1, H=6, W=7, C=24, cout=64, act="relu", res="after", in_buf_C=40, in_coff=12),
    _conv("pw_in_foreign_ns", 2, 1, 0, H=6, W=7, C=24, cout=64, act="relu", res="after", in_ns_extra=36, partial=1),
    _conv("pw_out_foreign_ns", 2, 1, 0, H=6, W=7, C=24, cout=64, act="relu", res="after", out_ns_extra=64),
    _conv("pw_out_slice", 2, 1, 1, H=6, W=7, C=24, cout=64, act="relu", out_buf_C=96, out_coff=16),
    _conv("pw_res_slice", 2, 1, 1, H=6, W=7, C=24, cout=64, act="relu", res="before", res_buf_C=96, res_coff=20),
    _conv("c3x3_res_slice", 2, 1, 0, H=6, W=7, C=8, cout=64, k=(3, 3), pad=(1, 1), act="silu", res="after", res_buf_C=80,
          res_coff=8),
    # residual forms
    _conv("pw_pool2_res_lt_cout", 2, 1, 0, H=5, W=6, C=24, cout=48, act="relu", res="pool2", res_C=24, partial=1),
    _conv("pw_pool2_res_lt_cout_slice", 3, 1, 0, H=5, W=6, C=24, cout=96, act="relu", res="pool2", res_C=24, res_buf_C=40,
          res_coff=8),
    _conv("pw_pool2_scalar", 1, 1, 0, H=5, W=6, C=24, cout=6, out_C=6, out_buf_C=8, act="relu", res="pool2", res_C=4),
    _conv("pw_shuffle_res_wider", 2, 1, 1, H=5, W=6, C=32, cout=64, act="silu", res="shuffle", res_C=96, res_buf_C=128),
    _conv("c3x3_shuffle", 1, 1, 0, H=5, W=6, C=8, cout=24, k=(3, 3), pad=(1, 1), act="relu", res="shuffle", res_C=32,
          res_buf_C=32),
    # a residual view of 6 channels inside an 8-channel buffer: channels 6, 7 add 0 (the op takes the scalar epilogue)
    _conv("pw_res_c6_of_8", 1, 1, 0, H=5, W=6, C=16, cout=8, act="relu", res="before", res_C=6, res_buf_C=8),
    _conv("c3x3_res_c6_of_8_pool2", 1, 1, 0, H=9, W=9, C=8, cout=12, k=(3, 3), stride=2, pad=(1, 1), OH=4, OW=4,
          act="relu", res="pool2", res_C=6, res_buf_C=8),
    _conv("pw_before_res_lt_cout", 2, 1, 1, H=5, W=6, C=16, cout=64, act="relu", res="before", res_C=24),
    # epilogue parameters
    _conv("pw_no_scale_no_bias", 1, 1, 1, H=5, W=6, C=16, cout=32, scale=False, bias=False),
    _conv("c3x3_no_scale_no_bias_scalar", 1, 1, 0, H=5, W=6, C=8, cout=6, out_C=6, out_buf_C=8, k=(3, 3), pad=(1, 1),
          scale=False, bias=False, act="relu"),
    _conv("pw_prelu_all_negative", 2, 1, 1, H=6, W=6, C=16, cout=64, act="prelu", special="neg"),
    _conv("c3x3_prelu_all_negative_scalar", 1, 1, 0, H=6, W=6, C=8, cout=6, out_C=6, out_buf_C=8, k=(3, 3), pad=(1, 1),
          act="prelu", special="neg"),
    # TF "same": pad 0, the window hangs over the bottom / right edge
    _conv("c3x3_s2_tf_same", 1, 1, 0, H=10, W=8, C=8, cout=24, k=(3, 3), stride=2, OH=5, OW=4, act="relu"),
    _conv("c5x5_s2_tf_same", 1, 1, 0, H=10, W=8, C=4, cin=3, cout=24, k=(5, 5), stride=2, pad=(1, 1), OH=5, OW=4, act="relu",
          partial=1),
    # rectangular windows and the large ones
    _conv("c1x7", 2, 1, 0, H=5, W=9, C=8, cout=64, k=(1, 7), pad=(0, 3), act="relu"),
    _conv("c7x1", 2, 1, 0, H=9, W=5, C=8, cout=64, k=(7, 1), pad=(3, 0), act="relu"),
    _conv("c7x7_s4", 3, 1, 0, H=27, W=23, C=4, cin=3, cout=96, k=(7, 7), stride=4, act="relu"),
    _conv("c7x7_fc_k18816", 4, 1, 0, H=7, W=7, C=384, cout=128, k=(7, 7), act="relu"),
    _conv("c2x2", 1, 1, 0, H=6, W=5, C=8, cout=16, k=(2, 2), act="prelu"),
    # <*, false, false>: an input view that is not 16-byte aligned (a hand-made 6-channel buffer)
    _conv("pw_unaligned_in_nb1", 1, 0, 0, H=5, W=6, C=6, cout=24, act="relu", partial=1),
    _conv("c3x3_unaligned_in_nb2", 2, 0, 0, H=5, W=6, C=6, cout=64, k=(3, 3), pad=(1, 1), act="prelu", res="after"),
    _conv("pw_unaligned_in_nb3", 3, 0, 0, H=5, W=6, C=6, cout=96, act="silu"),
    _conv("c3x3_unaligned_in_nb4_scalar", 4, 0, 0, H=5, W=6, C=6, cout=126, out_C=126, out_buf_C=128, k=(3, 3), stride=2,
          pad=(1, 1), act="relu"),
    _conv("pw_unaligned_slice_of_10", 1, 0, 0, H=5, W=6, C=6, cout=24, in_buf_C=10, in_coff=3, act="relu"),

    # ---- dwconv ---------------------------------------------------------------------------------------------------------
    _c("dw3_s1_ow8", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=2, H=6, W=8, C=64, k=(3, 3), pad=(1, 1), act="prelu"),
    _c("dw3_s1_ow9", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=2, H=6, W=9, C=12, k=(3, 3), pad=(1, 1), act="relu",
       partial=1),
    _c("dw3_s1_ow6", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=2, H=5, W=6, C=20, k=(3, 3), pad=(1, 1)),
    _c("dw3_s1_ow7_slices", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=2, H=5, W=7, C=12, k=(3, 3), pad=(1, 1),
       act="prelu", in_buf_C=20, in_coff=4, out_buf_C=24, out_coff=8),
    _c("dw3_s1_ow3", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=3, H=4, W=3, C=4, k=(3, 3), pad=(1, 1), act="relu"),
    _c("dw3_s1_w1", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=3, H=7, W=1, C=12, k=(3, 3), pad=(1, 1), act="relu"),
    _c("dw3_s1_h1", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=3, H=1, W=7, C=12, k=(3, 3), pad=(1, 1), act="prelu",
       partial=2),
    _c("dw3_s1_pad0", kind="dwconv", kernel="dwconv3_row_kernel<1>", N=2, H=7, W=8, C=20, k=(3, 3), scale=False, bias=False),
    _c("dw3_s2_pad1_ow5", kind="dwconv", kernel="dwconv3_row_kernel<2>", N=2, H=9, W=9, C=12, k=(3, 3), stride=2, pad=(1, 1),
       act="prelu", partial=1),
    _c("dw3_s2_hanging_ow6", kind="dwconv", kernel="dwconv3_row_kernel<2>", N=2, H=8, W=12, C=20, k=(3, 3), stride=2, OH=4,
       OW=6, act="relu"),
    _c("dw3_s2_hanging_slice_in", kind="dwconv", kernel="dwconv3_row_kernel<2>", N=2, H=8, W=8, C=64, k=(3, 3), stride=2,
       OH=4, OW=4, in_buf_C=72, in_coff=4, scale=False),
    _c("dw3_s2_ow3_w1_out", kind="dwconv", kernel="dwconv3_row_kernel<2>", N=2, H=5, W=2, C=4, k=(3, 3), stride=2, pad=(1, 1),
       bias=False),
    _c("dw3_s3", kind="dwconv", kernel="dwconv_kernel<3>", N=2, H=9, W=10, C=12, k=(3, 3), stride=3, pad=(1, 1), act="prelu"),
    _c("dw5_large_map", kind="dwconv", kernel="dwconv_kernel<5>", N=2, H=9, W=8, C=20, k=(5, 5), pad=(2, 2), act="relu",
       partial=1),
    _c("dw5_s2_hanging_slices", kind="dwconv", kernel="dwconv_kernel<5>", N=2, H=8, W=8, C=12, k=(5, 5), stride=2, pad=(1, 1),
       OH=4, OW=4, in_buf_C=16, in_coff=4, out_buf_C=16, act="prelu"),
    _c("dw7_large_map", kind="dwconv", kernel="dwconv_kernel<7>", N=2, H=9, W=10, C=12, k=(7, 7), pad=(3, 3), scale=False),
    _c("dw7_to_1x1", kind="dwconv", kernel="dwconv_kernel<7>", N=5, H=7, W=7, C=64, k=(7, 7)),

    # ---- maxpool --------------------------------------------------------------------------------------------------------
    _c("pool2_s2", kind="maxpool", kernel="maxpool_kernel", N=2, H=8, W=6, C=12, k=(2, 2), stride=2, special="inf"),
    _c("pool2_s2_hang1", kind="maxpool", kernel="maxpool_kernel", N=2, H=7, W=5, C=12, k=(2, 2), stride=2, OH=4, OW=3,
       special="inf", partial=1),
    _c("pool3_s2_hang2", kind="maxpool", kernel="maxpool_kernel", N=2, H=7, W=9, C=8, k=(3, 3), stride=2, OH=4, OW=5,
       special="inf"),
    _c("pool3_s2_pad1", kind="maxpool", kernel="maxpool_kernel", N=2, H=8, W=7, C=8, k=(3, 3), stride=2, pad=(1, 1),
       special="inf"),
    _c("pool3_s1_spp_slices", kind="maxpool", kernel="maxpool_kernel", N=2, H=6, W=5, C=8, k=(3, 3), pad=(1, 1), in_buf_C=32,
       in_coff=8, out_buf_C=32, out_coff=16, special="inf"),
    _c("pool5_s1_spp", kind="maxpool", kernel="maxpool_kernel", N=2, H=6, W=7, C=8, k=(5, 5), pad=(2, 2), special="inf",
       partial=1),
    _c("pool5_s2_hang4", kind="maxpool", kernel="maxpool_kernel", N=2, H=7, W=7, C=8, k=(5, 5), stride=2, OH=4, OW=4,
       special="inf"),
    _c("pool5_map_smaller_than_k", kind="maxpool", kernel="maxpool_kernel", N=3, H=3, W=2, C=8, k=(5, 5), pad=(2, 2),
       special="inf"),
    _c("pool3_h2_w1", kind="maxpool", kernel="maxpool_kernel", N=3, H=2, W=1, C=4, k=(3, 3), pad=(1, 1), special="inf"),
    # padding as wide as the window: the first windows lie wholly in the padding and give -inf
    _c("pool2_pad2_window_in_padding", kind="maxpool", kernel="maxpool_kernel", N=2, H=4, W=3, C=8, k=(2, 2), pad=(2, 2), OH=6,
       OW=5),
    _c("pool4_pad4_window_in_padding", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=4, W=5, C=8, k=(4, 4), stride=2,
       pad=(4, 4), OH=4, OW=5),
    _c("pool4_s2", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=9, W=8, C=8, k=(4, 4), stride=2, pad=(1, 1),
       special="inf"),
    _c("pool4_s2_hang3", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=7, W=7, C=8, k=(4, 4), stride=2, OH=4, OW=4,
       special="inf", partial=1),
    _c("pool7_s1_spp", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=6, W=5, C=8, k=(7, 7), pad=(3, 3),
       special="inf"),
    _c("pool9_s1_spp_slices", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=6, W=7, C=8, k=(9, 9), pad=(4, 4),
       in_buf_C=16, in_coff=8, out_buf_C=32, out_coff=24, special="inf"),
    _c("pool13_s1_spp", kind="maxpool", kernel="maxpool_generic_kernel", N=2, H=5, W=8, C=4, k=(13, 13), pad=(6, 6),
       special="inf"),

    # ---- upsample2x -----------------------------------------------------------------------------------------------------
    _c("up_1x1", kind="upsample", kernel="upsample2x_kernel", N=3, H=1, W=1, C=8, partial=1),
    _c("up_odd", kind="upsample", kernel="upsample2x_kernel", N=2, H=3, W=5, C=12, partial=1),
    _c("up_slice_to_concat_slice", kind="upsample", kernel="upsample2x_kernel", N=2, H=4, W=3, C=8, in_buf_C=24, in_coff=12,
       out_buf_C=40, out_coff=16),

    # ---- copy -----------------------------------------------------------------------------------------------------------
    _c("copy4_dense", kind="copy", kernel="copy4_kernel", N=2, H=5, W=6, C=16, partial=1),
    _c("copy4_slices", kind="copy", kernel="copy4_kernel", N=2, H=5, W=6, C=8, in_buf_C=24, in_coff=8, out_buf_C=32,
       out_coff=20),
    _c("copy4_rowpad", kind="copy", kernel="copy4_kernel", N=3, H=5, W=6, C=24, out_rowpad=True, partial=2),
    _c("copy_cmul2_even", kind="copy", kernel="copy_kernel", N=2, H=4, W=5, C=8, out_cmul=2),
    _c("copy_cmul2_odd", kind="copy", kernel="copy_kernel", N=2, H=4, W=5, C=8, out_cmul=2, out_coff=1, partial=1),
    _c("copy_unaligned", kind="copy", kernel="copy_kernel", N=2, H=4, W=5, C=6, in_buf_C=10, in_coff=3, out_buf_C=9,
       out_coff=2),

    # ---- l2norm ---------------------------------------------------------------------------------------------------------
    _c("l2_d4", kind="l2norm", kernel="l2norm_kernel", N=6, H=1, W=1, C=4),
    _c("l2_d60_m7", kind="l2norm", kernel="l2norm_kernel", N=7, H=1, W=1, C=60, partial=3),
    _c("l2_d64_map", kind="l2norm", kernel="l2norm_kernel", N=3, H=2, W=3, C=64, partial=1),
    _c("l2_d128_ld", kind="l2norm", kernel="l2norm_kernel", N=5, H=1, W=1, C=128, in_buf_C=160, in_coff=16, out_buf_C=136,
       out_coff=4),
    _c("l2_d512", kind="l2norm", kernel="l2norm_kernel", N=5, H=1, W=1, C=512, partial=2),
    _c("l2_d516_map_ld", kind="l2norm", kernel="l2norm_kernel", N=3, H=3, W=2, C=516, in_buf_C=520, out_buf_C=524, out_coff=8),
    _c("l2_in_foreign_ns", kind="l2norm", kernel="l2norm_kernel", N=5, H=1, W=1, C=128, in_ns_extra=24, partial=2),
    _c("l2_out_foreign_ns", kind="l2norm", kernel="l2norm_kernel", N=5, H=1, W=1, C=128, out_ns_extra=40),
    _c("l2_both_foreign_ns_map", kind="l2norm", kernel="l2norm_kernel", N=5, H=2, W=2, C=60, in_ns_extra=7, out_ns_extra=13,
       in_buf_C=64, out_buf_C=61, out_coff=1),
    _c("l2_zero_row", kind="l2norm", kernel="l2norm_kernel", N=5, H=1, W=3, C=64, special="zero_row"),
]


@functools.lru_cache(maxsize=None)
def cases():
    """Every case: one per census key, then the hand-written edges.  Names are unique."""
    out = [case_from_key(k, i) for i, k in enumerate(CENSUS_KEYS)] + HAND
    assert len({c.name for c in out}) == len(out)
    return out


def cases_of(kind):
    return [c for c in cases() if c.kind == kind]
