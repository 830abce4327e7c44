"""Case table, float64 references, write footprints, mutants and the product census for the stems and the Mobile-FaceNet fp32
kernels, the ops tests/generic_op_cases.py, split_conv_cases.py, blaze_op_cases.py and yolo_op_cases.py leave out:

  FP_OP_CONV on a 4-float-pixel image     -> stem_conv_kernel<3|5, 1|2, false>                  (csrc/stem.hip)
  FP_OP_STEM_U8                           -> stem_conv_kernel<3|5, 1|2, true>, stem5_u8_band_kernel, stem5_u8_x6_kernel
  FP_OP_CONV + FP_OPF_OUT_DW              -> stemdw_kernel<false|true>                          (csrc/stemdw.hip)
  FP_OP_DWPW, act2 none                   -> dwpw_kernel<1..4, 1|2|4, 1|2>, dwpw_wp_kernel<2|4, 1|2, 4>,
                                             dwpw_persist_kernel<2|4, 1|2>                      (csrc/dwpw.hip)
  FP_OP_CONV 1x1, K = 64 | 128            -> pws_kernel<64, 12>, pws_kernel<128, 8>             (csrc/pws.hip)
  FP_OP_DWBLOCK without FP_OPF_SPLIT3     -> dwblock_kernel<128, 14, 14, 1>, <128, 7, 7, 3>, <64, 28, 7, 1>   (csrc/dwblock.hip)

tests/test_stem_mfn_ops.py runs every case as a one-op plan.

* A Case says how to build the op with PlanBuilder, the instance the launcher must pick and what the data look like.  build()
  emits the plan, params() / inputs() draw the seeded data (He-scaled weights, affine scales in [0.5, 1.5], biases N(0, 0.2),
  PReLU slopes in [0.1, 0.3], inputs N(0, 1) with one all-zero interior pixel and one |x| = 30 corner pixel, u8 frames uniform),
  reference() computes the op in torch on the CPU in the requested dtype from the op semantics of include/facepath.h, the torch
  modules (modules/blazeface, modules/mobile_facenet) and oracle/image_ref.py -- never from the kernels.
* footprint() is the exact set of arena floats an op may write: dense and row-padded outputs, foreign image strides, under a
  row window the window's rows only.
* TOL is the project's per-op relative term of the fp64 bound (generic_op_cases.tolerance: 2e-7).  The two- and three-stage
  fused ops (stemdw, dwpw, dwblock) keep it, as tests/test_dwblock_x6_ops.py does: test_tolerance_is_not_vacuous holds
  2 * max|ref32 - ref64| + TOL * scale below 1e-5 * scale for every case at that figure.
* mutants() are float64 references of wrong ops: a replicated border, a symmetric pad for the 5x5 stem, R and B exchanged, pad
  colour 0, conv1 evaluated on conv2_dw's padding, a shifted depthwise tap, a dropped shortcut, the PReLU slopes of the wrong
  stage, a stride-2 phase off by one.
* census() / CENSUS_KEYS / case_from_key as in generic_op_cases: the feature keys with which the shipped plans reach these
  kernels (Mobile-FaceNet at the bench batches 528 and 1024 with the split kernels off included), each with a case.
"""
import dataclasses
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import generic_op_cases as G
from generic_op_cases import _raw_buf, hash_name, kernel_name, product_plans  # noqa: F401  (re-exported)
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import PlanBuilder
from oracle import image_ref

FAMILIES = ("stem_conv_kernel", "stem5_u8_band_kernel", "stem5_u8_x6_kernel", "stemdw_kernel", "dwpw_kernel", "dwpw_wp_kernel",
            "dwpw_persist_kernel", "pws_kernel", "dwblock_kernel")
ACTS = G.ACTS
TOL = G.tolerance(SimpleNamespace(act="none"))      # 2e-7 per op; kept for the fused two- and three-stage ops (module docstring)
CACHE_MAX_BYTES = 48 << 20                          # references() keeps what is smaller than this


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                # stem | stem_u8 | stemdw | dwpw | pws | dwblock
    kernel: str              # the instance fp_op_kernel_name must report
    N: int
    H: int = 0               # the input map (stem_u8: the letterbox canvas)
    W: int = 0
    K: int = 3               # stem, stem_u8: the window, stride 2 (3: pad 1; 5: F.pad(1, 2, 1, 2), i.e. pad_t = pad_l = 1 and a
    pad: int = 1             # last window that hangs over the edge by one more)
    cout: int = 0
    act: str = "none"        # stem, stem_u8, pws: none | relu | prelu
    scale: bool = True       # stem, stem_u8, pws: a per-channel scale in front of the bias
    rowpad: bool = False     # stem, stem_u8: the output in the row-padded layout
    frame_hw: tuple = ()     # stem_u8: size of the u8 frames
    swap_rb: bool = False    # stem_u8
    pad_value: int = 125     # stem_u8: the letterbox pad colour
    window: tuple = ()       # stem_u8 on the band kernels: (row_lo, row_end)
    x6: bool = False         # stem_u8, stemdw: the split-bf16 form (FP_OPF_SPLIT3)
    G: int = 0               # dwpw: depthwise channels; pws: K; dwblock: Cin = Cout
    stride: int = 1          # dwpw
    res: bool = False        # dwpw: FP_RES_ADD_AFTER_ACT of a separate view; dwblock: the shortcut
    out_slope: bool = False  # dwpw: PReLU on the 1x1 output
    in_ns_extra: int = 0     # stemdw: floats between the images beyond the dense size
    out_ns_extra: int = 0
    gain: float = 1.0        # stemdw: every conv1 weight and every bias times this power of two
    gated: bool = False      # the instance is chosen by the batch: batch independence is checked by reversing the images
    seed: str = ""           # the name that seeds parameters and inputs (default: name): twins share them


def out_hw(c):
    if c.kind in ("stem", "stem_u8"):
        extra = 2 * c.pad + (1 if c.K == 5 else 0)           # pad in front and behind; the 5x5 stem: one more behind
        return (c.H + extra - c.K) // 2 + 1, (c.W + extra - c.K) // 2 + 1
    if c.kind == "stemdw":
        return 56, 56
    if c.kind == "dwpw":
        return (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    return c.H, c.W


def in_C(c):
    return {"stem": 3, "stem_u8": 3, "stemdw": 3}.get(c.kind, c.G)


def out_C(c):
    return {"stemdw": 64, "dwblock": c.G}.get(c.kind, c.cout)


def stages(c):
    """Chained conv stages of the op."""
    return {"stemdw": 2, "dwpw": 2, "dwblock": 3}.get(c.kind, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(c):
    """Seeded parameters of a case in the shapes of the torch modules: conv weights [O, I, KH, KW], (scale, bias) of every
    eval-mode BatchNorm, PReLU slopes."""
    rng = np.random.default_rng(hash_name(c.seed or c.name) % (2 ** 31))

    def w(o, i, k):
        return rng.normal(0, (2.0 / (i * k * k)) ** 0.5, (o, i, k, k)).astype(np.float32)

    def dw(ch):
        return rng.normal(0, (2.0 / 9) ** 0.5, (ch, 1, 3, 3)).astype(np.float32)

    def aff(n):
        return rng.uniform(0.5, 1.5, n).astype(np.float32), rng.normal(0, 0.2, n).astype(np.float32)

    def slope(n):
        return rng.uniform(0.1, 0.3, n).astype(np.float32)

    if c.kind in ("stem", "stem_u8", "pws"):
        cin, k = (3, c.K) if c.kind != "pws" else (c.G, 1)
        s, b = aff(c.cout)
        return dict(w=w(c.cout, cin, k), scale=s if c.scale else None, bias=b, slope=slope(c.cout) if c.act == "prelu" else None)
    if c.kind == "stemdw":
        g = np.float32(c.gain)
        s1, b1 = aff(64)
        s2, b2 = aff(64)
        return dict(w=w(64, 3, 3) * g, aff1=(s1, b1 * g), slope1=slope(64), dw_w=dw(64), dw_aff=(s2, b2 * g), dw_slope=slope(64))
    if c.kind == "dwpw":
        p = dict(dw_w=dw(c.G), dw_aff=aff(c.G), dw_slope=slope(c.G), pw_w=w(c.cout, c.G, 1), pw_aff=aff(c.cout))
        if c.out_slope:
            p["out_slope"] = slope(c.cout)
        return p
    if c.kind == "dwblock":          # the parameters of tests/test_dwblock_x6_ops.py
        cin, cmid = c.G, 2 * c.G
        return dict(e_w=w(cmid, cin, 1), e_aff=aff(cmid), e_slope=slope(cmid), dw_w=dw(cmid), dw_aff=aff(cmid),
                    dw_slope=slope(cmid), pw_w=w(cin, cmid, 1), pw_aff=aff(cin))
    raise ValueError(c.kind)


@functools.lru_cache(maxsize=2)
def inputs(c):
    """Seeded inputs of a case, read-only: {"x": (N, H, W, C) float32 N(0, 1) with one all-zero pixel in the interior of image 0
    and one pixel of magnitude 30 (alternating signs) in the bottom-left corner of the last image, "res": dwpw's residual view};
    stem_u8: {"frames": (N, fh, fw, 3) uint8}."""
    rng = np.random.default_rng((hash_name(c.seed or c.name) + 1) % (2 ** 31))
    if c.kind == "stem_u8":
        d = {"frames": rng.integers(0, 256, (c.N, *c.frame_hw, 3), dtype=np.uint8)}
    else:
        ch = in_C(c)
        x = rng.standard_normal((c.N, c.H, c.W, ch), dtype=np.float32)
        big, zero = (c.N - 1, c.H - 1, 0), (0, c.H // 2, c.W // 2)
        if zero != big:
            x[zero] = 0.0
        x[big] = 30.0 * (1 - 2 * (np.arange(ch) % 2))
        d = {"x": x}
        if c.kind == "dwpw" and c.res:
            d["res"] = rng.standard_normal((c.N, *out_hw(c), c.cout), dtype=np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------------
def build(c, N=None):
    """Emit the one-op plan of a case through the public emitters -> (builder, {"x": Buf or None, "out": Buf, "res": Buf or
    None}).  A row window goes through PlanBuilder.window and is then set on the op itself, so that every run of the plan is the
    windowed one (CompiledPlan would prime the rows outside it with an unrestricted run first)."""
    pb = PlanBuilder(N or c.N)
    pb.X6 = c.x6
    oh, ow = out_hw(c)
    p = params(c)
    xb = rb = None
    if c.kind in ("stem", "stem_u8"):
        ob = pb.new_buf_rowpad(oh, ow, c.cout, dedicated=bool(c.window)) if c.rowpad else _raw_buf(pb, oh, ow, c.cout)
        kw = dict(pad=(c.pad, c.pad), scale=p["scale"], bias=p["bias"], slope=p["slope"], act=ACTS[c.act])
        if c.kind == "stem":
            xb = pb.new_buf(c.H, c.W, 3)
            got = pb.conv(xb.view(), p["w"], ob.view(), stride=2, **kw)
        else:
            got = pb.stem_u8((c.H, c.W, c.frame_hw[0], c.frame_hw[1], 0), p["w"], ob.view(), split=c.x6, **kw)
    elif c.kind == "stemdw":
        xb = _raw_buf(pb, 112, 112, 4, c.in_ns_extra)
        ob = _raw_buf(pb, 56, 56, 64, c.out_ns_extra)
        got = pb.conv(xb.view(), p["w"], ob.view(), stride=2, pad=(1, 1), scale=p["aff1"][0], bias=p["aff1"][1], slope=p["slope1"],
                      act=L.ACT_PRELU, out_dw=(p["dw_w"], p["dw_aff"], p["dw_slope"]))
    elif c.kind == "dwpw":
        xb = _raw_buf(pb, c.H, c.W, c.G)
        rb = _raw_buf(pb, oh, ow, c.cout) if c.res else None
        ob = _raw_buf(pb, oh, ow, c.cout)
        got = pb.dwpw(xb.view(), p["dw_w"], *p["dw_aff"], p["dw_slope"], p["pw_w"], *p["pw_aff"], ob.view(), c.stride,
                      res=rb.view() if rb is not None else None, out_slope=p.get("out_slope"))
    elif c.kind == "pws":
        xb = _raw_buf(pb, c.H, c.W, c.G)
        ob = _raw_buf(pb, c.H, c.W, c.cout)
        got = pb.conv(xb.view(), p["w"], ob.view(), scale=p["scale"], bias=p["bias"], slope=p["slope"], act=ACTS[c.act])
    elif c.kind == "dwblock":
        xb = pb.new_buf(c.H, c.W, c.G)
        ob = pb.new_buf(c.H, c.W, c.G)
        got = pb.dwblock(xb.view(), p["e_w"], p["e_aff"], p["e_slope"], p["dw_w"], p["dw_aff"], p["dw_slope"], p["pw_w"],
                         p["pw_aff"], ob.view(), c.res, stride=1, fp32=True)
    else:
        raise ValueError(c.kind)
    assert got is not None and len(pb.ops) == 1, c.name
    if c.window:
        pb.window(*c.window)
        (_, lo, end), = pb.windows
        pb.windows.clear()
        pb.ops[0].row_lo, pb.ops[0].row_end = lo, end
    return pb, {"x": xb, "out": ob, "res": rb}


def f32_twin(c):
    """The fp32-image stem with the parameters of a stem_u8 case, on a row-padded output (which only stem_conv_kernel writes:
    the op lands there at any batch)."""
    assert c.kind == "stem_u8"
    nb = (c.cout + 31) // 32
    return dataclasses.replace(c, name=c.name + "_f32", kind="stem", kernel=f"stem_conv_kernel<{c.K}, {nb}, false>", rowpad=True,
                               seed=c.seed or c.name, frame_hw=(), swap_rb=False, window=(), x6=False, gated=False)


# ---------------------------------------------------------------------------------------------------------------------------
# references (torch on the CPU, dtype dt)
# ---------------------------------------------------------------------------------------------------------------------------
def _t(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


def _nchw(a, dt):
    return _t(a, dt).permute(0, 3, 1, 2)


def _aff(v, sb, dt):
    s, b = sb
    if s is not None:
        v = v * _t(s, dt).view(1, -1, 1, 1)
    return v + _t(b, dt).view(1, -1, 1, 1)


def _prelu(v, slope, dt):
    return torch.where(v > 0, v, v * _t(slope, dt).view(1, -1, 1, 1))


def _act(v, act, slope, dt):
    if act == "relu":
        return torch.relu(v)
    return _prelu(v, slope, dt) if act == "prelu" else v


def _conv_pad1(v, w, stride, groups, mut):
    """3x3 conv, zero pad 1.  mut "replicate": the border replicated; "phase": the stride-2 windows start one pixel later."""
    if mut == "replicate":
        return F.conv2d(F.pad(v, (1, 1, 1, 1), mode="replicate"), w, stride=stride, groups=groups)
    if mut == "phase":
        return F.conv2d(F.pad(v, (0, 2, 0, 2)), w, stride=stride, groups=groups)
    return F.conv2d(v, w, stride=stride, padding=1, groups=groups)


def canvas(c, frames, mut=None):
    """The letterbox canvas of a stem_u8 case as (n, H, W, 3) float32: oracle/image_ref.pad_resize_image of every frame onto the
    W x H canvas with the case's pad colour, R and B exchanged if the case says so, through blaze_lut."""
    color = (0 if mut == "pad0" else c.pad_value,) * 3
    lb = np.stack([image_ref.pad_resize_image(f, (c.W, c.H), color) for f in frames])
    assert lb.shape[1:] == (c.H, c.W, 3)
    if c.swap_rb != (mut == "swap"):
        lb = lb[..., ::-1]
    return image_ref.blaze_lut()[lb]


def reference(c, data, dt, mut=None):
    """The op of case c on data (inputs(), or a prefix / selection of its images) in dtype dt -> (n, OH, OW, Cout) numpy.
    mut: a mutation of the op (mutants())."""
    p = params(c)
    oh, ow = out_hw(c)
    with torch.no_grad():
        if c.kind in ("stem", "stem_u8"):
            x = _nchw(canvas(c, data["frames"], mut) if c.kind == "stem_u8" else data["x"], dt)
            if mut == "sympad":          # F.pad(2, 2, 2, 2) in place of (1, 2, 1, 2)
                v = F.conv2d(F.pad(x, (2, 2, 2, 2)), _t(p["w"], dt), stride=2)[:, :, :oh, :ow]
            else:                        # include/facepath.h: pad_t = pad_l in front, zeros wherever the last window hangs over
                pad = 1 if mut == "pad1" else c.pad
                px, py = (ow - 1) * 2 + c.K - pad - c.W, (oh - 1) * 2 + c.K - pad - c.H
                xp = F.pad(x, (pad, max(px, 0), pad, max(py, 0)), mode="replicate" if mut == "replicate" else "constant")
                v = F.conv2d(xp, _t(p["w"], dt), stride=2)[:, :, :oh, :ow]
            v = _act(_aff(v, (p["scale"], p["bias"]), dt), c.act, p["slope"], dt)
        elif c.kind == "stemdw":
            x = _nchw(data["x"], dt)
            if mut == "c1_on_pad":       # conv1 + BN + PReLU evaluated at columns / rows -1 and 56, where conv2_dw pads with 0
                v = F.conv2d(F.pad(x, (3, 3, 3, 3)), _t(p["w"], dt), stride=2)
                v = _prelu(_aff(v, p["aff1"], dt), p["slope1"], dt)
                v = F.conv2d(v, _t(p["dw_w"], dt), groups=64)
            else:
                v = _prelu(_aff(_conv_pad1(x, _t(p["w"], dt), 2, 1, None), p["aff1"], dt), p["slope1"], dt)
                dww = _t(p["dw_w"], dt)
                if mut == "dw_shift":
                    dww = torch.roll(dww, 1, dims=3)
                v = _conv_pad1(v, dww, 1, 64, mut)
            v = _prelu(_aff(v, p["dw_aff"], dt), p["dw_slope"], dt)
        elif c.kind == "dwpw":
            x = _nchw(data["x"], dt)
            v = _aff(_conv_pad1(x, _t(p["dw_w"], dt), c.stride, c.G, mut), p["dw_aff"], dt)
            wrong = mut == "slope_stage"     # the depthwise slopes applied to the 1x1 output and the other way round
            if not wrong:
                v = _prelu(v, p["dw_slope"], dt)
            elif c.out_slope:
                v = _prelu(v, np.resize(p["out_slope"], c.G), dt)
            v = _aff(F.conv2d(v, _t(p["pw_w"], dt)), p["pw_aff"], dt)
            if wrong:
                v = _prelu(v, np.resize(p["dw_slope"], c.cout), dt)
            elif c.out_slope:
                v = _prelu(v, p["out_slope"], dt)
            if c.res and mut != "nores":
                v = v + _nchw(data["res"], dt)
        elif c.kind == "pws":
            b = np.roll(p["bias"], 1) if mut == "bias_roll" else p["bias"]
            v = _aff(F.conv2d(_nchw(data["x"], dt), _t(p["w"], dt)), (p["scale"], b), dt)
            v = _act(v, "none" if mut == "noact" else c.act, p["slope"], dt)
        elif c.kind == "dwblock":        # Depth_Wise.forward (modules/mobile_facenet), as tests/test_dwblock_x6_ops.py
            x = _nchw(data["x"], dt)
            s1, s2 = (p["dw_slope"], p["e_slope"]) if mut == "slope_stage" else (p["e_slope"], p["dw_slope"])
            v = _prelu(_aff(F.conv2d(x, _t(p["e_w"], dt)), p["e_aff"], dt), s1, dt)
            if mut == "e_on_pad":        # the expand stage evaluated on the depthwise conv's padding: PReLU(bias) where 0 belongs
                e0 = _prelu(_aff(torch.zeros(1, 2 * c.G, 1, 1, dtype=dt), p["e_aff"], dt), s1, dt)
                vp = e0.expand(v.shape[0], -1, c.H + 2, c.W + 2).clone()
                vp[:, :, 1:-1, 1:-1] = v
                v = F.conv2d(vp, _t(p["dw_w"], dt), groups=2 * c.G)
            else:
                v = _conv_pad1(v, _t(p["dw_w"], dt), 1, 2 * c.G, mut)
            v = _prelu(_aff(v, p["dw_aff"], dt), s2, dt)
            v = _aff(F.conv2d(v, _t(p["pw_w"], dt)), p["pw_aff"], dt)
            if c.res and mut != "nores":
                v = v + x
        else:
            raise ValueError(c.kind)
    return np.ascontiguousarray(v.permute(0, 2, 3, 1).numpy())


def mutants(c):
    """(label, mut) of the mutations of reference() that a wrong kernel of this kind would amount to."""
    out = []
    if c.kind in ("stem", "stem_u8") and c.pad:
        out.append(("border replicated instead of zero", "replicate"))
    if c.kind in ("stem", "stem_u8"):
        if c.pad == 0:
            out.append(("pad 1 instead of 0", "pad1"))
        if c.K == 5:
            out.append(("symmetric pad (2, 2, 2, 2) instead of (1, 2, 1, 2)", "sympad"))
    if c.kind == "stem_u8":
        out += [("R and B exchanged", "swap"), ("pad colour 0", "pad0")]
    if c.kind == "stemdw":
        out += [("conv1 evaluated on conv2_dw's padding", "c1_on_pad"), ("depthwise taps shifted by one column", "dw_shift")]
    if c.kind in ("dwpw", "dwblock"):
        out += [("border replicated instead of zero", "replicate"), ("PReLU slopes of the wrong stage", "slope_stage")]
        if c.res:
            out.append(("shortcut dropped", "nores"))
    if c.kind == "dwpw" and c.stride == 2:
        out.append(("stride-2 phase shifted by one", "phase"))
    if c.kind == "dwblock":
        out.append(("expand stage evaluated on the depthwise padding", "e_on_pad"))
    if c.kind == "pws":
        out.append(("bias of the neighbouring channel", "bias_roll"))
        if c.act != "none":
            out.append(("activation dropped", "noact"))
    return out


_REFS = {}
_BOUNDS = {}


def references(c):
    """(float64 reference, float32 reference) of a case on its own inputs, read-only; computed once and shared where they are
    small enough to keep (CACHE_MAX_BYTES)."""
    if c not in _REFS:
        data = inputs(c)
        pair = reference(c, data, torch.float64), reference(c, data, torch.float32)
        for r in pair:
            r.setflags(write=False)
        if pair[0].nbytes > CACHE_MAX_BYTES:
            return pair
        _REFS[c] = pair
    return _REFS[c]


def bound(c, r64=None, r32=None):
    """(bound, scale): 2 * max|ref32 - ref64| + TOL * max|ref64|, the bound of the split kernels' tests as well."""
    if r64 is None:
        if c not in _BOUNDS:
            _BOUNDS[c] = bound(c, *references(c))
        return _BOUNDS[c]
    scale = float(np.abs(r64).max())
    return 2.0 * float(np.abs(r32 - r64).max()) + TOL * scale, scale


# ---------------------------------------------------------------------------------------------------------------------------
# footprints
# ---------------------------------------------------------------------------------------------------------------------------
def footprint(op, n_run=None, rows=None):
    """Arena indices [n, rows, OW, Cout] of every float the op may write when it runs on n_run images (default op.N), from its
    output view: pixel (y, x) at y * (OW + 1) + x in a row-padded output and at y * OW + x in a dense one; under a row window
    only rows [row_lo, row_end).  rows: (lo, end) in place of the op's window."""
    n = op.N if n_run is None else n_run
    lo, end = rows or ((op.row_lo, op.row_end) if op.row_end > 0 else (0, op.OH))
    if op.kind == L.OP_CONV and (lo, end) == (0, op.OH):
        return G.footprint(op, n)
    pitch = op.OW + 1 if op.flags & L.OPF_OUT_ROWPAD else op.OW
    ni = np.arange(n, dtype=np.int64).reshape(-1, 1, 1, 1)
    yi = np.arange(lo, end, dtype=np.int64).reshape(1, -1, 1, 1)
    xi = np.arange(op.OW, dtype=np.int64).reshape(1, 1, -1, 1)
    ci = np.arange(op.Cout, dtype=np.int64).reshape(1, 1, 1, -1)
    return op.out_off + ni * op.out_ns + (yi * pitch + xi) * op.out_ld + ci


def out_view(op, n_run=None, rows=None):
    """The same set as a strided view of the arena: (offset, shape [n, rows, OW, Cout], strides), in floats."""
    n = op.N if n_run is None else n_run
    lo, end = rows or ((op.row_lo, op.row_end) if op.row_end > 0 else (0, op.OH))
    pitch = op.OW + 1 if op.flags & L.OPF_OUT_ROWPAD else op.OW
    return (op.out_off + lo * pitch * op.out_ld, (n, end - lo, op.OW, op.Cout), (op.out_ns, pitch * op.out_ld, op.out_ld, 1))


def in_view(buf, n, H, W, C):
    """The first C channels of n images of a dense input buffer as a strided view of the arena: (offset, shape, strides)."""
    return buf.off, (n, H, W, C), (buf.ns, W * buf.ld, buf.ld, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# census of the shipped plans
# ---------------------------------------------------------------------------------------------------------------------------
def feature_key(op, name=None, windowed=None):
    """The feature key of an op that lands on one of FAMILIES (dwpw_kernel: in its Mobile-FaceNet forms only, act2 none), or
    None: (instance, (KH, stride, pad_t), act, res_mode, output PReLU present, row-padded out, FP_OPF_IN_C3, FP_OPF_SPLIT3,
    row window present)."""
    name = name or kernel_name(op)
    fam = name.split("<")[0]
    if fam not in FAMILIES or (fam == "dwpw_kernel" and op.act2 != L.ACT_NONE):
        return None
    windowed = op.row_end > 0 if windowed is None else windowed
    return (name, (op.KH, op.stride, op.pad_t), op.act, op.res_mode, op.kind == L.OP_DWPW and op.bias_off >= 0,
            bool(op.flags & L.OPF_OUT_ROWPAD), bool(op.flags & L.OPF_IN_C3), bool(op.flags & L.OPF_SPLIT3), bool(windowed))


BENCH_BATCHES = (528, 1024)      # Mobile-FaceNet's bench batches: above product_plans()'s largest, 256


def bench_plans():
    """(label, builder) of Mobile-FaceNet at the bench batches with the split kernels off (--mfma fp32): only there do
    dwpw_persist_kernel<4, 1>, pws_kernel<128, 8> and dwblock_kernel<128, 7, 7, 3> appear."""
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    torch.manual_seed(0)
    net = MobileFaceNet(512)
    saved = PlanBuilder.X6
    try:
        PlanBuilder.X6 = False
        for n in BENCH_BATCHES:
            yield f"mobile_facenet/N={n}/X6=0", net._emit(n)[0]
    finally:
        PlanBuilder.X6 = saved


@functools.lru_cache(maxsize=None)
def census():
    """{feature key: label of the first plan that reaches one of FAMILIES with it} over product_plans() and bench_plans(); an
    op listed in the builder's `windows` is counted with and without its window (CompiledPlan runs it both ways)."""
    found = {}
    for source in (product_plans, bench_plans):
        for label, pb in source():
            ops = pb.finish()[0]
            win = {i for i, _, _ in pb.windows}
            for i, op in enumerate(ops):
                name = kernel_name(op)
                for w in ((False, True) if i in win else (None,)):
                    key = feature_key(op, name, w)
                    if key is not None:
                        found.setdefault(key, label)
    return found



# ---------------------------------------------------------------------------------------------------------------------------
# hand-written cases: the smallest shapes at which each kernel can still go wrong
# ---------------------------------------------------------------------------------------------------------------------------
def _st(name, k, nb, **kw):
    return Case(name, "stem", f"stem_conv_kernel<{k}, {nb}, false>", K=k, **kw)


def _u8(name, k, nb, **kw):
    return Case(name, "stem_u8", f"stem_conv_kernel<{k}, {nb}, true>", K=k, **kw)


def _band(name, x6=False, **kw):
    return Case(name, "stem_u8", "stem5_u8_x6_kernel" if x6 else "stem5_u8_band_kernel", N=16, H=256, W=256, K=5, cout=24,
                act="relu", scale=False, swap_rb=True, x6=x6, gated=True, seed="band_" + "x".join(map(str, kw["frame_hw"])), **kw)


def _sd(name, x6, **kw):
    return Case(name + ("_x6" if x6 else ""), "stemdw", f"stemdw_kernel<{'true' if x6 else 'false'}>", H=112, W=112, x6=x6,
                seed=name, **kw)


def _dk(name, nb, p, s, **kw):
    return Case(name, "dwpw", f"dwpw_kernel<{nb}, {p}, {s}>", stride=s, **kw)


def _blk(c, hw, rb, nimg, n, res):
    return Case(f"blk_{c}_{hw}_n{n}_{'res' if res else 'nores'}", "dwblock", f"dwblock_kernel<{c}, {hw}, {rb}, {nimg}>", N=n, H=hw,
                W=hw, G=c, res=res, seed=f"blk_{c}_{hw}_n{n}")


LAND, PORT = (24, 40), (40, 24)      # frames of the band stems: the 256 x 256 canvas pads above / below, left / right
# interior, touching row 0, touching row 127; a landscape frame's content lies in output rows 25 .. 102, a portrait one's in every row
WINDOWS = ((37, 90), (0, 33), (90, 128))

HAND = [
    # ---- stem_conv_kernel<K, NB, false>: a tile is 128 consecutive output pixels of one image --------------------------------
    _st("st_k3_nb1_rp_9x7", 3, 1, N=3, H=9, W=7, cout=8, rowpad=True),                          # 5 x 4 outputs: a tile of 5 rows
    _st("st_k3_nb2_rp_20x36", 3, 2, N=2, H=20, W=36, cout=40, rowpad=True, act="prelu"),        # OW = 18: tiles straddle rows
    _st("st_k5_nb1_rp_20x36", 5, 1, N=2, H=20, W=36, cout=24, rowpad=True, act="relu", scale=False),
    _st("st_k5_nb2_rp_10x6", 5, 2, N=2, H=10, W=6, cout=64, rowpad=True, act="prelu"),          # 5 x 3 outputs
    _st("st_k5_dense_n32_128", 5, 1, N=32, H=128, W=128, cout=24, act="relu", scale=False, gated=True),     # 1024 tiles on 768
    _st("st_k3_dense_n42_112", 3, 2, N=42, H=112, W=112, cout=64, act="prelu", gated=True),     # 24.5 tiles per image: ragged
    _st("st_k3_pad0_dense_n22_160", 3, 1, N=22, H=160, W=160, pad=0, cout=32, act="relu", gated=True),      # FaceNet's conv2d_1a
    # ---- stem_conv_kernel<K, NB, true>: the canvas resampled from u8 frames while a tile is staged ----------------------------
    _u8("u8_k5_nb1_20x36_rp", 5, 1, N=3, H=20, W=36, cout=24, frame_hw=(9, 13), act="relu", scale=False, swap_rb=True, rowpad=True),
    _u8("u8_k3_nb1_18x10", 3, 1, N=3, H=18, W=10, cout=16, frame_hw=(7, 5), act="prelu", pad_value=37),     # pads left and right
    _u8("u8_k3_nb2_20x36", 3, 2, N=3, H=20, W=36, cout=48, frame_hw=(9, 13), pad_value=200, swap_rb=True),
    _u8("u8_k5_nb2_12x12", 5, 2, N=2, H=12, W=12, cout=64, frame_hw=(4, 5), act="prelu", pad_value=1),      # (fp32 twin: 63 KB of LDS)
    _u8("u8_k5_800tiles_64x64", 5, 1, N=100, H=64, W=64, cout=24, frame_hw=(20, 30), act="relu", scale=False, swap_rb=True),
    # ---- the band stems: 16 frames onto the 256 x 256 canvas -------------------------------------------------------------------
    _band("band_land", frame_hw=LAND),
    _band("band_port_rp", frame_hw=PORT, rowpad=True),
    _band("band_port_rp_win_37_90", frame_hw=PORT, rowpad=True, window=WINDOWS[0]),
    _band("band_land_rp_win_0_33", frame_hw=LAND, rowpad=True, window=WINDOWS[1]),
    _band("band_port_rp_win_90_128", frame_hw=PORT, rowpad=True, window=WINDOWS[2]),
    _band("x6_land_rp", True, frame_hw=LAND, rowpad=True),
    _band("x6_port", True, frame_hw=PORT),
    _band("x6_port_rp_win_37_90", True, frame_hw=PORT, rowpad=True, window=WINDOWS[0]),
    _band("x6_port_rp_win_0_33", True, frame_hw=PORT, rowpad=True, window=WINDOWS[1]),
    _band("x6_land_rp_win_90_128", True, frame_hw=LAND, rowpad=True, window=WINDOWS[2]),
]
for _x6 in (False, True):
    HAND += [
        # ---- stemdw_kernel<X6>: 14 bands of 4 output rows per image on at most 512 persistent workgroups ----------------------
        _sd("sd_n1", _x6, N=1),
        _sd("sd_n3", _x6, N=3),
        _sd("sd_n38_532tiles", _x6, N=38),
        _sd("sd_n2_foreign_ns", _x6, N=2, in_ns_extra=40, out_ns_extra=76),
        _sd("sd_n2_gain_lo", _x6, N=2, gain=2.0 ** -20),
        _sd("sd_n2_gain_hi", _x6, N=2, gain=2.0 ** 20),
    ]
HAND += [
    # ---- dwpw_kernel<NB, P, S> in the forms and at the maps Mobile-FaceNet's plans reach it with (three images) -----------------
    _dk("dk_mfn_56_s2", 2, 4, 2, N=3, H=56, W=56, G=128, cout=64),
    _dk("dk_mfn_28_res", 2, 4, 1, N=3, H=28, W=28, G=128, cout=64, res=True),
    _dk("dk_mfn_28_s2", 4, 2, 2, N=3, H=28, W=28, G=256, cout=128),
    _dk("dk_mfn_14_res", 4, 2, 1, N=3, H=14, W=14, G=256, cout=128, res=True),
    _dk("dk_mfn_14_s2", 4, 1, 2, N=3, H=14, W=14, G=512, cout=128),
    _dk("dk_mfn_7_res", 4, 1, 1, N=3, H=7, W=7, G=256, cout=128, res=True),
    _dk("dk_mfn_56_oslope", 4, 4, 1, N=3, H=56, W=56, G=64, cout=128, out_slope=True),
]
# every other instance on 8 x 8 / 6 x 6 / 5 x 5 output maps of six images (M = 384 / 216 / 150: a tile spans images, the last
# one is ragged), the three forms in turn; the stride-2 P = 1 cases read an odd input map
_FORMS = (dict(), dict(res=True), dict(out_slope=True))
for _i, (_nb, _p, _s) in enumerate((nb, p, s) for nb in (1, 2, 3, 4) for p in (4, 2, 1) for s in (1, 2)):
    if not any(c.kernel == f"dwpw_kernel<{_nb}, {_p}, {_s}>" for c in HAND):
        _o = {4: 8, 2: 6, 1: 5}[_p]
        _h = _o * _s - (1 if (_s, _p) == (2, 1) else 0)
        HAND.append(_dk(f"dk_nb{_nb}_p{_p}_s{_s}", _nb, _p, _s, N=6, H=_h, W=_h, G=64, cout=32 * _nb, **_FORMS[_i % 3]))
HAND += [
    # ---- the size-gated DWPW kernels at about 1.5 times their gates ----------------------------------------------------------
    Case("wp_2_1_n126_28", "dwpw", "dwpw_wp_kernel<2, 1, 4>", N=126, H=28, W=28, G=128, cout=64, res=True, gated=True),
    Case("wp_2_2_n126_56", "dwpw", "dwpw_wp_kernel<2, 2, 4>", N=126, H=56, W=56, G=128, cout=64, stride=2, gated=True),
    Case("wp_4_1_n32_56_oslope", "dwpw", "dwpw_wp_kernel<4, 1, 4>", N=32, H=56, W=56, G=64, cout=128, out_slope=True, gated=True),
    Case("pers_4_1_n502_14", "dwpw", "dwpw_persist_kernel<4, 1>", N=502, H=14, W=14, G=256, cout=128, res=True, gated=True),
    Case("pers_2_1_n384_16", "dwpw", "dwpw_persist_kernel<2, 1>", N=384, H=16, W=16, G=320, cout=64, res=True, gated=True),
    Case("pers_2_2_n272_32", "dwpw", "dwpw_persist_kernel<2, 2>", N=272, H=32, W=32, G=320, cout=64, stride=2, gated=True),
    # ---- pws_kernel: M = N H W rows in tiles of 32 -----------------------------------------------------------------------------
    Case("pws64_n126_28", "pws", "pws_kernel<64, 12>", N=126, H=28, W=28, G=64, cout=128, act="prelu", gated=True),     # 3087 tiles
    Case("pws64_n126_28_relu", "pws", "pws_kernel<64, 12>", N=126, H=28, W=28, G=64, cout=128, act="relu", scale=False, gated=True),
    Case("pws128_n1536_8", "pws", "pws_kernel<128, 8>", N=1536, H=8, W=8, G=128, cout=128, act="prelu", gated=True),
    Case("pws128_n1536_8_c512", "pws", "pws_kernel<128, 8>", N=1536, H=8, W=8, G=128, cout=512, gated=True),   # four N tiles
]
# ---- dwblock_kernel: the blocks of tests/test_dwblock_x6_ops.py on the fp32 MFMA; <128, 7, 7, 3>: a last tile of 1 and of 2 images
HAND += [_blk(c, hw, rb, nimg, n, res) for c, hw, rb, nimg, ns in ((128, 14, 14, 1, (1, 3)), (64, 28, 7, 1, (1, 3)),
                                                                   (128, 7, 7, 3, (4, 5)))
         for n in ns for res in (False, True)]

# (gated case, batch just below the gate, the kernel that batch lands on)
GATES = [
    ("st_k5_dense_n32_128", 31, "conv_igemm_kernel"), ("st_k3_dense_n42_112", 41, "conv_igemm_kernel"),
    ("st_k3_pad0_dense_n22_160", 21, "conv_igemm_kernel"), ("pws64_n126_28_relu", 125, "conv_igemm_kernel"),
    ("band_land", 15, "stem_conv_kernel<5, 1, true>"), ("band_port_rp", 15, "stem_conv_kernel<5, 1, true>"),
    ("wp_2_1_n126_28", 83, "dwpw_kernel<2, 4, 1>"), ("wp_2_2_n126_56", 83, "dwpw_kernel<2, 4, 2>"),
    ("wp_4_1_n32_56_oslope", 20, "dwpw_kernel<4, 4, 1>"), ("pers_4_1_n502_14", 334, "dwpw_kernel<4, 2, 1>"),
    ("pers_2_1_n384_16", 255, "dwpw_kernel<2, 4, 1>"), ("pers_2_2_n272_32", 255, "dwpw_kernel<2, 4, 2>"),
    ("pws64_n126_28", 125, "conv_igemm_kernel"), ("pws128_n1536_8", 1535, "conv_igemm_kernel"),
    ("pws128_n1536_8_c512", 1535, "conv_igemm_kernel"),
]

INSTANCES = ({f"stem_conv_kernel<{k}, {nb}, {u}>" for k in (3, 5) for nb in (1, 2) for u in ("false", "true")} |
             {"stem5_u8_band_kernel", "stem5_u8_x6_kernel", "stemdw_kernel<false>", "stemdw_kernel<true>"} |
             {f"dwpw_kernel<{nb}, {p}, {s}>" for nb in (1, 2, 3, 4) for p in (1, 2, 4) for s in (1, 2)} |
             {"dwpw_wp_kernel<2, 1, 4>", "dwpw_wp_kernel<2, 2, 4>", "dwpw_wp_kernel<4, 1, 4>"} |
             {"dwpw_persist_kernel<4, 1>", "dwpw_persist_kernel<2, 1>", "dwpw_persist_kernel<2, 2>"} |
             {"pws_kernel<64, 12>", "pws_kernel<128, 8>"} |
             {"dwblock_kernel<128, 14, 14, 1>", "dwblock_kernel<128, 7, 7, 3>", "dwblock_kernel<64, 28, 7, 1>"})


# The feature keys census() found in the shipped plans when this table was last brought up to date (tests/test_stem_mfn_ops.py
# test_census_is_covered fails, printing the missing keys, as soon as census() finds one that is not here).
CENSUS_KEYS = [
    ('dwblock_kernel<128, 7, 7, 3>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_kernel<2, 4, 1>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_kernel<2, 4, 2>', (3, 2, 1), 2, 0, False, False, False, False, False),
    ('dwpw_kernel<4, 1, 1>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_kernel<4, 1, 2>', (3, 2, 1), 2, 0, False, False, False, False, False),
    ('dwpw_kernel<4, 2, 1>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_kernel<4, 2, 2>', (3, 2, 1), 2, 0, False, False, False, False, False),
    ('dwpw_persist_kernel<4, 1>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_wp_kernel<2, 1, 4>', (3, 1, 1), 2, 2, False, False, False, False, False),
    ('dwpw_wp_kernel<2, 2, 4>', (3, 2, 1), 2, 0, False, False, False, False, False),
    ('pws_kernel<128, 8>', (1, 1, 0), 2, 0, False, False, False, False, False),
    ('pws_kernel<64, 12>', (1, 1, 0), 2, 0, False, False, False, False, False),
    ('stem5_u8_band_kernel', (5, 2, 1), 1, 0, False, True, False, False, False),
    ('stem5_u8_band_kernel', (5, 2, 1), 1, 0, False, True, False, False, True),
    ('stem5_u8_x6_kernel', (5, 2, 1), 1, 0, False, True, False, True, False),
    ('stem5_u8_x6_kernel', (5, 2, 1), 1, 0, False, True, False, True, True),
    ('stem_conv_kernel<3, 1, false>', (3, 2, 0), 1, 0, False, False, True, False, False),
    ('stem_conv_kernel<5, 1, false>', (5, 2, 1), 1, 0, False, True, True, False, False),
    ('stem_conv_kernel<5, 1, true>', (5, 2, 1), 1, 0, False, True, False, False, False),
    ('stemdw_kernel<false>', (3, 2, 1), 2, 0, False, False, True, False, False),
    ('stemdw_kernel<true>', (3, 2, 1), 2, 0, False, False, True, True, False),
]


@functools.lru_cache(maxsize=None)
def hand_keys():
    """{feature key: the first hand-written case whose op has it}."""
    found = {}
    for c in HAND:
        pb, _ = build(c)
        found.setdefault(feature_key(pb.finish()[0][0]), c)
    return found


def case_from_key(key, i=0):
    """The case with exactly this feature key.  The shapes of these kernels are fixed (the band stems, stemdw, dwblock) or bounded
    below by a size gate, so the smallest case of a key is a hand-written one: every key of CENSUS_KEYS names one of HAND
    (feature_key of its op gives `key` back; test_stem_mfn_ops checks that), and a new key has no case until one is written."""
    return hand_keys().get(key)


def cases():
    """Every case: the hand-written ones (which hold every census key's case) and the fp32-image twin of every stem_u8 case that
    runs on an fp32-MFMA kernel."""
    out = list(HAND)
    out += [f32_twin(c) for c in HAND if c.kind == "stem_u8" and not c.x6 and not c.window]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out
