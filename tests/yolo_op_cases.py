"""Case table, float64 references, write footprints and the product census for the fused kernels a YOLOv5-face plan runs
outside the generic fp32 ops, the split-bf16 convs and conv3_kernel:

  FP_OP_YSTEM / FP_OP_YSTEM_U8  -> ystem_kernel<1|2, false|true>          (csrc/ystem.hip)
  FP_OP_YSTEM2                  -> ystem2_x6_kernel                        (csrc/ystem2.hip)
  FP_OP_SHUFDOWN                -> shufdown_x6_kernel<1, 64>               (csrc/shufdown.hip)
  FP_OP_SHUFUNIT                -> shufunit_x6_kernel<64>                  (csrc/shufdown.hip)
  FP_OP_DWPW + FP_OPF_SPLIT3    -> dwpwx6_kernel<4|8, 4, 1|2>              (csrc/dwpwx6.hip; <4, ...> with DWPW_X6_COUT = 64)
  FP_OP_DWPW without the flag   -> dwpw_kernel<2|4, 1|2|4, 1|2>, act2 = SiLU, with and without FP_RES_SHUFFLE2

tests/test_yolo_ops.py runs every case as a one-op plan.  Out of scope here: the Mobile-FaceNet-only DWPW forms (act2 none, output
PReLU, dwpw_persist_kernel, dwpw_wp_kernel), pws_kernel, the fp32 dwblock_kernel and the stems of csrc/stem.hip / stemdw.hip, which
tests/stem_mfn_op_cases.py + tests/test_stem_mfn_ops.py pin the same way; conv3_kernel (test_conv3_lds_image_kernel_vs_torch); the
three head ops (EMBED_HEAD, POOL_LRN, CLS_HEAD: float64 tests in test_facenet.py / test_age_gender.py).

* A Case says how to build the op with PlanBuilder, the instance the launcher must pick and what the views look like.
  build() emits the plan, params() / inputs() draw the seeded data (He-scaled weights, affine scales in [0.5, 1.5], biases
  N(0, 0.2), inputs N(0, 1) with one all-zero interior pixel and one |x| = 30 border pixel), reference() computes the op in
  torch on the CPU in the requested dtype from the op semantics of include/facepath.h and the module definitions of
  modules/yolov5_face -- never from the kernels.
* footprints() are the exact sets of arena floats an op may write, from its views (FP_OP_YSTEM has two).
* tolerances() is the relative term of the fp64 bound per output: generic_op_cases.tolerance's figure per fp_silu stage, times
  the number of chained stages where a CPU check shows that the second stage does not amplify the first one's error.
* census() / CENSUS_KEYS / case_from_key as in generic_op_cases: the feature keys with which the shipped plans reach these
  kernels, each with a small case.
"""
import dataclasses
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import generic_op_cases as G
from generic_op_cases import _raw_buf, hash_name, input_index, kernel_name, product_plans  # noqa: F401  (re-exported)
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import PlanBuilder

FAMILIES = ("ystem_kernel", "ystem2_x6_kernel", "shufdown_x6_kernel", "shufunit_x6_kernel", "dwpwx6_kernel", "dwpw_kernel")
FLAT = ("dwpwx6_kernel", "dwpw_kernel")                       # tiles of 128 flat pixels: a tile may span images
PERSISTENT = ("ystem", "ystem_u8", "ystem2", "shufdown", "shufunit")    # 2-D tiles walked by at most 512 workgroups
TWO_STAGE = ("ystem", "ystem_u8", "ystem2", "shufdown", "shufunit")     # two chained fp_silu stages
ACTS = G.ACTS
RES = G.RES
SILU_TOL = G.tolerance(SimpleNamespace(act="silu"))           # one fp_silu stage (hardware exp2 / rcp, csrc/common.h)
PLAIN_TOL = G.tolerance(SimpleNamespace(act="none"))
IN_C = {"ystem": 4, "ystem_u8": 3, "ystem2": 16, "shufdown": 32, "shufunit": 128}


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                # ystem | ystem_u8 | ystem2 | shufdown | shufunit | dwpw
    kernel: str              # the instance fp_op_kernel_name must report
    N: int
    H: int                   # the input map (ystem_u8: the letterbox canvas)
    W: int
    c1: int = 32             # ystem: stem_1's width, c2: stem_2a's
    c2: int = 16
    cin: int = 3             # ystem: 3 = FP_OPF_IN_C3 (the pad channel is never read), 4 = live fourth-channel weights
    folded: bool = False     # ystem, ystem2: the BatchNorms folded into the convs (scale = None)
    G: int = 0               # dwpw: channels of the depthwise conv
    cout: int = 0            # dwpw: outputs of the 1x1
    stride: int = 1          # dwpw
    act: str = "none"        # dwpw: "none" | "prelu" after the depthwise affine
    act2: str = "silu"       # dwpw: "none" | "silu" on the 1x1 output
    res: str = ""            # dwpw: "" | "after" | "shuffle"
    res_C: int = 0           # dwpw: channels of the residual view (0: cout)
    x6: bool = False         # dwpw: the split form (PlanBuilder.X6 on, DWPW_X6_COUT = cout while the op is emitted)
    in_buf_C: int = 0        # width of the input buffer (0: the view's): the view is channels [in_coff, in_coff + C)
    in_coff: int = 0
    in_ns_extra: int = 0     # floats between the images of the input buffer beyond H * W * in_buf_C
    out_buf_C: int = 0
    out_coff: int = 0
    out_ns_extra: int = 0
    res_buf_C: int = 0       # the second view: ystem's pooled map (written), ystem2's pooled map (read), dwpw's residual (read)
    res_coff: int = 0
    res_ns_extra: int = 0
    partial: int = 0         # > 0: also run(partial) on the plan of capacity N
    seed: str = ""           # the name that seeds parameters and inputs (default: name): twins share them
    frame_hw: tuple = ()     # ystem_u8: size of the u8 frames
    swap_rb: bool = False    # ystem_u8


def out_hw(c):
    if c.kind == "shufunit":
        return c.H, c.W
    if c.kind == "dwpw":
        return (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    return c.H // 2, c.W // 2


def in_C(c):
    return c.G if c.kind == "dwpw" else IN_C[c.kind]


def out_view_C(c):
    """Channels of the output view handed to the builder = fp_op.Cout."""
    return {"ystem": c.c2, "ystem_u8": c.c2, "ystem2": 32, "shufdown": 128, "shufunit": 128, "dwpw": c.cout}[c.kind]


def written_C(c):
    return 2 * c.cout if c.kind == "dwpw" and c.res == "shuffle" else out_view_C(c)


def res_shape(c):
    """(H, W, C) of the second view, or None."""
    oh, ow = out_hw(c)
    if c.kind in ("ystem", "ystem_u8"):
        return oh // 2, ow // 2, c.c1
    if c.kind == "ystem2":
        return oh, ow, 32
    if c.kind == "dwpw" and c.res:
        return oh, ow, c.res_C or c.cout
    return None


def stages(c):
    """Chained fp_silu stages of the `out` view."""
    if c.kind == "dwpw":
        return 1 if c.act2 == "silu" else 0
    return 2


# ---------------------------------------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(c):
    """Seeded parameters of a case in the shapes of the torch modules: conv weights [O, I, KH, KW], (scale or None, bias) of
    every eval-mode BatchNorm, PReLU slopes."""
    rng = np.random.default_rng(hash_name(c.seed or c.name) % (2 ** 31))

    def w(o, i, k):
        return rng.normal(0, (2.0 / (i * k * k)) ** 0.5, (o, i, k, k)).astype(np.float32)

    def dw(ch):
        return rng.normal(0, (2.0 / 9) ** 0.5, (ch, 1, 3, 3)).astype(np.float32)

    def aff(n, folded=False):
        s, b = rng.uniform(0.5, 1.5, n).astype(np.float32), rng.normal(0, 0.2, n).astype(np.float32)
        return (None if folded else s), b

    if c.kind in ("ystem", "ystem_u8"):
        return dict(w1=w(c.c1, 3 if c.kind == "ystem_u8" else c.cin, 3), aff1=aff(c.c1, c.folded), w2=w(c.c2, c.c1, 1),
                    aff2=aff(c.c2, c.folded))
    if c.kind == "ystem2":
        return dict(w2b=w(32, 16, 3), aff2b=aff(32, c.folded), w3=w(32, 64, 1), aff3=aff(32, c.folded))
    if c.kind == "shufdown":
        return dict(b1_dw=dw(32), b1_dw_aff=aff(32), b1_pw=w(64, 32, 1), b1_pw_aff=aff(64), pw1=w(64, 32, 1), pw1_aff=aff(64),
                    dw2=dw(64), dw2_aff=aff(64), pw2=w(64, 64, 1), pw2_aff=aff(64))
    if c.kind == "shufunit":
        return dict(pw1=w(64, 64, 1), pw1_aff=aff(64), dw2=dw(64), dw2_aff=aff(64), pw2=w(64, 64, 1), pw2_aff=aff(64))
    if c.kind == "dwpw":
        p = dict(dw_w=dw(c.G), dw_aff=aff(c.G), pw_w=w(c.cout, c.G, 1), pw_aff=aff(c.cout))
        if c.act == "prelu":
            p["dw_slope"] = rng.uniform(0.1, 0.3, c.G).astype(np.float32)
        return p
    raise ValueError(c.kind)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """Seeded inputs of a case, read-only: {"x": (N, H, W, C) float32 N(0, 1) with one all-zero pixel in the interior of image
    0 and one pixel of magnitude 30 (alternating signs) in the bottom-left corner of the last image, "res": the second view
    where the op READS it}; ystem_u8: {"frames": (N, fh, fw, 3) uint8}."""
    rng = np.random.default_rng((hash_name(c.seed or c.name) + 1) % (2 ** 31))
    if c.kind == "ystem_u8":
        d = {"frames": rng.integers(0, 256, (c.N, *c.frame_hw, 3), dtype=np.uint8)}
    else:
        ch = in_C(c)
        x = rng.normal(0, 1, (c.N, c.H, c.W, ch)).astype(np.float32)
        big, zero = (c.N - 1, c.H - 1, 0), (0, c.H // 2, c.W // 2)
        if zero != big:
            x[zero] = 0.0
        x[big] = 30.0 * (1 - 2 * (np.arange(ch) % 2))
        d = {"x": x}
        rs = res_shape(c)
        if rs is not None and c.kind != "ystem":
            d["res"] = rng.normal(0, 1, (c.N, *rs)).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------------
def build(c, N=None):
    """Emit the one-op plan of a case -> (builder, {"x": Buf or None, "out": Buf, "res": Buf or None})."""
    pb = PlanBuilder(N or c.N)
    pb.X6 = c.kind != "dwpw" or c.x6
    oh, ow = out_hw(c)
    xb = None if c.kind == "ystem_u8" else _raw_buf(pb, c.H, c.W, c.in_buf_C or in_C(c), c.in_ns_extra)
    rs = res_shape(c)
    rb = _raw_buf(pb, rs[0], rs[1], c.res_buf_C or rs[2], c.res_ns_extra) if rs is not None else None
    ob = _raw_buf(pb, oh, ow, c.out_buf_C or written_C(c), c.out_ns_extra)
    xv = xb.view(c.in_coff, in_C(c)) if xb is not None else None
    ov = ob.view(c.out_coff, out_view_C(c))
    rv = rb.view(c.res_coff, rs[2]) if rb is not None else None
    p = params(c)
    if c.kind in ("ystem", "ystem_u8"):
        u8 = (c.H, c.W, c.frame_hw[0], c.frame_hw[1], 0) if c.kind == "ystem_u8" else None
        got = pb.ystem(xv, p["w1"], *p["aff1"], p["w2"], *p["aff2"], ov, rv, u8=u8)
    elif c.kind == "ystem2":
        got = pb.ystem2(xv, rv, p["w2b"], p["aff2b"], p["w3"], p["aff3"], ov)
    elif c.kind == "shufdown":
        got = pb.shufdown(xv, p["b1_dw"], p["b1_dw_aff"], p["b1_pw"], p["b1_pw_aff"], p["pw1"], p["pw1_aff"], p["dw2"],
                          p["dw2_aff"], p["pw2"], p["pw2_aff"], ov)
    elif c.kind == "shufunit":
        got = pb.shufunit(xv, p["pw1"], p["pw1_aff"], p["dw2"], p["dw2_aff"], p["pw2"], p["pw2_aff"], ov)
    elif c.kind == "dwpw":
        saved = PlanBuilder.DWPW_X6_COUT
        if c.x6:
            PlanBuilder.DWPW_X6_COUT = c.cout
        try:
            got = pb.dwpw(xv, p["dw_w"], *p["dw_aff"], p.get("dw_slope"), p["pw_w"], *p["pw_aff"], ov, c.stride, res=rv,
                          out_act=ACTS[c.act2], shuffle=c.res == "shuffle")
        finally:
            PlanBuilder.DWPW_X6_COUT = saved
    else:
        raise ValueError(c.kind)
    assert got is not None and len(pb.ops) == 1, c.name
    return pb, {"x": xb, "out": ob, "res": rb}


def f32_twin(c):
    """The FP_OP_YSTEM case (FP_OPF_IN_C3, fp32 canvas) with the parameters and views of a ystem_u8 case."""
    assert c.kind == "ystem_u8"
    return dataclasses.replace(c, name=c.name + "_f32", kind="ystem", kernel=c.kernel.replace("true", "false"), cin=3,
                               seed=c.seed or c.name, frame_hw=(), swap_rb=False)


# ---------------------------------------------------------------------------------------------------------------------------
# references (torch on the CPU, dtype dt)
# ---------------------------------------------------------------------------------------------------------------------------
def live_tap(c):
    """A border tap (ky, kx) of the case's 3x3 windows that meets at least one pixel of the input map, or None (a 1 x 1 map
    at stride 1 has only its centre)."""
    s = 1 if c.kind == "shufunit" else (c.stride if c.kind == "dwpw" else 2)
    oh, ow = out_hw(c)

    def live(k, o, n):
        return any(0 <= i * s - 1 + k < n for i in range(o))
    return next(((ky, kx) for ky, kx in ((2, 2), (1, 2), (2, 1), (0, 0), (1, 0), (0, 1))
                 if live(ky, oh, c.H) and live(kx, ow, c.W)), None)


def _t(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


def _nchw(a, dt):
    return _t(a, dt).permute(0, 3, 1, 2)


def _aff(v, sb, dt):
    s, b = sb
    if s is not None:
        v = v * _t(s, dt).view(1, -1, 1, 1)
    return v + _t(b, dt).view(1, -1, 1, 1)


def _silu(v):
    return v * torch.sigmoid(v)


def _pw(v, w, dt):
    return F.conv2d(v, _t(w, dt))


def reference(c, data, dt, mut=None, perturb=None):
    """The op of case c on data (inputs(); ystem: {"x": the 4-float-pixel image}) in dtype dt -> {"out": (N, OH, OW, written
    channels), "pool": ystem's pooled map} as numpy.  mut: a mutation of the op (mutants()); perturb: a function applied to
    the first SiLU stage's output (tolerances())."""
    p = params(c)
    state = {"stage": 0}

    def conv3(v, w, stride, groups=1):
        """3x3 pad 1; stage i of the op's 3x3 convs carries the ("tap", i, ky, kx) and ("pad", i) mutations."""
        i = state["stage"]
        state["stage"] += 1
        w = _t(w, dt)
        if mut is not None and mut[:2] == ("tap", i):
            w = w.clone()
            w[:, :, mut[2], mut[3]] = 0
        if mut == ("pad", i):      # pad_t = pad_l = 0: the window starts one pixel later, the map ends in two pad lines
            return F.conv2d(F.pad(v, (0, 2, 0, 2)), w, stride=stride, groups=groups)
        return F.conv2d(v, w, stride=stride, padding=1, groups=groups)

    def first(v):
        return v if perturb is None else perturb(v)

    def interleave(even, odd):
        if mut == ("swap",):
            even, odd = odd, even
        return torch.stack([even, odd], dim=2).reshape(even.shape[0], 2 * even.shape[1], *even.shape[2:])

    x = _nchw(data["x"], dt)
    with torch.no_grad():
        if c.kind in ("ystem", "ystem_u8"):
            nin = p["w1"].shape[1]
            s1 = first(_silu(_aff(conv3(x[:, :nin], p["w1"], 2), p["aff1"], dt)))
            out = {"out": _silu(_aff(_pw(s1, p["w2"], dt), p["aff2"], dt))}
            if mut == ("pool",):   # the 2x2 window shifted by one pixel
                out["pool"] = F.max_pool2d(F.pad(s1, (0, 1, 0, 1), value=float("-inf"))[:, :, 1:, 1:], 2)
            else:
                out["pool"] = F.max_pool2d(s1, 2)
        elif c.kind == "ystem2":
            b = first(_silu(_aff(conv3(x, p["w2b"], 2), p["aff2b"], dt)))
            out = {"out": _silu(_aff(_pw(torch.cat([b, _nchw(data["res"], dt)], 1), p["w3"], dt), p["aff3"], dt))}
        elif c.kind == "shufdown":
            b1 = _silu(_aff(_pw(_aff(conv3(x, p["b1_dw"], 2, 32), p["b1_dw_aff"], dt), p["b1_pw"], dt), p["b1_pw_aff"], dt))
            t = first(_silu(_aff(_pw(x, p["pw1"], dt), p["pw1_aff"], dt)))
            b2 = _silu(_aff(_pw(_aff(conv3(t, p["dw2"], 2, 64), p["dw2_aff"], dt), p["pw2"], dt), p["pw2_aff"], dt))
            out = {"out": interleave(b1, b2)}
        elif c.kind == "shufunit":
            x1, x2 = x[:, :64], x[:, 64:]
            if mut == ("x1x2",):
                x1, x2 = x2, x1
            t = first(_silu(_aff(_pw(x2, p["pw1"], dt), p["pw1_aff"], dt)))
            b2 = _silu(_aff(_pw(_aff(conv3(t, p["dw2"], 1, 64), p["dw2_aff"], dt), p["pw2"], dt), p["pw2_aff"], dt))
            out = {"out": interleave(x1, b2)}
        elif c.kind == "dwpw":
            v = _aff(conv3(x, p["dw_w"], c.stride, c.G), p["dw_aff"], dt)
            if c.act == "prelu":
                v = torch.where(v > 0, v, v * _t(p["dw_slope"], dt).view(1, -1, 1, 1))
            y = _aff(_pw(v, p["pw_w"], dt), p["pw_aff"], dt)
            if c.act2 == "silu":
                y = _silu(y)
            if c.res:
                r = _nchw(data["res"], dt)
                rc = min(r.shape[1], c.cout)                       # fp_op.res_C: channels beyond it add 0 / are not read
                r = F.pad(r[:, :rc], (0, 0, 0, 0, 0, c.cout - rc))
                y = y + r if c.res == "after" else interleave(r, y)
            out = {"out": y}
        else:
            raise ValueError(c.kind)
    return {k: np.ascontiguousarray(v.permute(0, 2, 3, 1).numpy()) for k, v in out.items()}


def mutants(c):
    """(label, mut) of the mutations of reference() that a wrong kernel of this kind would amount to: one border tap of each
    3x3 stage zeroed, each stage's padding off by one, the shuffle interleave swapped, the pooling window shifted by one,
    x1 / x2 exchanged."""
    n3 = 2 if c.kind == "shufdown" else 1
    tap = live_tap(c)
    out = []
    for i in range(n3):
        if tap is not None:
            out.append((f"stage {i}: tap {tap} zeroed", ("tap", i, *tap)))
        out.append((f"stage {i}: padding off by one", ("pad", i)))
    if c.kind in ("shufdown", "shufunit") or (c.kind == "dwpw" and c.res == "shuffle"):
        out.append(("interleave swapped", ("swap",)))
    if c.kind in ("ystem", "ystem_u8"):
        out.append(("pooling window shifted by one", ("pool",)))
    if c.kind == "shufunit":
        out.append(("x1 / x2 exchanged", ("x1x2",)))
    return out


@functools.lru_cache(maxsize=None)
def references(c):
    """(float64 reference, float32 reference) of a case on its own inputs, each {"out": ..., "pool": ...}, read-only, computed
    once and shared."""
    assert c.kind != "ystem_u8"
    data = inputs(c)
    r64, r32 = reference(c, data, torch.float64), reference(c, data, torch.float32)
    for r in (r64, r32):
        for v in r.values():
            v.setflags(write=False)
    return r64, r32


@functools.lru_cache(maxsize=None)
def propagation(c):
    """How far the `out` view of a two-stage case moves, relative to its scale, when every value of the float64 reference's
    first SiLU stage is perturbed by a seeded relative error of up to SILU_TOL.  The error is relative to each value, as
    fp_silu's is (csrc/common.h: v_exp_f32 and v_rcp_f32 are within 1 ulp each, so the result is off by a fraction of itself):
    the |x| = 30 pixel puts the stage's maximum at 20 .. 150 against a median of 0.26, and an error of SILU_TOL of that
    maximum on every element -- one the hardware cannot make -- would alone move the outputs by 4e-6 .. 4e-5 of scale."""
    assert c.kind in TWO_STAGE and c.kind != "ystem_u8"
    rng = torch.Generator().manual_seed(hash_name(c.name) % (2 ** 31))

    def perturb(v):
        return v * (1 + SILU_TOL * (2 * torch.rand(v.shape, generator=rng, dtype=v.dtype) - 1))
    want = references(c)[0]["out"]
    moved = reference(c, inputs(c), torch.float64, perturb=perturb)["out"]
    return float(np.abs(moved - want).max() / np.abs(want).max())


def tolerances(c):
    """The relative term of the fp64 bound per output.  One fp_silu stage: SILU_TOL (generic_op_cases.tolerance); none:
    PLAIN_TOL.  Two chained stages: twice SILU_TOL if the second does not amplify the first one's error on this case's data
    (propagation() <= SILU_TOL), else what the first stage's error propagates to plus the last stage's SILU_TOL.  ystem's pooled
    map is a maximum of first-stage values: one stage."""
    if c.kind == "dwpw":
        return {"out": SILU_TOL if c.act2 == "silu" else PLAIN_TOL}
    prop = propagation(c)
    tol = {"out": 2 * SILU_TOL if prop <= SILU_TOL else prop + SILU_TOL}
    if c.kind == "ystem":
        tol["pool"] = SILU_TOL
    return tol


def bounds(c):
    """{output: (bound, scale)}: 2 * max|ref32 - ref64| + tol * max|ref64|."""
    r64, r32 = references(c)
    tol = tolerances(c)
    return {k: (2.0 * np.abs(r32[k] - r64[k]).max() + tol[k] * np.abs(r64[k]).max(), np.abs(r64[k]).max()) for k in r64}


# ---------------------------------------------------------------------------------------------------------------------------
# footprints
# ---------------------------------------------------------------------------------------------------------------------------
def view_index(off, ns, ld, n, H, W, C):
    ni = np.arange(n, dtype=np.int64).reshape(-1, 1, 1, 1)
    pi = np.arange(H * W, dtype=np.int64).reshape(1, H, W, 1)
    ci = np.arange(C, dtype=np.int64).reshape(1, 1, 1, -1)
    return off + ni * ns + pi * ld + ci


def footprints(op, n_run=None):
    """{"out": arena indices [n, OH, OW, Cw], "pool": ...} of every float the op may write when it runs on n_run images
    (default op.N), from its views.  Cw = Cout dense channels (2 * Cout under FP_RES_SHUFFLE2: both interleaved halves);
    FP_OP_YSTEM / FP_OP_YSTEM_U8 also write maxpool2x2(stem_1): res_C channels on OH/2 x OW/2 of the res view."""
    n = op.N if n_run is None else n_run
    cw = 2 * op.Cout if op.kind == L.OP_DWPW and op.res_mode == L.RES_SHUFFLE2 else op.Cout
    fp = {"out": view_index(op.out_off, op.out_ns, op.out_ld, n, op.OH, op.OW, cw)}
    if op.kind in (L.OP_YSTEM, L.OP_YSTEM_U8):
        fp["pool"] = view_index(op.res_off, op.res_ns, op.res_ld, n, op.OH // 2, op.OW // 2, op.res_C)
    return fp


# ---------------------------------------------------------------------------------------------------------------------------
# census of the shipped plans
# ---------------------------------------------------------------------------------------------------------------------------
def feature_key(op, name=None):
    """The feature key of an op that lands on one of FAMILIES (dwpw_kernel: in its YOLOv5-face forms only, act2 = SiLU), or None:
    (instance, stride, act, act2, res_mode, scale present, FP_OPF_IN_C3, sliced in, out, res, foreign image stride in, out, res,
    OHW < 128 on the flat-tile kernels)."""
    name = name or kernel_name(op)
    fam = name.split("<")[0]
    if fam not in FAMILIES or (fam == "dwpw_kernel" and op.act2 != L.ACT_SILU):
        return None
    u8 = op.kind == L.OP_YSTEM_U8
    ohw = op.OH * op.OW
    cw = 2 * op.Cout if op.kind == L.OP_DWPW and op.res_mode == L.RES_SHUFFLE2 else op.Cout
    ystem = op.kind in (L.OP_YSTEM, L.OP_YSTEM_U8)
    has_res = ystem or op.kind == L.OP_YSTEM2 or op.res_mode != L.RES_NONE
    rhw = (op.OH // 2) * (op.OW // 2) if ystem else ohw
    return (name, op.stride, op.act, op.act2, op.res_mode, op.scale_off >= 0, bool(op.flags & L.OPF_IN_C3),
            (not u8) and op.in_ld != op.Cin, op.out_ld != cw, has_res and op.res_ld != op.res_C,
            (not u8) and op.in_ns != op.H * op.W * op.in_ld, op.out_ns != ohw * op.out_ld,
            has_res and op.res_ns != rhw * op.res_ld, fam in FLAT and ohw < 128)


@functools.lru_cache(maxsize=None)
def census():
    """{feature key: label of the first plan that reaches one of FAMILIES with it} over product_plans()."""
    found = {}
    for label, pb in product_plans():
        for op in pb.finish()[0]:
            key = feature_key(op)
            if key is not None:
                found.setdefault(key, label)
    return found


_ACT_NAMES = {v: k for k, v in ACTS.items()}
_RES_NAMES = {v: k for k, v in RES.items()}


def case_from_key(key, i):
    """A small case with exactly this feature key (feature_key of its op gives `key` back; test_yolo_ops checks that)."""
    (name, stride, act, act2, res_mode, scale, c3, sl_in, sl_out, sl_res, fns_in, fns_out, fns_res, small) = key
    fam = name.split("<")[0]
    targs = [a.strip() for a in name.split("<")[1].rstrip(">").split(",")] if "<" in name else []
    tag = f"census{i:02d}"
    kw = dict(N=3, partial=1 if i % 2 == 0 else 0, in_ns_extra=8 if fns_in else 0, out_ns_extra=12 if fns_out else 0,
              res_ns_extra=20 if fns_res else 0)
    if fam == "ystem_kernel":
        c2 = 16 if targs[0] == "1" else 32
        kw.update(H=20, W=72, c1=32, c2=c2, cin=3 if c3 else 4, folded=not scale, out_buf_C=c2 + 8 if sl_out else 0,
                  out_coff=4 if sl_out else 0, res_buf_C=64 if sl_res else 0, res_coff=32 if sl_res else 0)
        if targs[1] == "true":
            return Case(f"{tag}_ystem_u8", "ystem_u8", name, frame_hw=(30, 50), swap_rb=True, **kw)
        return Case(f"{tag}_ystem", "ystem", name, **kw)
    if fam == "ystem2_x6_kernel":
        return Case(f"{tag}_ystem2", "ystem2", name, H=10, W=36, in_buf_C=24 if sl_in else 0, in_coff=4 if sl_in else 0,
                    out_buf_C=48 if sl_out else 0, out_coff=8 if sl_out else 0, res_buf_C=64 if sl_res else 0,
                    res_coff=32 if sl_res else 0, **kw)
    if fam == "shufdown_x6_kernel":
        return Case(f"{tag}_shufdown", "shufdown", name, H=10, W=36, in_buf_C=40 if sl_in else 0, in_coff=4 if sl_in else 0,
                    out_buf_C=160 if sl_out else 0, out_coff=16 if sl_out else 0, **kw)
    if fam == "shufunit_x6_kernel":
        return Case(f"{tag}_shufunit", "shufunit", name, H=9, W=18, in_buf_C=256 if sl_in else 0, in_coff=64 if sl_in else 0,
                    out_buf_C=256 if sl_out else 0, out_coff=128 if sl_out else 0, **kw)
    if fam in FLAT:
        x6 = fam == "dwpwx6_kernel"
        cout = (16 if x6 else 32) * int(targs[0])
        ow = {4: 8, 2: 6, 1: 5}[int(targs[1])]
        oh = 4 if small else 128 // ow + 1
        res = _RES_NAMES[res_mode]
        wc = 2 * cout if res == "shuffle" else cout
        return Case(f"{tag}_dwpw", "dwpw", name, H=oh * stride, W=ow * stride, G=64, cout=cout, stride=stride,
                    act=_ACT_NAMES[act], act2=_ACT_NAMES[act2], res=res, x6=x6, in_buf_C=128 if sl_in else 0,
                    in_coff=64 if sl_in else 0, out_buf_C=wc + 64 if sl_out else 0, out_coff=64 if sl_out else 0,
                    res_buf_C=cout + 64 if sl_res else 0, **kw)
    raise ValueError(key)


# The feature keys census() found in the shipped plans when this table was last brought up to date (tests/test_yolo_ops.py
# test_census_is_covered fails, printing the missing keys, as soon as census() finds one that is not here).
CENSUS_KEYS = [
    ('dwpw_kernel<2, 4, 1>', 1, 0, 3, 4, False, False, False, False, True, False, False, False, False),
    ('dwpw_kernel<2, 4, 1>', 1, 0, 3, 4, False, False, False, True, True, False, False, False, False),
    ('dwpw_kernel<2, 4, 2>', 2, 0, 3, 0, False, False, True, False, False, False, False, False, False),
    ('dwpw_kernel<2, 4, 2>', 2, 0, 3, 4, False, False, False, False, False, False, False, False, False),
    ('dwpw_kernel<4, 4, 1>', 1, 0, 3, 4, False, False, False, False, True, False, False, False, False),
    ('dwpw_kernel<4, 4, 1>', 1, 0, 3, 4, False, False, False, True, True, False, False, False, False),
    ('dwpw_kernel<4, 4, 2>', 2, 0, 3, 0, False, False, True, False, False, False, False, False, False),
    ('dwpw_kernel<4, 4, 2>', 2, 0, 3, 4, False, False, False, False, False, False, False, False, False),
    ('dwpwx6_kernel<8, 4, 1>', 1, 0, 3, 4, False, False, False, False, True, False, False, False, False),
    ('dwpwx6_kernel<8, 4, 1>', 1, 0, 3, 4, False, False, False, True, True, False, False, False, False),
    ('dwpwx6_kernel<8, 4, 2>', 2, 0, 3, 0, False, False, True, False, False, False, False, False, False),
    ('dwpwx6_kernel<8, 4, 2>', 2, 0, 3, 4, False, False, False, False, False, False, False, False, False),
    ('shufdown_x6_kernel<1, 64>', 2, 3, 3, 0, False, False, False, False, False, False, False, False, False),
    ('shufunit_x6_kernel<64>', 1, 3, 3, 0, False, False, False, False, False, False, False, False, False),
    ('shufunit_x6_kernel<64>', 1, 3, 3, 0, False, False, False, True, False, False, False, False, False),
    ('ystem2_x6_kernel', 2, 3, 3, 0, False, False, False, False, True, False, False, False, False),
    ('ystem_kernel<1, false>', 2, 3, 0, 0, True, True, False, False, True, False, False, False, False),
    ('ystem_kernel<1, true>', 2, 3, 0, 0, True, False, False, False, True, False, False, False, False),
]


# ---------------------------------------------------------------------------------------------------------------------------
# hand-written cases: the smallest shapes at which each kernel can still go wrong
# ---------------------------------------------------------------------------------------------------------------------------
def _ys(name, nb2, **kw):
    return Case(name, "ystem", f"ystem_kernel<{nb2}, false>", **kw)


def _u8(name, nb2, **kw):
    return Case(name, "ystem_u8", f"ystem_kernel<{nb2}, true>", H=40, W=72, **kw)


def _x6(name, nt, **kw):
    return Case(name, "dwpw", f"dwpwx6_kernel<{nt}, 4, {kw.get('stride', 1)}>", cout=16 * nt, x6=True, **kw)


def _dk(name, nb, p, **kw):
    return Case(name, "dwpw", f"dwpw_kernel<{nb}, {p}, {kw.get('stride', 1)}>", cout=32 * nb, **kw)


# Relative term of the fp64 bound (tolerances(); test_tolerance_is_not_vacuous prints propagation() for every case): on the
# two-stage kinds a first-stage error of 2e-6 moves `out` by 3.6e-7 (sd_18x66) .. 1.7e-6 (sd_550tiles) of scale, so tol = 4e-6,
# except where the data amplify it: ys_nb2_c24_rgba 2.13e-6, ys_16x64_c24 2.32e-6, ys_u8_nb2_c24_f32 2.38e-6 and
# ys_u8_exact_c16_f32 4.58e-6 (its `out` scale is 4.0 against a stem_1 scale of 33), where tol = that figure + 2e-6.  ystem's
# pooled map and the SiLU forms of dwpw: 2e-6; dwpw without SiLU: 2e-7.  The largest bound of all is 7.6e-6 of scale.
HAND = [
    # ---- ystem_kernel<NB2, false>: a tile is 8 x 32 stem_1 pixels = 16 x 64 input pixels -------------------------------------
    _ys("ys_4x4", 1, N=3, H=4, W=4, partial=1),                                    # one tile, ragged both ways, pooled map 1 x 1
    _ys("ys_16x64_c24", 1, N=2, H=16, W=64, c1=24, c2=12, folded=True, res_buf_C=48, res_coff=24),     # exactly one tile
    _ys("ys_20x72_c16_rgba", 1, N=5, H=20, W=72, c1=16, c2=8, cin=4, res_buf_C=32, res_coff=16,        # 2 x 2 tiles, both seams,
        partial=3),                                                                # both ragged edges; 20 tiles: G % 8 = 4
    _ys("ys_13tiles_rgba", 1, N=1, H=16, W=832, cin=4, res_buf_C=64, res_coff=32),     # 13 workgroups: 5 XCDs get 2, 3 get 1
    _ys("ys_520tiles", 1, N=5, H=208, W=512, res_buf_C=64, res_coff=32, partial=2),    # 512 workgroups, 8 walk a second tile
    _ys("ys_nb2_c24_rgba", 2, N=2, H=20, W=72, c2=24, cin=4),
    _ys("ys_nb2_c32", 2, N=3, H=12, W=68, c2=32, folded=True, res_buf_C=64, res_coff=32, partial=2),
    _ys("ys_views", 1, N=3, H=20, W=72, in_ns_extra=8, out_buf_C=24, out_coff=4, out_ns_extra=20, res_buf_C=72, res_coff=36,
        res_ns_extra=12, partial=1),
    # ---- ystem_kernel<NB2, true>: a 40 x 72 canvas (3 x 2 tiles) from frames that pad each side in turn ---------------------------
    _u8("ys_u8_wide", 1, N=3, frame_hw=(30, 100), res_buf_C=64, res_coff=32, partial=1),          # pads above and below
    _u8("ys_u8_tall_c24", 1, N=2, frame_hw=(90, 50), c1=24, c2=12, res_buf_C=48, res_coff=24),    # pads left and right
    _u8("ys_u8_exact_c16", 1, N=2, frame_hw=(80, 144), c1=16, c2=8, folded=True, res_buf_C=32, res_coff=16),
    _u8("ys_u8_swap_nb2_c32", 2, N=3, frame_hw=(45, 64), c2=32, swap_rb=True, res_buf_C=64, res_coff=32, out_ns_extra=16,
        res_ns_extra=8, partial=2),
    _u8("ys_u8_nb2_c24", 2, N=2, frame_hw=(30, 100), c2=24, folded=True),
    # ---- ystem2_x6_kernel: a tile is 4 x 16 outputs ------------------------------------------------------------------------
    Case("y2_2x2", "ystem2", "ystem2_x6_kernel", N=3, H=2, W=2, partial=1),
    Case("y2_8x32", "ystem2", "ystem2_x6_kernel", N=2, H=8, W=32, folded=True, res_buf_C=64, res_coff=32),
    Case("y2_18x66", "ystem2", "ystem2_x6_kernel", N=3, H=18, W=66, res_buf_C=64, res_coff=32, partial=2),
    Case("y2_550tiles", "ystem2", "ystem2_x6_kernel", N=5, H=88, W=320, res_buf_C=64, res_coff=32, partial=2),
    Case("y2_views", "ystem2", "ystem2_x6_kernel", N=3, H=18, W=66, folded=True, in_buf_C=24, in_coff=4, in_ns_extra=8,
         res_buf_C=72, res_coff=36, res_ns_extra=12, out_buf_C=48, out_coff=8, out_ns_extra=20, partial=1),
    # ---- shufdown_x6_kernel<1, 64>: a tile is 4 x 16 outputs ------------------------------------------------------------------
    Case("sd_2x2", "shufdown", "shufdown_x6_kernel<1, 64>", N=3, H=2, W=2, partial=1),
    Case("sd_8x32", "shufdown", "shufdown_x6_kernel<1, 64>", N=2, H=8, W=32),
    Case("sd_18x66", "shufdown", "shufdown_x6_kernel<1, 64>", N=3, H=18, W=66, partial=2),
    Case("sd_550tiles", "shufdown", "shufdown_x6_kernel<1, 64>", N=5, H=88, W=320, partial=2),
    Case("sd_views", "shufdown", "shufdown_x6_kernel<1, 64>", N=3, H=18, W=66, in_buf_C=40, in_coff=4, in_ns_extra=8,
         out_buf_C=160, out_coff=16, out_ns_extra=20, partial=1),
    # ---- shufunit_x6_kernel<64>: a tile is 8 x 16 pixels ------------------------------------------------------------------------
    Case("su_1x1", "shufunit", "shufunit_x6_kernel<64>", N=3, H=1, W=1, partial=1),
    Case("su_8x16", "shufunit", "shufunit_x6_kernel<64>", N=2, H=8, W=16),
    Case("su_9x33_out192", "shufunit", "shufunit_x6_kernel<64>", N=3, H=9, W=33, out_buf_C=192, out_coff=64, partial=2),
    Case("su_522tiles", "shufunit", "shufunit_x6_kernel<64>", N=9, H=225, W=17, partial=4),      # 29 x 2 tiles per image
    Case("su_views_out256", "shufunit", "shufunit_x6_kernel<64>", N=3, H=9, W=33, in_buf_C=256, in_coff=64, in_ns_extra=8,
         out_buf_C=256, out_coff=128, out_ns_extra=20, partial=1),
    # ---- dwpwx6_kernel<NT, 4, S>: 128 flat pixels per tile -----------------------------------------------------------------------
    _x6("dx_1x4", 8, N=1, H=1, W=4, G=64),                                        # M = 4, the minimum: 31 clamped tail groups
    _x6("dx_n9_4x4_shuffle", 8, N=9, H=4, W=4, G=128, res="shuffle", res_C=192, res_buf_C=256, out_buf_C=384, out_coff=128,
        partial=4),                                                               # M = 144: tile 0 holds 8 images, tile 1 16 pixels
    _x6("dx_m256_prelu_after", 4, N=2, H=8, W=16, G=192, act="prelu", act2="none", res="after", res_C=32),      # M = 2 * 128
    _x6("dx_s2_16_shuffle_views", 8, N=3, H=16, W=16, G=128, stride=2, res="shuffle", in_buf_C=256, in_coff=128, res_buf_C=256,
        res_coff=64, out_buf_C=384, out_coff=64, partial=1),
    _x6("dx_s2_15_c64", 4, N=3, H=15, W=15, G=64, stride=2, in_ns_extra=12, partial=2),                       # odd input map
    _x6("dx_s1_c64_shuffle", 4, N=4, H=5, W=8, G=64, res="shuffle", res_buf_C=128, out_buf_C=256, out_coff=64, partial=3),
    _x6("dx_s2_c64_prelu_after", 4, N=2, H=10, W=16, G=128, stride=2, act="prelu", res="after", res_C=48, res_buf_C=128,
        res_coff=64, in_buf_C=256),
    _x6("dx_s1_g256_plain", 8, N=2, H=6, W=12, G=256, act2="none"),
    _x6("dx_s2_g256_prelu", 8, N=2, H=12, W=24, G=256, stride=2, act="prelu", in_ns_extra=8),
    _x6("dx_twin", 8, N=3, H=6, W=8, G=128, res="shuffle", res_buf_C=128, out_buf_C=256, seed="dwpw_twin", partial=2),
    # ---- dwpw_kernel<NB, P, S> in the forms YOLOv5-face produces (act2 = SiLU): where the op lands when OW % 4 != 0 or X6 is off ---
    _dk("dk_twin", 4, 4, N=3, H=6, W=8, G=128, res="shuffle", res_buf_C=128, out_buf_C=256, seed="dwpw_twin", partial=2),
    _dk("dk_nb2_p4_s1_shuffle", 2, 4, N=3, H=5, W=8, G=64, res="shuffle", res_buf_C=128, out_buf_C=192, out_coff=64, partial=1),
    _dk("dk_nb2_p2_s1", 2, 2, N=3, H=5, W=6, G=64, in_ns_extra=8),
    _dk("dk_nb2_p1_s1_shuffle", 2, 1, N=9, H=4, W=5, G=128, res="shuffle", res_C=128, res_buf_C=256, res_coff=64, out_buf_C=256,
        out_coff=128, partial=4),                                                  # M = 180: a tile spans seven images
    _dk("dk_nb2_p4_s2", 2, 4, N=2, H=8, W=16, G=64, stride=2, partial=1),
    _dk("dk_nb2_p2_s2_shuffle", 2, 2, N=3, H=8, W=12, G=64, stride=2, res="shuffle", in_buf_C=256, in_coff=64),
    _dk("dk_nb2_p1_s2", 2, 1, N=3, H=9, W=9, G=64, stride=2, in_ns_extra=12, partial=2),          # odd input map
    _dk("dk_nb4_p4_s1", 4, 4, N=2, H=9, W=16, G=64),                                              # M = 288: two full tiles + 32
    _dk("dk_nb4_p2_s1_shuffle", 4, 2, N=3, H=5, W=6, G=128, res="shuffle", in_buf_C=256, res_buf_C=256, out_buf_C=384, partial=1),
    _dk("dk_nb4_p1_s1", 4, 1, N=3, H=5, W=5, G=64, out_buf_C=192, out_coff=64),
    _dk("dk_nb4_p4_s2_shuffle", 4, 4, N=3, H=8, W=16, G=128, stride=2, res="shuffle", res_C=192, res_buf_C=256, out_buf_C=256,
        partial=2),
    _dk("dk_nb4_p2_s2", 4, 2, N=2, H=8, W=12, G=128, stride=2),
    _dk("dk_nb4_p1_s2_shuffle", 4, 1, N=3, H=10, W=10, G=128, stride=2, res="shuffle", partial=1),
]

INSTANCES = ({f"ystem_kernel<{nb}, {u}>" for nb in (1, 2) for u in ("false", "true")} |
             {"ystem2_x6_kernel", "shufdown_x6_kernel<1, 64>", "shufunit_x6_kernel<64>"} |
             {f"dwpwx6_kernel<{nt}, 4, {s}>" for nt in (4, 8) for s in (1, 2)} |
             {f"dwpw_kernel<{nb}, {p}, {s}>" for nb in (2, 4) for p in (1, 2, 4) for s in (1, 2)})


def cases():
    """Every case: the hand-written ones, the fp32-canvas twin of every u8 case, one per census key."""
    out = list(HAND) + [case_from_key(k, i) for i, k in enumerate(CENSUS_KEYS)]
    out += [f32_twin(c) for c in out if c.kind == "ystem_u8"]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out
