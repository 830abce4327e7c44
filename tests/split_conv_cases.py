"""Case table and product census for the split-bf16 conv kernels of csrc/pwx6.hip (pwx6_kernel<NT16, MT, UP>,
convx6_kernel<NT16>): the dense convs a plan carries as FP_OPF_SPLIT3.  tests/test_split_conv_ops.py runs every case as a
one-op plan.  The machinery is generic_op_cases' (Case, inputs, weights, reference, footprint, input_index, product_plans);
what is added here:

* build() emits the case with PlanBuilder.X6 on and x6_all set, so that every conv the launchers take runs split, and hangs
  the half-size map of an FP_OPF_IN_UP2 case on the input view (Case.up_C / up_buf_C / up_coff).
* reference32() is the fp32 yardstick of the fp64 bound: torch's CPU conv up to K = KH * KW * Cin = 720, the k-ordered fp32
  fmaf chain (the arithmetic the split replaces) on the im2col matrix above that (torch's blocked sums beat
  any k-ordered fp32 kernel at K = 1152).
* feature_key() / census() / CENSUS_KEYS / case_from_key(): as in generic_op_cases, for ops that land on the two split
  kernels.  A network that sends a new combination to them makes census() grow past CENSUS_KEYS: add the key here.
"""
import functools
from dataclasses import replace

import numpy as np
import torch
import torch.nn.functional as F

import generic_op_cases as G
from generic_op_cases import Case, footprint, hash_name, input_index, inputs, kernel_name, product_plans, reference  # noqa: F401
from generic_op_cases import tolerance, weights  # noqa: F401
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import PlanBuilder

SPLIT = ("pwx6_kernel", "convx6_kernel")
K_TORCH_MAX = 720          # above: reference32 is the fmaf chain


def kdim(c):
    return c.k[0] * c.k[1] * c.C


def build(c, N=None):
    """Emit the one-op plan of a case on the split kernels -> (builder, {"x", "out", "res", "up": Buf or None}).
    PlanBuilder.X6 is on while the op is emitted and restored afterwards; x6_all sends every conv the launchers take there."""
    saved = PlanBuilder.X6
    PlanBuilder.X6 = True
    try:
        pb = PlanBuilder(N or c.N)
        pb.x6_all = True
        oh, ow = G._out_hw(c)
        xb = G._raw_buf(pb, c.H, c.W, c.in_buf_C or c.C, c.in_ns_extra)
        rb = ub = None
        if c.res:
            rb = G._raw_buf(pb, oh, ow, c.res_buf_C or c.res_C or G._out_view_C(c))
        if c.up_C:
            ub = G._raw_buf(pb, c.H // 2, c.W // 2, c.up_buf_C or c.up_C)
        wc = G._written_C(c)
        ob = G._raw_buf(pb, oh, ow, c.out_buf_C or wc)
        xv = xb.view(c.in_coff, c.C)
        if ub is not None:
            xv.up = ub.view(c.up_coff, c.up_C)
        ov = ob.view(c.out_coff, G._out_view_C(c))
        p = weights(c)
        rv = rb.view(c.res_coff, c.res_C or G._out_view_C(c)) if rb is not None else None
        pb.conv(xv, p["w"], ov, stride=c.stride, pad=c.pad, scale=p.get("scale"), bias=p.get("bias"), slope=p.get("slope"),
                act=G.ACTS[c.act], res=rv, res_mode=G.RES[c.res])
    finally:
        PlanBuilder.X6 = saved
    assert len(pb.ops) == 1, [o.kind for o in pb.ops]      # (a half-size map that was not folded shows as an upsample op)
    return pb, {"x": xb, "out": ob, "res": rb, "up": ub}


def _chain_conv(xp, w, stride):
    """F.conv2d(xp, w, stride=stride) in fp32 as the k-ordered fmaf chain: k = (dy * KW + dx) * Cin + channel, the order of
    the kernels' K loop (test_gpu_parity._fmaf_chain on the im2col matrix)."""
    from test_gpu_parity import _fmaf_chain
    n, cin, hp, wp = xp.shape
    co, _, kh, kw = w.shape
    oh, ow = (hp - kh) // stride + 1, (wp - kw) // stride + 1
    cols = F.unfold(xp, (kh, kw), stride=stride).reshape(n, cin, kh * kw, oh * ow)         # [n][c][tap][pix]
    a = cols.permute(0, 3, 2, 1).reshape(n * oh * ow, kh * kw * cin).numpy()
    b = w.reshape(co, cin, kh * kw).permute(2, 1, 0).reshape(kh * kw * cin, co).numpy()
    v = _fmaf_chain(np.ascontiguousarray(a), np.ascontiguousarray(b))
    return torch.from_numpy(v).reshape(n, oh, ow, co).permute(0, 3, 1, 2)


def reference32(c, data):
    """The fp32 yardstick of the bound 2 * max|ref32 - ref64| + tol * max|ref64|."""
    return reference(c, data, torch.float32, conv=None if kdim(c) <= K_TORCH_MAX else _chain_conv)


# ---------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------
def feature_key(op, name=None):
    """The feature key of an op that runs on pwx6_kernel / convx6_kernel, None for any other op:
    (instance, KH, KW, stride, pad_t, pad_l, act, res_mode, OH*OW < 32, OW == 1, OH*OW == 1 (the kernel skips its
     multiply-high divisions in these two), flat (Cin < 32), Cin % 32 != 0, Cout % 16 != 0, FP_OPF_IN_C3, FP_OPF_IN_UP2,
     sliced in, sliced out, foreign image stride in, scale present, bias present)"""
    name = name or kernel_name(op)
    if name.split("<")[0] not in SPLIT:
        return None
    ohw = op.OH * op.OW
    wc = 2 * op.Cout if op.res_mode == L.RES_SHUFFLE2 else op.Cout
    return (name, op.KH, op.KW, op.stride, op.pad_t, op.pad_l, op.act, op.res_mode, ohw < 32, op.OW == 1, ohw == 1,
            op.Cin < 32, op.Cin % 32 != 0, op.Cout % 16 != 0, bool(op.flags & L.OPF_IN_C3), bool(op.flags & L.OPF_IN_UP2),
            op.in_ld != op.Cin, op.out_ld != wc, op.in_ns != op.H * op.W * op.in_ld, op.scale_off >= 0, op.bias_off >= 0)


@functools.lru_cache(maxsize=None)
def census():
    """{feature key: label of the first plan that reaches a split conv kernel with it} over product_plans()."""
    found = {}
    for label, pb in product_plans():
        for op in pb.finish()[0]:
            key = feature_key(op)
            if key is not None:
                found.setdefault(key, label)
    return found


_ACT_NAMES = {v: k for k, v in G.ACTS.items()}
_RES_NAMES = {v: k for k, v in G.RES.items()}
# pwx6_kernel<NT16, 4, *>: enough rows for pwx6_small_tiles to leave the large form: ceil(M / 256) * nchunk = 360 workgroups
# = 0.703 rounds of the 512 slots (>= 0.7: large).  (Cout, N) on a 48 x 48 map.
_PW_LARGE = {3: (48, 40), 4: (64, 40), 8: (512, 10)}
_PW_COUT = {3: 48, 4: 64, 8: 128}
_CX_COUT = {2: (32, None), 3: (48, 36), 4: (64, 52), 6: (96, 84)}       # NT16 -> Cout with Cout % 16 == 0 / != 0


def case_from_key(key, i):
    """A small case with exactly this feature key (test_split_conv_ops checks that feature_key gives it back)."""
    (name, kh, kw, stride, pt, pl, act, res_mode, small, ow1, ohw1, flat, c32, c16, c3, up2, sl_in, sl_out, fns_in, scale,
     bias) = key
    fam, targs = name.split("<")
    targs = [t.strip() for t in targs.rstrip(">").split(",")]
    nt = int(targs[0])
    res = _RES_NAMES[res_mode]
    N = 3
    if fam == "pwx6_kernel":
        C, up_C = 64, (32 if up2 else 0)
        cout = _PW_COUT[nt]
    else:
        cout = _CX_COUT[nt][1 if c16 else 0]
        C = 4 if c3 else 16 if flat else 40 if c32 else 32
        up_C = (16 if c32 else 8) if up2 else 0
    if ohw1:
        oh = ow = 1
    elif ow1:
        oh, ow = (5 if small else 40), 1
    else:
        oh, ow = (2, 4) if small else (6, 10)
    if fam == "pwx6_kernel" and targs[1] == "4":
        cout, N = _PW_LARGE[nt]
        oh = ow = 48
    H, W = (oh - 1) * stride + kh - 2 * pt, (ow - 1) * stride + kw - 2 * pl
    assert H >= 1 and W >= 1, key
    wc = 2 * cout if res == "shuffle" else cout
    big = N > 3
    return Case(f"census{i:02d}_{fam[:-7]}", "conv", name, N, H, W, C, cin=3 if c3 else 0, cout=cout, k=(kh, kw), stride=stride,
                pad=(pt, pl), act=_ACT_NAMES[act], scale=scale, bias=bias, res=res, up_C=up_C,
                in_buf_C=C + 8 if sl_in else 0, in_coff=4 if sl_in else 0, in_ns_extra=20 if fns_in else 0,
                out_buf_C=wc + 8 if sl_out else 0, out_coff=4 if sl_out else 0,
                partial=0 if big else (1 if i % 2 == 0 else 0))


# The feature keys census() found in the shipped plans when this table was last brought up to date
# (tests/test_split_conv_ops.py test_census_is_covered fails, printing the missing keys, as soon as census() finds a new one).
CENSUS_KEYS = [
    ('convx6_kernel<2>', 3, 3, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<2>', 3, 3, 1, 0, 0, 2, 0, False, False, False, True, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<2>', 3, 3, 1, 0, 0, 2, 0, False, False, False, True, True, False, True, False, False, False, False, False, True),
    ('convx6_kernel<2>', 3, 3, 1, 0, 0, 2, 0, True, False, False, True, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<2>', 3, 3, 1, 0, 0, 2, 0, True, True, True, True, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<2>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<2>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('convx6_kernel<2>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, True, True, False, True, True),
    ('convx6_kernel<2>', 3, 3, 2, 0, 0, 1, 0, False, False, False, True, True, False, True, False, False, False, False, True, True),
    ('convx6_kernel<3>', 1, 1, 1, 0, 0, 0, 0, False, False, False, False, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<3>', 3, 3, 1, 0, 0, 2, 0, False, False, False, True, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<3>', 3, 3, 1, 1, 1, 3, 0, False, False, False, False, True, False, False, False, False, True, False, True, True),
    ('convx6_kernel<3>', 3, 3, 1, 1, 1, 3, 2, False, False, False, False, True, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 1, 7, 1, 0, 3, 1, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('convx6_kernel<4>', 2, 2, 1, 0, 0, 2, 0, True, False, False, False, False, False, False, False, False, False, False, False, True),
    ('convx6_kernel<4>', 2, 2, 1, 0, 0, 2, 0, True, False, False, False, True, False, False, False, False, False, False, False, True),
    ('convx6_kernel<4>', 3, 3, 1, 0, 0, 2, 0, False, False, False, False, False, False, False, False, False, False, False, False, True),
    ('convx6_kernel<4>', 3, 3, 1, 0, 0, 2, 0, True, True, True, False, False, False, False, False, False, False, False, False, True),
    ('convx6_kernel<4>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<4>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('convx6_kernel<4>', 3, 3, 1, 1, 1, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 3, 3, 2, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<4>', 3, 3, 2, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 3, 3, 2, 0, 0, 1, 0, True, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 3, 3, 2, 0, 0, 1, 0, True, False, False, False, False, False, False, False, True, True, False, True, True),
    ('convx6_kernel<4>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 5, 5, 1, 2, 2, 1, 0, False, False, False, False, False, False, False, False, True, True, False, False, True),
    ('convx6_kernel<4>', 7, 1, 1, 3, 0, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<4>', 7, 7, 1, 0, 0, 1, 0, True, True, True, False, False, False, False, False, True, True, False, False, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, True, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, True, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, True, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, True, True, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, True, True, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, True, True, False, False, True, False, False, True, True),
    ('convx6_kernel<6>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, True, True, False, True, False, False, False, True, True),
    ('convx6_kernel<6>', 1, 3, 1, 0, 1, 1, 0, True, False, False, False, False, False, False, False, True, False, False, True, True),
    ('convx6_kernel<6>', 3, 1, 1, 1, 0, 1, 0, True, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 1, 0, 0, 1, 0, False, False, False, False, True, False, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 3, 3, 1, 1, 1, 1, 0, False, False, False, False, False, False, False, False, True, True, False, False, True),
    ('convx6_kernel<6>', 3, 3, 1, 1, 1, 3, 0, False, False, False, False, True, True, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 1, 1, 1, 3, 2, False, False, False, False, True, True, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 0, 0, 1, 0, True, False, False, False, False, False, False, False, True, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, False, True, False, False, True, False, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, True, False, False, False, False, False, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, True, True, False, False, False, True, False, True, True),
    ('convx6_kernel<6>', 3, 3, 2, 1, 1, 3, 0, False, False, False, False, True, True, False, False, True, False, False, True, True),
    ('convx6_kernel<6>', 7, 7, 4, 0, 0, 1, 0, False, False, False, True, True, False, True, False, False, False, False, False, True),
    ('pwx6_kernel<3, 2, false>', 1, 1, 1, 0, 0, 0, 0, False, False, False, False, False, False, False, False, False, False, False, False, True),
    ('pwx6_kernel<3, 4, false>', 1, 1, 1, 0, 0, 0, 0, False, False, False, False, False, False, False, False, False, False, False, False, True),
    ('pwx6_kernel<4, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<4, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<4, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<4, 2, true>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, True, False, False, False, True, True),
    ('pwx6_kernel<4, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<4, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<4, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<4, 4, true>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, True, False, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 0, 0, True, True, True, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 0, 1, True, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 0, True, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 0, True, True, True, False, False, False, False, False, True, True, False, False, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 1, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 1, 1, True, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 2, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<8, 2, false>', 1, 1, 1, 0, 0, 3, 4, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 2, true>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, True, False, False, False, True, True),
    ('pwx6_kernel<8, 4, false>', 1, 1, 1, 0, 0, 1, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 4, false>', 1, 1, 1, 0, 0, 1, 1, False, False, False, False, False, False, False, False, True, False, False, True, True),
    ('pwx6_kernel<8, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, False, False, True, True),
    ('pwx6_kernel<8, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, False, True, False, True, True),
    ('pwx6_kernel<8, 4, false>', 1, 1, 1, 0, 0, 3, 0, False, False, False, False, False, False, False, False, True, False, False, True, True),
]


# ---------------------------------------------------------------------------------------------------------------------------
# hand-written edges
# ---------------------------------------------------------------------------------------------------------------------------
def _cx(name, nt, **kw):
    kw.setdefault("N", 2)
    return Case(name=name, kind="conv", kernel=f"convx6_kernel<{nt}>", **kw)


def _pw(name, nt, mt=2, up=False, **kw):
    kw.setdefault("N", 2)
    return Case(name=name, kind="conv", kernel=f"pwx6_kernel<{nt}, {mt}, {'true' if up else 'false'}>", **kw)


_ACT4 = ("none", "relu", "prelu", "silu")
_RES4 = ("", "before", "after", "shuffle")


def _epilogues():
    """Every activation x residual mode on both kernels; the residual is narrower than the output where eligibility allows it
    (FP_RES_SHUFFLE2 needs res_C >= Cout), and sits inside a wider buffer."""
    out = []
    for a, act in enumerate(_ACT4):
        for r, res in enumerate(_RES4):
            tag = f"{act}_{res or 'nores'}"
            rc = {"": {}, "before": dict(res_C=24, res_buf_C=32, res_coff=4), "after": dict(res_C=24, res_buf_C=24),
                  "shuffle": dict(res_C=0, res_buf_C=0)}[res]
            part = dict(partial=1) if (a + r) % 3 == 0 else {}
            out.append(_pw(f"pw_epi_{tag}", 4, H=3, W=5, C=64, cout=64, act=act, res=res, **rc, **part))
            out.append(_cx(f"c3x3_epi_{tag}", 3, H=3, W=5, C=32, cout=36, k=(3, 3), pad=(1, 1), act=act, res=res,
                           **(dict(rc, res_C=36, res_buf_C=40) if res == "shuffle" else rc), **part))
    return out


HAND = [
    # ---- convx6_kernel: windows the launcher accepts and no network uses yet -----------------------------------------------
    _cx("pw_s2", 2, H=7, W=7, C=32, cout=32, stride=2, act="relu", partial=1),
    _cx("pw_s4_c40", 3, H=9, W=10, C=40, cout=48, stride=4, act="silu"),
    _cx("c4x4_s4_c8_flat", 2, H=12, W=12, C=8, cout=32, k=(4, 4), stride=4, act="relu", partial=1),
    _cx("c7x7_s4_p3_c12_flat", 3, H=10, W=9, C=12, cout=36, k=(7, 7), stride=4, pad=(3, 3), act="relu"),
    _cx("c5x5_p2_map2x2", 2, N=3, H=2, W=2, C=32, cout=32, k=(5, 5), pad=(2, 2), act="relu", partial=2),
    _cx("c3x3_pad20", 4, H=5, W=6, C=32, cout=64, k=(3, 3), pad=(2, 0), act="prelu"),
    _cx("c6x6_s2_pad51", 2, H=7, W=8, C=32, cout=32, k=(6, 6), stride=2, pad=(5, 1), act="relu", partial=1),
    _cx("c3x3_ow1", 2, N=3, H=6, W=3, C=32, cout=32, k=(3, 3), act="relu", partial=1),
    _cx("c3x3_shuffle_prelu", 2, H=5, W=6, C=32, cout=32, k=(3, 3), pad=(1, 1), act="prelu", res="shuffle", res_C=32),
    _cx("c3x3_cout112_chunks_of_4", 4, H=5, W=6, C=32, cout=112, k=(3, 3), pad=(1, 1), act="relu"),
    _cx("pw_c36_cout272_chunks_of_6", 6, N=1, H=1, W=257, C=36, cout=272, act="relu"),      # 2 row tiles x 3 chunks = 6 workgroups
    # ---- windows of the shipped plans that only whole-network tests reached ------------------------------------------------
    _cx("c2x2_valid", 2, H=5, W=6, C=32, cout=32, k=(2, 2), act="prelu", partial=1),
    _cx("c7x7_fc_n5", 2, N=5, H=7, W=7, C=32, cout=32, k=(7, 7), act="relu", partial=2),
    _cx("c7x7_fc_n70", 2, N=70, H=7, W=7, C=32, cout=32, k=(7, 7), act="relu", partial=33),
    _cx("c5x5_p2", 3, H=6, W=7, C=32, cout=48, k=(5, 5), pad=(2, 2), act="relu", scale=False),
    _cx("c3x3_c28_flat_no_scale", 3, H=6, W=5, C=28, cout=48, k=(3, 3), act="prelu", scale=False, partial=1),
    _cx("c1x7_map3x3", 2, N=3, H=3, W=3, C=32, cout=32, k=(1, 7), pad=(0, 3), act="relu", partial=1),
    _cx("c7x1_map3x3", 2, N=3, H=3, W=3, C=32, cout=32, k=(7, 1), pad=(3, 0), act="relu"),
    _cx("c5x5_s4_c32", 2, H=9, W=13, C=32, cout=32, k=(5, 5), stride=4, pad=(2, 2), act="relu"),
    # ---- flat K: FP_OPF_IN_C3, a slab that holds one tap and part of the next, a last slab that is mostly padding -----------
    _cx("c3x3_s2_in_c3", 2, H=9, W=9, C=4, cin=3, cout=32, k=(3, 3), stride=2, act="relu", partial=1),
    _cx("c7x7_s4_in_c3", 6, H=15, W=11, C=4, cin=3, cout=96, k=(7, 7), stride=4, act="relu"),
    _cx("c3x3_c8_flat", 2, H=5, W=6, C=8, cout=32, k=(3, 3), pad=(1, 1), act="silu"),
    _cx("c3x3_c12_flat", 2, H=5, W=6, C=12, cout=32, k=(3, 3), pad=(1, 1), stride=2, act="relu", partial=1),
    _cx("c3x3_c16_flat", 3, H=5, W=6, C=16, cout=36, k=(3, 3), pad=(1, 1), stride=2, act="silu"),
    _cx("c3x3_c24_flat", 2, H=5, W=6, C=24, cout=32, k=(3, 3), act="relu", partial=1),
    _cx("c3x3_c28_flat", 2, H=5, W=6, C=28, cout=32, k=(3, 3), pad=(1, 1), act="prelu"),
    _cx("pw_s4_c8_flat", 2, H=9, W=9, C=8, cout=32, stride=4, act="relu", partial=1),
    _cx("c2x3_s4_c12_flat", 2, H=9, W=9, C=12, cout=32, k=(2, 3), stride=4, pad=(1, 1), act="relu"),
    _cx("c5x5_s4_c16_flat", 2, H=9, W=10, C=16, cout=32, k=(5, 5), stride=4, pad=(2, 2), act="relu", partial=1),
    _cx("c4x4_s4_c24_flat", 2, H=8, W=12, C=24, cout=32, k=(4, 4), stride=4, act="prelu"),
    _cx("c7x7_s4_c28_flat", 2, H=11, W=7, C=28, cout=32, k=(7, 7), stride=4, pad=(3, 3), act="relu", partial=1),   # K = 1372
    # ---- a partial last channel slab (k_lo true, k_hi false) and widths beyond Cout that are not stored ----------------------
    _cx("c3x3_c36_cout84", 6, H=4, W=5, C=36, cout=84, k=(3, 3), pad=(1, 1), act="relu", out_buf_C=96, out_coff=4),
    _cx("c3x3_c80_cout100", 4, H=4, W=5, C=80, cout=100, k=(3, 3), pad=(1, 1), act="relu", out_buf_C=112, out_coff=8, partial=1),
    _cx("pw_c92_cout36", 3, H=4, W=5, C=92, cout=36, act="silu", in_buf_C=104, in_coff=8, out_buf_C=44, out_coff=4),
    _cx("c3x3_c184", 2, H=3, W=4, C=184, cout=32, k=(3, 3), pad=(1, 1), act="relu", partial=1),                         # K = 1656
    # ---- views ------------------------------------------------------------------------------------------------------------
    _cx("c3x3_in_slice", 2, H=4, W=5, C=40, cout=32, k=(3, 3), pad=(1, 1), act="relu", in_buf_C=72, in_coff=16),
    _cx("c3x3_in_foreign_ns", 2, N=3, H=4, W=5, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu", in_ns_extra=36, partial=2),
    _cx("c3x3_out_slice", 3, H=4, W=5, C=32, cout=36, k=(3, 3), pad=(1, 1), act="relu", out_buf_C=64, out_coff=12),
    _cx("c3x3_shuffle_in_wider", 3, H=4, W=5, C=32, cout=36, k=(3, 3), pad=(1, 1), act="relu", res="shuffle", res_C=36,
        res_buf_C=48, res_coff=8, out_buf_C=96, out_coff=8, partial=1),
    _pw("pw_in_slice", 4, H=4, W=5, C=64, cout=64, act="relu", in_buf_C=96, in_coff=16),
    _pw("pw_out_slice", 3, H=4, W=5, C=64, cout=48, act="silu", out_buf_C=80, out_coff=12, partial=1),
    _pw("pw_shuffle_in_wider", 4, H=4, W=5, C=96, cout=64, act="silu", res="shuffle", res_C=64, res_buf_C=80, res_coff=12,
        out_buf_C=160, out_coff=16),
    # ---- rows: M = 1, a wave's 64 rows, one more than the 128- and 256-row tiles, grids that are no multiple of 8 -------------
    _pw("pw_m1", 8, N=1, H=1, W=1, C=64, cout=128, act="relu"),
    _pw("pw_m63", 4, N=1, H=7, W=9, C=64, cout=64, act="relu"),
    _pw("pw_m64", 4, N=1, H=8, W=8, C=64, cout=64, act="prelu"),
    _pw("pw_m65", 4, N=1, H=5, W=13, C=64, cout=64, act="relu"),
    _pw("pw_m129", 3, N=3, H=1, W=43, C=64, cout=48, act="relu", partial=1),
    _pw("pw_m1300_grid11", 4, N=1, H=26, W=50, C=64, cout=64, act="relu"),
    _pw("pw_large_m92161", 4, 4, N=1, H=1, W=92161, C=64, cout=64, act="relu"),               # 360 tiles of 256 rows + 1 row
    _pw("pw_cout256_grid6", 8, N=3, H=9, W=13, C=128, cout=256, act="silu", partial=2),        # 351 rows: 3 tiles x 2 chunks
    _cx("c3x3_m1", 2, N=1, H=3, W=3, C=32, cout=32, k=(3, 3), act="relu"),
    _cx("c3x3_m63", 2, N=1, H=7, W=9, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu"),
    _cx("c3x3_m64", 2, N=1, H=8, W=8, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu"),
    _cx("c3x3_m65", 2, N=1, H=5, W=13, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu"),
    _cx("c3x3_m768_grid3", 2, N=3, H=16, W=16, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu", partial=2),
    # ---- FP_OPF_IN_UP2: the concat slice the fold replaces holds NaN ---------------------------------------------------------
    _pw("pw_up2_map2x2", 4, up=True, N=3, H=2, W=2, C=64, cout=64, up_C=32, act="silu", partial=1),
    _pw("pw_up2_map6x10", 8, up=True, H=6, W=10, C=96, cout=128, up_C=64, up_buf_C=80, up_coff=8, act="silu", in_buf_C=112,
        in_coff=8),
    _pw("pw_up2_cout48", 3, up=True, H=4, W=6, C=64, cout=48, up_C=32, act="relu", partial=1),
    _pw("pw_up2_large_cout48", 3, 4, True, N=40, H=48, W=48, C=64, cout=48, up_C=32, act="silu"),
    _cx("pw_up2_c56_map2x2", 3, N=3, H=2, W=2, C=56, cout=48, up_C=24, act="silu", partial=2),
    _cx("pw_up2_c56_map6x10", 3, H=6, W=10, C=56, cout=36, up_C=24, up_buf_C=40, up_coff=12, act="silu", in_buf_C=64, in_coff=4),
    # ---- data ---------------------------------------------------------------------------------------------------------------
    _pw("pw_prelu_all_negative", 4, H=4, W=5, C=64, cout=64, act="prelu", special="neg"),
    _cx("c3x3_prelu_all_negative", 3, H=4, W=5, C=32, cout=36, k=(3, 3), pad=(1, 1), act="prelu", special="neg"),
    _pw("pw_inf", 4, H=4, W=5, C=64, cout=64, special="inf_pair"),
    _cx("c3x3_inf", 2, H=6, W=7, C=32, cout=32, k=(3, 3), pad=(1, 1), special="inf_pair"),
    _pw("pw_zero_row", 4, H=4, W=5, C=64, cout=64, act="relu", special="zero_row"),
    _cx("c3x3_zero_row", 2, H=4, W=5, C=32, cout=32, k=(3, 3), pad=(1, 1), act="relu", special="zero_row"),
] + _epilogues()


@functools.lru_cache(maxsize=None)
def cases():
    """Every case: one per census key, then the hand-written edges.  Names are unique."""
    out = [case_from_key(k, i) for i, k in enumerate(CENSUS_KEYS)] + HAND
    assert len({c.name for c in out}) == len(out)
    return out


def padded(c):
    """The case has padding (some window reaches outside the map)."""
    return c.pad != (0, 0)


def mutants(c):
    """(label, fp64 reference of a wrong conv) for a case with padding: the weights of one border tap (the first tap that
    lies in the padding for some output pixels and inside the map for others) zeroed, and pad_l off by one."""
    data = inputs(c)
    p = weights(c)
    p = dict(p, w=p["w"].copy())
    oh, ow = G._out_hw(c)

    def mixed(d, o, pad, size):      # tap offset d: inside the map for some of the o outputs, outside for others
        inside = [0 <= i * c.stride - pad + d < size for i in range(o)]
        return any(inside) and not all(inside)

    dy, dx = next((dy, dx) for dy in range(c.k[0]) for dx in range(c.k[1])
                  if (mixed(dy, oh, c.pad[0], c.H) and any(0 <= i * c.stride - c.pad[1] + dx < c.W for i in range(ow))) or
                  (mixed(dx, ow, c.pad[1], c.W) and any(0 <= i * c.stride - c.pad[0] + dy < c.H for i in range(oh))))
    p["w"][:, :, dy, dx] = 0.0
    yield "border tap zeroed", reference(c, data, torch.float64, p=p)
    yield "pad_l + 1", reference(replace(c, pad=(c.pad[0], c.pad[1] + 1), OH=oh, OW=ow), data, torch.float64)
