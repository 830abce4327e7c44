"""FaceNet (Inception-ResNet-v1, modules/facenet/inception_resnet_v1.py): state dict, plans, the split-MFMA conv's
rectangular / unpadded windows (csrc/pwx6.hip convx6_kernel), the embedding head (csrc/embedhead.hip), and the whole network
against a float64 torch restatement of the architecture written here, independent of the HIP module."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.facenet.inception_resnet_v1 import InceptionResnetV1
from face_detection_and_recognition_amd.plan import CompiledPlan, PlanBuilder, validate_on_host
from face_detection_and_recognition_amd.synth import synth_state_dict


# ---------------------------------------------------------------------------------------------------------------------
# float64 oracle: the published architecture (facenet-pytorch's module tree), torch.nn.functional on the CPU

def _bc(sd, p, x, stride=1, pad=(0, 0)):
    w = sd[p + ".conv.weight"].double()
    y = F.conv2d(x, w, stride=stride, padding=pad)
    g, b, m, v = (sd[p + ".bn." + k].double().view(1, -1, 1, 1) for k in ("weight", "bias", "running_mean", "running_var"))
    return torch.relu((y - m) / torch.sqrt(v + 1e-3) * g + b)


def _up(sd, p, x, cat, scale, relu):
    y = x + scale * F.conv2d(cat, sd[p + ".conv2d.weight"].double(), sd[p + ".conv2d.bias"].double())
    return torch.relu(y) if relu else y


def _block35(sd, p, x):
    b0 = _bc(sd, p + ".branch0", x)
    b1 = _bc(sd, p + ".branch1.1", _bc(sd, p + ".branch1.0", x), pad=(1, 1))
    b2 = _bc(sd, p + ".branch2.0", x)
    b2 = _bc(sd, p + ".branch2.2", _bc(sd, p + ".branch2.1", b2, pad=(1, 1)), pad=(1, 1))
    return _up(sd, p, x, torch.cat([b0, b1, b2], 1), 0.17, True)


def _block17(sd, p, x):
    b0 = _bc(sd, p + ".branch0", x)
    b1 = _bc(sd, p + ".branch1.2", _bc(sd, p + ".branch1.1", _bc(sd, p + ".branch1.0", x), pad=(0, 3)), pad=(3, 0))
    return _up(sd, p, x, torch.cat([b0, b1], 1), 0.10, True)


def _block8(sd, p, x, scale=0.20, relu=True):
    b0 = _bc(sd, p + ".branch0", x)
    b1 = _bc(sd, p + ".branch1.2", _bc(sd, p + ".branch1.1", _bc(sd, p + ".branch1.0", x), pad=(0, 1)), pad=(1, 0))
    return _up(sd, p, x, torch.cat([b0, b1], 1), scale, relu)


def oracle_forward(sd, x, normalize):
    """x: (B, 3, 160, 160) -> (B, D) in float64."""
    x = torch.as_tensor(x).double()
    x = _bc(sd, "conv2d_1a", x, stride=2)
    x = _bc(sd, "conv2d_2a", x)
    x = _bc(sd, "conv2d_2b", x, pad=(1, 1))
    x = F.max_pool2d(x, 3, 2)
    x = _bc(sd, "conv2d_3b", x)
    x = _bc(sd, "conv2d_4a", x)
    x = _bc(sd, "conv2d_4b", x, stride=2)
    for i in range(5):
        x = _block35(sd, f"repeat_1.{i}", x)
    b0 = _bc(sd, "mixed_6a.branch0", x, stride=2)
    b1 = _bc(sd, "mixed_6a.branch1.2", _bc(sd, "mixed_6a.branch1.1", _bc(sd, "mixed_6a.branch1.0", x), pad=(1, 1)), stride=2)
    x = torch.cat([b0, b1, F.max_pool2d(x, 3, 2)], 1)
    for i in range(10):
        x = _block17(sd, f"repeat_2.{i}", x)
    b0 = _bc(sd, "mixed_7a.branch0.1", _bc(sd, "mixed_7a.branch0.0", x), stride=2)
    b1 = _bc(sd, "mixed_7a.branch1.1", _bc(sd, "mixed_7a.branch1.0", x), stride=2)
    b2 = _bc(sd, "mixed_7a.branch2.2", _bc(sd, "mixed_7a.branch2.1", _bc(sd, "mixed_7a.branch2.0", x), pad=(1, 1)), stride=2)
    x = torch.cat([b0, b1, b2, F.max_pool2d(x, 3, 2)], 1)
    for i in range(5):
        x = _block8(sd, f"repeat_3.{i}", x)
    x = _block8(sd, "block8", x, scale=1.0, relu=False)
    x = x.mean(dim=(2, 3)) @ sd["last_linear.weight"].double().T
    g, b, m, v = (sd["last_bn." + k].double() for k in ("weight", "bias", "running_mean", "running_var"))
    x = (x - m) / torch.sqrt(v + 1e-3) * g + b
    return F.normalize(x, dim=1, eps=1e-12) if normalize else x


# the table of the issue / DESIGN: (prefix, conv shape) of every BasicConv, plus the up-projections and the head
def expected_shapes(D):
    s = {}

    def bc(p, cin, cout, kh, kw):
        s[p + ".conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            s[p + ".bn." + k] = (cout,)
        s[p + ".bn.num_batches_tracked"] = ()
    bc("conv2d_1a", 3, 32, 3, 3); bc("conv2d_2a", 32, 32, 3, 3); bc("conv2d_2b", 32, 64, 3, 3)
    bc("conv2d_3b", 64, 80, 1, 1); bc("conv2d_4a", 80, 192, 3, 3); bc("conv2d_4b", 192, 256, 3, 3)
    for i in range(5):
        p = f"repeat_1.{i}"
        bc(p + ".branch0", 256, 32, 1, 1); bc(p + ".branch1.0", 256, 32, 1, 1); bc(p + ".branch1.1", 32, 32, 3, 3)
        bc(p + ".branch2.0", 256, 32, 1, 1); bc(p + ".branch2.1", 32, 32, 3, 3); bc(p + ".branch2.2", 32, 32, 3, 3)
        s[p + ".conv2d.weight"], s[p + ".conv2d.bias"] = (256, 96, 1, 1), (256,)
    bc("mixed_6a.branch0", 256, 384, 3, 3); bc("mixed_6a.branch1.0", 256, 192, 1, 1)
    bc("mixed_6a.branch1.1", 192, 192, 3, 3); bc("mixed_6a.branch1.2", 192, 256, 3, 3)
    for i in range(10):
        p = f"repeat_2.{i}"
        bc(p + ".branch0", 896, 128, 1, 1); bc(p + ".branch1.0", 896, 128, 1, 1)
        bc(p + ".branch1.1", 128, 128, 1, 7); bc(p + ".branch1.2", 128, 128, 7, 1)
        s[p + ".conv2d.weight"], s[p + ".conv2d.bias"] = (896, 256, 1, 1), (896,)
    bc("mixed_7a.branch0.0", 896, 256, 1, 1); bc("mixed_7a.branch0.1", 256, 384, 3, 3)
    bc("mixed_7a.branch1.0", 896, 256, 1, 1); bc("mixed_7a.branch1.1", 256, 256, 3, 3)
    bc("mixed_7a.branch2.0", 896, 256, 1, 1); bc("mixed_7a.branch2.1", 256, 256, 3, 3); bc("mixed_7a.branch2.2", 256, 256, 3, 3)
    for p in [f"repeat_3.{i}" for i in range(5)] + ["block8"]:
        bc(p + ".branch0", 1792, 192, 1, 1); bc(p + ".branch1.0", 1792, 192, 1, 1)
        bc(p + ".branch1.1", 192, 192, 1, 3); bc(p + ".branch1.2", 192, 192, 3, 1)
        s[p + ".conv2d.weight"], s[p + ".conv2d.bias"] = (1792, 384, 1, 1), (1792,)
    s["last_linear.weight"] = (D, 1792)
    for k in ("weight", "bias", "running_mean", "running_var"):
        s["last_bn." + k] = (D,)
    s["last_bn.num_batches_tracked"] = ()
    return s


def synth_sd(D, seed):
    return synth_state_dict(InceptionResnetV1(D).state_dict(), seed)


def seeded_input(n, seed):
    return np.random.default_rng(seed).normal(0.0, 1.0, (n, 3, 160, 160)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU

@pytest.mark.parametrize("D", [128, 512])
def test_state_dict_layout(D):
    sd = InceptionResnetV1(D).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == expected_shapes(D)
    n = sum(v.numel() for k, v in sd.items() if not k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"))
    assert round(n / 1e6, 2) == {128: 22.79, 512: 23.48}[D]


def test_state_dict_loading():
    sd = synth_sd(128, 1)
    net = InceptionResnetV1(128, normalize=False)
    bare = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    extra = dict(bare, **{"logits.weight": torch.zeros(10, 128), "logits.bias": torch.zeros(10)})
    for d in (sd, bare, extra):
        net.load_state_dict(d)
        assert torch.equal(net.repeat_2[3].branch1[1].conv.weight, sd["repeat_2.3.branch1.1.conv.weight"])
    missing = dict(bare)
    del missing["repeat_3.2.branch1.2.bn.running_var"]
    with pytest.raises(RuntimeError):
        net.load_state_dict(missing)
    bad = dict(bare, **{"repeat_2.0.branch1.1.conv.weight": torch.zeros(128, 128, 7, 1)})   # 7x1 where 1x7 belongs
    with pytest.raises(RuntimeError):
        net.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        net.load_state_dict(dict(bare, **{"repeat_9.0.conv2d.bias": torch.zeros(3)}))       # unexpected key
    with pytest.raises(RuntimeError):
        InceptionResnetV1(512).load_state_dict(bare)                                        # a 128-d head in a 512-d net


@pytest.mark.parametrize("x6", [True, False])
@pytest.mark.parametrize("D", [128, 512])
def test_plans_validate(lib, D, x6):
    net = InceptionResnetV1(D, normalize=D == 512)
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        for n in (1, 3, 256, 1024):
            assert validate_on_host(net._emit(n)[0]) == 0
    finally:
        PlanBuilder.X6 = saved


def test_x6_plan_has_no_fp32_convs(lib):
    """With the split kernels on, EVERY conv of the plan -- the 3->32 stem, the unpadded 3x3s, the 1x7 / 7x1 / 1x3 / 3x1 windows,
    the 32- and 80-channel convs on 17 x 17 and smaller maps -- carries FP_OPF_SPLIT3 and none runs on conv_igemm_kernel."""
    for D in (128, 512):
        for n in (1, 64, 1024):
            ops = InceptionResnetV1(D, normalize=D == 512)._emit(n)[0].finish()[0]
            names = [lib.fp_op_kernel_name(ctypes.byref(op)).decode() for op in ops]
            convs = [(op, nm) for op, nm in zip(ops, names) if op.kind == L.OP_CONV]
            assert len(convs) == 104
            for op, nm in convs:
                assert op.flags & L.OPF_SPLIT3, (op.KH, op.KW, op.pad_t, op.pad_l, op.stride, op.Cin, op.Cout, nm)
                assert nm.startswith(("convx6_kernel", "pwx6_kernel")), nm
            assert not any(nm.startswith("conv_igemm_kernel") for nm in names)
            assert names[-1] == "embed_head_kernel" and ops[-1].kind == L.OP_EMBED_HEAD
            assert bool(ops[-1].flags & L.OPF_OUT_L2) == (D == 512)
            windows = {(op.KH, op.KW, op.pad_t, op.pad_l, op.stride) for op, _ in convs}
            assert {(3, 3, 0, 0, 1), (3, 3, 0, 0, 2), (1, 7, 0, 3, 1), (7, 1, 3, 0, 1), (1, 3, 0, 1, 1), (3, 1, 1, 0, 1)} <= windows


def _window_op(cin, cout, kh, kw, pt, pl, stride, H, W):
    """A CONV op carrying FP_OPF_SPLIT3 as PlanBuilder.conv emits it (no weights packed: the validator sees the offsets)."""
    OH, OW = (H + 2 * pt - kh) // stride + 1, (W + 2 * pl - kw) // stride + 1
    if OH <= 0 or OW <= 0:
        return None
    pb = PlanBuilder(2)
    x, out = pb.new_buf(H, W, cin).view(), pb.new_buf(OH, OW, cout).view()
    op = pb._base(L.OP_CONV, x, out, OH, OW)
    op.Cout, op.KH, op.KW, op.stride, op.pad_t, op.pad_l = cout, kh, kw, stride, pt, pl
    op.act, op.flags, op.w_off = L.ACT_RELU, op.flags | L.OPF_SPLIT3, 0
    return pb, x, out, op


def test_conv_splits_exactly_where_the_launcher_takes_it(lib, monkeypatch):
    """With x6_all, PlanBuilder.conv emits FP_OPF_SPLIT3 over a grid of windows, paddings, strides and widths exactly when
    fp_plan_validate (the launchers' eligibility, csrc/pwx6.hip) accepts the split op, and the fp32 form otherwise.  The
    weights are not packed here (their layouts are the parity tests' business): conv_weights is stubbed."""
    monkeypatch.setattr(PlanBuilder, "conv_weights", classmethod(lambda cls, *a: np.zeros(4, np.float32)))

    def emits_split(pb, x, out, cin, cout, kh, kw, stride, pad):
        pb.x6_all = True
        w = np.broadcast_to(np.float32(0), (cout, cin, kh, kw))
        pb.conv(x, w, out, stride=stride, pad=pad, act=L.ACT_RELU)
        return bool(pb.ops[-1].flags & L.OPF_SPLIT3)

    big = 1 << 40
    seen = {True: 0, False: 0}
    grid = itertools.product((32, 80, 128, 896), (32, 80, 96, 384), range(1, 9), range(1, 9), (1, 2), ((17, 17), (8, 8), (3, 3)))
    for cin, cout, kh, kw, stride, (H, W) in grid:
        if (kh > 7 or kw > 7) and (cin, cout, H) != (128, 96, 17):
            continue
        for pt in range(kh + 1):
            for pl in range(kw + 1):
                built = _window_op(cin, cout, kh, kw, pt, pl, stride, H, W)
                if built is None:
                    continue
                pb, x, out, op = built
                c_ok = lib.fp_plan_validate(ctypes.byref(op), 1, big, big) == 0
                assert emits_split(pb, x, out, cin, cout, kh, kw, stride, (pt, pl)) == c_ok, \
                    (cin, cout, kh, kw, pt, pl, stride, H, W, c_ok)
                if pt >= kh or pl >= kw or kh > 7 or kw > 7:
                    assert not c_ok
                seen[c_ok] += 1
    assert seen[True] > 1000 and seen[False] > 1000
    # maps beyond the split kernel's 16-bit window coordinates or 32-bit pixel offsets are refused by both, the largest maps
    # within them are taken by both
    for cin, kh, kw, pt, pl, stride, H, W, want in ((32, 1, 3, 0, 1, 1, 1, 33000, False), (32, 3, 1, 1, 0, 1, 33000, 1, False),
                                                    (16, 3, 3, 1, 1, 2, 2, 40000, False), (512, 1, 3, 0, 1, 1, 2048, 2048, False),
                                                    (32, 1, 3, 0, 1, 1, 1, 32767, True), (16, 3, 3, 1, 1, 2, 2, 32768, True),
                                                    (508, 1, 3, 0, 1, 1, 2048, 2048, True)):
        pb, x, out, op = _window_op(cin, 32, kh, kw, pt, pl, stride, H, W)
        assert (lib.fp_plan_validate(ctypes.byref(op), 1, big, big) == 0) == want, (cin, kh, kw, H, W)
        assert emits_split(pb, x, out, cin, 32, kh, kw, stride, (pt, pl)) == want, (cin, kh, kw, H, W)
    # input channels not a multiple of 4, and an input narrower than 32 under anything but a 3x3, are refused by both
    for cin, kh, kw in ((34, 3, 3), (30, 1, 7), (16, 1, 3), (4, 1, 1)):
        pb, x, out, op = _window_op(cin, 64, kh, kw, 0, 0, 1, 9, 9)
        x.buf.C = x.C = cin
        op.Cin = op.in_ld = cin
        op.in_ns = 81 * cin
        assert lib.fp_plan_validate(ctypes.byref(op), 1, big, big) != 0
        assert not emits_split(pb, x, out, cin, 64, kh, kw, 1, (0, 0))


def test_embed_head_validation(lib):
    pb = PlanBuilder(3)
    x, o = pb.new_buf(3, 3, 1792), pb.new_buf(1, 1, 128)
    pb.embed_head(x.view(), np.zeros((128, 1792), np.float32), o.view(0, 128), scale=np.ones(128), bias=np.zeros(128),
                  normalize=True)
    ops, w, arena = pb.finish()
    arr = (L.FpOp * 1)(*ops)
    assert lib.fp_plan_validate(arr, 1, w.size, arena) == 0
    assert lib.fp_op_kernel_name(ctypes.byref(arr[0])).decode() == "embed_head_kernel"
    assert lib.fp_plan_validate(arr, 1, 128 * 1792 - 1, arena) == L.FP_OK - 2          # the Linear weight ends behind the blob
    for field, v in (("act", L.ACT_RELU), ("res_mode", L.RES_ADD_AFTER_ACT), ("Cin", 1790), ("OH", 2)):
        bad = (L.FpOp * 1)(*ops)
        setattr(bad[0], field, v)
        assert lib.fp_plan_validate(bad, 1, w.size, arena) != 0, field
    bad = (L.FpOp * 1)(*ops)
    bad[0].kind = L.OP_CONV                                                             # FP_OPF_OUT_L2 belongs to the head only
    assert lib.fp_plan_validate(bad, 1, w.size, arena) != 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: single-op plans of the new windows

WINDOWS = [
    # cin, cout, kh, kw, pad, stride, (N, H, W), epilogue
    (32, 32, 3, 3, (0, 0), 1, (5, 79, 79), "relu"),          # conv2d_2a
    (80, 36, 3, 3, (0, 0), 1, (1, 9, 11), "relu"),           # unpadded 3x3, Cout not a multiple of 16, a partial channel slab
    (256, 84, 3, 3, (0, 0), 2, (5, 17, 17), "concat"),       # mixed_6a.branch0 form into a concat slice
    (192, 100, 3, 3, (0, 0), 2, (257, 8, 8), "relu"),        # mixed_7a: 8 x 8 -> 3 x 3, rows flattened over 257 images
    (128, 132, 1, 7, (0, 3), 1, (257, 8, 8), "concat"),      # Block17 branch1.1
    (128, 128, 7, 1, (3, 0), 1, (5, 8, 8), "residual"),      # Block17 branch1.2 with a residual-plus-ReLU epilogue
    (192, 196, 1, 3, (0, 1), 1, (257, 3, 3), "residual"),    # Block8 branch1.1
    (192, 192, 3, 1, (1, 0), 1, (1, 3, 3), "concat"),        # Block8 branch1.2
    (4, 32, 3, 3, (0, 0), 2, (5, 33, 33), "stem"),           # conv2d_1a: 3 channels in 4-float pixels, the flat form
]


def _run_window(dev, x6, cin, cout, kh, kw, pad, stride, shape, epi, seed):
    N, H, W = shape
    OH, OW = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
    rng = np.random.default_rng(seed)
    lc = 3 if epi == "stem" else cin
    x = rng.normal(0, 1, (N, lc, H, W)).astype(np.float32)
    w = rng.normal(0, (2.0 / (lc * kh * kw)) ** 0.5, (cout, lc, kh, kw)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    bias = rng.normal(0, 0.2, cout).astype(np.float32)
    r = rng.normal(0, 1, (N, cout, OH, OW)).astype(np.float32)
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        pb = PlanBuilder(N)
        pb.x6_all = True
        xb = pb.new_buf(H, W, lc)
        coff = 24 if epi == "concat" else 0
        ob = pb.new_buf(OH, OW, cout + (coff + 40 if epi == "concat" else 0))
        rb = pb.new_buf(OH, OW, cout)
        res = epi == "residual"
        pb.conv(xb.view(), w, ob.view(coff, cout), stride=stride, pad=pad, scale=scale, bias=bias, act=L.ACT_RELU,
                res=rb.view() if res else None, res_mode=L.RES_ADD_BEFORE_ACT if res else L.RES_NONE)
        plan = CompiledPlan(pb, dev)
    finally:
        PlanBuilder.X6 = saved
    name = plan.kernel_name(0)
    assert name.startswith("convx6_kernel") if x6 else not name.startswith(("convx6", "pwx6")), name
    xt = torch.zeros((N, H, W, xb.C), device=dev)
    xt[..., :lc] = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1)
    plan.buf_tensor(xb, N).copy_(xt)
    plan.buf_tensor(rb, N).copy_(torch.from_numpy(r).to(dev).permute(0, 2, 3, 1))
    out_t = plan.buf_tensor(ob, N)
    out_t.fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    full = out_t.permute(0, 3, 1, 2).cpu().numpy()
    got = full[:, coff:coff + cout]
    if epi == "concat":      # the channels around the slice are untouched
        assert np.isnan(full[:, :coff]).all() and np.isnan(full[:, coff + cout:]).all()
    v = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), stride=stride, padding=pad)
    v = v * torch.from_numpy(scale).double().view(1, -1, 1, 1) + torch.from_numpy(bias).double().view(1, -1, 1, 1)
    if res:
        v = v + torch.from_numpy(r).double()
    return got, torch.relu(v).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: f"{c[2]}x{c[3]}_p{c[4][0]}{c[4][1]}_s{c[5]}_{c[0]}to{c[1]}_{c[7]}")
def test_window_conv_vs_fp64(dev, case):
    cin, cout, kh, kw, pad, stride, shape, epi = case
    seed = cin * 7 + cout + 10 * kh + kw
    got6, want = _run_window(dev, True, cin, cout, kh, kw, pad, stride, shape, epi, seed)
    got32, _ = _run_window(dev, False, cin, cout, kh, kw, pad, stride, shape, epi, seed)
    assert np.isfinite(got6).all() and np.isfinite(got32).all()
    assert rel_err(got6, want) < 1e-5
    assert rel_err(got32, want) < 1e-5
    assert rel_err(got6, got32) < 5e-6


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [True, False])
def test_embed_head_vs_fp64(dev, normalize):
    N, C, D = 7, 1792, 128
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (N, 3, 3, C)).astype(np.float32)
    w = rng.normal(0, C ** -0.5, (D, C)).astype(np.float32)
    s, b = rng.uniform(0.5, 1.5, D).astype(np.float32), rng.normal(0, 0.1, D).astype(np.float32)
    pb = PlanBuilder(N)
    xb, ob = pb.new_buf(3, 3, C), pb.new_buf(1, 1, D)
    pb.embed_head(xb.view(), w, ob.view(0, D), scale=s, bias=b, normalize=normalize)
    plan = CompiledPlan(pb, dev)
    plan.buf_tensor(xb, N).copy_(torch.from_numpy(x).to(dev))
    plan.run()
    got = plan.buf_tensor(ob, N).reshape(N, D).cpu().numpy()
    want = torch.from_numpy(x).double().mean(dim=(1, 2)) @ torch.from_numpy(w).double().T
    want = want * torch.from_numpy(s).double() + torch.from_numpy(b).double()
    if normalize:
        want = F.normalize(want, dim=1)
    assert rel_err(got, want.numpy()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the whole network against the float64 oracle

@pytest.fixture(scope="module")
def nets(dev):
    out = {}
    for D, norm in ((128, False), (512, True)):
        sd = synth_sd(D, 40 + D)
        net = InceptionResnetV1(D, normalize=norm)
        net.load_state_dict(sd)
        out[D] = (net.to(dev), sd, norm)
    return out


def _check(got, ref, norm):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    if norm:
        assert err < 1e-4, err
    else:
        assert rel_err(got, ref) < 1e-4
    if len(ref) > 1:     # the rows are nearly parallel with random weights: the error must be small against what varies too
        assert err <= 1e-3 * np.abs(ref - ref.mean(axis=0)).max(), (err, np.abs(ref - ref.mean(axis=0)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [128, 512])
def test_network_vs_fp64_oracle(dev, nets, D):
    """Batches 1, 7, 64 against the oracle on every row; batch 1000 against it on 48 rows spread over the batch, and its
    rows bit-identical to the same crops run as batches of 7."""
    net, sd, norm = nets[D]
    for n in (1, 7, 64):
        x = seeded_input(n, 100 + n)
        got = net(torch.from_numpy(x)).cpu().numpy()
        assert got.shape == (n, D)
        _check(got, oracle_forward(sd, x, norm).numpy(), norm)
    x = seeded_input(1000, 7)
    got = net(torch.from_numpy(x)).cpu().numpy()
    rows = np.linspace(0, 999, 48).astype(int)
    _check(got[rows], oracle_forward(sd, x[rows], norm).numpy(), norm)
    for start in (0, 497, 993):
        small = net(torch.from_numpy(x[start:start + 7])).cpu().numpy()
        assert np.array_equal(small, got[start:start + 7]), start
