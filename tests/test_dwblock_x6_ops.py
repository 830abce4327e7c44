"""The whole-block Depth_Wise split kernels of csrc/dwblockx6.hip, one op at a time, against float64 and their write
footprints: every instance the launcher can pick -- dwblock_x6_kernel<128, 14> and <64, 28>, dwblock_x6q_kernel<7> (stride 1,
with and without the shortcut), dwblock_x6d_kernel<64, 128, 64, 56>, <64, 256, 128, 28> and <128, 512, 128, 14> (stride 2, no
shortcut; 28 -> 14 ends in a band of 2 output rows, 14 -> 7 in one of 3).

Every case is a one-op plan for three images (PlanBuilder.dwblock with the split form on).  The whole arena starts as a
seeded finite pattern; the input images the run must not read (images >= n) and the whole output buffer are NaN; the op runs.
Inside its footprint every element is compared with the float64 block under the bound tests/test_split_conv_ops.py uses for
split GEMMs (2 * the fp32 block's own error + 2e-7 of scale; every K here is <= 512, so the fp32 yardstick is torch's CPU
conv as in split_conv_cases.reference32); outside it the arena is bit-identical to what it was; a second run repeats the
first bit for bit; and image i of the three-image run -- where the XCD-aware tile order puts bands of different images side
by side -- equals the one-image run of that image bit for bit.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from generic_op_cases import hash_name, kernel_name
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import CompiledPlan, PlanBuilder, validate_on_host

N_IMAGES = 3
TOL = 2e-7           # the relative term of the split kernels' fp64 bound (generic_op_cases.tolerance: no SiLU here)

# name -> (instance, Cin, Cmid, Cout, H = W, stride)
SHAPES = {
    "s1_128_14": ("dwblock_x6_kernel<128, 14>", 128, 256, 128, 14, 1),
    "s1_64_28": ("dwblock_x6_kernel<64, 28>", 64, 128, 64, 28, 1),
    "s1_128_7": ("dwblock_x6q_kernel<7>", 128, 256, 128, 7, 1),
    "s2_64_56": ("dwblock_x6d_kernel<64, 128, 64, 56>", 64, 128, 64, 56, 2),
    "s2_64_28": ("dwblock_x6d_kernel<64, 256, 128, 28>", 64, 256, 128, 28, 2),
    "s2_128_14": ("dwblock_x6d_kernel<128, 512, 128, 14>", 128, 512, 128, 14, 2),
}
# (shape, shortcut): the stride-2 blocks of the network have none and the launcher takes none
CASES = [(name, res) for name, s in SHAPES.items() for res in ((True, False) if s[5] == 1 else (False,))]
IDS = [f"{name}_{'res' if res else 'nores'}" for name, res in CASES]


@functools.lru_cache(maxsize=None)
def _params(name):
    """Seeded parameters of a block in the shapes of the torch module: conv weights, (scale, bias) of each eval-mode
    BatchNorm, PReLU slopes."""
    _, cin, cmid, cout, _, _ = SHAPES[name]
    rng = np.random.default_rng(hash_name(name) % (2 ** 31))

    def aff(n):
        return rng.uniform(0.5, 1.5, n).astype(np.float32), rng.normal(0, 0.2, n).astype(np.float32)

    return dict(e_w=rng.normal(0, (2.0 / cin) ** 0.5, (cmid, cin, 1, 1)).astype(np.float32), e_aff=aff(cmid),
                e_slope=rng.uniform(0.1, 0.3, cmid).astype(np.float32),
                dw_w=rng.normal(0, (2.0 / 9) ** 0.5, (cmid, 1, 3, 3)).astype(np.float32), dw_aff=aff(cmid),
                dw_slope=rng.uniform(0.1, 0.3, cmid).astype(np.float32),
                pw_w=rng.normal(0, (2.0 / cmid) ** 0.5, (cout, cmid, 1, 1)).astype(np.float32), pw_aff=aff(cout))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    _, cin, _, _, hw, _ = SHAPES[name]
    rng = np.random.default_rng((hash_name(name) + 1) % (2 ** 31))
    x = rng.normal(0, 1, (N_IMAGES, hw, hw, cin)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(name, res, dt):
    """Depth_Wise.forward in dtype dt on the CPU -> (N, OH, OW, Cout) numpy, read-only."""
    stride = SHAPES[name][5]
    p = _params(name)

    def t(a):
        return torch.tensor(np.asarray(a), dtype=dt)

    def bn(v, aff):
        return v * t(aff[0]).view(1, -1, 1, 1) + t(aff[1]).view(1, -1, 1, 1)

    def prelu(v, slope):
        return torch.where(v > 0, v, v * t(slope).view(1, -1, 1, 1))

    x = t(_inputs(name)).permute(0, 3, 1, 2)
    with torch.no_grad():
        v = prelu(bn(F.conv2d(x, t(p["e_w"])), p["e_aff"]), p["e_slope"])
        v = prelu(bn(F.conv2d(v, t(p["dw_w"]), stride=stride, padding=1, groups=v.shape[1]), p["dw_aff"]), p["dw_slope"])
        v = bn(F.conv2d(v, t(p["pw_w"])), p["pw_aff"])
        if res:
            v = v + x
    out = np.ascontiguousarray(v.permute(0, 2, 3, 1).numpy())
    out.setflags(write=False)
    return out


def _build(name, res):
    """The one-op plan of a case -> (builder, input Buf, output Buf)."""
    _, cin, _, cout, hw, stride = SHAPES[name]
    p = _params(name)
    saved = PlanBuilder.X6
    PlanBuilder.X6 = True
    try:
        pb = PlanBuilder(N_IMAGES)
        xb = pb.new_buf(hw, hw, cin)
        ob = pb.new_buf(hw // stride, hw // stride, cout)
        got = pb.dwblock(xb.view(), p["e_w"], p["e_aff"], p["e_slope"], p["dw_w"], p["dw_aff"], p["dw_slope"], p["pw_w"],
                         p["pw_aff"], ob.view(), res, stride=stride, fp32=False)
    finally:
        PlanBuilder.X6 = saved
    assert got is not None and len(pb.ops) == 1
    return pb, xb, ob


def _footprint(op, n):
    """Arena indices [n, OH, OW, Cout] of every float the op may write when it runs on n images."""
    ni = np.arange(n, dtype=np.int64).reshape(-1, 1, 1, 1)
    pi = np.arange(op.OH * op.OW, dtype=np.int64).reshape(1, op.OH, op.OW, 1)
    ci = np.arange(op.Cout, dtype=np.int64).reshape(1, 1, 1, -1)
    return op.out_off + ni * op.out_ns + pi * op.out_ld + ci


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_validates_and_lands_on_its_kernel(lib, case):
    """Every case builds, passes fp_plan_validate, is a split op and gets exactly the instance the table names, at three
    images and at one."""
    name, res = case
    pb, xb, ob = _build(name, res)
    assert validate_on_host(pb) == 0
    op = pb.ops[0]
    assert op.kind == L.OP_DWBLOCK and op.flags & L.OPF_SPLIT3
    assert (op.res_mode == L.RES_ADD_AFTER_ACT) == res
    for n in (N_IMAGES, 1):
        op.N = n
        assert kernel_name(op) == SHAPES[name][0]
    # the buffers are disjoint and the footprint is the whole output buffer, nothing else
    idx = _footprint(op, N_IMAGES)
    assert idx.min() == ob.off and idx.max() == ob.off + N_IMAGES * ob.ns - 1 and idx.size == N_IMAGES * ob.ns
    assert xb.off + N_IMAGES * xb.ns <= ob.off or ob.off + N_IMAGES * ob.ns <= xb.off


def test_every_instance_has_a_case():
    """The six instantiations fp_launch_dwblock_x6 can pick; the stride-2 shapes whose last band is short are among them
    (14 output rows in bands of 4: the last has 2; 7 output rows: the last has 3)."""
    want = {"dwblock_x6_kernel<128, 14>", "dwblock_x6_kernel<64, 28>", "dwblock_x6q_kernel<7>",
            "dwblock_x6d_kernel<64, 128, 64, 56>", "dwblock_x6d_kernel<64, 256, 128, 28>",
            "dwblock_x6d_kernel<128, 512, 128, 14>"}
    assert {s[0] for s in SHAPES.values()} == want
    assert (SHAPES["s2_64_28"][4] // 2) % 4 == 2 and (SHAPES["s2_128_14"][4] // 2) % 4 == 3
    for name, s in SHAPES.items():
        if s[5] == 1:
            assert (name, True) in CASES and (name, False) in CASES


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tolerance_is_not_vacuous(case):
    """The bound of the GPU comparison is below 1e-5 of scale: the yardstick's own fp32 error does not swallow a defect."""
    r64, r32 = _reference(*case, torch.float64), _reference(*case, torch.float32)
    scale = np.abs(r64).max()
    bound = 2.0 * np.abs(r32 - r64).max() + TOL * scale
    print(f"{case[0]} res={case[1]}: bound {bound / scale:.2e} of scale {scale:.3g}")
    assert scale > 0 and bound < 1e-5 * scale


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _run(plan, xb, name, images, dev):
    """Seed the arena, put `images` (indices into the case's inputs) into the first image slots, NaN into the other input
    slots and the whole output buffer, run on len(images) images twice -> the output [n, OH, OW, Cout]."""
    n = len(images)
    op = plan.ops[0]
    rng = np.random.default_rng(hash_name(name) % 1000 + 7)
    host = rng.uniform(-2.0, 2.0, plan.arena_floats).astype(np.float32)
    x = _inputs(name)
    host[xb.off: xb.off + N_IMAGES * xb.ns] = np.float32("nan")
    host[xb.off: xb.off + n * xb.ns] = x[list(images)].reshape(-1)
    host[_footprint(op, N_IMAGES).reshape(-1)] = np.float32("nan")
    plan.arena.copy_(torch.from_numpy(host).to(dev))
    before = host.view(np.int32)
    plan.run(n)
    torch.cuda.synchronize()
    after = plan.arena.cpu().numpy()
    idx = _footprint(op, n)
    assert idx.min() >= 0 and idx.max() < plan.arena_floats
    mask = np.ones(plan.arena_floats, bool)
    mask[idx.reshape(-1)] = False
    stray = np.nonzero(mask & (after.view(np.int32) != before))[0]
    assert stray.size == 0, f"{name} n={n}: {stray.size} floats written outside the footprint, first at {stray[:8]}"
    plan.run(n)                                   # the same plan again: the same bits
    torch.cuda.synchronize()
    np.testing.assert_array_equal(plan.arena.cpu().numpy().view(np.int32), after.view(np.int32))
    return after[idx]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwblock_x6_vs_fp64(dev, case):
    name, res = case
    pb, xb, _ = _build(name, res)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == SHAPES[name][0]
    r64, r32 = _reference(name, res, torch.float64), _reference(name, res, torch.float32)
    full = _run(plan, xb, name, range(N_IMAGES), dev)
    runs = [(N_IMAGES, slice(None), full)]
    for i in range(N_IMAGES):
        one = _run(plan, xb, name, [i], dev)
        np.testing.assert_array_equal(one.view(np.int32), full[i:i + 1].view(np.int32))     # image i of N = 3 == its N = 1 run
        runs.append((1, slice(i, i + 1), one))
    for n, sl, got in runs[:2]:                   # N = 3 and N = 1 (the other one-image runs are the same bits as `full`)
        want, w32 = r64[sl], r32[sl]
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.isfinite(got).all(), f"{name} n={n}: {(~np.isfinite(got)).sum()} elements not written or not finite"
        scale = np.abs(want).max()
        err, ref_err = np.abs(got - want).max(), np.abs(w32 - want).max()
        print(f"{name} res={res} n={n}: err {err / scale:.2e}, fp32 reference {ref_err / scale:.2e} of scale {scale:.3g}")
        assert err <= 2.0 * ref_err + TOL * scale
