"""The fused kernels of a YOLOv5-face plan (ystem_kernel, ystem2_x6_kernel, shufdown_x6_kernel, shufunit_x6_kernel, dwpwx6_kernel
and the YOLOv5-face forms of dwpw_kernel), one op at a time, against float64 references and their write footprints.  Every case
of tests/yolo_op_cases.py is a one-op plan.

CPU (wherever the library is built): the case validates and lands on the instance the table names, at full batch and at one
image; every feature key with which the shipped networks reach these kernels has a case; every instance in scope has a case;
the fp64 bound is below 1e-5 of scale, its relative term derived per case from a perturbation of the first SiLU stage; a wrong
border tap, a wrong padding, a swapped interleave, a shifted pooling window and exchanged halves each move the reference by
more than the bound; the launchers refuse odd maps, aliased views and ineligible split ops.

GPU: the whole arena starts as a seeded finite pattern; everything the op must not read is NaN (the channels of the input
buffers outside their views, the floats between foreign-stride images, images >= n, the fourth channel of an FP_OPF_IN_C3
pixel) and so are the output footprints; the op runs; inside its footprints every element is compared with float64, outside
them the arena is bit-identical to what it was; a second run repeats the first bit for bit; a partial run equals the full
run's first images bit for bit; on the persistent tile kernels image i of the N-image run equals the one-image run of that
image bit for bit.  The u8 instances of ystem_kernel must equal, bit for bit, the fp32 instance fed the canvas of the
stand-alone letterbox (test_resize_normalize_vs_oracle pins that one); the fp32 instance with the same parameters and views
is itself one of the fp64 cases.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import yolo_op_cases as Y
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import CompiledPlan, PlanBuilder, validate_on_host

CASES = Y.cases()
IDS = [c.name for c in CASES]
F64 = [c for c in CASES if c.kind != "ystem_u8"]          # compared with float64 (the u8 cases: with their fp32 twin, bit for bit)
F64_IDS = [c.name for c in F64]
HAND64 = [c for c in Y.HAND if c.kind != "ystem_u8"]
CENSUS_FLOOR = 10
BIG = 1 << 40


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_validates_and_lands_on_its_kernel(lib, case):
    """Every case builds, passes fp_plan_validate and gets exactly the instance the table names, at N, at its partial batch
    and at one image; its footprints are disjoint from each other and from the views it reads."""
    pb, bufs = Y.build(case)
    assert validate_on_host(pb) == 0
    op = pb.ops[0]
    assert case.kernel.split("<")[0] in Y.FAMILIES
    if case.kind == "dwpw":
        assert bool(op.flags & L.OPF_SPLIT3) == case.x6 and op.act2 == Y.ACTS[case.act2] and op.res_mode == Y.RES[case.res]
    if case.kind == "ystem":
        assert bool(op.flags & L.OPF_IN_C3) == (case.cin == 3)
    if case.kind in ("ystem", "ystem_u8"):
        assert (op.scale_off < 0) == case.folded
    if case.partial:
        assert 0 < case.partial < case.N
    for n in (case.N, case.partial or case.N, 1):
        op.N = n
        assert Y.kernel_name(op) == case.kernel
    op.N = case.N
    fps = Y.footprints(op)
    flat = np.concatenate([f.reshape(-1) for f in fps.values()])
    assert flat.min() >= 0 and flat.max() < pb.finish()[2] and np.unique(flat).size == flat.size
    written = np.zeros(pb.finish()[2], bool)
    written[flat] = True
    for key, coff, ch in (("x", case.in_coff, Y.in_C(case)), ("res", case.res_coff, (Y.res_shape(case) or (0, 0, 0))[2])):
        buf = bufs[key]
        if buf is not None and not (key == "res" and case.kind in ("ystem", "ystem_u8")):
            assert not written[Y.input_index(case, buf, coff, ch, case.N, buf.H, buf.W)].any(), key


def test_census_cases_have_their_key(lib):
    """The case made for a census key has exactly that key."""
    for i, key in enumerate(Y.CENSUS_KEYS):
        case = Y.case_from_key(key, i)
        pb, _ = Y.build(case)
        pb.finish()
        assert Y.feature_key(pb.ops[0]) == key, (case.name, Y.feature_key(pb.ops[0]), key)


def test_census_is_covered(lib):
    """Every feature key with which a shipped plan reaches one of the kernels in scope is in yolo_op_cases.CENSUS_KEYS, and so
    has a case.  A network that sends a new combination (instance, epilogue, view shape, image stride ...) to them fails here
    until the key (and, for a new edge, a hand-written case) is added."""
    found = Y.census()
    missing = {k: v for k, v in found.items() if k not in set(Y.CENSUS_KEYS)}
    for k, v in sorted(missing.items(), key=str):
        print("uncovered:", k, "first seen in", v)
    assert not missing, (f"{len(missing)} feature keys of the shipped plans have no case in tests/yolo_op_cases.py: " +
                         "; ".join(f"{k} first seen in {v}" for k, v in sorted(missing.items(), key=str)))
    assert len(found) >= CENSUS_FLOOR, len(found)      # the census itself still sees the networks
    # the shipped forms the hand-written cases were modelled on are really there
    seen = {k[0] for k in found}
    assert {"ystem_kernel<1, false>", "ystem_kernel<1, true>", "ystem2_x6_kernel", "shufdown_x6_kernel<1, 64>",
            "shufunit_x6_kernel<64>", "dwpwx6_kernel<8, 4, 1>", "dwpwx6_kernel<8, 4, 2>"} <= seen, sorted(seen)


def test_every_instance_has_a_case():
    """Every instance in scope has a hand-written case, ystem_kernel<2, *> and dwpwx6_kernel<4, 4, *> (which no shipped plan
    reaches) included; every family runs a partial batch somewhere; the dwpw twins share their data."""
    names = {c.kernel for c in Y.HAND}
    assert names == Y.INSTANCES, (sorted(Y.INSTANCES - names), sorted(names - Y.INSTANCES))
    for fam in Y.FAMILIES:
        assert any(c.partial for c in Y.HAND if c.kernel.startswith(fam)), fam
    for kind in ("ystem", "ystem2", "shufdown", "shufunit", "dwpw"):
        assert any(c.in_ns_extra for c in Y.HAND if c.kind == kind), kind
    a, b = (next(c for c in Y.HAND if c.name == n) for n in ("dx_twin", "dk_twin"))
    assert a.x6 and not b.x6 and Y.params(a).keys() == Y.params(b).keys()
    assert all(np.array_equal(Y.params(a)[k], Y.params(b)[k]) for k in ("dw_w", "pw_w"))
    assert np.array_equal(Y.inputs(a)["x"], Y.inputs(b)["x"])
    # every u8 case has its fp32-canvas twin among the float64 cases, with the same parameters
    for c in CASES:
        if c.kind == "ystem_u8":
            t = next(t for t in F64 if t.name == c.name + "_f32")
            assert np.array_equal(Y.params(t)["w1"], Y.params(c)["w1"]) and np.array_equal(Y.params(t)["w2"], Y.params(c)["w2"])


def test_tile_walk_edges_are_exercised(lib):
    """The persistent kernels' tile walk at its edges: a grid that is no multiple of 8 (ystem_kernel's XCD-aware order with a
    remainder) and more tiles than the 512 workgroups, for each persistent kernel."""
    def tiles(name, th, tw):
        c = next(c for c in Y.HAND if c.name == name)
        oh, ow = Y.out_hw(c)
        return c.N * -(-oh // th) * -(-ow // tw)
    assert tiles("ys_13tiles_rgba", 8, 32) == 13 and tiles("ys_20x72_c16_rgba", 8, 32) == 20
    assert tiles("ys_520tiles", 8, 32) == 520 and tiles("y2_550tiles", 4, 16) == 550
    assert tiles("sd_550tiles", 4, 16) == 550 and tiles("su_522tiles", 8, 16) == 522


@pytest.mark.parametrize("case", F64, ids=F64_IDS)
def test_tolerance_is_not_vacuous(case):
    """The bound of the GPU comparison, 2 * max|ref32 - ref64| + tol * max|ref64|, is below 1e-5 * max|ref64| for every output;
    tol is one fp_silu stage's figure per stage where the second stage does not amplify the first one's error on this
    case's data (yolo_op_cases.propagation), else the propagated error plus the last stage's figure."""
    tol = Y.tolerances(case)
    if case.kind in Y.TWO_STAGE:
        prop = Y.propagation(case)
        print(f"{case.name}: a first-stage error of {Y.SILU_TOL:.0e} of scale moves the output by {prop:.2e} of scale")
        assert tol["out"] == (2 * Y.SILU_TOL if prop <= Y.SILU_TOL else prop + Y.SILU_TOL)
    else:
        assert tol["out"] == Y.SILU_TOL * Y.stages(case) or (Y.stages(case) == 0 and tol["out"] == Y.PLAIN_TOL)
    for key, (bound, scale) in Y.bounds(case).items():
        print(f"{case.name} {key}: tol {tol[key]:.2e}, bound {bound / scale:.2e} of scale {scale:.3g}")
        assert scale > 0 and bound < 1e-5 * scale


@pytest.mark.parametrize("case", HAND64, ids=[c.name for c in HAND64])
def test_mutants_are_caught(case):
    """The data of every hand-written case exercise its edges: the float64 reference with one border tap of a 3x3 stage
    zeroed, a stage's padding off by one, the shuffle interleave swapped, the pooling window shifted by one or x1 / x2
    exchanged differs from the true one by more than the case's bound, in at least one output."""
    want = Y.references(case)[0]
    bounds = Y.bounds(case)
    muts = Y.mutants(case)
    assert len(muts) >= (1 if Y.live_tap(case) is None else 2)
    for label, mut in muts:
        bad = Y.reference(case, Y.inputs(case), torch.float64, mut=mut)
        worst = max(np.abs(bad[k] - want[k]).max() / bounds[k][0] for k in want)
        print(f"{case.name}: {label}: moves the reference by {worst:.3g} bounds")
        assert worst > 1.0, label


def _rc(lib, op):
    return lib.fp_plan_validate(ctypes.byref(op), 1, BIG, BIG)


def _op_of(name, **kw):
    """A copy of the op of a hand-written case with some fields changed."""
    pb, _ = Y.build(next(c for c in Y.HAND if c.name == name))
    pb.finish()
    op = L.FpOp.from_buffer_copy(pb.ops[0])
    for k, v in kw.items():
        setattr(op, k, v)
    return op


def _refused(lib, op):
    return _rc(lib, op) != 0 and Y.kernel_name(op) == "?" and PlanBuilder.probe(op) is None


def test_launchers_refuse_maps_they_cannot_tile(lib):
    """shufdown / ystem2 need even H and W, ystem multiples of 4 (tests/test_host_logic.py test_shufflev2_block_ops_validation
    has shufdown's odd H)."""
    for name in ("sd_18x66", "y2_18x66"):
        assert _rc(lib, _op_of(name)) == 0
        assert _refused(lib, _op_of(name, W=65)) and _refused(lib, _op_of(name, W=67))
        assert _refused(lib, _op_of(name, H=17)) and _refused(lib, _op_of(name, H=19))
    assert _rc(lib, _op_of("ys_20x72_c16_rgba")) == 0
    for kw in (dict(H=18, OH=9), dict(H=22, OH=11), dict(W=70, OW=35), dict(W=74, OW=37), dict(H=21), dict(W=73)):
        assert _refused(lib, _op_of("ys_20x72_c16_rgba", **kw)), kw


def test_launchers_refuse_outputs_that_overlap_an_input(lib):
    """shufunit and ystem2 read their neighbours' pixels after a tile may have been written: an output view that shares a
    single float with an input view (fp_views_overlap) is refused, one that starts right behind it is taken
    (test_shufflev2_block_ops_validation has the views that coincide)."""
    op = _op_of("su_9x33_out192")
    last = (op.N - 1) * op.in_ns + (op.H * op.W - 1) * op.in_ld + op.Cin - 1            # the input view's last float
    assert _refused(lib, _op_of("su_9x33_out192", out_off=op.in_off + last - 3, out_ns=op.H * op.W * op.out_ld + 4))
    assert _rc(lib, _op_of("su_9x33_out192", out_off=op.in_off + last + 1, out_ns=op.H * op.W * op.out_ld + 4)) == 0
    first = op.out_off - ((op.N - 1) * op.in_ns + (op.H * op.W - 1) * op.in_ld + op.Cin)
    assert _refused(lib, _op_of("su_9x33_out192", in_off=first + 4)) and _rc(lib, _op_of("su_9x33_out192", in_off=first)) == 0
    op = _op_of("y2_18x66")
    ohw = op.OH * op.OW
    far = 1 << 30                                                                       # where the other input view goes
    for other, view_off, ns, ext in (("res_off", op.in_off, op.in_ns, (op.H * op.W - 1) * op.in_ld + op.Cin),
                                     ("in_off", op.res_off, op.res_ns, (ohw - 1) * op.res_ld + op.res_C)):
        end = view_off + (op.N - 1) * ns + ext                                          # one past the view's last float
        kw = {other: far, "out_ns": ohw * op.out_ld + 4}
        assert _refused(lib, _op_of("y2_18x66", out_off=end - 4, **kw))
        assert _rc(lib, _op_of("y2_18x66", out_off=end, **kw)) == 0


def test_split_dwpw_refusals(lib):
    """A DWPW with OW % 4 != 0, with a foreign output image stride or with 288 channels is not a split op; without the flag,
    where the fp32 launcher's own limits allow it, the same op names a dwpw_kernel instance."""
    base = _op_of("dx_n9_4x4_shuffle")
    assert _rc(lib, base) == 0

    def width(w):      # the same op on a 4 x w map at stride 1, every image stride following
        return dict(W=w, OW=w, in_ns=4 * w * base.in_ld, out_ns=4 * w * base.out_ld, res_ns=4 * w * base.res_ld, res_W=w)
    assert _rc(lib, _op_of("dx_n9_4x4_shuffle", **width(8))) == 0
    for w, p in ((6, 2), (5, 1)):
        assert _refused(lib, _op_of("dx_n9_4x4_shuffle", **width(w)))
        op = _op_of("dx_n9_4x4_shuffle", flags=0, **width(w))
        assert _rc(lib, op) == 0 and Y.kernel_name(op) == f"dwpw_kernel<4, {p}, 1>"
    foreign = dict(out_ns=base.out_ns + 64)
    assert _refused(lib, _op_of("dx_n9_4x4_shuffle", **foreign))
    assert _refused(lib, _op_of("dx_n9_4x4_shuffle", flags=0, **foreign))      # the fp32 kernel's tiles are flat as well
    wide = dict(Cin=288, in_ld=288, in_ns=base.H * base.W * 288)
    assert _refused(lib, _op_of("dx_n9_4x4_shuffle", **wide))
    assert _refused(lib, _op_of("dx_n9_4x4_shuffle", flags=0, **wide))         # 288 is no multiple of the fp32 kernel's 64
    wide = dict(Cin=320, in_ld=320, in_ns=base.H * base.W * 320)               # beyond the split kernel's 256, fine for fp32
    assert _refused(lib, _op_of("dx_n9_4x4_shuffle", **wide))
    assert Y.kernel_name(_op_of("dx_n9_4x4_shuffle", flags=0, **wide)) == "dwpw_kernel<4, 4, 1>"
    # the builder follows the launcher: the same emitter call on a 4 x 6 map gives the fp32 op
    case = next(c for c in Y.HAND if c.name == "dk_nb4_p2_s1_shuffle")
    saved = PlanBuilder.X6
    PlanBuilder.X6 = True
    try:
        pb, _ = Y.build(dataclasses.replace(case, x6=True))
    finally:
        PlanBuilder.X6 = saved
    assert not pb.ops[0].flags & L.OPF_SPLIT3 and Y.kernel_name(pb.ops[0]) == case.kernel


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _prepare(case, plan, bufs, data, dev, images):
    """Whole arena = seeded finite pattern; the input views of the first len(images) slots = those images of the case's data;
    NaN in everything the op must not read and in the whole output footprints (module docstring).  -> the arena as int32 on
    the host"""
    N, n = plan.N, len(images)
    rng = np.random.default_rng(Y.hash_name(case.name) % 1000 + 7)
    host = rng.uniform(-2.0, 2.0, plan.arena_floats).astype(np.float32)
    op = plan.ops[0]
    nan = np.float32("nan")
    views = [("x", case.in_coff, Y.in_C(case))] if "x" in data else []
    if "res" in data:
        views.append(("res", case.res_coff, data["res"].shape[-1]))
    for key, coff, vc in views:
        buf = bufs[key]
        host[buf.off: buf.off + N * buf.ns] = nan
        d = data[key][list(images)].copy()
        if key == "x" and op.flags & L.OPF_IN_C3:
            d[..., 3] = nan                        # include/facepath.h: any value in the fourth channel
        host[Y.input_index(case, buf, coff, vc, n, d.shape[1], d.shape[2])] = d
    for idx in Y.footprints(op, N).values():
        host[idx.reshape(-1)] = nan
    plan.arena.copy_(torch.from_numpy(host).to(dev))
    return host.view(np.int32)


def _run_once(case, plan, bufs, data, dev, images, bind=None):
    """Prepare, run on len(images) images, check the arena outside the footprints and the repeat -> {output: [n, h, w, c]}."""
    n = len(images)
    before = _prepare(case, plan, bufs, data, dev, images)
    if bind is not None:
        bind(images)
    plan.run(n)
    torch.cuda.synchronize()
    after = plan.arena.cpu().numpy()
    fps = Y.footprints(plan.ops[0], n)
    mask = np.ones(plan.arena_floats, bool)
    size = 0
    for idx in fps.values():
        assert idx.min() >= 0 and idx.max() < plan.arena_floats
        mask[idx.reshape(-1)] = False
        size += idx.size
    assert plan.arena_floats - np.count_nonzero(mask) == size          # no index twice
    # outside the footprints: bit-identical (channel slices next door, the floats between images, images >= n, every other buffer)
    stray = np.nonzero(mask & (after.view(np.int32) != before))[0]
    assert stray.size == 0, f"{case.name} n={n}: {stray.size} floats written outside the footprint, first at {stray[:8]}"
    plan.run(n)                                                        # the same plan again: the same bits
    torch.cuda.synchronize()
    np.testing.assert_array_equal(plan.arena.cpu().numpy().view(np.int32), after.view(np.int32))
    got = {k: after[idx] for k, idx in fps.items()}
    for k, g in got.items():
        assert np.isfinite(g).all(), f"{case.name} n={n} {k}: {(~np.isfinite(g)).sum()} elements not written or not finite"
    return got


def _same_bits(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=f"{what}: {k}")


def _image_runs(case, plan, bufs, data, dev, full, bind=None):
    """Image i of the N-image run equals the one-image run of that image bit for bit (every image on small arenas, the first,
    the middle and the last on large ones)."""
    N = case.N
    picks = range(N) if plan.arena_floats <= (1 << 21) else sorted({0, N // 2, N - 1})
    for i in picks:
        one = _run_once(case, plan, bufs, data, dev, [i], bind)
        _same_bits(one, {k: v[i:i + 1] for k, v in full.items()}, f"{case.name}: image {i} alone")


def _run_case(case, dev):
    pb, bufs = Y.build(case)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == case.kernel
    data = Y.inputs(case)
    r64, r32 = Y.references(case)
    tol = Y.tolerances(case)
    runs = {}
    for n in ([case.N, case.partial] if case.partial else [case.N]):
        got = runs[n] = _run_once(case, plan, bufs, data, dev, range(n))
        for k, g in got.items():
            want, w32 = r64[k][:n], r32[k][:n]
            assert g.shape == want.shape, (k, g.shape, want.shape)
            scale = np.abs(want).max()
            err, ref_err = np.abs(g - want).max(), np.abs(w32 - want).max()
            print(f"{case.name} n={n} {k}: err {err / scale:.2e}, fp32 reference {ref_err / scale:.2e} of scale {scale:.3g}, "
                  f"tol {tol[k]:.1e}")
            assert err <= 2.0 * ref_err + tol[k] * scale, (k, err / scale)
            np.testing.assert_allclose(g, want, rtol=2e-5, atol=2e-5 * scale)
    if case.partial:      # images < n of the partial run equal the full run bit for bit
        _same_bits(runs[case.partial], {k: v[:case.partial] for k, v in runs[case.N].items()}, f"{case.name}: partial run")
    if case.kind == "shufunit":      # the x1 half passes through: the even channels are the input's first 64, bit for bit
        np.testing.assert_array_equal(runs[case.N]["out"][..., 0::2].view(np.int32), data["x"][..., :64].view(np.int32))
    if case.kind in Y.PERSISTENT:
        _image_runs(case, plan, bufs, data, dev, runs[case.N])


def _names(fam, u8=False):
    """The cases of a kernel family as parameters whose ids name the case and the instance it runs on."""
    return [pytest.param(c.name, id=f"{c.name}:{c.kernel}") for c in CASES
            if c.kernel.startswith(fam) and (c.kind == "ystem_u8") == u8]


def _case(name):
    return next(c for c in CASES if c.name == name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("ystem_kernel"))
def test_ystem_vs_fp64(dev, name):
    """ystem_kernel<1|2, false>: stem_2a's output and the pooled stem_1 map, tiles and seams, the tile walk, every width,
    3- and 4-channel images, folded BatchNorms, sliced and foreign-stride views."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("ystem2_x6_kernel"))
def test_ystem2_vs_fp64(dev, name):
    """ystem2_x6_kernel: 1 x 1 output, one exact tile, seams and ragged edges, more tiles than workgroups, three sliced views."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("shufdown_x6_kernel"))
def test_shufdown_vs_fp64(dev, name):
    """shufdown_x6_kernel<1, 64>: both branches interleaved, the same map ladder, in_ld 40 and out_ld 160."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("shufunit_x6_kernel"))
def test_shufunit_vs_fp64(dev, name):
    """shufunit_x6_kernel<64>: the x1 half bit for bit, branch 2 against float64, concat buffers of 192 and 256 channels."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dwpwx6_kernel"))
def test_dwpwx6_vs_fp64(dev, name):
    """dwpwx6_kernel<4|8, 4, 1|2>: tiles that span images, clamped tail groups, every epilogue, sliced views."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dwpw_kernel"))
def test_dwpw_yolo_forms_vs_fp64(dev, name):
    """dwpw_kernel<2|4, 1|2|4, 1|2> with SiLU on the 1x1, with and without the ShuffleV2 interleave."""
    _run_case(_case(name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("ystem_kernel", u8=True))
def test_ystem_u8_equals_fp32_on_the_letterbox_canvas(dev, name):
    """ystem_kernel<1|2, true> resamples the canvas from the u8 frames while it stages a tile: both outputs equal, bit for bit,
    those of the fp32 instance (same parameters, same views: one of the float64 cases above) on the canvas letterbox_batch
    makes of the same frames; same footprint, NaN, repeat, partial-run and single-image checks."""
    from face_detection_and_recognition_amd.modules.utils.image import bind_letterbox, letterbox_batch
    case = _case(name)
    twin = _case(name + "_f32")
    frames = torch.from_numpy(Y.inputs(case)["frames"].copy()).to(dev)
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)
    canvas = torch.zeros((case.N, case.H, case.W, 4), device=dev)
    letterbox_batch(frames, (case.W, case.H), lut, canvas, pad_value=125, swap_rb=case.swap_rb)
    torch.cuda.synchronize()
    canvas = canvas.cpu().numpy()
    assert float(np.abs(canvas[..., 3]).max()) == 0.0 and len(np.unique(canvas[..., :3])) > 16
    tpb, tbufs = Y.build(twin)
    tplan = CompiledPlan(tpb, dev)
    assert tplan.kernel_name(0) == twin.kernel
    want = _run_once(twin, tplan, tbufs, {"x": canvas}, dev, range(case.N))

    pb, bufs = Y.build(case)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == case.kernel
    plan.frame_hw, plan.canvas_hw, plan.tables = tuple(case.frame_hw), (case.H, case.W), None

    def bind(images):
        bind_letterbox(plan, frames[list(images)].contiguous(), lut, pad_value=125, swap_rb=case.swap_rb)
    full = _run_once(case, plan, bufs, {}, dev, range(case.N), bind)
    _same_bits(full, want, f"{case.name}: u8 against the fp32 canvas")
    if case.partial:
        part = _run_once(case, plan, bufs, {}, dev, range(case.partial), bind)
        _same_bits(part, {k: v[:case.partial] for k, v in full.items()}, f"{case.name}: partial run")
    _image_runs(case, plan, bufs, {}, dev, full, bind)
