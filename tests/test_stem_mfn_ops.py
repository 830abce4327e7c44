"""The stems (stem_conv_kernel, stem5_u8_band_kernel, stem5_u8_x6_kernel, stemdw_kernel) and the Mobile-FaceNet fp32 kernels
(dwpw_kernel in its Mobile-FaceNet forms, dwpw_wp_kernel, dwpw_persist_kernel, pws_kernel, dwblock_kernel), one op at a time,
against float64 references and their write footprints.  Every case of tests/stem_mfn_op_cases.py is a one-op plan.

CPU (wherever the library is built): the case validates and lands on the instance the table names; the size gates of the
launchers are where the table says (the batch just below a gate names the per-tile kernel); every instance the five launchers
can name has a case; every feature key with which the shipped networks reach these kernels has a case; the fp64 bound
2 * max|ref32 - ref64| + 2e-7 * scale is below 1e-5 of scale at the per-op figure, for the two- and three-stage fused ops as
well; wrong borders, pads, colours, slopes, shortcuts and phases each move the reference by more than the bound (under a row
window: inside the window's rows); and the GPU protocol itself, run on the host against a stand-in that computes the op with
the float32 oracle, passes -- and fails once the stand-in nudges one element by three bounds, writes one float just outside
the footprint or leaves one footprint element unwritten.

GPU: the whole arena starts as a seeded finite pattern; everything the op must not read is NaN (the fourth channel of the
4-float pixels, the floats between foreign-stride images, images >= n) and so is the output footprint; the op runs; inside its
footprint every element is finite and within the bound of float64, outside it the arena is bit-identical to what it was; a
second run repeats the first bit for bit.  Batch independence: image i of the N-image run equals its one-image run bit for bit
(the kernel name unchanged); on the size-gated instances the same plan on the images in reversed order gives the reversed
outputs bit for bit.  The u8 stems are held to the float64 conv of LUT[letterbox] with the letterbox of oracle/image_ref.py;
those on the fp32 MFMA also equal, bit for bit, the stand-alone letterbox followed by the fp32-image stem on the same weights,
the band kernel equals stem_conv_kernel<5, 1, true> (the same plan at 15 images), and a windowed run equals the window's rows
of the unwindowed one.
"""
import numpy as np
import pytest
import torch

import stem_mfn_op_cases as S
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import CompiledPlan, validate_on_host

CASES = S.cases()
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
CENSUS_FLOOR = 21          # 21 keys when the table was written
I32 = torch.int32


def _some(n):
    """The images a check visits: all of up to three, else the first, the middle and the last."""
    return list(range(n)) if n <= 3 else sorted({0, n // 2, n - 1})


def _subset(case, images):
    return {k: v[list(images)] for k, v in S.inputs(case).items()}


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_validates_and_lands_on_its_kernel(lib, case):
    """Every case builds through the public emitters, passes fp_plan_validate (with its row window) and gets exactly the instance
    the table names -- a kernel without a size gate at one image as well; its footprint lies inside the arena, away from the
    views it reads, and is exactly the output buffer where the op fills one (a row-padded buffer: all of it but the pads)."""
    pb, bufs = S.build(case)
    assert validate_on_host(pb) == 0
    ops, _, floats = pb.finish()
    op = ops[0]
    assert case.kernel in S.INSTANCES and S.kernel_name(op) == case.kernel
    assert (op.row_lo, op.row_end) == (case.window or (0, 0))
    assert bool(op.flags & L.OPF_SPLIT3) == case.x6 and bool(op.flags & L.OPF_OUT_ROWPAD) == case.rowpad
    if case.kind in ("stem", "stemdw"):
        assert op.flags & L.OPF_IN_C3
    if case.kind in ("dwpw", "dwblock"):
        assert (op.res_mode == L.RES_ADD_AFTER_ACT) == case.res and op.act == L.ACT_PRELU and op.act2 == L.ACT_NONE
    if case.kind == "dwpw":
        assert (op.bias_off >= 0) == case.out_slope
    if not case.gated:
        op.N = 1
        assert S.kernel_name(op) == case.kernel
        op.N = case.N
    idx = S.footprint(op)
    oh, ow = S.out_hw(case)
    rows = case.window[1] - case.window[0] if case.window else oh
    assert idx.shape == (case.N, rows, ow, S.out_C(case))
    flat = idx.reshape(-1)
    assert flat.min() >= 0 and flat.max() < floats
    if idx.size < (1 << 22):
        assert np.unique(flat).size == flat.size
        off, shape, strides = S.out_view(op)      # the strided form the GPU protocol uses is the same set
        view = np.lib.stride_tricks.as_strided(np.arange(floats, dtype=np.int64)[off:], shape, [8 * s for s in strides])
        assert np.array_equal(view, idx)
    ob = bufs["out"]
    if case.rowpad:        # every pixel of the buffer, none of its pads
        assert flat.min() == ob.off + (case.window[0] * (ow + 1) * ob.C if case.window else 0)
        px = (flat - ob.off) % ob.ns // ob.C
        assert (px % (ow + 1) < ow).all() and (px // (ow + 1) < oh).all()
    elif not case.out_ns_extra:
        assert flat.min() == ob.off and flat.max() == ob.off + case.N * ob.ns - 1 and flat.size == case.N * ob.ns
    else:                  # a foreign image stride: the floats between the images are not the op's
        assert ob.ns == oh * ow * 64 + case.out_ns_extra and op.out_ns == ob.ns and flat.size == case.N * oh * ow * 64
    for key in ("x", "res"):
        b = bufs[key]
        if b is not None and b is not ob:
            assert b.off + case.N * b.ns <= flat.min() or flat.max() < b.off, key
    if case.in_ns_extra:
        assert op.in_ns == 112 * 112 * 4 + case.in_ns_extra


def test_every_instance_has_a_case():
    """The set of instance names in the table equals the set the five launchers (fp_launch_stem / fp_launch_stem_u8,
    fp_launch_stemdw, fp_launch_dwpw, fp_launch_pws, fp_launch_dwblock) can name, written out here."""
    want = {
        "stem_conv_kernel<3, 1, false>", "stem_conv_kernel<3, 2, false>", "stem_conv_kernel<5, 1, false>",
        "stem_conv_kernel<5, 2, false>", "stem_conv_kernel<3, 1, true>", "stem_conv_kernel<3, 2, true>",
        "stem_conv_kernel<5, 1, true>", "stem_conv_kernel<5, 2, true>", "stem5_u8_band_kernel", "stem5_u8_x6_kernel",
        "stemdw_kernel<false>", "stemdw_kernel<true>",
        "dwpw_kernel<1, 1, 1>", "dwpw_kernel<1, 1, 2>", "dwpw_kernel<1, 2, 1>", "dwpw_kernel<1, 2, 2>", "dwpw_kernel<1, 4, 1>",
        "dwpw_kernel<1, 4, 2>", "dwpw_kernel<2, 1, 1>", "dwpw_kernel<2, 1, 2>", "dwpw_kernel<2, 2, 1>", "dwpw_kernel<2, 2, 2>",
        "dwpw_kernel<2, 4, 1>", "dwpw_kernel<2, 4, 2>", "dwpw_kernel<3, 1, 1>", "dwpw_kernel<3, 1, 2>", "dwpw_kernel<3, 2, 1>",
        "dwpw_kernel<3, 2, 2>", "dwpw_kernel<3, 4, 1>", "dwpw_kernel<3, 4, 2>", "dwpw_kernel<4, 1, 1>", "dwpw_kernel<4, 1, 2>",
        "dwpw_kernel<4, 2, 1>", "dwpw_kernel<4, 2, 2>", "dwpw_kernel<4, 4, 1>", "dwpw_kernel<4, 4, 2>",
        "dwpw_wp_kernel<2, 1, 4>", "dwpw_wp_kernel<2, 2, 4>", "dwpw_wp_kernel<4, 1, 4>",
        "dwpw_persist_kernel<4, 1>", "dwpw_persist_kernel<2, 1>", "dwpw_persist_kernel<2, 2>",
        "pws_kernel<64, 12>", "pws_kernel<128, 8>",
        "dwblock_kernel<128, 14, 14, 1>", "dwblock_kernel<128, 7, 7, 3>", "dwblock_kernel<64, 28, 7, 1>",
    }
    names = {c.kernel for c in S.HAND}
    assert names == want == S.INSTANCES, (sorted(want - names), sorted(names - want))
    # the forms and edges the table was written for
    dk = [c for c in S.HAND if c.kernel.startswith("dwpw_kernel")]
    assert any(c.res for c in dk) and any(c.out_slope for c in dk) and any(not c.res and not c.out_slope for c in dk)
    assert {c.act for c in S.HAND if c.kind == "pws"} == {"none", "relu", "prelu"}
    for kind in ("stem", "stem_u8"):
        cs = [c for c in S.HAND if c.kind == kind]
        assert {c.act for c in cs} == {"none", "relu", "prelu"} and {c.scale for c in cs} == {True, False}
    u8 = [c for c in S.HAND if c.kind == "stem_u8"]
    assert {c.swap_rb for c in u8} == {True, False} and all(c.pad_value != 0 for c in u8) and len({c.pad_value for c in u8}) > 2
    for fam in ("stem5_u8_band_kernel", "stem5_u8_x6_kernel"):
        cs = [c for c in S.HAND if c.kernel == fam]
        assert {c.window for c in cs} == {(), *S.WINDOWS} and {c.rowpad for c in cs if not c.window} == {True, False}
        assert {c.frame_hw for c in cs} == {S.LAND, S.PORT} and all(max(c.frame_hw) <= 40 and min(c.frame_hw) <= 24 for c in cs)
    assert S.WINDOWS[1][0] == 0 and S.WINDOWS[2][1] == 128 and 0 < S.WINDOWS[0][0] and S.WINDOWS[0][1] < 128
    for c in S.HAND:
        if c.kind == "dwblock":
            assert any(o.res != c.res and o.seed == c.seed for o in S.HAND)
    assert {c.N % 3 for c in S.HAND if c.kernel == "dwblock_kernel<128, 7, 7, 3>"} == {1, 2}      # a last tile of 1 and of 2 images


def test_tile_walks_run_past_the_first_round(lib):
    """The persistent kernels get more tiles than workgroups where the table says so, and ragged last tiles."""
    def tiles(name, per_image=None):
        c = BY_NAME[name]
        oh, ow = S.out_hw(c)
        return c.N * (per_image or -(-oh * ow // 128))
    assert tiles("st_k5_dense_n32_128") == 1024 > 768 and tiles("st_k3_dense_n42_112") == 1050 and (56 * 56) % 128 == 64
    assert tiles("u8_k5_800tiles_64x64") == 800 > 768
    assert tiles("sd_n38_532tiles", 14) == 532 > 512
    c = BY_NAME["wp_2_1_n126_28"]
    assert -(-c.N * 28 * 28 // 128) == 772 and (c.N * 28 * 28) % 128
    for name, nt in (("pers_4_1_n502_14", 769), ("pers_2_1_n384_16", 768), ("pers_2_2_n272_32", 544)):
        c = BY_NAME[name]
        oh, ow = S.out_hw(c)
        assert -(-c.N * (oh // 2) * (ow // 2) // 32) == nt > 512, name      # tiles of 32 2 x 2 patches on 512 workgroups
    c = BY_NAME["pws64_n126_28"]
    assert c.N * 28 * 28 // 32 == 3087 and 3087 % (12 * 256) == 15          # 15 row tiles in a second round
    for c in S.HAND:       # an OW that does not divide 128, and one small enough that a tile covers many rows
        if c.name in ("st_k3_nb2_rp_20x36", "st_k5_nb1_rp_20x36", "u8_k5_nb1_20x36_rp"):
            assert 128 % S.out_hw(c)[1]
    assert S.out_hw(BY_NAME["st_k3_nb1_rp_9x7"]) == (5, 4) and S.out_hw(BY_NAME["st_k5_nb2_rp_10x6"]) == (5, 3)


@pytest.mark.parametrize("name,below,lands", S.GATES, ids=[g[0] for g in S.GATES])
def test_size_gates(lib, name, below, lands):
    """The gated instances start where the table says: at `below` images the same op names the per-tile kernel, one image more
    names the gated one; every gated DWPW case runs at about 1.5 times its gate (dwpw_persist_kernel<2, 2>, whose arena would pass
    500 MB: just past one round of workgroups)."""
    case = BY_NAME[name]
    pb, _ = S.build(case)
    op = pb.finish()[0][0]
    op.N = below
    assert S.kernel_name(op).startswith(lands), S.kernel_name(op)
    op.N = below + 1
    assert S.kernel_name(op) == case.kernel
    assert case.gated and case.N >= below + 1
    if case.kind == "dwpw" and case.name != "pers_2_2_n272_32":
        assert 1.4 <= case.N / (below + 1) <= 1.6


def test_split_band_stem_has_no_small_batch_form(lib):
    """The split 5x5 stem exists in the band kernel only: the same op at 15 images names no kernel (BlazeFace emits the fp32
    form below 16 images, which lands on stem_conv_kernel<5, 1, true>: test_size_gates), and neither does a windowed op of
    either band kernel."""
    for name in ("x6_land_rp", "x6_port", "x6_port_rp_win_37_90", "band_port_rp_win_37_90"):
        pb, _ = S.build(BY_NAME[name])
        op = pb.finish()[0][0]
        op.N = 15
        assert S.kernel_name(op) == "?", name
        op.N = 16
        assert S.kernel_name(op) == BY_NAME[name].kernel


def test_pointwise_shapes_that_stay_on_the_generic_kernel(lib):
    """pws_kernel needs M = N H W >= 98304 in whole 32-row tiles: 125 x 28 x 28 (M = 98000) and 502 x 14 x 14 (M = 98392 = 3074
    tiles + 24 rows) stay on conv_igemm_kernel."""
    import dataclasses
    for base, n, hw in (("pws64_n126_28", 125, 28), ("pws64_n126_28", 502, 14), ("pws128_n1536_8", 502, 14)):
        pb, _ = S.build(dataclasses.replace(BY_NAME[base], N=n, H=hw, W=hw))
        assert S.kernel_name(pb.finish()[0][0]).startswith("conv_igemm_kernel"), (base, n, hw)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tolerance_is_not_vacuous(case):
    """The bound of the GPU comparison, 2 * max|ref32 - ref64| + tol * max|ref64|, is below 1e-5 * max|ref64| with tol the
    project's per-op figure, 2e-7 -- for the two- and three-stage fused ops too, so no case multiplies it by its stages."""
    assert S.TOL == 2e-7
    bound, scale = S.bound(case)
    print(f"{case.name}: {S.stages(case)} stage(s), bound {bound / scale:.2e} of scale {scale:.3g}")
    assert scale > 0 and bound < 1e-5 * scale


@pytest.mark.parametrize("case", S.HAND, ids=[c.name for c in S.HAND])
def test_mutants_are_caught(case):
    """The data of every hand-written case exercise its edges: the float64 reference of each wrong op of
    stem_mfn_op_cases.mutants differs from the true one by more than the case's bound -- under a row window inside the window's
    rows.  (On the first, middle and last image of the large batches: the bound is that of the whole case.)"""
    images = _some(case.N)
    data = _subset(case, images)
    bound, scale = S.bound(case)
    want = S.references(case)[0][images] if case.N <= 3 else S.reference(case, data, torch.float64)
    lo, end = case.window or (0, want.shape[1])
    muts = S.mutants(case)
    assert len(muts) >= (1 if case.kind in ("stem", "pws") else 2), muts
    for label, mut in muts:
        bad = S.reference(case, data, torch.float64, mut=mut)
        worst = np.abs(bad - want)[:, lo:end].max() / bound
        print(f"{case.name}: {label}: moves the reference by {worst:.3g} bounds")
        assert worst > 1.0, label


def test_census_cases_have_their_key(lib):
    """The case named for a census key is a hand-written one and has exactly that key."""
    for i, key in enumerate(S.CENSUS_KEYS):
        case = S.case_from_key(key, i)
        assert case is not None and case in S.HAND, key
        pb, _ = S.build(case)
        assert S.feature_key(pb.finish()[0][0]) == key, (case.name, key)


def test_census_is_covered(lib):
    """Every feature key with which a shipped plan reaches one of the kernels in scope -- the product plans, Mobile-FaceNet at
    the bench batches with the split kernels off, BlazeFace-back's row windows -- is in CENSUS_KEYS, and so has a case; the
    frozen copy holds nothing the plans no longer do.  A network that sends a new combination to these kernels fails here until
    the key and its case are added."""
    found = S.census()
    missing = {k: v for k, v in found.items() if k not in set(S.CENSUS_KEYS)}
    for k, v in sorted(missing.items(), key=str):
        print("uncovered:", k, "first seen in", v)
    assert not missing, (f"{len(missing)} feature keys of the shipped plans have no case in tests/stem_mfn_op_cases.py: " +
                         "; ".join(f"{k} first seen in {v}" for k, v in sorted(missing.items(), key=str)))
    assert set(found) == set(S.CENSUS_KEYS), sorted(set(S.CENSUS_KEYS) - set(found), key=str)
    assert len(found) >= CENSUS_FLOOR, len(found)      # the census itself still sees the networks
    seen = {k[0] for k in found}
    assert {"dwpw_persist_kernel<4, 1>", "pws_kernel<128, 8>", "dwblock_kernel<128, 7, 7, 3>"} <= seen      # the bench batches
    assert any(k[-1] for k in found), "no windowed stem in any plan"


# ---------------------------------------------------------------------------------------------------------------------------
# the protocol (GPU tests; on the host against a stand-in)
# ---------------------------------------------------------------------------------------------------------------------------
def _sync(plan):
    if plan.arena.is_cuda:
        torch.cuda.synchronize()


def _np_view(host, view):
    off, shape, strides = view
    return np.lib.stride_tricks.as_strided(host[off:], shape, [4 * s for s in strides])


def _prepare(case, plan, bufs, images, data=None):
    """Whole arena = seeded finite pattern; the input views of the first len(images) slots = those images of the case's data;
    NaN in everything the op must not read (the rest of the input buffers: the fourth channel of a 4-float pixel, the floats
    between foreign-stride images, the slots of images >= n) and in the whole output footprint of the plan's capacity."""
    N, n = plan.N, len(images)
    rng = np.random.default_rng(S.hash_name(case.name) % 1000 + 7)
    host = rng.random(plan.arena_floats, dtype=np.float32) * np.float32(4.0) - np.float32(2.0)
    nan = np.float32("nan")
    data = S.inputs(case) if data is None else data
    for key in ("x", "res"):
        buf = bufs.get(key)
        if buf is not None and key in data:
            host[buf.off: buf.off + N * buf.ns] = nan
            d = data[key][list(images)]
            _np_view(host, S.in_view(buf, n, d.shape[1], d.shape[2], d.shape[3]))[...] = d
    _np_view(host, S.out_view(plan.ops[0], N))[...] = nan
    plan.arena.copy_(torch.from_numpy(host))


def _run_once(case, plan, bufs, images, bind, data=None):
    """Prepare, bind, run on len(images) images; check the footprint, the arena outside it and the repeat
    -> the output [n, rows, OW, Cout] as numpy.  data: inputs other than the case's own."""
    n = len(images)
    _prepare(case, plan, bufs, images, data)
    before = plan.arena.clone()
    bind(list(images))
    plan.run(n)
    _sync(plan)
    after = plan.arena.clone()
    off, shape, strides = S.out_view(plan.ops[0], n)
    assert off >= 0 and off + sum((d - 1) * s for d, s in zip(shape, strides)) < plan.arena_floats
    changed = after.view(I32) != before.view(I32)
    changed.as_strided(shape, strides, off).fill_(False)
    stray = torch.nonzero(changed).reshape(-1)
    assert stray.numel() == 0, (f"{case.name} n={n}: {stray.numel()} floats written outside the footprint, first at "
                                f"{stray[:8].tolist()}")
    got = after.as_strided(shape, strides, off)
    holes = int((~torch.isfinite(got)).sum())
    assert holes == 0, f"{case.name} n={n}: {holes} footprint elements not written or not finite"
    plan.run(n)                                   # the same plan again: the same bits
    _sync(plan)
    assert torch.equal(plan.arena.view(I32), after.view(I32)), f"{case.name} n={n}: the second run differs from the first"
    return got.cpu().numpy()


def _same_bits(a, b, what):
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=what)


def _compare(case, got, want, w32, what):
    """Every element within 2 * the float32 reference's own error + TOL * scale of float64."""
    lo, end = case.window or (0, want.shape[1])
    want, w32 = want[:, lo:end], w32[:, lo:end]
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = np.abs(want).max()
    err, ref_err = np.abs(got - want).max(), np.abs(w32 - want).max()
    print(f"{case.name} {what}: err / scale {err / scale:.2e}, fp32 reference err / scale {ref_err / scale:.2e}, scale {scale:.3g}")
    assert err <= 2.0 * ref_err + S.TOL * scale, (f"{case.name} {what}: err {err / scale:.3e} of scale above the bound "
                                                  f"{(2.0 * ref_err + S.TOL * scale) / scale:.3e}")


def _run_case(case, plan, bufs, bind):
    """The whole protocol of one case on `plan` (a CompiledPlan, or the host stand-in) -> the full run's output."""
    assert plan.kernel_name(0) == case.kernel
    r64, r32 = S.references(case)
    N = case.N
    full = _run_once(case, plan, bufs, range(N), bind)
    _compare(case, full, r64, r32, f"n={N}")
    if case.gated:         # the same plan on the images in reversed order: the reversed outputs
        rev = _run_once(case, plan, bufs, range(N - 1, -1, -1), bind)
        _same_bits(rev, full[::-1], f"{case.name}: the images in reversed order")
    else:                  # image i of the N-image run == its one-image run, on the same kernel
        for i in _some(N):
            one = _run_once(case, plan, bufs, [i], bind)
            assert plan.kernel_name(0) == case.kernel
            _same_bits(one, full[i:i + 1], f"{case.name}: image {i} alone")
            if i == 0 and N > 1:
                _compare(case, one, r64[:1], r32[:1], "n=1")
    return full


class _HostPlan:
    """A stand-in for CompiledPlan on the host: run(n) computes the op with the float32 oracle on the images the protocol bound
    and writes the result into the footprint -- with one planted defect, if any."""

    def __init__(self, case, pb, fault=None):
        self.ops, _, self.arena_floats = pb.finish()
        self.N, self.case, self.fault, self.images = pb.N, case, fault, None
        self.arena = torch.zeros(self.arena_floats)

    def kernel_name(self, i):
        return S.kernel_name(self.ops[i])

    def bind(self, images):
        self.images = images

    def run(self, n):
        case, op = self.case, self.ops[0]
        op.N = n
        assert len(self.images) == n
        # one image at a time: torch's CPU conv blocks a batch by its size, and the protocol asks for batch independence
        out = np.concatenate([S.reference(case, _subset(case, [i]), torch.float32) for i in self.images])
        lo, end = case.window or (0, out.shape[1])
        out = out[:, lo:end].copy()
        off, shape, strides = S.out_view(op, n)
        if self.fault == "nudge":                # one element off by three times the bound
            out[-1, -1, 0, -1] += np.float32(3.0 * S.bound(case)[0])
        dst = self.arena.as_strided(shape, strides, off)
        hole = float(dst[0, 0, -1, 0])
        dst.copy_(torch.from_numpy(out))
        if self.fault == "hole":                 # one footprint element left as it was (NaN)
            dst[0, 0, -1, 0] = hole
        if self.fault == "stray":                # one float just behind the last footprint element
            last = off + sum((d - 1) * s for d, s in zip(shape, strides))
            self.arena[last + 1 if last + 1 < self.arena_floats else off - 1] = 3.0      # (or in front of its first one)
        if self.fault == "stray_row" and case.window:      # one float in the row in front of the window
            self.arena[off - 1 - (strides[1] - shape[2] * strides[2])] = 3.0


HOST = ["st_k3_nb2_rp_20x36", "u8_k3_nb1_18x10", "band_port_rp_win_90_128", "sd_n2_foreign_ns", "dk_nb1_p2_s2", "blk_128_7_n4_res"]
FAULTS = [(name, fault, msg) for name in HOST for fault, msg in (("nudge", "above the bound"), ("stray", "outside the footprint"),
                                                                 ("hole", "not written"))]
FAULTS.append(("band_port_rp_win_90_128", "stray_row", "outside the footprint"))


def _host_case(name, fault=None):
    case = BY_NAME[name]
    pb, bufs = S.build(case)
    plan = _HostPlan(case, pb, fault)
    return case, plan, bufs


@pytest.mark.parametrize("name", HOST)
def test_protocol_passes_the_oracle_on_the_host(lib, name):
    """The GPU protocol run on the CPU against a stand-in that computes the op with the float32 oracle passes ..."""
    case, plan, bufs = _host_case(name)
    _run_case(case, plan, bufs, plan.bind)


@pytest.mark.parametrize("name,fault,message", FAULTS, ids=[f"{n}-{f}" for n, f, _ in FAULTS])
def test_protocol_catches_a_fault_on_the_host(lib, name, fault, message):
    """... and the same stand-in with one planted defect is reported: one element nudged by three times the bound, one float
    written just outside the footprint (behind it: into a pad of a row-padded output, into the gap between foreign-stride
    images; in front of a row window), one footprint element left NaN."""
    case, plan, bufs = _host_case(name, fault)
    with pytest.raises(AssertionError, match=message):
        _run_case(case, plan, bufs, plan.bind)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_RESULTS = {}      # case name -> the full run's output (the unwindowed runs the windowed ones are compared with)


def _lut(dev):
    from oracle import image_ref
    return torch.from_numpy(image_ref.blaze_lut().copy()).to(dev)


def _gpu_case(case, dev):
    """(plan, bufs, bind) of a case on the device; a stem_u8 plan is bound to the images' frames."""
    pb, bufs = S.build(case)
    plan = CompiledPlan(pb, dev)
    if case.kind != "stem_u8":
        return plan, bufs, lambda images: None
    from face_detection_and_recognition_amd.modules.utils.image import bind_letterbox
    frames = torch.from_numpy(S.inputs(case)["frames"].copy()).to(dev)
    lut = _lut(dev)
    plan.frame_hw, plan.canvas_hw, plan.tables = tuple(case.frame_hw), (case.H, case.W), None

    def bind(images):
        bind_letterbox(plan, frames[images].contiguous(), lut, pad_value=case.pad_value, swap_rb=case.swap_rb)
    return plan, bufs, bind


def _result(case, dev):
    if case.name not in _RESULTS:
        plan, bufs, bind = _gpu_case(case, dev)
        full = _run_case(case, plan, bufs, bind)
        if case.kind != "stem_u8":
            return full
        _RESULTS[case.name] = full
    return _RESULTS[case.name]


def _names(*fams, kind=None, window=None):
    return [pytest.param(c.name, id=f"{c.name}:{c.kernel}") for c in CASES
            if c.kernel.split("<")[0] in fams and kind in (None, c.kind) and window in (None, bool(c.window))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stem_conv_kernel", kind="stem"))
def test_stem_conv_vs_fp64(dev, name):
    """stem_conv_kernel<3|5, 1|2, false>: row-padded outputs at any size (tiles of many rows, tiles that straddle rows, ragged
    last tiles), dense outputs past the size gate (a second tile per workgroup), none / ReLU / PReLU, with and without scale,
    pad 1 and pad 0; the fp32-image twins of the u8 cases."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stemdw_kernel"))
def test_stemdw_vs_fp64(dev, name):
    """stemdw_kernel<false|true>: one and three images, 532 tiles on 512 workgroups, image strides beyond the dense size (NaN
    between the input images, the floats between the output images untouched), weight gains 2^-20 and 2^20."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dwpw_kernel"))
def test_dwpw_mobile_facenet_forms_vs_fp64(dev, name):
    """dwpw_kernel<1..4, 1|2|4, 1|2> with a depthwise PReLU and no activation on the 1x1: plain, with the residual, with the
    output PReLU; Mobile-FaceNet's own maps and six-image maps whose tiles span images."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dwpw_wp_kernel", "dwpw_persist_kernel"))
def test_dwpw_persistent_vs_fp64(dev, name):
    """dwpw_wp_kernel<2, 1, 4>, <2, 2, 4>, <4, 1, 4> and dwpw_persist_kernel<4, 1>, <2, 1>, <2, 2> past their size gates: more
    tiles than workgroups, a ragged last tile."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("pws_kernel"))
def test_pws_vs_fp64(dev, name):
    """pws_kernel<64, 12> and <128, 8>: row tiles in a second round, one and four N tiles, none / ReLU / PReLU."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dwblock_kernel"))
def test_dwblock_fp32_vs_fp64(dev, name):
    """dwblock_kernel<128, 14, 14, 1>, <64, 28, 7, 1> and <128, 7, 7, 3> (a last tile of one and of two images), with and
    without the shortcut."""
    _result(BY_NAME[name], dev)


def _equals_letterbox_then_fp32_stem(case, full, dev):
    """The u8 stem == the stand-alone letterbox (letterbox_batch) followed by the fp32-image stem on the same weights."""
    from face_detection_and_recognition_amd.modules.utils.image import letterbox_batch
    twin = BY_NAME[case.name + "_f32"]
    frames = torch.from_numpy(S.inputs(case)["frames"].copy()).to(dev)
    canvas = torch.zeros((case.N, case.H, case.W, 4), device=dev)
    letterbox_batch(frames, (case.W, case.H), _lut(dev), canvas, pad_value=case.pad_value, swap_rb=case.swap_rb)
    torch.cuda.synchronize()
    canvas = canvas.cpu().numpy()
    assert float(np.abs(canvas[..., 3]).max()) == 0.0
    # the stand-alone letterbox is the oracle's (a disagreement at these small frame geometries is a finding of its own)
    np.testing.assert_array_equal(canvas[..., :3], S.canvas(case, S.inputs(case)["frames"]))
    pb, bufs = S.build(twin)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == twin.kernel
    want = _run_once(twin, plan, bufs, range(case.N), lambda images: None, data={"x": canvas[..., :3]})
    _same_bits(full, want, f"{case.name}: u8 against letterbox + fp32 stem")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stem_conv_kernel", kind="stem_u8"))
def test_stem_u8_vs_fp64_and_letterbox(dev, name):
    """stem_conv_kernel<3|5, 1|2, true>: landscape, portrait and square frames, every activation, three pad colours, R / B
    exchanged or not, 800 tiles on 768 workgroups (tile k + 1 staged while tile k computes)."""
    case = BY_NAME[name]
    _equals_letterbox_then_fp32_stem(case, _result(case, dev), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stem5_u8_band_kernel", window=False))
def test_stem_band_vs_fp64_letterbox_and_generic_kernel(dev, name):
    """stem5_u8_band_kernel, dense and row-padded: float64, letterbox + fp32 stem bit for bit, and stem_conv_kernel<5, 1, true>
    (the same plan at 15 images) bit for bit."""
    case = BY_NAME[name]
    full = _result(case, dev)
    _equals_letterbox_then_fp32_stem(case, full, dev)
    plan, bufs, bind = _gpu_case(case, dev)
    got = _run_once(case, plan, bufs, range(15), bind)
    assert plan.kernel_name(0) == "stem_conv_kernel<5, 1, true>"
    _same_bits(got, full[:15], f"{case.name}: the generic u8 kernel at 15 images")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stem5_u8_x6_kernel", window=False))
def test_stem_x6_vs_fp64(dev, name):
    """stem5_u8_x6_kernel, dense and row-padded, under the split kernels' bound."""
    _result(BY_NAME[name], dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("stem5_u8_band_kernel", "stem5_u8_x6_kernel", window=True))
def test_stem_band_row_window(dev, name):
    """Both band kernels under a row window in the interior, one that touches row 0 and one that touches row 127: the footprint
    is the window's rows, they are within the bound of float64 and equal the unwindowed run's rows bit for bit."""
    case = BY_NAME[name]
    got = _result(case, dev)
    whole = next(c for c in S.HAND if not c.window and c.seed == case.seed and c.x6 == case.x6)
    lo, end = case.window
    _same_bits(got, _result(whole, dev)[:, lo:end], f"{case.name}: the unwindowed run's rows")
