"""The generic fp32 plan ops of csrc/conv.hip, one op at a time, against float64 references and their write footprints.

conv_igemm_kernel<NB, VEC, PWD>, dwconv_kernel<KS>, dwconv3_row_kernel<S>, maxpool_kernel<K>, maxpool_generic_kernel,
upsample2x_kernel, copy_kernel, copy4_kernel and l2norm_kernel run whatever the specialised kernels refuse, and they are the
reference side of most "fused and unfused plans agree" tests.  Every case of tests/generic_op_cases.py is a one-op plan:

CPU (wherever the library is built): the case validates and lands on the kernel instance the table names; every feature
key with which the shipped networks reach these kernels (generic_op_cases.census) has a case; every instance has a case;
the fp64 bound is far below the activation bound the suite uses elsewhere.

GPU: the whole arena starts as a seeded finite pattern, everything the op must not read is NaN, the op runs once; inside
its footprint the result is compared with the reference (bit for bit for pool / upsample / copy, against the reference's own
fp32 error for conv / dwconv / l2norm), outside its footprint the arena is bit-identical to what it was.
"""
import numpy as np
import pytest
import torch

import generic_op_cases as G
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.plan import CompiledPlan, validate_on_host

CASES = G.cases()
IDS = [c.name for c in CASES]


def _ids(kind):
    return [c.name for c in G.cases_of(kind)]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_validates_and_lands_on_its_kernel(lib, case):
    """Every case builds, passes fp_plan_validate and gets exactly the kernel instance the table says (at full batch and at
    the batch of its partial run)."""
    pb, _ = G.build(case)
    assert validate_on_host(pb) == 0
    op = pb.ops[0]
    assert G.kernel_name(op) == case.kernel
    assert case.kernel.split("<")[0] in G.GENERIC
    if case.partial:
        assert 0 < case.partial < case.N
        op.N = case.partial
        assert G.kernel_name(op) == case.kernel
    if case.special == "neg":      # PReLU's negative branch in every channel
        pre = G.reference(case, G.inputs(case), torch.float64, pre=True)
        assert (pre.reshape(-1, pre.shape[-1]).min(axis=0)[:case.cout] < 0).all()


def test_census_cases_have_their_key(lib):
    """The case made for a census key has exactly that key."""
    for i, key in enumerate(G.CENSUS_KEYS):
        case = G.case_from_key(key, i)
        pb, _ = G.build(case)
        pb.finish()
        assert G.feature_key(pb.ops[0]) == key, (case.name, G.feature_key(pb.ops[0]), key)


def test_census_is_covered(lib):
    """Every feature key with which a shipped plan reaches a generic kernel is covered by a case with the same key.  A new
    network that sends a new combination (window, stride, padding, activation, residual mode, view shape ...) to a generic
    kernel fails here until generic_op_cases.CENSUS_KEYS (and, for a new edge, HAND) has a case for it."""
    have = set()
    for case in CASES:
        pb, _ = G.build(case)
        pb.finish()
        have.add(G.feature_key(pb.ops[0]))
    found = G.census()
    missing = {k: v for k, v in found.items() if k not in have}
    for k, v in sorted(missing.items(), key=str):
        print("uncovered:", k, "first seen in", v)
    assert not missing, f"{len(missing)} feature keys of the shipped plans have no case in tests/generic_op_cases.py"
    assert len(found) >= 80        # the census itself still sees the networks (89 keys when the table was written)


def test_every_instance_has_a_case(lib):
    """All twelve conv_igemm_kernel instances, dwconv_kernel<3|5|7>, dwconv3_row_kernel<1|2>, maxpool_kernel for K = 2, 3, 5,
    maxpool_generic_kernel, upsample2x_kernel, copy_kernel, copy4_kernel and l2norm_kernel each have at least one case.
    Every one of them is reachable with a plan that validates: <*, false, false> through an input view that is not 16-byte
    aligned (a hand-made 6-channel Buf), dwconv_kernel<3> through stride 3."""
    names = {c.kernel for c in CASES}
    want = {f"conv_igemm_kernel<{nb}, {v}, {p}>" for nb in (1, 2, 3, 4)
            for v, p in (("true", "true"), ("true", "false"), ("false", "false"))}
    want |= {"dwconv_kernel<3>", "dwconv_kernel<5>", "dwconv_kernel<7>", "dwconv3_row_kernel<1>", "dwconv3_row_kernel<2>",
             "maxpool_kernel", "maxpool_generic_kernel", "upsample2x_kernel", "copy_kernel", "copy4_kernel", "l2norm_kernel"}
    assert not want - names, sorted(want - names)
    pool_k = {c.k[0] for c in CASES if c.kernel == "maxpool_kernel"}      # the name does not carry K
    assert pool_k == {2, 3, 5}
    assert {c.k[0] for c in CASES if c.kernel == "maxpool_generic_kernel"} >= {4, 7, 9, 13}
    for kind in G.KINDS:           # a partial run for at least one case of every kind, and for a third of all cases
        assert any(c.partial for c in G.cases_of(kind)), kind
    assert 3 * sum(1 for c in CASES if c.partial) >= len(CASES), sum(1 for c in CASES if c.partial)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind not in G.EXACT_KINDS],
                         ids=[c.name for c in CASES if c.kind not in G.EXACT_KINDS])
def test_tolerance_is_not_vacuous(case):
    """2 * max|ref32 - ref64| + tol * max|ref64|, the bound of the GPU comparison, is below 1e-5 * max|ref64|, the
    activation bound the suite uses for these kernels elsewhere: the reference's own fp32 error does not swallow a defect."""
    data = G.inputs(case)
    r64 = G.reference(case, data, torch.float64)
    r32 = G.reference(case, data, torch.float32)
    ok = np.isfinite(r64)
    assert (np.isfinite(r32) == ok).all()
    scale = np.abs(r64[ok]).max()
    bound = 2.0 * np.abs(r32[ok] - r64[ok]).max() + G.tolerance(case) * scale
    print(f"{case.name}: bound {bound / scale:.2e} of scale")
    assert scale > 0 and bound < 1e-5 * scale


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _prepare(case, plan, bufs, data, dev, n):
    """Whole arena = seeded finite pattern; the input views = the case's data; NaN in everything the op must not read: the
    channels of the input and residual buffers outside the views, the floats between foreign-stride images, their images
    >= n, and the whole output footprint (an element the op fails to write stays NaN).  Channels of the input view whose weights are zero hold
    finite values, as include/facepath.h allows (channel padding, FP_OPF_IN_C3).  -> (arena int32 snapshot on the host)"""
    N = plan.N
    rng = np.random.default_rng(G.hash_name(case.name) % 1000 + 7)
    host = rng.uniform(-2.0, 2.0, plan.arena_floats).astype(np.float32)
    op = plan.ops[0]
    nan = np.float32("nan")
    for key, coff, vc in (("x", case.in_coff, case.C), ("res", case.res_coff, data["res"].shape[-1] if case.res else 0)):
        buf = bufs[key]
        if buf is None:
            continue
        host[buf.off: buf.off + N * buf.ns] = nan
        d = data[key][:n]
        host[G.input_index(case, buf, coff, vc, n, d.shape[1], d.shape[2])] = d
    host[G.footprint(op, N).reshape(-1)] = nan
    plan.arena.copy_(torch.from_numpy(host).to(dev))
    return host.view(np.int32).copy()


def _run_case(case, dev):
    pb, bufs = G.build(case)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == case.kernel
    data = G.inputs(case)
    r64 = G.reference(case, data, torch.float64)
    runs = {}
    for n in ([case.N, case.partial] if case.partial else [case.N]):
        before = _prepare(case, plan, bufs, data, dev, n)
        plan.run(n)
        torch.cuda.synchronize()
        after = plan.arena.cpu().numpy()
        idx = G.footprint(plan.ops[0], n)
        assert idx.min() >= 0 and idx.max() < plan.arena_floats
        assert np.unique(idx).size == idx.size
        got = after[idx]
        # outside the footprint: bit-identical (channel slices next door, pad pixels of a row-padded buffer, the other
        # parity of an out_cmul = 2 write, the floats between images, images >= n)
        mask = np.ones(plan.arena_floats, bool)
        mask[idx.reshape(-1)] = False
        a32 = after.view(np.int32)
        stray = np.nonzero(mask & (a32 != before))[0]
        assert stray.size == 0, f"{case.name} n={n}: {stray.size} floats written outside the footprint, first at {stray[:8]}"
        runs[n] = got
        want = r64[:n]
        assert got.shape == want.shape, (got.shape, want.shape)
        if case.kind in G.EXACT_KINDS:
            np.testing.assert_array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
            continue
        r32 = G.reference(case, data, torch.float32)[:n]
        fin = np.isfinite(want)
        assert (np.isfinite(got) == fin).all(), f"{case.name}: non-finite values differ from the reference's"
        if case.special == "zero_row":
            assert (~fin).sum() == case.C and np.isnan(got[~fin]).all()       # 0 / 0 on both sides
        else:
            assert fin.all()
        scale = np.abs(want[fin]).max()
        err, ref_err = np.abs(got[fin] - want[fin]).max(), np.abs(r32[fin] - want[fin]).max()
        print(f"{case.name} n={n}: err {err / scale:.2e}, fp32 reference {ref_err / scale:.2e} of scale {scale:.3g}")
        assert err <= 2.0 * ref_err + G.tolerance(case) * scale
        np.testing.assert_allclose(got[fin], want[fin], rtol=2e-5, atol=2e-5 * scale)
    if case.partial:      # images < n of the partial run equal the full run bit for bit
        np.testing.assert_array_equal(runs[case.partial].view(np.int32), runs[case.N][:case.partial].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("conv"))
def test_conv_vs_fp64(dev, name):
    """conv_igemm_kernel, all twelve instances: windows, strides, paddings, activations, residual modes, view shapes."""
    _run_case(next(c for c in CASES if c.name == name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("dwconv"))
def test_dwconv_vs_fp64(dev, name):
    """dwconv3_row_kernel<1|2> and dwconv_kernel<3|5|7>."""
    _run_case(next(c for c in CASES if c.name == name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("maxpool"))
def test_maxpool_bit_exact(dev, name):
    """maxpool_kernel<2|3|5> and maxpool_generic_kernel, bit for bit.  The inputs hold -inf and +inf; no NaN, and no window
    holding both +0.0 and -0.0 (the inputs are continuous random values: no zero at all) -- fmaxf leaves the result of those
    two unspecified where torch defines it."""
    _run_case(next(c for c in CASES if c.name == name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("upsample"))
def test_upsample2x_bit_exact(dev, name):
    _run_case(next(c for c in CASES if c.name == name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("copy"))
def test_copy_bit_exact(dev, name):
    """copy4_kernel (dense, slices, row-padded output: its pad pixels and pad rows are outside the footprint) and copy_kernel
    (out_cmul = 2 at both parities, unaligned views)."""
    _run_case(next(c for c in CASES if c.name == name), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids("l2norm"))
def test_l2norm_vs_fp64(dev, name):
    """l2norm_kernel on general views (off + n*ns + pix*ld + c): image strides other than H*W*ld on either side, maps, row
    pitches wider than D; an all-zero row is all NaN on both sides (no epsilon)."""
    _run_case(next(c for c in CASES if c.name == name), dev)
