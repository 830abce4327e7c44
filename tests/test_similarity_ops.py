"""The kernels behind the similarity filter (csrc/sim.hip: cosine_tile_kernel, cosine_x6_kernel<4 | 2>, cosine_finalize_kernel,
split3_rows_kernel, row_inv_norm_kernel, l2_mean_thres_kernel, l2_filter_kernel) against float64 references, at every row, with
write footprints and the tie rule.  Every case of tests/similarity_cases.py.

CPU (wherever the library is built): every filter case passes its entry point's argument checks;
fp_cosine_filter_x6_tile_rows -- the launcher's only gate -- reports what the table names, both tile sizes appear, and the gate
lies where the table says; the fp64 bound 2 * max|ref32 - ref64| + 2e-7 * scale (the filter's float32 reference in both
summation orders, similarity_cases' docstring) is below 1e-5 on every case, the reference
itself is sure of the argmax on at least 99.9 % of the rows and puts every planted tie at its lowest index; operands cut to two
bf16 pieces, a dropped K tail, a dropped column chunk and an inverse norm off by 4 ulp each move the float32 reference by more
than the bound on the cases named for them; and the filter protocol itself, run on the host against a stand-in that answers
with a float32 evaluation, passes -- and fails once the stand-in nudges one score by three bounds, returns the higher index of
a tie, writes one guard element, leaves one row unwritten or answers > for >= at tau.

GPU, filter (both entry points): best, arg, keep and packed carry 64 guard elements behind M and start as sentinels; after the call
the guards are unchanged and every element below M is written; for every row |best - max_j S64| and |best - S64[m, arg]| are within
the bound; arg is the float64 argmax wherever the float64 gap between the two best exceeds twice the bound (at least 99.9 % of
the rows) and the lowest index of every tied set exactly; keep == (best >= tau) bit for bit, true with tau at the bits of a
produced best[m], false one ulp above; a second run repeats the first bit for bit; the first 100 rows of (300, 131001, 32) run
alone land on the 128-row form and equal the same rows of the 300-row run; the x6 result's float64 error is at most twice the
fp32 kernel's + 1e-7; garbage in the padding rows of the planes changes nothing.  A zero gallery row gives NaN, -1, False, a
zero reference row never wins, an explicit rinv of 0 scores exactly 0 and is not excluded.
GPU, the other entry points: fp_split3_rows equals plan.split3_bf16 in the layout [D / 32][3][Npad][32] bit for bit over a
buffer prefilled with 0xFF, zero padding rows, h + m + l == x in float64; fp_row_inv_norm within the bound, +inf for a zero row;
fp_l2_mean_thres / fp_l2_filter: mean, thres and dist within the bound, every reference row kept, the farthest reference row's
dist has the bits of thres, keep == (dist <= thres), thres == 0 for identical rows; guards unchanged everywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

import similarity_cases as C
from face_detection_and_recognition_amd import _lib as L

F_IDS = [c.name for c in C.FILTER_CASES]
F_KEYS = {c.key: c for c in C.FILTER_CASES}          # one case per data set
SENT_BEST, SENT_ARG, SENT_KEEP, SENT_PACKED = 0x7FC0BEEF, -7, 0xAB, 0x5A5A5A5A5A5A5A5A
I32 = torch.int32


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the table, the gate, the bound, the mutants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.FILTER_CASES, ids=F_IDS)
def test_filter_case_passes_the_argument_checks(lib, case):
    """Nr, D and the alignment of a case are accepted (the checks run before the M == 0 return, so no device is needed); the x6
    entry point has a tile size for the case's M, and refuses a D that is no multiple of 32."""
    M, Nr, D = case.shape
    buf = torch.zeros(64)
    assert buf.data_ptr() % 16 == 0
    p = L.ptr(buf)
    fn = getattr(lib, case.entry)
    assert fn(p, p, 0, p, p, Nr, D, 0.0, p, p, p, p, None) == L.FP_OK
    if case.entry == C.FILTER_X6:
        assert lib.fp_cosine_filter_x6_tile_rows(M, Nr) in (128, 256)
    elif D % 32:
        assert lib.fp_cosine_filter_x6(p, p, 0, p, p, Nr, D, 0.0, p, p, p, p, None) != L.FP_OK
    assert fn(p, p, 0, p, p, 0, D, 0.0, p, p, p, p, None) == L.FP_ERR_INVALID_ARG
    assert fn(p, None, 0, p, p, Nr, D, 0.0, p, p, p, p, None) == L.FP_ERR_INVALID_ARG


def test_tile_rows_reports_what_the_table_names(lib):
    """fp_cosine_filter_x6_tile_rows on every x6 case; both tile sizes appear; the gate ceil(M / 256) * ceil(Nr / 128) >= 2048
    lies where the table says; 0 for what the launcher refuses."""
    tile = lib.fp_cosine_filter_x6_tile_rows
    x6 = [c for c in C.FILTER_CASES if c.entry == C.FILTER_X6]
    for c in x6:
        assert tile(c.shape[0], c.shape[1]) == c.tile_rows, c.name
        if c.sub_rows:
            assert tile(c.sub_rows, c.shape[1]) == 128 != c.tile_rows, c.name
    assert {c.tile_rows for c in x6} == {128, 256}
    big = {c.shape for c in x6 if c.tile_rows == 256}
    assert {(300, 131001, 32), (524033, 5, 32), (4196, 15400, 96)} <= big and (300, 130944, 32) not in big
    # (300, 131001): 2 row tiles x 1024 chunks.  130945 is the first Nr with 1024 chunks: one reference row fewer, or a chunk's
    # worth of columns fewer, and the 128-row form runs; so it does with one row tile
    assert (tile(300, 130945), tile(300, 130944), tile(300, 131001 - 128)) == (256, 128, 128)
    assert (tile(257, 131001), tile(256, 131001)) == (256, 128)
    assert (tile(524033, 5), tile(524032, 5), tile(524033, 129)) == (256, 128, 256)
    assert (tile(0, 5), tile(1, 1)) == (128, 128)
    assert (tile(-1, 5), tile(5, 0), tile(5, -3)) == (0, 0, 0)
    assert tile(1 << 40, 5) == 0 and tile((1 << 31) * 256 - 256, 1) == 256          # a grid of 2^31 workgroups is refused


@pytest.mark.parametrize("key", list(F_KEYS))
def test_filter_reference_is_sure_and_the_bound_is_tight(key):
    """The bound is below 1e-5 (it is below 2.2e-6, and below 1.1e-6 without a score of 1 at D = 512), the float64 reference is sure of the argmax (gap above twice the bound) on at
    least 99.9 % of the rows, the float32 reference agrees with it there, and every planted tie sits at its lowest index with a
    score of 1."""
    c = F_KEYS[key]
    r, bound, d = C.filter_references(c), C.filter_bound(c), C.filter_inputs(c)
    print(f"{key}: bound {bound:.3e}")
    assert C.TOL < bound < (2.2e-6 if key == "130x257x512_ties" else 1.1e-6) < 1e-5
    ok = ~np.isnan(r["best64"])
    sure = ok & (r["best64"] - r["second64"] > 2 * bound)
    assert sure.sum() >= 0.999 * ok.sum(), (int(sure.sum()), int(ok.sum()))
    np.testing.assert_array_equal(r["arg32"][sure], r["arg64"][sure])
    assert (~ok).sum() == (c.kind == "zero_rows") and np.array_equal(np.isnan(r["best32"]), ~ok)
    for m, j0, j1, label in d["ties"]:
        assert r["arg64"][m] == j0 and sure[m] and abs(r["best64"][m] - 1.0) < 1e-12, (m, j0, j1, label)
        assert j1 is None or (np.array_equal(d["R"][j0], d["R"][j1]) and j1 > j0)
    if c.kind == "ties":
        assert {t[3] for t in d["ties"]} == {t[0] for t in C.TIE_OFFSETS} | {"the last column alone"}
    if c.kind == "negative":
        b = r["best64"]
        assert (b < -0.05).any() and (b == 0).any() and (b > 0.05).any()
    if c.kind == "zero_rows":
        assert np.isnan(r["best64"][d["zero_g"]]) and r["arg64"][d["zero_g"]] == -1 and not (r["arg64"] == d["zero_r"]).any()


@pytest.mark.parametrize("label,mut,name", [(lab, mut, n) for lab, mut, names in C.MUTANTS for n in names],
                         ids=[f"{mut if isinstance(mut, str) else mut[0]}-{n}" for _, mut, names in C.MUTANTS for n in names])
def test_mutants_move_the_float32_reference(label, mut, name):
    c = C.BY_NAME[name]
    shift, bound = C.mutant_shift(c, mut), C.filter_bound(c)
    print(f"{name}: {label}: moves best by {shift:.3e}, bound {bound:.3e}")
    assert shift > bound, f"{name}: {label} moves the reference by {shift:.3e}, not above the bound {bound:.3e}"


def test_other_bounds_are_tight():
    """fp_row_inv_norm, fp_l2_mean_thres and fp_l2_filter: the bound is below 1e-5 of the scale on every case."""
    for c in C.INV_NORM_CASES:
        x = C.inv_norm_inputs(c)
        r64, r32 = C.inv_norm_reference(x, torch.float64), C.inv_norm_reference(x, torch.float32)
        assert C.bound_of(r32, r64) < 1e-5 * r64[np.isfinite(r64)].max(), c.name
        assert np.array_equal(np.isinf(r64), ~x.any(axis=1)) and np.isinf(r64).sum() == (c.shape[0] >= 3)
    for c in C.L2_CASES:
        d = C.l2_inputs(c)
        for a64, a32 in zip(C.l2_reference(d["ref"], d["E"], torch.float64), C.l2_reference(d["ref"], d["E"], torch.float32)):
            a64, a32 = np.atleast_1d(a64), np.atleast_1d(a32)
            assert C.bound_of(a32, a64) <= 1e-5 * np.abs(a64).max(), c.name
        if c.kind == "zero_rows":
            assert C.l2_reference(d["ref"], d["E"], torch.float32)[1] == 0 == C.l2_reference(d["ref"], d["E"], torch.float64)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the filter protocol (GPU tests; on the host against a stand-in)
# ---------------------------------------------------------------------------------------------------------------------------
class _Device:
    """The entry points of libfacepath on device tensors."""

    def __init__(self, dev):
        self.dev, self.lib = dev, L.load()

    def tile_rows(self, M, Nr):
        return self.lib.fp_cosine_filter_x6_tile_rows(M, Nr)

    def filter(self, c, T, M, tau):
        _, Nr, D = c.shape
        second = T["r3"] if c.entry == C.FILTER_X6 else T["R"]
        fn = getattr(self.lib, c.entry)
        L.check(fn(L.ptr(T["G"]), L.ptr(T["ginv"]), M, L.ptr(second), L.ptr(T["rinv"]), Nr, D, ctypes.c_float(tau), L.ptr(T["best"]),
                   L.ptr(T["arg"]), L.ptr(T["keep"]), L.ptr(T["packed"]), L.current_stream(self.dev)), c.entry)
        torch.cuda.synchronize()


class _Host:
    """A stand-in for the entry points on the host: the filter evaluated in float32, every score a plain sum over D (identical
    rows get identical bits, the first index wins) -- with one planted defect, if any."""

    def __init__(self, fault=None):
        self.dev, self.fault = torch.device("cpu"), fault

    def tile_rows(self, M, Nr):
        return L.load().fp_cosine_filter_x6_tile_rows(M, Nr)

    def filter(self, c, T, M, tau):
        G, R = T["G"][:M].numpy(), T["R"].numpy()
        with np.errstate(all="ignore"):
            S = (G[:, None, :] * R[None]).sum(-1, dtype=np.float32) / (np.linalg.norm(G, axis=1)[:, None] * np.linalg.norm(R, axis=1)[None])
        S[np.isnan(S)] = -np.inf
        arg = S.argmax(axis=1).astype(np.int32)
        best = S[np.arange(M), arg]
        none = np.isneginf(best)
        best, arg = np.where(none, np.float32("nan"), best).astype(np.float32), np.where(none, -1, arg).astype(np.int32)
        if self.fault == "nudge":
            best[np.flatnonzero(~none)[-1]] += np.float32(3.0 * C.filter_bound(c))
        if self.fault == "tie_high":
            m, _, j1, _ = next(t for t in C.filter_inputs(c)["ties"] if t[2] is not None and t[0] < M)
            arg[m] = j1
        with np.errstate(invalid="ignore"):
            keep = (best > np.float32(tau)) if self.fault == "gt" else (best >= np.float32(tau))
        rows = np.arange(M)
        if self.fault == "hole":
            rows = np.delete(rows, M // 2)
        idx = torch.from_numpy(rows)
        T["best"][idx] = torch.from_numpy(best)[idx]
        T["arg"][idx] = torch.from_numpy(arg)[idx]
        T["keep"][idx] = torch.from_numpy(keep.astype(np.uint8))[idx]
        T["packed"][idx] = idx
        if self.fault == "guard":
            T["arg"][M] = 3


def _filter_tensors(c, be):
    d = C.filter_inputs(c)
    M = c.shape[0]
    T = {k: torch.from_numpy(d[k].copy()).to(be.dev) for k in ("G", "R", "ginv", "rinv")}
    if c.entry == C.FILTER_X6:
        T["r3"] = torch.from_numpy(C.planes(d["R"]).view(np.int16)).to(be.dev)
    n = M + C.GUARD
    T["best"] = torch.empty(n, dtype=torch.float32, device=be.dev)
    T["arg"] = torch.empty(n, dtype=I32, device=be.dev)
    T["keep"] = torch.empty(n, dtype=torch.uint8, device=be.dev)
    T["packed"] = torch.empty(n, dtype=torch.int64, device=be.dev)
    return T


def _call(c, be, T, M, tau):
    """Sentinels into the four outputs, one call on the first M rows; the guards (everything behind M) unchanged, every element
    below M written -> {"best", "arg", "keep", "packed"} of the M rows as numpy."""
    T["best"].view(I32).fill_(SENT_BEST)
    T["arg"].fill_(SENT_ARG)
    T["keep"].fill_(SENT_KEEP)
    T["packed"].fill_(SENT_PACKED)
    be.filter(c, T, M, tau)
    out = {"best": T["best"].view(I32).cpu().numpy(), "arg": T["arg"].cpu().numpy(), "keep": T["keep"].cpu().numpy(),
           "packed": T["packed"].cpu().numpy()}
    for (k, v), sent in zip(out.items(), (SENT_BEST, SENT_ARG, SENT_KEEP, SENT_PACKED)):
        stray = np.flatnonzero(v[M:] != sent)
        assert stray.size == 0, f"{c.name} M={M}: {stray.size} guard elements of {k} written, first at {M + stray[:8]}"
        holes = np.flatnonzero(v[:M] == sent)
        assert holes.size == 0, f"{c.name} M={M}: {holes.size} elements of {k} not written, first at {holes[:8]}"
        out[k] = v[:M].copy()
    out["best"] = out["best"].view(np.float32)
    return out


def _keep_rule(c, got, tau, what):
    with np.errstate(invalid="ignore"):
        want = (got["best"] >= np.float32(tau)).astype(np.uint8)
    bad = np.flatnonzero(got["keep"] != want)
    assert bad.size == 0, f"{c.name} {what}: keep differs from best >= tau on {bad.size} rows, first {bad[:8]}"


def _same(c, a, b, what, keys=("best", "arg", "keep", "packed")):
    for k in keys:
        x, y = a[k], b[k]
        if k == "best":
            x, y = x.view(np.int32), y.view(np.int32)
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, f"{c.name}: {what}: {k} differs on {bad.size} rows, first {bad[:8]}"


def _error(c, got, M):
    """max |best - best64| over the rows with a score."""
    b64 = C.filter_references(c)["best64"][:M]
    ok = ~np.isnan(b64)
    return float(np.abs(got["best"][ok].astype(np.float64) - b64[ok]).max())


def _check_against_fp64(c, got, M, tau):
    """Scores, argmax, ties and keep of one result (module docstring) -> error / bound."""
    Nr = c.shape[1]
    r, bound, d = C.filter_references(c), C.filter_bound(c), C.filter_inputs(c)
    b64, a64, s64 = r["best64"][:M], r["arg64"][:M], r["second64"][:M]
    best, arg = got["best"], got["arg"]
    empty = np.isnan(b64)
    bad = np.flatnonzero(empty & ~(np.isnan(best) & (arg == -1) & (got["keep"] == 0)))
    assert bad.size == 0, f"{c.name}: rows without a valid score must give NaN, -1, False: {bad[:8]}"
    ok = np.flatnonzero(~empty)
    assert np.isfinite(best[ok]).all() and ((arg[ok] >= 0) & (arg[ok] < Nr)).all(), f"{c.name}: a best that is not finite or an arg outside [0, Nr)"
    err = np.abs(best[ok].astype(np.float64) - b64[ok])
    at = np.abs(best[ok].astype(np.float64) - C.score64(c, ok, arg[ok]))
    print(f"{c.name} M={M}: max |best - fp64| {err.max():.3e}, max |best - S64[m, arg]| {at.max():.3e}, bound {bound:.3e}, "
          f"ratio {max(err.max(), at.max()) / bound:.3f}")
    w = int(err.argmax())
    assert err.max() <= bound, f"{c.name}: |best - max_j S64| = {err.max():.3e} above the bound {bound:.3e} at row {ok[w]}"
    w = int(at.argmax())
    assert at.max() <= bound, f"{c.name}: |best - S64[m, arg]| = {at.max():.3e} above the bound {bound:.3e} at row {ok[w]}"
    for m, j0, j1, label in d["ties"]:
        if m < M:
            assert arg[m] == j0, f"{c.name}: tie {j0} / {j1} ({label}): row {m} reports {arg[m]}, not the lowest index"
    # every other row: a copied reference row (the j1 of a tie) ties with its original in EVERY gallery row and the reference
    # leaves it out, so a row whose best column has a copy is held to the lowest index here as well
    sure = np.flatnonzero(~empty & (b64 - s64 > 2 * bound))
    assert sure.size >= 0.999 * ok.size, f"{c.name}: the reference is sure of only {sure.size} of {ok.size} rows"
    bad = sure[arg[sure] != a64[sure]]
    assert bad.size == 0, (f"{c.name}: arg differs from the float64 argmax on {bad.size} rows with a clear gap, first "
                           f"{[(int(m), int(arg[m]), int(a64[m])) for m in bad[:6]]}")
    _keep_rule(c, got, tau, "first run")
    return max(err.max(), at.max()) / bound


def _run_filter_case(c, be):
    """The whole protocol of one filter case on a backend -> (first result, error / bound)."""
    M, Nr, D = c.shape
    x6 = c.entry == C.FILTER_X6
    if x6:
        assert be.tile_rows(M, Nr) == c.tile_rows
    T = _filter_tensors(c, be)
    b64 = C.filter_references(c)["best64"]
    tau = float(np.float32(np.nanmedian(b64)))
    got = _call(c, be, T, M, tau)
    ratio = _check_against_fp64(c, got, M, tau)
    _same(c, _call(c, be, T, M, tau), got, "the second run")
    # tau at the bits of one produced score, and one ulp above
    rows = np.flatnonzero(np.isfinite(got["best"]))
    m = int(rows[len(rows) // 2])
    for t, want in ((got["best"][m], 1), (np.nextafter(got["best"][m], np.float32(np.inf), dtype=np.float32), 0)):
        at = _call(c, be, T, M, float(t))
        _same(c, at, got, f"tau = {t!r}", keys=("best", "arg", "packed"))
        _keep_rule(c, at, t, f"tau = {t!r}")
        assert at["keep"][m] == want, f"{c.name}: keep[{m}] = {at['keep'][m]} with best = {got['best'][m]!r} and tau = {t!r}"
    if c.sub_rows:      # the first rows alone: the other tile form, the same bits
        assert be.tile_rows(c.sub_rows, Nr) == 128 != c.tile_rows
        sub = _call(c, be, T, c.sub_rows, tau)
        _same(c, sub, {k: v[:c.sub_rows] for k, v in got.items()}, f"the first {c.sub_rows} rows alone (128-row tiles)")
    if x6 and Nr % C.CHUNK:      # garbage in the padding rows of the planes
        T["r3"][:, :, Nr:] = -1
        _same(c, _call(c, be, T, M, tau), got, "0xFFFF in the padding rows of the planes")
    return got, ratio


HOST = ["f32_33x129x32_zero_rows", "f32_129x128x4_normal", "f32_130x257x512_ties", "x6_130x257x512_ties", "x6_70x2x64_negative",
        "f32_70x1x36_negative"]
FAULTS = [("f32_130x257x512_ties", "nudge", "above the bound"), ("x6_70x2x64_negative", "nudge", "above the bound"),
          ("f32_130x257x512_ties", "tie_high", "not the lowest index"), ("x6_130x257x512_ties", "tie_high", "not the lowest index"),
          ("f32_130x257x512_ties", "guard", "guard elements of arg written"), ("f32_33x129x32_zero_rows", "guard", "guard elements"),
          ("f32_130x257x512_ties", "hole", "not written"), ("x6_70x2x64_negative", "hole", "not written"),
          ("f32_130x257x512_ties", "gt", "keep"), ("f32_70x1x36_negative", "gt", "keep")]


@pytest.mark.parametrize("name", HOST)
def test_protocol_passes_the_float32_stand_in_on_the_host(lib, name):
    _run_filter_case(C.BY_NAME[name], _Host())


@pytest.mark.parametrize("name,fault,message", FAULTS, ids=[f"{n}-{f}" for n, f, _ in FAULTS])
def test_protocol_catches_a_fault_on_the_host(lib, name, fault, message):
    with pytest.raises(AssertionError, match=message):
        _run_filter_case(C.BY_NAME[name], _Host(fault))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_GOT = {}          # (data key, entry point) -> the first result of the protocol


def _result(c, dev):
    if (c.key, c.entry) not in _GOT:
        _GOT[c.key, c.entry] = _run_filter_case(c, _Device(dev))[0]
    return _GOT[c.key, c.entry]


@pytest.mark.gpu
@pytest.mark.parametrize("name", F_IDS)
def test_filter_vs_fp64(dev, name):
    """The whole protocol of the module docstring on one case; an x6 case is also held to the fp32 kernel's error on the same data."""
    c = C.BY_NAME[name]
    M = c.shape[0]
    got = _result(c, dev)
    if c.entry == C.FILTER_X6:
        twin = C.BY_NAME["f32_" + c.key]
        e6, e32 = _error(c, got, M), _error(twin, _result(twin, dev), M)
        print(f"{name}: x6 error {e6:.3e}, fp32 kernel error {e32:.3e}")
        assert e6 <= 2.0 * e32 + 1e-7, f"{name}: x6 error {e6:.3e} above 2 * {e32:.3e} + 1e-7"


@pytest.mark.gpu
def test_cosine_filter_zero_rows_and_masks(dev):
    """What similarity.cosine_filter's docstring says: a zero gallery row gives NaN, -1, False; a zero reference row never wins;
    an explicitly passed rinv of 0 scores exactly 0 and is NOT excluded (unlike cosine_topk's ginv)."""
    from face_detection_and_recognition_amd import similarity as sim
    c = C.BY_NAME["f32_130x257x512_zero_rows"]
    d = C.filter_inputs(c)
    G, R = torch.from_numpy(d["G"].copy()).to(dev), torch.from_numpy(d["R"].copy()).to(dev)
    for x6 in (False, True):
        best, arg, keep = (t.cpu().numpy() for t in sim.cosine_filter(G, R, -2.0, x6=x6))      # inverse norms from fp_row_inv_norm
        zg = d["zero_g"]
        assert np.isnan(best[zg]) and arg[zg] == -1 and not keep[zg]
        others = np.delete(np.arange(len(best)), zg)
        assert np.isfinite(best[others]).all() and keep[others].all() and not (arg == d["zero_r"]).any()
        np.testing.assert_array_equal(arg[others], C.filter_references(c)["arg64"][others])
    # Nr = 2, rinv[1] = 0: column 1 scores +-0 in every row and wins wherever column 0 is negative
    c = C.BY_NAME["x6_70x2x64_negative"]
    d = C.filter_inputs(c)
    G, R = torch.from_numpy(d["G"].copy()).to(dev), torch.from_numpy(d["R"].copy()).to(dev)
    rinv = torch.from_numpy(d["rinv"].copy()).to(dev)
    rinv[1] = 0.0
    col0 = C.score64(c, np.arange(70), np.zeros(70, np.int64))
    neg, pos = col0 < -1e-3, col0 > 1e-3
    assert neg.sum() >= 10 and pos.sum() >= 10
    for x6 in (False, True):
        best, arg, keep = (t.cpu().numpy() for t in sim.cosine_filter(G, R, 0.0, rinv=rinv, x6=x6))
        assert (best[neg] == 0).all() and (arg[neg] == 1).all() and keep[neg].all()
        assert (arg[pos] == 0).all() and np.abs(best[pos] - col0[pos]).max() <= C.filter_bound(c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.SPLIT3_CASES])
def test_split3_rows_is_exact(dev, name):
    c = C.BY_NAME[name]
    Nr, D = c.shape
    lib = L.load()
    R = C.split3_inputs(c)
    want = C.planes(R)
    nbytes = lib.fp_split3_bytes(Nr, D)
    assert nbytes == want.nbytes
    out = torch.full((nbytes + C.GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    Rd = torch.from_numpy(R.copy()).to(dev)
    L.check(lib.fp_split3_rows(L.ptr(Rd), Nr, D, L.ptr(out), L.current_stream(dev)), "fp_split3_rows")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[nbytes:] == 0xFF).all(), f"{name}: bytes behind the planes written"
    got = host[:nbytes].view(np.uint16).reshape(want.shape)
    assert not (got[:, :, Nr:] != 0).any(), f"{name}: padding rows are not zero"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{name}: {len(bad)} plane elements differ from plan.split3_bf16 (unwritten ones read 0xFFFF), first {bad[:4].tolist()}"
    pieces = (got[:, :, :Nr].astype(np.uint32) << 16).view(np.float32).astype(np.float64)       # [D / 32][3][Nr][32]
    np.testing.assert_array_equal(pieces.sum(axis=1).transpose(1, 0, 2).reshape(Nr, D), R.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.INV_NORM_CASES])
def test_row_inv_norm_vs_fp64(dev, name):
    c = C.BY_NAME[name]
    M, D = c.shape
    x = C.inv_norm_inputs(c)
    r64, r32 = C.inv_norm_reference(x, torch.float64), C.inv_norm_reference(x, torch.float32)
    bound = C.bound_of(r32, r64)
    out = torch.full((M + C.GUARD,), SENT_BEST, dtype=I32, device=dev)
    xd = torch.from_numpy(x.copy()).to(dev)
    L.check(L.load().fp_row_inv_norm(L.ptr(xd), M, D, L.ptr(out), L.current_stream(dev)), "fp_row_inv_norm")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[M:] == SENT_BEST).all() and not (host[:M] == SENT_BEST).any(), f"{name}: guards written or rows not written"
    got = host[:M].view(np.float32)
    zero = np.isinf(r64)
    assert np.array_equal(got[zero], np.full(zero.sum(), np.inf, np.float32)), f"{name}: a zero row must give +inf"
    err = np.abs(got[~zero].astype(np.float64) - r64[~zero]).max()
    print(f"{name}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{name}: err {err:.3e} above the bound {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.L2_CASES])
def test_l2_mean_thres_and_filter_vs_fp64(dev, name):
    c = C.BY_NAME[name]
    R, D = c.shape
    lib = L.load()
    d = C.l2_inputs(c)
    M = d["E"].shape[0]
    ref64, ref32 = C.l2_reference(d["ref"], d["E"], torch.float64), C.l2_reference(d["ref"], d["E"], torch.float32)
    refd, Ed = torch.from_numpy(d["ref"].copy()).to(dev), torch.from_numpy(d["E"].copy()).to(dev)
    mean = torch.full((D + C.GUARD,), SENT_BEST, dtype=I32, device=dev)
    thres = torch.full((1 + C.GUARD,), SENT_BEST, dtype=I32, device=dev)
    dist = torch.full((M + C.GUARD,), SENT_BEST, dtype=I32, device=dev)
    keep = torch.full((M + C.GUARD,), SENT_KEEP, dtype=torch.uint8, device=dev)
    s = L.current_stream(dev)
    L.check(lib.fp_l2_mean_thres(L.ptr(refd), R, D, L.ptr(mean), L.ptr(thres), s), "fp_l2_mean_thres")
    L.check(lib.fp_l2_filter(L.ptr(Ed), M, D, L.ptr(mean), L.ptr(thres), L.ptr(dist), L.ptr(keep), s), "fp_l2_filter")
    torch.cuda.synchronize()
    got = {}
    for k, t, n, sent in (("mean", mean, D, SENT_BEST), ("thres", thres, 1, SENT_BEST), ("dist", dist, M, SENT_BEST),
                          ("keep", keep, M, SENT_KEEP)):
        h = t.cpu().numpy()
        assert (h[n:] == sent).all(), f"{name}: guard elements of {k} written"
        assert not (h[:n] == sent).any(), f"{name}: elements of {k} not written"
        got[k] = h[:n] if k == "keep" else h[:n].view(np.float32)
    for k, a64, a32 in zip(("mean", "thres", "dist"), ref64, ref32):
        a64, a32 = np.atleast_1d(a64), np.atleast_1d(a32)
        bound, err = C.bound_of(a32, a64), np.abs(got[k].astype(np.float64) - a64).max()
        print(f"{name} {k}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound if bound else 0.0:.3f}")
        assert err <= bound, f"{name}: {k} err {err:.3e} above the bound {bound:.3e}"
    th = got["thres"][0]
    np.testing.assert_array_equal(got["keep"], (got["dist"] <= th).astype(np.uint8), err_msg=f"{name}: keep != (dist <= thres)")
    assert got["keep"][:R].all(), f"{name}: a reference row is not kept"
    far = int(np.argmax(np.sqrt(((d["ref"].astype(np.float64) - ref64[0][None]) ** 2).sum(1))))
    assert got["dist"][far].view(np.int32) == th.view(np.int32) and got["dist"][:R].max() == th, f"{name}: the farthest reference row's dist is not thres"
    if c.kind == "zero_rows":
        assert th == 0 and (got["dist"][:R] == 0).all() and not got["keep"][R:].any()
