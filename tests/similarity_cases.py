"""Case table, float64 references, bounds and mutants for the kernels behind the similarity filter (csrc/sim.hip):

  fp_cosine_filter        -> cosine_tile_kernel (fp32 MFMA, 128 x 128 tiles, K chunks of 32) + cosine_finalize_kernel
  fp_cosine_filter_x6     -> cosine_x6_kernel<4> (256-row tiles) | cosine_x6_kernel<2> (128-row tiles) + cosine_finalize_kernel
  fp_row_inv_norm         -> row_inv_norm_kernel
  fp_split3_rows          -> split3_rows_kernel
  fp_l2_mean_thres        -> l2_mean_thres_kernel
  fp_l2_filter            -> l2_filter_kernel

tests/test_similarity_ops.py runs every case.

* A Case names its entry point, its shape, what the data look like and the instance it must land on (for fp_cosine_filter_x6 the
  tile rows fp_cosine_filter_x6_tile_rows reports; the other entry points have one kernel).  A filter shape whose D is a multiple
  of 32 appears twice, once per entry point; the twins share data and references (Case.seed).
* filter_inputs() / inv_norm_inputs() / split3_inputs() / l2_inputs() draw the seeded data.  The inverse norms a filter case hands to the kernels are the correctly rounded fp32 values of
  1 / sqrt(sum of squares in float64) -- inputs like G and R, not results of the code under test.
* filter_reduce(G, R, dtype) / inv_norm_reference(x, dtype) / l2_reference(ref, E, dtype) compute the operation in torch / numpy on the CPU from the semantics of oracle/similarity_ref.py and the
  docstrings of similarity.py -- never from the kernels: float64 is the truth, float32 the yardstick.  The filter's scores are
  S = (G R^T) / (|G| |R|^T); a NaN score (a zero row on either side) never wins and a row without any valid score is NaN, -1;
  score matrices exist one row block at a time (BLOCK_BYTES).  The L2 mean is summed in row order, as np.mean(axis=0) of the
  oracle does on a C-contiguous array.
* filter_bound() / bound_of(): the project's bound of the earlier pins, 2 * max|ref32 - ref64| + TOL * scale, with the reference's outputs (best;
  inverse norms; mean, thres, dist) as what is compared; scale is 1 for cosines and max|ref64| for norms, means and distances.
  The summation-order term of the filter.  torch's float32 matrix product sums K in blocks and vector lanes; both filter
  kernels are MFMA accumulator chains, which add the K products IN SEQUENCE (D / 2 and 6 D / 32 dependent fp32 additions per
  score).  A sequential fp32 sum of n terms carries up to n roundings of 2^-24 of the growing partial sum where a blocked one
  carries about log2(n) + n / lanes: on a tie row, a score of 1 whose partial sums grow steadily, at D = 512 the blocked
  reference errs by 3.6e-7 and the plain loop acc = acc + g[k] * r[k] by 9.5e-7.  The order of the sum is no part of the
  operation, so the float32 yardstick is evaluated in both orders -- the blocked product over the whole matrix (best32) and
  the plain loop at the winning column of every row (seq32, seq_score32) -- and max|ref32 - ref64| is the larger of the two
  errors.  On the cases without a score near 1 the two errors differ by at most 5.1e-8; only the bound of f32 / x6_130x257x512_ties
  (9.2e-7 -> 2.1e-6) moves by more than 1.1e-7.  cosine_tile_kernel met the blocked-only bound on every other case and missed it
  on that one alone (9.54e-7 against 9.15e-7, at a tie row); with the term the largest error is 0.45 of the bound there.
* Data kinds of the filter cases
    normal     rows N(0, 1), each row times a power of two from 2^-20 .. 2^20 where Case.scaled (the cosine does not change; the
               inverse norms and the bf16 split see fp32's range)
    ties       normal, and TIE_OFFSETS: query row m equals reference row j0, which is copied to j1 > j0 (the lowest index must
               win); one more query row equals the LAST reference row, which has no copy (a dropped last chunk shows)
    negative   Nr = 1 or 2: gallery rows -R[0] (best = -1 where Nr = 1), unit axes on which R[0] is zero (score exactly +0) and
               random rows: best negative, zero and positive.  R[0] holds sixteen entries of +-1/4: a norm of exactly 1
    zero_rows  one all-zero gallery row and one all-zero reference row among normal rows
* MUTANTS / mutant_shift(): float32 references of wrong kernels, each with the cases that must catch it.
"""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from face_detection_and_recognition_amd.plan import split3_bf16

TOL = 2e-7                       # the per-op relative term of the earlier pins (generic_op_cases.tolerance)
BLOCK_BYTES = 64 << 20           # no score matrix block larger than this
CHUNK = 128                      # reference columns of a workgroup (both filter kernels); the planes are padded to a multiple
GUARD = 64                       # guard elements behind every output of the protocol

FILTER, FILTER_X6 = "fp_cosine_filter", "fp_cosine_filter_x6"
INV_NORM, SPLIT3, L2 = "fp_row_inv_norm", "fp_split3_rows", "fp_l2_mean_thres+fp_l2_filter"


@dataclass(frozen=True)
class Case:
    name: str
    entry: str               # FILTER | FILTER_X6 | INV_NORM | SPLIT3 | L2
    shape: tuple             # filter: (M, Nr, D); INV_NORM: (M, D); SPLIT3: (Nr, D); L2: (R, D)
    kind: str = "normal"     # normal | ties | negative | zero_rows (module docstring)
    tile_rows: int = 0       # FILTER_X6: what fp_cosine_filter_x6_tile_rows must report (256 | 128)
    scaled: bool = False     # filter: every row times its own power of two
    sub_rows: int = 0        # FILTER_X6 at 256: this many first rows run alone land on the 128-row form and must give the same bits
    seed: str = ""           # the name that seeds the data (default: name): twins share data and references

    @property
    def key(self):
        return self.seed or self.name


def _rng(name, salt=0):
    return np.random.default_rng((zlib.crc32(name.encode()) + salt) % (2 ** 31))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _pow2(rng, n):
    return np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]


def inv_norm32(x):
    """The correctly rounded fp32 inverse norms of the rows of x: float32(1 / sqrt(sum of squares in float64)); +inf for a
    zero row."""
    with np.errstate(divide="ignore"):
        return (1.0 / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# the filter: data
# ---------------------------------------------------------------------------------------------------------------------------
# (label, j1 - j0, j0 within its 128-column chunk): where the two members of a tie meet
TIE_OFFSETS = (("same four-column group (x6) / neighbouring lane (fp32)", 1, 8),
               ("another q lane of the x6 epilogue", 4, 16),
               ("another 16-column accumulator", 16, 32),
               ("another nb block of the fp32 kernel", 32, 64),
               ("another workgroup: the atomicMax decides", 128, 3),
               ("a later chunk far away", None, 40))


def tie_plan(M, Nr):
    """[(query row m, j0, j1, label)] of a ties case: every kind of TIE_OFFSETS from chunk 0 and, where the columns reach that
    far, again from the middle chunk; the far member is the last-but-one column.  Plus (m, Nr - 1, None, ...): a query row that
    equals the last reference row alone."""
    out, i = [], 0
    nchunks = -(-Nr // CHUNK)
    for k, c0 in enumerate(sorted({0, (nchunks // 2) * CHUNK})):
        for label, off, j in TIE_OFFSETS:
            j0 = c0 + j
            j1 = Nr - 2 - k if off is None else j0 + off
            if j1 <= j0 + (0 if off else CHUNK) or j1 >= Nr - 1:
                continue
            out.append(((i * 53 + 5) % M, j0, j1, label))
            i += 1
    out.append(((i * 53 + 5) % M, Nr - 1, None, "the last column alone"))
    rows = [t[0] for t in out]
    cols = [j for t in out for j in t[1:3] if j is not None]
    assert len(set(rows)) == len(rows) and len(set(cols)) == len(cols), (M, Nr)
    return out


@functools.lru_cache(maxsize=2)
def filter_inputs(c):
    """{"G": (M, D), "R": (Nr, D), "ginv": (M,), "rinv": (Nr,)} float32, read-only; "ties": tie_plan() of a ties case;
    "zero_g" / "zero_r": the all-zero rows of a zero_rows case."""
    M, Nr, D = c.shape
    rng = _rng(c.key)
    G = rng.standard_normal((M, D), dtype=np.float32)
    R = rng.standard_normal((Nr, D), dtype=np.float32)
    d = {"ties": [], "zero_g": None, "zero_r": None}
    if c.kind == "negative":
        assert Nr in (1, 2) and D >= 24
        # R[0]: zero on the first eight axes, then sixteen entries of +-1/4.  Its norm is exactly 1, the power of two at which an
        # ulp is relatively largest, and its scores against -R[0] and the axes are exact in fp32 in any summation order
        R[0] = 0.0
        R[0, 8:24] = np.where(rng.integers(0, 2, 16) == 1, np.float32(0.25), np.float32(-0.25))
        for m in range(M):
            if m % 4 == 0:
                G[m] = -R[0]
            elif m % 4 == 1:
                G[m] = 0.0                   # every axis with both signs: against a second reference row one of them is negative
                G[m, (m // 4) % 8] = 1.0 if (m // 32) % 2 == 0 else -1.0
    if c.scaled:
        G *= _pow2(rng, M)
        R *= _pow2(rng, Nr)
    if c.kind == "ties":
        d["ties"] = tie_plan(M, Nr)
        for m, j0, j1, _ in d["ties"]:
            if j1 is not None:
                R[j1] = R[j0]
            G[m] = R[j0]
    if c.kind == "zero_rows":
        d["zero_g"], d["zero_r"] = M // 2, Nr // 3
        G[d["zero_g"]] = 0.0
        R[d["zero_r"]] = 0.0
    d.update(G=G, R=R, ginv=inv_norm32(G), rinv=inv_norm32(R))
    _ro(G, R, d["ginv"], d["rinv"])
    return d


def planes(R):
    """The planes fp_cosine_filter_x6 reads, built on the host from plan.split3_bf16: uint16 [D / 32][3][Npad][32], zero rows in
    the padding."""
    Nr, D = R.shape
    npad = -(-Nr // CHUNK) * CHUNK
    out = np.zeros((D // 32, 3, npad, 32), np.uint16)
    out[:, :, :Nr] = split3_bf16(R).reshape(3, Nr, D // 32, 32).transpose(2, 0, 1, 3)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the filter: references
# ---------------------------------------------------------------------------------------------------------------------------
def _step_ulps(v, n):
    v = np.float32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return v


def filter_scores(G, R, dt, mut=None):
    """Row blocks of S = (G R^T) / (|G| |R|^T) in dtype dt, NaN replaced by -inf: yields (first row, S block as numpy).
    mut: "hm" the dot products of operands cut to the first two bf16 pieces; "ktail" without the K chunk behind the last
    multiple of 32; "lastchunk" without the last 128-column chunk; ("inv4", j) the norm of reference row j four ulps up."""
    M, D = G.shape
    Nr = R.shape[0]
    Gt, Rt = torch.tensor(G, dtype=dt), torch.tensor(R, dtype=dt)
    gn, rn = Gt.norm(dim=1), Rt.norm(dim=1)
    if mut == "hm":
        cut = lambda x: torch.from_numpy((split3_bf16(x)[:2].astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(0)).to(dt)  # noqa: E731
        Gt, Rt = cut(G), cut(R)
    elif mut == "ktail":
        Gt, Rt = Gt[:, :D // 32 * 32], Rt[:, :D // 32 * 32]
    elif mut == "lastchunk":
        keep = (-(-Nr // CHUNK) - 1) * CHUNK
        Rt, rn = Rt[:keep], rn[:keep]
    elif mut is not None:
        assert mut[0] == "inv4" and dt == torch.float32
        rn = rn.clone()
        rn[mut[1]] = float(_step_ulps(rn[mut[1]].item(), 4))
    rows = max(1, BLOCK_BYTES // (max(Rt.shape[0], 1) * 8))
    with torch.no_grad(), np.errstate(all="ignore"):
        for lo in range(0, M, rows):
            S = (Gt[lo:lo + rows] @ Rt.T) / (gn[lo:lo + rows, None] * rn[None, :])
            S[torch.isnan(S)] = -np.inf
            yield lo, S.numpy()


def filter_reduce(G, R, dt, ties=(), mut=None):
    """(best, arg, second) of the filter over filter_scores: the best score of every row, the lowest index that attains it, the
    best score of the OTHER columns (-inf if none); a row without a valid score is NaN, -1.  ties: (m, j0, j1, label) of planted
    ties -- reference row j1 is a copy of row j0 < j1, so in EVERY gallery row column j1 ties with j0 and must lose: it is left
    out, so that best / arg are right whatever bits a blocked matrix product gives identical rows, and `second` is the best of
    the columns outside the tie."""
    M = G.shape[0]
    best = np.empty(M, np.float64 if dt == torch.float64 else np.float32)
    arg, second = np.empty(M, np.int32), np.empty(M, best.dtype)
    drop = [j1 for _, _, j1, _ in ties if j1 is not None]
    for lo, S in filter_scores(G, R, dt, mut):
        n = S.shape[0]
        S[:, [j for j in drop if j < S.shape[1]]] = -np.inf
        if S.shape[1] == 0:
            best[lo:lo + n], arg[lo:lo + n], second[lo:lo + n] = np.nan, -1, -np.inf
            continue
        a = S.argmax(axis=1)
        r = np.arange(n)
        b = S[r, a].copy()
        S[r, a] = -np.inf
        second[lo:lo + n] = S.max(axis=1)
        none = np.isneginf(b)
        best[lo:lo + n] = np.where(none, np.nan, b)
        arg[lo:lo + n] = np.where(none, -1, a)
    return best, arg, second


def score64(c, rows, cols):
    """float64 scores S[rows[i], cols[i]] of a filter case, computed directly (NaN where a norm is zero)."""
    d = filter_inputs(c)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    out = np.empty(len(rows), np.float64)
    with np.errstate(all="ignore"):
        for lo in range(0, len(rows), 65536):
            g = d["G"][rows[lo:lo + 65536]].astype(np.float64)
            r = d["R"][cols[lo:lo + 65536]].astype(np.float64)
            out[lo:lo + 65536] = (g * r).sum(1) / (np.sqrt((g * g).sum(1)) * np.sqrt((r * r).sum(1)))
    return out


def seq_score32(G, R, rows, cols):
    """float32 scores S[rows[i], cols[i]] with the sum over K taken IN SEQUENCE, acc = acc + g[k] * r[k] with both roundings in
    fp32 -- the plain loop; the rest of the formula as filter_scores (NaN for cols[i] < 0)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    g, r = G[rows], R[np.maximum(cols, 0)]
    acc = np.zeros(len(rows), np.float32)
    for k in range(G.shape[1]):
        acc = acc + g[:, k] * r[:, k]
    with np.errstate(all="ignore"):
        s = acc / (torch.tensor(g).norm(dim=1).numpy() * torch.tensor(r).norm(dim=1).numpy())
    return np.where(cols < 0, np.float32("nan"), s).astype(np.float32)


_REFS = {}


def filter_references(c):
    """{"best64", "arg64", "second64", "best32", "arg32", "seq32"} of a filter case on its own inputs, read-only, computed once
    per seed; seq32: seq_score32 at (m, arg64[m])."""
    if c.key not in _REFS:
        d = filter_inputs(c)
        b64, a64, s64 = filter_reduce(d["G"], d["R"], torch.float64, d["ties"])
        b32, a32, _ = filter_reduce(d["G"], d["R"], torch.float32, d["ties"])
        q32 = seq_score32(d["G"], d["R"], np.arange(c.shape[0]), a64)
        _ro(b64, a64, s64, b32, a32, q32)
        _REFS[c.key] = dict(best64=b64, arg64=a64, second64=s64, best32=b32, arg32=a32, seq32=q32)
    return _REFS[c.key]


def _max_abs(a, b):
    """max |a - b| over the elements where b is finite (a NaN or an infinity of the truth is checked as such, not by distance)."""
    ok = np.isfinite(b)
    return float(np.abs(a[ok].astype(np.float64) - b[ok]).max()) if ok.any() else 0.0


def filter_bound(c):
    """2 * max|ref32 - best64| + TOL (cosines: scale 1), ref32 the float32 reference in both of its summation orders (module
    docstring): torch's blocked product over the whole matrix and the plain sequential loop at the winning column."""
    r = filter_references(c)
    return 2.0 * max(_max_abs(r["best32"], r["best64"]), _max_abs(r["seq32"], r["best64"])) + TOL


def bound_of(r32, r64):
    """2 * max|ref32 - ref64| + TOL * max|ref64| over the finite elements of the truth."""
    ok = np.isfinite(r64)
    scale = float(np.abs(r64[ok]).max()) if ok.any() else 0.0
    return 2.0 * _max_abs(r32, r64) + TOL * scale


# (label, mutation, names of the cases that must catch it); ("inv4", None): the column is the argmax of the row with the largest
# |best| (the negative cases with Nr = 1: gallery row -R[0], a score of exactly -1, and R[0]'s norm is exactly 1, where four ulps
# are 4.8e-7 of the value)
MUTANTS = (
    ("operands cut to their h + m pieces", "hm", ("f32_1000x77x128_normal", "f32_4196x15400x96_normal")),
    ("the last K chunk dropped at D = 100", "ktail", ("f32_257x3000x100_normal", "f32_257x3000x100_ties")),
    ("the last column chunk dropped", "lastchunk", ("f32_130x257x512_ties", "f32_300x131001x32_ties", "f32_257x3000x100_ties")),
    ("one inverse norm off by 4 ulp", ("inv4", None), ("f32_70x1x32_negative", "f32_70x1x36_negative")),
)


def mutant_shift(c, mut):
    """max |best of the mutated float32 reference - best of the float32 reference| of a case."""
    d, r = filter_inputs(c), filter_references(c)
    if isinstance(mut, tuple) and mut[1] is None:
        m = int(np.nanargmax(np.abs(r["best32"])))
        mut = (mut[0], int(r["arg32"][m]))
    b, _, _ = filter_reduce(d["G"], d["R"], torch.float32, d["ties"], mut)
    both = np.isfinite(b) & np.isfinite(r["best32"])
    gone = int((np.isfinite(r["best32"]) & ~np.isfinite(b)).sum())
    return np.inf if gone else float(np.abs(b[both].astype(np.float64) - r["best32"][both]).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the other entry points: data and references
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inv_norm_inputs(c):
    """x (M, D) float32 N(0, 1), read-only; row M - 2 is all zero where M >= 3."""
    M, D = c.shape
    x = _rng(c.key).standard_normal((M, D), dtype=np.float32)
    if M >= 3:
        x[M - 2] = 0.0
    return _ro(x)


def inv_norm_reference(x, dt):
    """1 / sqrt(sum of squares) of every row in dtype dt (+inf for a zero row)."""
    t = torch.tensor(x, dtype=dt)
    return (1.0 / torch.sqrt((t * t).sum(dim=1))).numpy()


@functools.lru_cache(maxsize=None)
def split3_inputs(c):
    """R (Nr, D) float32, read-only: normals times 2^-30 .. 2^30, and, from the first element on, +0, -0, two all-ones mantissas
    and values exactly halfway between two bf16 neighbours (even and odd lower neighbour, both signs, in the first piece;
    0x3F804040 and 0x3F8040C0: a remainder halfway between two 8-bit values in the second piece)."""
    Nr, D = c.shape
    rng = _rng(c.key)
    R = rng.standard_normal((Nr, D), dtype=np.float32) * np.exp2(rng.integers(-30, 31, (Nr, D))).astype(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x3FFFFFFF, 0xC07FFFFF, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,
                        0x3F804040, 0x3F8040C0, 0x7E7FFFFF], np.uint32).view(np.float32)
    flat = R.reshape(-1)
    n = min(len(special), flat.size)
    flat[:n] = special[:n]
    if flat.size > 3 * len(special):
        flat[-len(special):] = special          # in the last row as well
    return _ro(R)


@functools.lru_cache(maxsize=None)
def l2_inputs(c):
    """{"ref": (R, D), "E": (R + 257, D)} float32, read-only: E holds the reference rows themselves, then 257 random rows.
    zero_rows: the R reference rows are one row of multiples of 2^-10 below 4, whose row-order sum and mean are exact."""
    R, D = c.shape
    rng = _rng(c.key)
    if c.kind == "zero_rows":
        row = (rng.integers(-4095, 4096, D) / 1024.0).astype(np.float32)
        ref = np.repeat(row[None], R, axis=0)
    else:
        ref = rng.standard_normal((R, D), dtype=np.float32)
    E = np.concatenate([ref, rng.standard_normal((257, D), dtype=np.float32)])
    return {"ref": _ro(ref), "E": _ro(E)}


def l2_reference(ref, E, dt):
    """(mean (D,), thres (), dist (M,)) in dtype dt: the mean summed in row order (np.mean(axis=0) of a C-contiguous array, as
    oracle/similarity_ref.ref_mean_and_thres), thres = max_i |mean - ref_i|, dist = |e - mean|."""
    r, e = torch.tensor(ref, dtype=dt), torch.tensor(E, dtype=dt)
    s = torch.zeros(r.shape[1], dtype=dt)
    for i in range(r.shape[0]):
        s = s + r[i]
    mean = s / r.shape[0]
    thres = torch.sqrt(((mean[None] - r) ** 2).sum(dim=1)).max()
    dist = torch.sqrt(((e - mean[None]) ** 2).sum(dim=1))
    return mean.numpy(), thres.numpy(), dist.numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
# (M, Nr, D), kinds, tile rows of the x6 form, scaled rows, rows of the sub-run
_FILTER_SHAPES = (
    ((1, 1, 32), ("normal",), 128, False, 0),                    # the smallest problem
    ((1, 1, 512), ("normal",), 128, False, 0),
    ((33, 129, 32), ("normal", "zero_rows"), 128, False, 0),     # the last chunk holds one column; waves wholly past the last row
    ((129, 128, 4), ("normal",), 0, False, 0),                   # the smallest D
    ((257, 3000, 100), ("normal", "ties"), 0, False, 0),         # fp32 kernel only: the last K chunk holds 4 of 32
    ((130, 257, 512), ("normal", "ties", "zero_rows"), 128, True, 0),    # ragged rows and chunks at the workload's D
    ((1000, 77, 128), ("normal",), 128, False, 0),               # a single ragged chunk
    ((300, 131001, 32), ("normal", "ties"), 256, True, 100),     # two row tiles, the second with 44 rows; 1024 chunks, the last with 57
    ((524033, 5, 32), ("normal",), 256, True, 0),                # 2047 full row tiles and a one-row tile; 5 columns
    ((4196, 15400, 96), ("normal",), 256, True, 0),              # three k-slabs
    ((300, 130944, 32), ("normal",), 128, False, 0),             # just below the gate
    ((70, 1, 32), ("negative",), 128, False, 0),
    ((70, 2, 64), ("negative",), 128, True, 0),
    ((70, 1, 36), ("negative",), 0, False, 0),
)


def _filter_cases():
    out = []
    for shape, kinds, tile, scaled, sub in _FILTER_SHAPES:
        for kind in kinds:
            stem = "x".join(map(str, shape)) + "_" + kind
            out.append(Case("f32_" + stem, FILTER, shape, kind, scaled=scaled, seed=stem))
            if shape[2] % 32 == 0:
                out.append(Case("x6_" + stem, FILTER_X6, shape, kind, tile_rows=tile, scaled=scaled,
                                sub_rows=sub if tile == 256 else 0, seed=stem))
    return out


FILTER_CASES = _filter_cases()
INV_NORM_CASES = [Case(f"inv_{m}x{d}", INV_NORM, (m, d)) for m in (1, 3, 4, 5, 1000) for d in (1, 4, 63, 64, 65, 100, 512, 700)]
SPLIT3_CASES = [Case(f"split_{n}x{d}", SPLIT3, (n, d)) for n, d in ((1, 32), (127, 32), (128, 64), (129, 96), (3000, 512))]
_L2_SHAPES = ((1, 1), (1, 512), (5, 100), (6, 128), (37, 700), (300, 512))
L2_CASES = ([Case(f"l2_{r}x{d}", L2, (r, d)) for r, d in _L2_SHAPES] +
            [Case(f"l2_{r}x{d}_same", L2, (r, d), "zero_rows") for r, d in _L2_SHAPES])


def cases():
    out = FILTER_CASES + INV_NORM_CASES + SPLIT3_CASES + L2_CASES
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


BY_NAME = {c.name: c for c in cases()}
