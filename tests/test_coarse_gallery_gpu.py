"""The compressed gallery on the device (csrc/simi8.hip): row quantisation and the integer coarse search pinned to their numpy
restatements by equality, the rerank and the two-stage search against fp64, the footprint, and FacePipeline(gallery=).

Tolerances: SCORE_TOL and GAP are the project's (tests/test_topk_gpu.py); everything integer is compared by equality."""
import numpy as np
import pytest
import torch

from face_detection_and_recognition_amd import similarity as S

SCORE_TOL = 1e-4      # the project's score tolerance
GAP = 1e-5            # an fp64 gap above which the order of two candidates is unambiguous in fp32 arithmetic
SPLITS = (0, 1, 3, 6)


def _ids(s):
    return "x".join(map(str, s))


# ---- quantise ---------------------------------------------------------------------------------------------------------------
QUANT_SHAPES = [(1, 64), (5, 128), (257, 512), (3000, 100), (130, 1024)]


def _quant_rows(N, D, seed):
    rng = np.random.default_rng(seed)
    X = (rng.normal(0, 1, (N, D)) * rng.uniform(1e-3, 30, (N, 1))).astype(np.float32)
    if N >= 5:                                           # the special rows of the CPU test
        X[0] = 0.37 * np.where(np.arange(D) % 3 == 0, -1, 1)
        X[1] = 0
        X[2, D // 2] = np.nan
        X[3, D - 1] = -np.inf
        X[4] = 0
        X[4, :8] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, 63.5, -126.5]
    return X


@pytest.mark.gpu
@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=_ids)
def test_quantize_equals_numpy(dev, shape):
    N, D = shape
    X = _quant_rows(N, D, 5)
    q8, scale = S.quantize_rows_i8(torch.from_numpy(X).to(dev))
    wq, ws = S.quantize_rows_i8_numpy(X)
    D64 = (D + 63) // 64 * 64
    assert tuple(q8.shape) == (D64 // 64, (N + 127) // 128 * 128, 64) and q8.dtype == torch.int8
    assert not q8[:, N:].any()                           # zero rows in the padding
    assert np.array_equal(S.unstage_rows_i8(q8, N).cpu().numpy(), wq)
    assert np.array_equal(scale.cpu().numpy().view(np.uint32), ws.view(np.uint32))
    if N >= 5:
        assert np.all(np.abs(wq[0, :D]) == 127) and not wq[1:4].any() and not ws[1:4].any()


# ---- integer walk -------------------------------------------------------------------------------------------------------------
WALK_SHAPES = [(1, 1, 64, 1), (3, 5, 128, 16), (130, 257, 512, 32), (37, 1000, 64, 16), (257, 3000, 128, 64), (64, 20000, 512, 32)]


def _walk_operands(shape, kind):
    """int8 codes in [-127, 127] with structure that is symmetric in nothing: per-feature and per-row ramps under the noise.
    kind "identity": query i is 127 at feature (7 i + 3) % D and a small 1 at the next one, so that its dots read single
    gallery entries -- a permuted k order or a row / column swap changes them."""
    M, N, D, pool = shape
    rng = np.random.default_rng(1000 * M + N + D)
    g = rng.integers(-127, 128, (N, D))
    g = np.clip(g // 2 + (np.arange(D)[None, :] % 61) - (np.arange(N)[:, None] % 29), -127, 127).astype(np.int8)
    if kind == "identity":
        q = np.zeros((M, D), np.int8)
        q[np.arange(M), (7 * np.arange(M) + 3) % D] = 127
        q[np.arange(M), (7 * np.arange(M) + 4) % D] = 1
    else:
        q = rng.integers(-127, 128, (M, D))
        q = np.clip(q // 2 + (np.arange(D)[None, :] % 37) - (np.arange(M)[:, None] % 17), -127, 127).astype(np.int8)
    return q, g


def _run_i8(dev, q, g, u, w, pool, ns):
    s, i = S.cosine_topk_i8(S.stage_rows_i8(torch.from_numpy(q).to(dev)), torch.from_numpy(u).to(dev),
                            S.stage_rows_i8(torch.from_numpy(g).to(dev)), torch.from_numpy(w).to(dev), g.shape[0], pool, ns)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "identity"])
@pytest.mark.parametrize("shape", WALK_SHAPES, ids=_ids)
def test_integer_walk_equals_numpy(dev, shape, kind):
    M, N, D, pool = shape
    q, g = _walk_operands(shape, kind)
    u, w = np.ones(M, np.float32), np.ones(N, np.float32)
    want = S.cosine_topk_i8_numpy(q, u, g, w, pool)      # with u = w = 1 the scores ARE the integer dots
    dots = q.astype(np.int64) @ g.astype(np.int64).T
    kv = min(pool, N)
    assert np.array_equal(want[0][:, :kv], -np.sort(-dots, axis=1)[:, :kv].astype(np.float32))
    for ns in SPLITS:
        got = _run_i8(dev, q, g, u, w, pool, ns)
        assert got[0].shape == (M, pool) and got[0].dtype == np.float32 and got[1].dtype == np.int32
        assert np.array_equal(got[1], want[1]), (shape, kind, ns)
        assert _same(got, want), (shape, kind, ns)
    assert np.all(np.isneginf(want[0][:, kv:])) and np.all(want[1][:, kv:] == -1)      # N < pool: the tail


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 70000, 64, 16), (3, 530000, 64, 8)], ids=_ids)
def test_integer_walk_with_prefix_passes(dev, shape):
    """Galleries of 65 536 rows and more are searched in passes over growing prefixes (16 384 rows, 8-fold steps), each handing
    the next a score floor: two passes at 70 000 rows, three at 530 000.  The result is still the restatement's, exactly --
    with the best rows of query 0 behind the first prefix, ties across the prefix edge, and a masked best row."""
    M, N, D, pool = shape
    q, g = _walk_operands(shape, "random")
    g[[7, 16383, 16384, N - 1]] = g[N // 2]               # equal rows inside, at the edge of and behind the first prefix
    g[N - 3] = np.where(q[0] >= 0, 127, -127)             # the best row of query 0, near the end ...
    g[N - 2] = g[N - 3]                                   # ... and its masked twin
    u, w = np.ones(M, np.float32), np.ones(N, np.float32)
    w[::3] = 0.5                                          # real weights: the order is not the dots' order
    w[N - 2] = 0
    want = S.cosine_topk_i8_numpy(q, u, g, w, pool)
    assert want[1][0, 0] == N - 3 and not (want[1] == N - 2).any() and want[1].min() >= 0
    for ns in SPLITS:
        assert _same(_run_i8(dev, q, g, u, w, pool, ns), want), ns


@pytest.mark.gpu
def test_integer_walk_at_the_largest_dot(dev):
    """D = 1024, every code +-127: |dot| reaches 1024 * 127^2 = 16 516 096 < 2^24, still exact in fp32."""
    M, N, D, pool = 5, 300, 1024, 8
    rng = np.random.default_rng(9)
    g = np.where(rng.random((N, D)) < 0.5, -127, 127).astype(np.int8)
    q = np.where(rng.random((M, D)) < 0.5, -127, 127).astype(np.int8)
    g[131], g[17], g[250] = q[0], -q[1], q[2]
    u, w = np.ones(M, np.float32), np.ones(N, np.float32)
    want = S.cosine_topk_i8_numpy(q, u, g, w, pool)
    assert want[0][0, 0] == 1024 * 127 * 127 and want[1][0, 0] == 131 and want[1][2, 0] == 250
    for ns in SPLITS:
        assert _same(_run_i8(dev, q, g, u, w, pool, ns), want), ns
    w[:] = -1                                            # ... and the most negative one, in front
    want = S.cosine_topk_i8_numpy(q, u, g, w, pool)
    assert want[0][1, 0] == 1024 * 127 * 127 and want[1][1, 0] == 17
    assert _same(_run_i8(dev, q, g, u, w, pool, 0), want)


# ---- weights, ties, masks ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_weights_ties_masks_equal_numpy(dev):
    from face_detection_and_recognition_amd.gallery import CompressedGallery
    N, D, M, pool = 700, 128, 70, 16
    rng = np.random.default_rng(12)
    G = (rng.normal(0, 1, (N, D)) * rng.uniform(0.1, 10, (N, 1))).astype(np.float32)
    Q = rng.normal(0, 1, (M, D)).astype(np.float32)
    G[[40, 300, 301, 655]] = Q[3] * 2.5                   # four identical rows, the best of query 3
    G[[10, 11]] = Q[5] * 0.5                              # the best of query 5: removed below
    G[20] = 0                                             # a dead gallery row
    Q[7] = 0                                              # dead query rows
    Q[8, 3] = np.nan
    gal = CompressedGallery(G, np.zeros(N, np.int32), device=dev, rows=None)
    removed = np.zeros(N, bool)
    removed[[10, 11, 500]] = True
    gal.remove(removed)
    qq, sq = S.quantize_rows_i8(torch.from_numpy(Q).to(dev))
    qinv = S.row_inv_norm(torch.from_numpy(Q).to(dev))
    u = sq * torch.where(torch.isfinite(qinv), qinv, torch.zeros_like(qinv))
    un, wn = u.cpu().numpy(), gal.w.cpu().numpy()
    assert wn[20] == 0 and np.all(wn[removed] == 0) and un[7] == 0 and un[8] == 0 and (wn != 0).sum() == N - 4
    want = S.cosine_topk_i8_numpy(S.unstage_rows_i8(qq, M).cpu().numpy(), un, S.unstage_rows_i8(gal.g8, N).cpu().numpy(), wn, pool)
    for ns in SPLITS:
        s, i = S.cosine_topk_i8(qq, u, gal.g8, gal.w, N, pool, ns)
        got = (s.cpu().numpy(), i.cpu().numpy())
        assert _same(got, want), ns                       # real w and u: exact equality
        assert got[1][3, :4].tolist() == [40, 300, 301, 655], ns       # identical rows: the lowest index first
        assert not np.isin(got[1], [10, 11, 20, 500]).any(), ns        # w == 0 never returns
        for dead in (7, 8):
            assert np.all(np.isneginf(got[0][dead])) and np.all(got[1][dead] == -1), ns
        assert np.all(got[0][:, 1:] <= got[0][:, :-1])    # non-increasing
    live = [m for m in range(M) if m not in (7, 8)]
    assert np.all(want[1][live] >= 0)
    # coarse-only search: the best k of that list, with its scores
    s, i = gal.search(torch.from_numpy(Q).to(dev), 4)
    assert np.array_equal(i.cpu().numpy(), want[1][:, :4]) and np.array_equal(s.cpu().numpy().view(np.uint32), want[0][:, :4].view(np.uint32))
    # the coarse score approximates the cosine: codes are within half a level of 127 per side
    S64 = (Q[live].astype(np.float64) / np.linalg.norm(Q[live].astype(np.float64), axis=1, keepdims=True)) @ \
        (G.astype(np.float64) / np.maximum(np.linalg.norm(G.astype(np.float64), axis=1, keepdims=True), 1e-30)).T
    err = np.abs(want[0][live] - np.take_along_axis(S64, want[1][live].astype(np.int64), 1)).max()
    print(f"coarse score error against fp64: {err:.2e}")
    assert err < 0.02


# ---- rerank alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rerank_against_fp64_and_compact_mode(dev):
    M, N, D, pool, k = 37, 500, 100, 24, 5
    rng = np.random.default_rng(21)
    Q = rng.normal(0, 1, (M, D)).astype(np.float32)
    G = rng.normal(0, 1, (N, D)).astype(np.float32)
    cand = np.stack([rng.permutation(N)[:pool] for _ in range(M)]).astype(np.int32)
    cand[rng.random((M, pool)) < 0.2] = -1                # holes in the list
    cand[5, :] = -1                                       # nothing to rerank
    cand[6, 3:] = -1                                      # fewer than k
    masked = np.zeros(N, bool)
    masked[rng.permutation(N)[:60]] = True
    Gd = S.pad_features64(torch.from_numpy(G).to(dev))
    ginv = S.row_inv_norm(Gd)
    ginv[torch.from_numpy(masked).to(dev)] = 0
    cd = torch.from_numpy(cand).to(dev)
    s, i = S.rerank_topk(torch.from_numpy(Q).to(dev), cd, k, G=Gd, ginv=ginv)
    block = Gd[cd.clamp(min=0).long()].contiguous()       # (M, pool, D64): what a host-resident gallery uploads
    s2, i2 = S.rerank_topk(torch.from_numpy(Q).to(dev), cd, k, rows=block, ginv=ginv)
    s3, i3 = S.rerank_topk(torch.from_numpy(Q).to(dev), cd, k, G=Gd, ginv=ginv)
    torch.cuda.synchronize()
    assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))       # compact == indexed, bit for bit
    assert torch.equal(i, i3) and torch.equal(s.view(torch.int32), s3.view(torch.int32))       # and run == run
    s, i = s.cpu().numpy(), i.cpu().numpy()
    q64, g64 = Q.astype(np.float64), G.astype(np.float64)
    S64 = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (g64 / np.linalg.norm(g64, axis=1, keepdims=True)).T
    checked = 0
    for m in range(M):
        ok = [c for c in cand[m].tolist() if c >= 0 and not masked[c]]
        ok.sort(key=lambda c: (-S64[m, c], c))
        kv = min(k, len(ok))
        assert np.all(np.isneginf(s[m, kv:])) and np.all(i[m, kv:] == -1), m
        assert set(i[m, :kv].tolist()) <= set(ok), m       # -1 entries and masked rows never come back
        assert len(set(i[m, :kv].tolist())) == kv
        assert np.abs(s[m, :kv] - S64[m, i[m, :kv]]).max(initial=0) < SCORE_TOL, m
        assert np.all(s[m, 1:kv] <= s[m, :kv - 1]) if kv > 1 else True
        sc = [S64[m, c] for c in ok] + [-np.inf]
        for p in range(kv):                               # the order is exact wherever fp64 separates the neighbours
            if (p == 0 or sc[p - 1] - sc[p] > GAP) and sc[p] - sc[p + 1] > GAP:
                assert i[m, p] == ok[p], (m, p)
                checked += 1
    assert checked > 0.9 * (M - 2) * k


# ---- two stages end to end ---------------------------------------------------------------------------------------------------
E2E_SHAPES = [(512, 20000, 64, 5, 32), (64, 1000, 37, 5, 16), (128, 3000, 64, 16, 64)]       # D, N, M, k, pool
_e2e = {}


def _e2e_inputs(shape):
    """Planted neighbours: query i plus noise of 0.3 + 0.1 j written into k gallery rows, over Gaussian rows.  Computed once:
    the fp64 order, the positions its gaps decide, and the restated coarse top-pool."""
    if shape not in _e2e:
        D, N, M, k, pool = shape
        rng = np.random.default_rng(0)
        Q = rng.normal(0, 1, (M, D)).astype(np.float32)
        G = rng.normal(0, 1, (N, D)).astype(np.float32)
        where = rng.permutation(N)[:M * k].reshape(M, k)
        for j in range(k):
            G[where[:, j]] = Q + (0.3 + 0.1 * j) * rng.normal(0, 1, (M, D)).astype(np.float32)
        q64, g64 = Q.astype(np.float64), G.astype(np.float64)
        S64 = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (g64 / np.linalg.norm(g64, axis=1, keepdims=True)).T
        order = np.argsort(-S64, axis=1, kind="stable")[:, :k + 1]
        top = np.take_along_axis(S64, order, 1)
        gaps = top[:, :-1] - top[:, 1:]                   # gaps[p] = between positions p and p + 1
        decided = gaps > GAP
        decided[:, 1:] &= gaps[:, :-1] > GAP
        qq, sq = S.quantize_rows_i8_numpy(Q)
        qg, sg = S.quantize_rows_i8_numpy(G)
        one = np.float32(1)
        u = sq * (one / np.sqrt((Q * Q).sum(1, dtype=np.float32)))
        w = sg * (one / np.sqrt((G * G).sum(1, dtype=np.float32)))
        cs, ci = S.cosine_topk_i8_numpy(qq, u, qg, w, pool)
        cerr = np.abs(cs - np.take_along_axis(S64, ci.astype(np.int64), 1)).max()
        _e2e[shape] = (Q, G, order[:, :k], decided, ci, cerr)
    return _e2e[shape]


@pytest.mark.parametrize("shape", E2E_SHAPES, ids=_ids)
def test_two_stage_inputs_satisfy_their_conditions(shape):
    """No device: conditions on the INPUTS of the next test, from fp64 and the numpy restatement alone."""
    D, N, M, k, pool = shape
    Q, G, order, decided, ci, cerr = _e2e_inputs(shape)
    for m in range(M):                                    # every fp64 top-k row is inside the restated coarse top-pool
        assert set(order[m].tolist()) <= set(ci[m].tolist()), m
    assert (~decided).sum() <= 0.05 * decided.size        # positions left out for a small fp64 gap: at most 5 %
    print(f"{shape}: coarse cosine error {cerr:.2e}, undecided positions {(~decided).sum()} of {decided.size}")
    assert cerr <= 4.4e-3


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["device", "host"])
@pytest.mark.parametrize("shape", E2E_SHAPES, ids=_ids)
def test_two_stage_search_finds_the_fp64_neighbours(dev, shape, rows):
    from face_detection_and_recognition_amd.gallery import CompressedGallery
    D, N, M, k, pool = shape
    Q, G, order, decided, ci, cerr = _e2e_inputs(shape)
    for m in range(M):
        assert set(order[m].tolist()) <= set(ci[m].tolist()), m
    assert (~decided).sum() <= 0.05 * decided.size
    gal = CompressedGallery(G, np.zeros(N, np.int32), device=dev, rows=rows)
    s, i = gal.search(torch.from_numpy(Q).to(dev), k, pool)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert s.shape == (M, k) and i.shape == (M, k) and i.dtype == np.int32
    bad = np.argwhere(decided & (i != order))
    assert len(bad) == 0, bad[:10]
    q64, g64 = Q.astype(np.float64), G.astype(np.float64)
    exact = np.einsum("md,mkd->mk", q64 / np.linalg.norm(q64, axis=1, keepdims=True),
                      g64[i] / np.linalg.norm(g64[i], axis=2, keepdims=True))
    assert np.abs(s - exact).max() < SCORE_TOL            # exact scores, not coarse ones
    assert np.all(s[:, 1:] <= s[:, :-1])


# ---- footprint, conversions, files -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_footprint_and_conversions(dev, tmp_path):
    from face_detection_and_recognition_amd.gallery import CompressedGallery, FaceGallery
    N, D = 1000, 100
    rng = np.random.default_rng(4)
    G = rng.normal(0, 1, (N, D)).astype(np.float32)
    labels = (np.arange(N) % 7).astype(np.int32)
    full = FaceGallery(G, labels, {0: "zero"}, device=dev)
    full.remove(np.arange(N) % 50 == 0)
    coarse_only = full.compress(rows=None)
    Npad, Dpad = 1024, 128
    assert coarse_only.device_bytes() <= Npad * (Dpad + 12) + N * 4     # codes + w, ginv, scale per row, + labels
    on_device = full.compress(rows="device")
    assert on_device.device_bytes() == coarse_only.device_bytes() + N * Dpad * 4
    on_host = full.compress(rows="host")
    assert on_host.device_bytes() == coarse_only.device_bytes() and on_host.rows.is_pinned() and not on_host.rows.is_cuda
    Q = torch.from_numpy(G[::9] + 0.05 * rng.normal(0, 1, G[::9].shape).astype(np.float32)).to(dev)
    want_s, want_i = full.search(Q, 3)
    for g in (on_device, on_host):
        s, i = g.search(Q, 3)
        assert torch.equal(i, want_i) and (s - want_s).abs().max() < SCORE_TOL
        assert not np.isin(i.cpu().numpy(), np.arange(0, N, 50)).any()          # removed rows stay removed
    clear = want_s[:, 0] > 0.9                            # queries whose own row is live: even the coarse list has it in front
    cs, ci = coarse_only.search(Q, 3)
    assert int(clear.sum()) > 100 and torch.equal(ci[clear, 0], want_i[clear, 0]) and (cs - want_s)[clear, 0].abs().max() < 0.02
    # files: either class loads the other's
    p = on_host.save(str(tmp_path / "c.npz"))
    back = FaceGallery.load(p, device=dev)
    assert torch.equal(back.embeddings, full.embeddings) and torch.equal(back.ginv == 0, full.ginv == 0) and back.names == full.names
    again = CompressedGallery.load(full.save(str(tmp_path / "f.npz")), device=dev, rows="device")
    assert torch.equal(again.w, on_device.w) and torch.equal(again.g8, on_device.g8)
    # add rebuilds; rows removed before stay removed
    on_device.add(G[:5] * 2, labels[:5], {9: "nine"})
    assert len(on_device) == N + 5 and on_device.g8.shape[1] == 1024 and on_device.names[9] == "nine"
    assert bool((on_device.w[:N] == 0).cpu().numpy()[::50].all()) and int((on_device.w == 0).sum()) == N // 50
    s, i = on_device.search(torch.from_numpy(G[1:2]).to(dev), 2)
    assert i.cpu().tolist() == [[1, N + 1]] and (s.cpu() - 1).abs().max() < SCORE_TOL        # the row and its new scaled copy


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_takes_a_compressed_gallery(dev):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.gallery import CompressedGallery, FaceGallery
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    emb = W.build_embedder(dev)
    ref = W.make_reference(64, dev)
    frames = W.make_frames(4, dev, seed=7)
    plain = FacePipeline(det, emb, ref, tau=0.3).step(frames)
    torch.cuda.synchronize()
    E = plain["emb"].cpu().numpy().astype(np.float64)
    n, D = E.shape
    assert n > 0
    # one-hot-like unit rows, far apart: cosine between two of them ~ 0; the best row of a face is its largest coordinate
    R = 12
    rows = np.zeros((R, D), np.float32)
    rows[np.arange(R), np.arange(R) * 37 % D] = 1
    rows += 0.001
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    S64 = (E / np.linalg.norm(E, axis=1, keepdims=True)) @ rows.astype(np.float64).T
    best = np.sort(S64, axis=1)[:, ::-1]
    top = np.sort(best[:, 0])
    cut = int(np.argmax(np.diff(top))) if n > 1 else 0
    tau = float((top[cut] + top[cut + 1]) / 2) if n > 1 else float(top[0] - 0.1)
    print(f"{n} faces, tau = {tau:.4f} inside a gap of {top[min(cut + 1, n - 1)] - top[cut]:.2e}, "
          f"smallest best-to-second gap {(best[:, 0] - best[:, 1]).min():.2e}")
    assert n == 1 or top[cut + 1] - top[cut] > 10 * SCORE_TOL          # identify_tau well inside the gap
    assert np.all(best[:, 0] - best[:, 1] > GAP)                       # and every face's best row is unambiguous in fp32
    labels = torch.arange(R, dtype=torch.int32) + 100
    want = FacePipeline(det, emb, ref, gallery=FaceGallery(rows, labels, device=dev), identify_tau=tau).step(frames)
    expect = np.where(best[:, 0] >= tau, S64.argmax(1) + 100, -1)
    assert want["identity"].cpu().tolist() == expect.tolist()
    for where in ("device", "host"):
        got = FacePipeline(det, emb, ref, gallery=CompressedGallery(rows, labels, device=dev, rows=where), identify_tau=tau).step(frames)
        torch.cuda.synchronize()
        assert torch.equal(got["identity"], want["identity"]), where
        assert torch.equal(got["top_idx"][:, 0], want["top_idx"][:, 0]), where
        assert (got["top_scores"] - want["top_scores"]).abs().max() < SCORE_TOL
