import pytest
"""world_size-2 gloo tests (CPU) of the multi-GPU data path: frame sharding and the one exchange step."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from face_detection_and_recognition_amd.distributed import shard_range


def test_shard_range_partitions():
    for n in (0, 1, 7, 256, 1001):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from face_detection_and_recognition_amd import distributed as D
    from oracle import similarity_ref
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(5)
    G = rng.normal(0, 1, (101, 64)).astype(np.float32)
    R = rng.normal(0, 1, (37, 64)).astype(np.float32)
    g0, g1 = D.shard_range(len(G), rank, world)
    r0, r1 = D.shard_range(len(R), rank, world)

    def filter_fn(g, r, tau):      # the checker stands in for the HIP kernel on CPU tensors
        b, a, k, _ = similarity_ref.cosine_filter(g.numpy(), r.numpy(), tau)
        return torch.from_numpy(b), torch.from_numpy(a), torch.from_numpy(k)

    best, arg, keep = D.sharded_cosine_filter(torch.from_numpy(G[g0:g1]), torch.from_numpy(R[r0:r1]), 0.1, filter_fn)
    rb, ra, rk, _ = similarity_ref.cosine_filter(G, R, 0.1)
    ok = np.allclose(best.numpy(), rb[g0:g1], atol=1e-6) and np.array_equal(arg.numpy(), ra[g0:g1]) and \
        np.array_equal(keep.numpy(), rk[g0:g1])
    rows, offs = D.all_gather_rows(torch.from_numpy(R[r0:r1]))
    ok = ok and np.array_equal(rows.numpy(), R) and offs[-1] == len(R)
    # equal-size reference blocks (BASELINE configs[4]): one all_gather_into_tensor, no size exchange
    Re = R[:36]
    e0, e1 = rank * 18, rank * 18 + 18
    b2, a2, k2 = D.sharded_cosine_filter(torch.from_numpy(G[g0:g1]), torch.from_numpy(Re[e0:e1]), 0.1, filter_fn,
                                         equal_blocks=True)
    rb2, ra2, rk2, _ = similarity_ref.cosine_filter(G, Re, 0.1)
    ok = ok and np.allclose(b2.numpy(), rb2[g0:g1], atol=1e-6) and np.array_equal(a2.numpy(), ra2[g0:g1])
    # the step exchange of bench.py: fixed-capacity blocks + device-side counts, each rank's faces against the OTHER
    # ranks' faces (own and padding rows masked by a zero inverse norm)
    cap, D_ = 24, 64
    n_loc = [17, 9][rank]
    E_all = [rng.normal(0, 1, (n, D_)).astype(np.float32) for n in (17, 9)]
    block = np.zeros((cap, D_), np.float32)
    block[:n_loc] = E_all[rank]
    block[n_loc:] = 7.0                                      # junk in the padding rows must not matter

    def filter_rinv(g, r, tau, rinv):
        gn = g.numpy() / np.maximum(np.linalg.norm(g.numpy(), axis=1, keepdims=True), 1e-30)
        s = gn @ (r.numpy() * rinv.numpy()[:, None]).T
        return torch.from_numpy(s.max(1)), torch.from_numpy(s.argmax(1).astype(np.int32)), torch.from_numpy(s.max(1) >= tau)

    def inv_norm(r):
        return 1.0 / torch.linalg.norm(r, dim=1).clamp_min(1e-30)

    best3, arg3, keep3, counts = D.cross_rank_match(torch.from_numpy(block), torch.tensor([n_loc]), 0.1, filter_rinv,
                                                    inv_norm)
    other = E_all[1 - rank]
    mine = E_all[rank]
    sref = (mine / np.linalg.norm(mine, axis=1, keepdims=True)) @ (other / np.linalg.norm(other, axis=1, keepdims=True)).T
    ok = ok and counts.tolist() == [17, 9]
    ok = ok and np.allclose(best3.numpy()[:n_loc], sref.max(1), atol=1e-5)
    ok = ok and np.array_equal(arg3.numpy()[:n_loc], (1 - rank) * cap + sref.argmax(1))
    # every cross-rank cosine negative (rank 0's faces cluster around +c, rank 1's around -c): the row maximum lands on
    # a masked column (score 0) -> arg -1, keep False, best -1; and a step in which the peer found no face at all
    centre = rng.normal(0, 1, (1, D_)).astype(np.float32)
    base = centre + 0.1 * rng.normal(0, 1, (6, D_)).astype(np.float32)
    blk = np.zeros((cap, D_), np.float32)
    blk[:6] = base if rank == 0 else -base
    b4, a4, k4, _ = D.cross_rank_match(torch.from_numpy(blk), torch.tensor([6]), 0.1, filter_rinv, inv_norm)
    ok = ok and (a4.numpy()[:6] == -1).all() and not k4.numpy()[:6].any() and (b4.numpy()[:6] == -1.0).all()
    n5 = [5, 0][rank]
    b5, a5, k5, c5 = D.cross_rank_match(torch.from_numpy(block), torch.tensor([n5]), -0.5, filter_rinv, inv_norm)
    if rank == 0:      # no peer rows: nothing can match, whatever tau is
        ok = ok and c5.tolist() == [5, 0] and (a5.numpy()[:5] == -1).all() and not k5.numpy()[:5].any()
    # the overlapped form (bench.py N > 1): StepExchange hands step k's result out while step k + 1 is submitted; same
    # numbers as the in-step exchange, one step late, block reuse after two steps
    ex = D.StepExchange(cap, D_, "cpu", 0.1, filter_rinv, inv_norm)
    steps = []
    for k in range(4):
        nk = [5 + 3 * k, 11 - 2 * k][rank]
        ek = torch.from_numpy(rng.normal(0, 1, (20, D_)).astype(np.float32)[:nk] + (0.5 if rank else -0.25) * k)
        blk_k = torch.zeros((cap, D_))
        blk_k[:nk] = ek
        want = D.cross_rank_match(blk_k, torch.tensor([nk]), 0.1, filter_rinv, inv_norm)
        got = ex.submit(ek, nk)
        steps.append((want, nk))
        if k == 0:
            ok = ok and got is None
        else:
            prev, npv = steps[k - 1]       # rows past the step's face count are padding (stale rows of the reused block)
            ok = ok and all(torch.equal(a[:npv], b[:npv]) for a, b in zip(got[:3], prev[:3])) and torch.equal(got[3], prev[3])
    last = ex.drain()
    ok = ok and all(torch.equal(a[:steps[-1][1]], b[:steps[-1][1]]) for a, b in zip(last[:3], steps[-1][0][:3]))
    # capacity growth: a step in which some rank has more faces than the gather block holds does not raise
    # and drops nothing -- every rank reads the same gathered counts at hand-out time, enlarges its blocks, re-runs that
    # step's exchange and keeps the larger capacity.  Same matches as an exchange with a block that was big enough.
    ex2 = D.StepExchange(8, D_, "cpu", 0.1, filter_rinv, inv_norm, grow=8)
    big, wants, caps_seen = 40, [], []
    for k in range(4):
        nk = [[3, 19, 5, 7], [6, 4, 30, 2]][rank][k]
        ek = torch.from_numpy(rng.normal(0, 1, (40, D_)).astype(np.float32)[:nk] + (0.5 if rank else -0.25) * k)
        blk_k = torch.zeros((big, D_))
        blk_k[:nk] = ek
        wants.append((D.cross_rank_match(blk_k, torch.tensor([nk]), 0.1, filter_rinv, inv_norm), nk))
        got = ex2.submit(ek, nk)
        outs = [got] if k else []
        if k == 3:
            outs.append(ex2.drain())
        for j, g in enumerate(outs):
            (wb, wa, wk, wc), nw = wants[k - 1 + j]
            gb, ga, gk, gc, gcap = g
            caps_seen.append(gcap)
            ok = ok and torch.equal(gc, wc) and gcap >= int(wc.max()) and torch.allclose(gb[:nw], wb[:nw], atol=1e-6)
            ok = ok and torch.equal(gk[:nw], wk[:nw])
            wa64, ga64 = wa[:nw].long(), ga[:nw].long()
            ok = ok and torch.equal(ga64 < 0, wa64 < 0)
            ok = ok and torch.equal(torch.where(ga64 < 0, ga64, ga64 // gcap * big + ga64 % gcap), wa64)   # same (rank, row)
    # (step 3 was submitted before the hand-out of step 2 grew the blocks: it ran, and fitted, at 24 rows)
    ok = ok and caps_seen == [8, 24, 32, 24] and ex2.regrown == 2 and ex2.cap == 32
    rows_g, valid_g, _ = D.all_gather_blocks(torch.from_numpy(block), torch.tensor([n_loc]))
    ok = ok and valid_g.tolist() == [i < 17 for i in range(cap)] + [i < 9 for i in range(cap)]
    mean = D.sharded_l2_mean(torch.from_numpy(R[r0:r1]))
    ok = ok and np.allclose(mean.numpy(), R.mean(0), atol=1e-6)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_sharded_similarity_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def _worker_n(rank, world, port, q):
    """The same data path at any world size: every rank holds a ragged share, the expected matches are computed from ALL
    ranks' rows with numpy (each rank can regenerate them: same seed)."""
    sys.path.insert(0, ROOT)
    from face_detection_and_recognition_amd import distributed as D
    from oracle import similarity_ref
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(11)
    G = rng.normal(0, 1, (203, 32)).astype(np.float32)
    R = rng.normal(0, 1, (world * 9 + 5, 32)).astype(np.float32)
    g0, g1 = D.shard_range(len(G), rank, world)
    r0, r1 = D.shard_range(len(R), rank, world)

    def filter_fn(g, r, tau):
        b, a, k, _ = similarity_ref.cosine_filter(g.numpy(), r.numpy(), tau)
        return torch.from_numpy(b), torch.from_numpy(a), torch.from_numpy(k)

    best, arg, keep = D.sharded_cosine_filter(torch.from_numpy(G[g0:g1]), torch.from_numpy(R[r0:r1]), 0.2, filter_fn)
    rb, ra, rk, _ = similarity_ref.cosine_filter(G, R, 0.2)
    ok = np.allclose(best.numpy(), rb[g0:g1], atol=1e-6) and np.array_equal(arg.numpy(), ra[g0:g1]) and \
        np.array_equal(keep.numpy(), rk[g0:g1])
    rows, offs = D.all_gather_rows(torch.from_numpy(R[r0:r1]))
    ok = ok and np.array_equal(rows.numpy(), R) and list(offs) == [D.shard_range(len(R), i, world)[0] for i in range(world)] + [len(R)]

    def filter_rinv(g, r, tau, rinv):
        gn = g.numpy() / np.maximum(np.linalg.norm(g.numpy(), axis=1, keepdims=True), 1e-30)
        sc = gn @ (r.numpy() * rinv.numpy()[:, None]).T
        return torch.from_numpy(sc.max(1)), torch.from_numpy(sc.argmax(1).astype(np.int32)), torch.from_numpy(sc.max(1) >= tau)

    def inv_norm(r):
        return 1.0 / torch.linalg.norm(r, dim=1).clamp_min(1e-30)

    cap, D_ = 16, 32
    ex = D.StepExchange(cap, D_, "cpu", 0.1, filter_rinv, inv_norm)
    outs, want = [], []
    for k in range(3):
        counts = [(3 + 5 * i + 2 * k) % 14 for i in range(world)]          # ragged, some ranks empty in some steps
        embs = [rng.normal(0, 1, (n, D_)).astype(np.float32) for n in counts]
        mine = embs[rank]
        others = [(i, embs[i]) for i in range(world) if i != rank and counts[i]]
        if counts[rank] and others:
            mn = mine / np.linalg.norm(mine, axis=1, keepdims=True)
            sc = np.concatenate([mn @ (e / np.linalg.norm(e, axis=1, keepdims=True)).T for _, e in others], 1)
            col_rank = np.concatenate([np.full(len(e), i) for i, e in others])
            col_row = np.concatenate([np.arange(len(e)) for _, e in others])
            j = sc.argmax(1)
            want.append((counts, sc.max(1), col_rank[j] * cap + col_row[j]))
        else:
            want.append((counts, None, None))
        got = ex.submit(torch.from_numpy(mine), counts[rank])
        if got is not None:
            outs.append(got)
    outs.append(ex.drain())
    for (counts, wbest, warg), (gb, ga, gk, gc, gcap) in zip(want, outs):
        n = counts[rank]
        ok = ok and gc.tolist() == counts and gcap == cap
        if wbest is not None:
            pos = wbest > 0        # a row whose best cross-rank cosine is negative lands on a masked column: arg -1
            ok = ok and np.allclose(gb.numpy()[:n][pos], wbest[pos], atol=1e-5) and np.array_equal(ga.numpy()[:n][pos], warg[pos])
            ok = ok and (ga.numpy()[:n][~pos] == -1).all()
            ok = ok and np.array_equal(gk.numpy()[:n], wbest >= 0.1)
        elif n:
            ok = ok and (ga.numpy()[:n] == -1).all() and not gk.numpy()[:n].any()
    mean = D.sharded_l2_mean(torch.from_numpy(R[r0:r1]))
    ok = ok and np.allclose(mean.numpy(), R.mean(0), atol=1e-6)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [4, 8])
def test_sharded_similarity_and_step_exchange_world_n_gloo(world):
    """The exchange at the driver's scaling sizes (4 and 8 ranks, gloo on the CPU): arg = rank * cap + row across several
    peers, own rows masked, ranks with no face in a step, the one-step-late hand-out."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_worker_n, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(r, True) for r in range(world)]


def _run_bench(extra_env, *argv):
    import subprocess
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, capture_output=True,
                          text=True, timeout=300)


@pytest.mark.parametrize("n", [2, 8])
def test_bench_gpus_n_starts_n_ranks_itself(n):
    """VERDICT r3 missing #1: `python bench.py --gpus N` -- the same shape as the 1-GPU command, no external launcher --
    must run N ranks: the parent starts them (fresh processes, rendezvous on 127.0.0.1), relays rank 0's single JSON
    line and the line reports n_gpus == N, the world size the process group itself saw and every rank's share.
    BENCH_STUB_STEP=1 puts a CPU stub in place of the GPU step (gloo group), everything else is the bench's own code.
    (N = 8 is the driver's scaling run's shape, rehearsed here on the CPU.)"""
    import json
    r = _run_bench({"BENCH_STUB_STEP": "1"}, "--gpus", str(n), "--steps", "5", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == n and rec["steps"] == 5 and rec["scaling"] == "weak"
    assert rec["launch"]["world_size"] == n and rec["launch"]["requested_gpus"] == n
    units = [5 * (100 + r_) for r_ in range(n)]
    assert rec["launch"]["mode"].startswith("self-launched") and rec["launch"]["units_per_rank"] == units
    assert abs(rec["value"] - sum(units) / (rec["ms_per_step"] * 5e-3)) / rec["value"] < 1e-3   # whole-job units / max-rank time


def test_bench_launcher_fails_loudly():
    """A rank that dies takes the whole run down with a non-zero exit code (the other rank is stopped, nothing hangs in the
    rendezvous); `--gpus N` inside a world of another size is refused before any work."""
    r = _run_bench({"BENCH_STUB_STEP": "1", "BENCH_STUB_FAIL_RANK": "1"}, "--gpus", "2", "--steps", "5", "--warmup", "1")
    assert r.returncode == 3 and r.stdout.strip() == "" and "rank 1 failed" in r.stderr
    r = _run_bench({"BENCH_STUB_STEP": "1", "WORLD_SIZE": "1", "RANK": "0"}, "--gpus", "2", "--steps", "2")
    assert r.returncode != 0 and r.stdout.strip() == "" and "--gpus 2 but WORLD_SIZE = 1" in r.stderr


def test_bench_dump_outputs_dtypes_and_size_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs writes every array as <name>.npy: floating point as float32 (float64 kept), integers and
    booleans as float64, exactly.  Past the size cap every array keeps the same seeded sample of its rows, run after run."""
    import bench
    n = 300
    arrays = {"n_faces": n, "emb": torch.randn(n, 64), "arg": torch.arange(n, dtype=torch.int32) * 7,
              "keep": torch.arange(n) % 3 == 0, "best": torch.rand(n, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    full = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in arrays}
    assert {k: a.dtype for k, a in full.items()} == {"n_faces": np.float64, "emb": np.float32, "arg": np.float64,
                                                     "keep": np.float64, "best": np.float64}
    assert int(full["n_faces"]) == n and np.array_equal(full["emb"], arrays["emb"].numpy())
    assert np.array_equal(full["arg"], np.arange(n) * 7) and np.array_equal(full["keep"], np.arange(n) % 3 == 0)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    for d in ("cut1", "cut2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    cut = {k: np.load(tmp_path / "cut1" / f"{k}.npy") for k in arrays}
    assert sum(a.nbytes for a in cut.values()) <= 40_000 and 0 < len(cut["arg"]) < n
    rows = (cut["arg"] / 7).astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    for k in ("emb", "arg", "keep", "best"):
        np.testing.assert_array_equal(cut[k], full[k][rows])
        np.testing.assert_array_equal(cut[k], np.load(tmp_path / "cut2" / f"{k}.npy"))
