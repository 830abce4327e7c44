"""gloo tests (CPU, world size 2 and 3) of distributed.sharded_cosine_topk: a gallery sharded by rows gives every rank the
single-rank result on the concatenated gallery, ties and short shards included."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

K = 5


def topk_cpu(q, g, k):
    """The CPU stand-in for similarity.cosine_topk: fp64 cosine scores, stable descending order, -inf / -1 beyond the rows."""
    q, g = q.numpy().astype(np.float64), g.numpy().astype(np.float64)
    s = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-300)).T
    s = s.astype(np.float32)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    sc = np.full((q.shape[0], k), -np.inf, np.float32)
    ix = np.full((q.shape[0], k), -1, np.int32)
    sc[:, :order.shape[1]] = np.take_along_axis(s, order, axis=1)
    ix[:, :order.shape[1]] = order
    return torch.from_numpy(sc), torch.from_numpy(ix)


def _bounds(world):
    """Shard boundaries: rank 0 takes 20 rows, the last rank only 3 (fewer than K), the rest the middle."""
    return {2: [0, 20, 23], 3: [0, 20, 40, 43]}[world]


def _gallery(world):
    rng = np.random.default_rng(7)
    n = _bounds(world)[-1]
    G = rng.normal(0, 1, (n, 32)).astype(np.float32)
    G[20] = G[19]                      # a duplicate pair straddling the boundary of shards 0 and 1
    Q = np.concatenate([G[[19]], rng.normal(0, 1, (9, 32)).astype(np.float32)])
    return Q, G


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from face_detection_and_recognition_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ok = _checks(D, rank, world)
    except Exception as e:                # (reported, so that the parent does not wait for a result that never comes)
        ok = repr(e)
    q.put((rank, ok))
    dist.destroy_process_group()


def _checks(D, rank, world):
    Q, G = _gallery(world)
    b = _bounds(world)
    sc, ix = D.sharded_cosine_topk(torch.from_numpy(Q), torch.from_numpy(G[b[rank]:b[rank + 1]]), K, topk_cpu)
    wsc, wix = topk_cpu(torch.from_numpy(Q), torch.from_numpy(G), K)
    ok = torch.equal(sc, wsc) and torch.equal(ix, wix) and ix.dtype == torch.int32
    ok = ok and ix[0, :2].tolist() == [19, 20] and float(sc[0, 0]) == float(sc[0, 1])      # lower global index first
    # fewer gallery rows in all than k: the tail stays -inf / -1 after the merge
    tiny = torch.from_numpy(G[rank:rank + 1])
    sc2, ix2 = D.sharded_cosine_topk(torch.from_numpy(Q), tiny, K, topk_cpu)
    wsc2, wix2 = topk_cpu(torch.from_numpy(Q), torch.from_numpy(G[:world]), K)
    ok = ok and torch.equal(sc2, wsc2) and torch.equal(ix2, wix2) and bool((ix2[:, world:] == -1).all())
    return bool(ok)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_cosine_topk_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(r, True) for r in range(world)]
