"""Video-level retrieval without a GPU: the CPU provider, evaluate_videos on the CPU device, the id -> result-row mapping and
the sharded protocol over a gloo world of 2, each against a plain numpy statement on the dense moment scores (stable
(distance, global id) sort, first occurrence per video, first k, videos ahead of the own video)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import MemoryDataset, make_model, problem

CPU_THREADS = 1


def expected(S, counts, k, own=None, id_base=0):
    counts = np.asarray(counts, np.int64)
    M = counts * (counts + 1) // 2
    vid_of = np.repeat(np.arange(len(counts)), M)
    ids = id_base + np.arange(S.shape[1], dtype=np.int64)
    Nq = S.shape[0]
    od = np.full((Nq, k), np.inf, np.float32)
    oi = np.full((Nq, k), -1, np.int64)
    ov = np.full((Nq, k), -1, np.int64)
    ranks = np.zeros(Nq, np.int64) if own is not None else None
    for q in range(Nq):
        order = np.lexsort((ids, S[q]))
        v = vid_of[order]
        _, first = np.unique(v, return_index=True)
        pos = order[np.sort(first)]
        n = min(k, len(pos))
        od[q, :n], oi[q, :n], ov[q, :n] = S[q, pos[:n]], ids[pos[:n]], vid_of[pos[:n]]
        if own is not None:
            ranks[q] = int(np.nonzero(vid_of[pos] == own[q])[0][0])
    return od, oi, ov, ranks


def _cpu_problem(seed=4, nv=30, nq=12, D=16):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 9, nv).astype(np.int64)
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    for v in range(0, nv, 6):                                 # repeated-clip videos
        a = int(counts[:v].sum())
        V[a:a + counts[v]] = V[a]
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    own = rs.randint(0, nv, nq).astype(np.int64)
    return Q, V, counts, own


def test_cpu_provider_matches_numpy_statement():
    from vfr_amd import engine
    Q, V, counts, own = _cpu_problem()
    ops = engine.TorchCpuOps()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), 0)
    S = ops._dense(torch.from_numpy(Q), bank).numpy()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    od_own = np.array([S[q, mo[v]:mo[v + 1]].min() for q, v in enumerate(own)], np.float32)
    oi_own = np.array([mo[v] + int(np.lexsort((np.arange(mo[v + 1] - mo[v]), S[q, mo[v]:mo[v + 1]]))[0])
                       for q, v in enumerate(own)], np.int64)
    for k in (1, 5, len(counts) + 3):
        d, i, c = ops.score_video_topk(torch.from_numpy(Q), bank, k, torch.from_numpy(od_own), torch.from_numpy(oi_own))
        wd, wi, _, wr = expected(S, counts, k, own)
        assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd) and np.array_equal(c.numpy(), wr)


def _reference_videos(p, k):
    """evaluate_videos' numbers from the numpy statement on the CPU device's own embeddings and scores."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16)
    ops = engine.TorchCpuOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, "cpu", ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Q = engine.encode_queries(model, torch.cat(tokens), "cpu", ops)
    S = ops._dense(Q.float(), shard.bank).numpy()
    own = np.asarray([names.index(x) for x in q_videos], np.int64)
    wd, wi, wv, wr = expected(S, shard.counts_all, k, own)
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 10: (wr < 10).astype(int), 100: (wr < 100).astype(int), "MR": wr})
    return {"video": want}, wd, wi, wv


def test_evaluate_videos_cpu():
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        model.train()
        vi, li = ds.iterators()
        metrics, (d, i, v) = vevaluate.evaluate_videos(model, vi, li, ds.annotations, "cpu", return_topk=10)
        assert model.training
        want, wd, wi, wv = _reference_videos(p, 10)
    finally:
        torch.set_num_threads(threads)
    assert metrics == want
    assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd) and np.array_equal(v.numpy(), wv)


def test_result_rows_map_ids_to_names_and_spans():
    from vfr_amd import engine
    from vfr_amd.utils import generate_moments
    counts = np.array([3, 1, 4], np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    names = ["a", "b", "c"]
    ids = np.array([[mo[2] + 5, mo[1], -1], [2, mo[2] + 9, 4]], np.int64)
    dist = np.array([[0.5, 0.75, np.inf], [1.0, 1.5, 2.0]], np.float32)
    rows = engine.video_results(ids, dist, names, counts, mo)
    s, e = generate_moments(4)[5]
    assert rows[0] == [("c", s, e, 0.5), ("b", 0, 0, 0.75)]
    s9, e9 = generate_moments(4)[9]
    s4, e4 = generate_moments(3)[4]
    assert rows[1] == [("a", 2, 2, 1.0), ("c", s9, e9, 1.5), ("a", s4, e4, 2.0)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(CPU_THREADS)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vfr_amd import evaluate as vevaluate
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        vi, li = ds.iterators()
        metrics, (d, i, v) = vevaluate.evaluate_videos(model, vi, li, ds.annotations, "cpu", rank=rank, world=world,
                                                       return_topk=10)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), metrics=repr(metrics), d=d.numpy(), i=i.numpy(), v=v.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_video_topk_equals_single_process(tmp_path):
    from vfr_amd import evaluate as vevaluate
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        vi, li = ds.iterators()
        ref, (rd, ri, rv) = vevaluate.evaluate_videos(make_model(p["sd"], feat_dim=64, hidden=16), vi, li, ds.annotations,
                                                      "cpu", return_topk=10)
    finally:
        torch.set_num_threads(threads)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npz")
        assert str(got["metrics"]) == repr(ref)
        assert np.array_equal(got["i"], ri.numpy()) and np.array_equal(got["d"], rd.numpy())
        assert np.array_equal(got["v"], rv.numpy())
