"""Candidate-restricted retrieval without a GPU: the CSR builder, the CPU provider against a plain numpy statement on the dense
moment scores (both levels, shards, rank counts), the two identities, the reference's own embeddings (G2), evaluate_candidates
on the CPU device against evaluate / evaluate_videos, a gloo world of 2, and the C entry point's host-side argument checks."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import MemoryDataset, make_model, problem
from subset_reference import keys_of, split_keys, statement

CPU_THREADS = 1


def _ragged(seed, nv=30, nq=11, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 9, nv).astype(np.int64)
    counts[3] = counts[2]
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    for v in range(0, nv, 7):                                 # repeated-clip videos: exact ties inside a triangle
        a = int(counts[:v].sum())
        V[a:a + counts[v]] = V[a]
    a, b = int(counts[:2].sum()), int(counts[:3].sum())
    V[b:b + counts[3]] = V[a:b]                               # video 3 duplicates video 2: equal scores, ids break the ties
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts


def _bank(ops, V, counts, id_base=0):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)


def _random_pools(rs, nq, nv, sizes):
    return [sorted(rs.choice(nv, min(int(s), nv), replace=False).tolist()) for s in sizes[:nq]]


def test_candidate_lists_sort_dedup_names_and_errors():
    from vfr_amd import engine
    names = [f"v{i}" for i in range(6)]
    cl = engine.candidate_lists([[3, 1, 3, 0], ["v5", 2, "v2"], [], ("v4",)], names=names)
    assert cl.off.tolist() == [0, 3, 5, 5, 6] and cl.vid.tolist() == [0, 1, 3, 2, 5, 4]
    assert cl.off.dtype == np.int64 and cl.vid.dtype == np.int32 and cl.max_list == 3 and cl.num_queries == 4
    off_t, vid_t = cl.on("cpu")
    assert off_t.tolist() == cl.off.tolist() and vid_t.dtype == torch.int32
    cl = engine.candidate_lists([np.array([4, 4, 2])], num_videos=5)
    assert cl.vid.tolist() == [2, 4] and cl.max_list == 2
    assert engine.candidate_lists([]).off.tolist() == [0] and engine.candidate_lists([]).max_list == 0
    with pytest.raises(ValueError):
        engine.candidate_lists([["nope"]], names=names)
    with pytest.raises(ValueError):
        engine.candidate_lists([[6]], names=names)
    with pytest.raises(ValueError):
        engine.candidate_lists([[-1]], num_videos=3)
    with pytest.raises(ValueError):
        engine.candidate_lists([["v1"]])                      # a name without the corpus' names


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("level", ["moments", "videos"])
def test_cpu_provider_matches_statement(seed, level):
    from vfr_amd import engine
    Q, V, counts = _ragged(seed)
    ops = engine.TorchCpuOps()
    rs = np.random.RandomState(100 + seed)
    nq, nv = Q.shape[0], len(counts)
    # a shard: videos [7, 7 + 15) of a corpus of nv videos; lists name corpus-global indices, some outside the shard
    lo, hi = 7, 22
    sub = counts[lo:hi]
    c0 = int(counts[:lo].sum())
    id_base = int((counts[:lo] * (counts[:lo] + 1) // 2).sum())
    bank = _bank(ops, V[c0:c0 + int(sub.sum())], sub, id_base)
    S = ops._dense(torch.from_numpy(Q), bank).numpy()
    sizes = [0, 1, 3, 5, nv, 9, 2, 12, 30, 4, 6]
    cl = engine.candidate_lists(_random_pools(rs, nq, nv, sizes), num_videos=nv)
    Kall = keys_of(S, id_base)
    for R in range(5):
        rk = Kall[np.arange(nq)[None, :].repeat(R, 0), rs.randint(0, S.shape[1], (R, nq))] if R else None
        for k in (0, 1, 7, 40, 448):
            if k == 0 and R == 0:
                continue
            rd, ri = split_keys(rk) if R else (None, None)
            d, i, c = ops.score_subset(torch.from_numpy(Q), bank, torch.from_numpy(cl.off), torch.from_numpy(cl.vid), k, level, lo, rd, ri)
            wd, wi, wc = statement(S, sub, cl.off, cl.vid, k, level, lo, id_base, rk)
            if k:
                assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd), (R, k)
            if R:
                assert np.array_equal(c.numpy(), wc), (R, k)


def test_cpu_identities():
    """A: every list = every video gives the full-corpus entry points; B: the own video alone gives its score_own row."""
    from vfr_amd import engine
    Q, V, counts = _ragged(3)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts, 5)
    nq, nv = Q.shape[0], len(counts)
    Qt = torch.from_numpy(Q)
    full = engine.candidate_lists([range(nv)] * nq, num_videos=nv)
    S = ops._dense(Qt, bank).numpy()
    rk = keys_of(S, 5)[np.arange(nq), (np.arange(nq) * 13) % S.shape[1]][None]
    rd, ri = split_keys(rk)
    for k in (1, 10, 100):
        d, i, c = ops.score_subset(Qt, bank, torch.from_numpy(full.off), torch.from_numpy(full.vid), k, "moments", 0, rd, ri)
        wd, wi, wc = ops.score_topk(Qt, bank, k, rd, ri)
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c, wc)
        d, i, c = ops.score_subset(Qt, bank, torch.from_numpy(full.off), torch.from_numpy(full.vid), k, "videos", 0, rd, ri)
        wd, wi, wc = ops.score_video_topk(Qt, bank, k, rd[0], ri[0])
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c[0], wc)
    own = np.arange(nq) % nv
    one = engine.candidate_lists([[int(v)] for v in own], num_videos=nv)
    sc = ops.score_own(Qt, bank, torch.from_numpy(own.astype(np.int32))).numpy()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    for k in (1, 4, 50):
        d, i, _ = ops.score_subset(Qt, bank, torch.from_numpy(one.off), torch.from_numpy(one.vid), k, "moments")
        for q in range(nq):
            M = int(mo[own[q] + 1] - mo[own[q]])
            order = np.argsort(sc[q, :M], kind="stable")[:k]
            n = min(k, M)
            assert np.array_equal(d[q, :n].numpy(), sc[q, order]) and np.array_equal(i[q, :n].numpy(), 5 + mo[own[q]] + order)
            assert np.all(np.isinf(d[q, n:].numpy())) and np.all(i[q, n:].numpy() == -1)


def test_cpu_empty_lists_and_padding():
    from vfr_amd import engine
    Q, V, counts = _ragged(5, nv=6, nq=3)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts)
    cl = engine.candidate_lists([[], [2], [0, 5]], num_videos=6)
    rd = torch.zeros((1, 3), dtype=torch.float32) + 1e9
    ri = torch.zeros((1, 3), dtype=torch.int64)
    for level in ("moments", "videos"):
        d, i, c = ops.score_subset(torch.from_numpy(Q), bank, torch.from_numpy(cl.off), torch.from_numpy(cl.vid), 448, level, 0, rd, ri)
        S = ops._dense(torch.from_numpy(Q), bank).numpy()
        wd, wi, wc = statement(S, counts, cl.off, cl.vid, 448, level, rank_keys=keys_of(np.full((1, 3), 1e9, np.float32)))
        assert np.array_equal(d.numpy(), wd) and np.array_equal(i.numpy(), wi) and np.array_equal(c.numpy(), wc)
        assert np.all(i[0].numpy() == -1) and c[0, 0] == 0
        n1 = 1 if level == "videos" else int(counts[2] * (counts[2] + 1) // 2)
        assert (i[1].numpy() >= 0).sum() == n1


@pytest.mark.parametrize("tag", ["n6", "ragged", "n21"])
def test_g2_reference_embeddings_full_pools(golden, tag):
    """The reference's own embeddings: with every pool = the whole corpus, the moment ranks through get_metrics are the
    reference's corpus metrics, and the top-100 is the reference's list (up to its fp32 rounding, as test_oracle_golden)."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    g = golden(f"g2_scoring_{tag}.npz")
    ops = engine.TorchCpuOps()
    counts = g["counts"].astype(np.int64)
    shard = engine.corpus_from_embeddings(torch.from_numpy(g["visual_emb"]), counts, "cpu", ops)
    Q = torch.from_numpy(g["query_emb"])
    own = g["own"].astype(np.int64)
    nq, nv = len(own), len(counts)
    labels = engine.gt_labels([t for t in g["times"].tolist()], counts[own], [0.5, 0.7], True, "cpu", ops)
    keys = engine.best_positive_keys(shard, Q, engine.prepare_gt(shard, own, labels), ops)
    full = engine.candidate_lists([range(nv)] * nq, num_videos=nv)
    d, i, v, ranks = engine.corpus_subset_topk(shard, Q, 100, full, "moments", ops=ops, rank_keys=keys)
    ref = json.loads(str(g["corpus_metrics"]))
    for r, thr in enumerate((0.5, 0.7)):
        rk = ranks[r].numpy()
        got = vevaluate.get_metrics({1: (rk < 1).astype(int), 10: (rk < 10).astype(int), 100: (rk < 100).astype(int), "MR": rk})
        for name, val in ref[f"model, IoU={thr}"].items():
            assert got[name] == pytest.approx(val, abs=1e-9), (thr, name)
    ri = i.numpy()
    assert float(np.abs(d.numpy() - g["top_dist"]).max()) < 2e-6
    assert np.array_equal(ri[:, :10], g["top_idx"][:, :10]) and (ri == g["top_idx"]).mean() >= 0.995
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    assert np.array_equal(v.numpy(), np.searchsorted(mo, ri, side="right") - 1)


def _evaluate_pair(p, level, pools=None, rank=0, world=1):
    from vfr_amd import evaluate as vevaluate
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16)
    nv = len(p["counts"])
    if pools is None:
        pools = [range(nv)] * len(p["own"])
    vi, li = ds.iterators()
    return vevaluate.evaluate_candidates(model, vi, li, ds.annotations, "cpu", pools, level=level, rank=rank, world=world,
                                         return_topk=20), ds, model


def test_evaluate_candidates_full_pools_equal_evaluate_cpu():
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        (got, (d, i, v)), ds, model = _evaluate_pair(p, "moments")
        vi, li = ds.iterators()
        want = vevaluate.evaluate(model, vi, li, ds.annotations, "cpu")
        assert got == want
        vi, li = ds.iterators()
        wantd, (wd, wi) = vevaluate.evaluate(model, vi, li, ds.annotations, "cpu", return_topk=20)
        assert torch.equal(d, wd) and torch.equal(i, wi)
        (got, (d, i, v)), ds, model = _evaluate_pair(p, "videos")
        vi, li = ds.iterators()
        want, (wd, wi, wv) = vevaluate.evaluate_videos(model, vi, li, ds.annotations, "cpu", return_topk=20)
        assert got == want and torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(v, wv)
        # a pool of the own video alone: video rank 0 for every query; the moment ranks are those inside the own video
        (got, _), _, _ = _evaluate_pair(p, "videos", pools=[[]] * len(p["own"]))
        assert got["video"]["R@1"] == 100.0 and got["video"]["MR"] == 0
    finally:
        torch.set_num_threads(threads)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pools_for(p, seed=9):
    rs = np.random.RandomState(seed)
    nv = len(p["counts"])
    return [rs.choice(nv, rs.randint(0, nv), replace=False).tolist() for _ in range(len(p["own"]))]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(CPU_THREADS)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        res = {}
        for level in ("moments", "videos"):
            (metrics, (d, i, v)), _, _ = _evaluate_pair(p, level, _pools_for(p), rank, world)
            res[level] = (repr(metrics), d.numpy(), i.numpy(), v.numpy())
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{f"{lv}_{n}": x for lv, t in res.items() for n, x in zip("mdiv", t)})
    finally:
        dist.destroy_process_group()


def test_two_rank_subset_equals_single_process(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        ref = {level: _evaluate_pair(p, level, _pools_for(p))[0] for level in ("moments", "videos")}
    finally:
        torch.set_num_threads(threads)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npz")
        for level, (metrics, (d, i, v)) in ref.items():
            assert str(got[f"{level}_m"]) == repr(metrics)
            assert np.array_equal(got[f"{level}_d"], d.numpy()) and np.array_equal(got[f"{level}_i"], i.numpy())
            assert np.array_equal(got[f"{level}_v"], v.numpy())


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 16)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def call(Nq=4, max_clips=21, k=10, level=0, cand_off=dummy, D=100, num_rank=0, nnz=8, max_list=4):
        return lib.vfr_score_subset_f32(dummy, Nq, dummy, dummy, dummy, 10, 210, 21, max_clips, D, 1e-6, 0, 0, cand_off, dummy, nnz,
                                        max_list, level, k, dummy, dummy, num_rank, None, None, None, None, dummy, 1 << 16, None)
    assert call(k=449) == -1
    assert call(max_clips=65) == -1
    assert call(cand_off=None) == -1
    assert call(level=2) == -1 and call(level=-1) == -1
    assert call(num_rank=5) == -1 and call(num_rank=1) == -1     # rank keys without their arrays
    assert call(nnz=-1) == -1 and call(max_list=-1) == -1
    assert b"vfr_score_subset_f32" in lib.vfr_last_error()
    assert lib.vfr_score_subset_workspace_bytes(4, 8, 4, 10, 2) == 0
    assert lib.vfr_score_subset_workspace_bytes(4, 8, 4, 10, 1) >= 8 * 8
    # moments: (nnz + 63 Nq) / 64 chunks x k keys, no more than Nq ceil(max_list / 64) chunks
    assert lib.vfr_score_subset_workspace_bytes(4, 8, 4, 10, 0) >= 4 * 10 * 8
    assert lib.vfr_score_subset_workspace_bytes(5000, 500000, 100, 100, 0) < 13000 * 100 * 8 + 65536
