"""Diversified moment retrieval without a GPU: the exact IoU table of the C ABI, a hand-worked example, the CPU provider against
the plain statement (tests/nms_reference.py) and against the video / moment top-k it reduces to, evaluate_moments_nms on the
CPU device and the sharded protocol over a gloo world of 2."""
import ctypes
import itertools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import MemoryDataset, make_model, problem
from nms_reference import expected_nms

CPU_THREADS = 1
THRESHOLDS = (0.0, 0.1 + 0.2, 1 / 3, 0.5, 0.69999999, 0.7, 0.9999, 1.0)


def test_inter_table_equals_float64_iou():
    from vfr_amd import _vfr
    from vfr_amd.utils import generate_moments, get_iou
    spans = np.asarray(generate_moments(64), np.int64)
    s, e = spans[:, 0], spans[:, 1]
    for thr in THRESHOLDS:
        tab = _vfr.nms_inter_table(thr, 64)
        assert tab.shape == (65,)
        for a in range(0, len(spans), 7):                    # every 7th span against all 2080 (n = 64 covers n < 64)
            want = get_iou(spans, int(s[a]), int(e[a])) > thr
            inter = np.maximum(np.minimum(e, e[a]) + 1 - np.maximum(s, s[a]), 0)
            union = np.maximum(e, e[a]) + 1 - np.minimum(s, s[a])
            assert np.array_equal(inter >= tab[union], want), (thr, a)
    # the fp32 trap of the issue: 7/10 > 0.69999999 in float64 only
    assert _vfr.nms_inter_table(0.69999999, 10)[10] == 7
    assert np.float32(0.7) <= np.float32(0.69999999)


def test_inter_table_rejects_bad_thresholds():
    from vfr_amd import _vfr
    buf = (ctypes.c_int32 * 65)()
    assert _vfr.lib().vfr_nms_inter_table(float("nan"), 64, buf) == -1
    assert _vfr.lib().vfr_nms_inter_table(-0.1, 64, buf) == -1
    assert _vfr.lib().vfr_nms_inter_table(0.5, -1, buf) == -1
    assert _vfr.lib().vfr_nms_inter_table(0.5, 64, None) == -1
    assert _vfr.lib().vfr_nms_inter_table(2.0, 64, buf) == 0 and all(buf[u] == u + 1 for u in range(1, 65))


def _cpu_bank(V, counts, id_base=0):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ops, ops.make_bank(torch.from_numpy(np.ascontiguousarray(V, np.float32)), torch.from_numpy(off), id_base)


def test_hand_worked_three_and_four_clip_videos():
    """D = 1, query 0: a moment's score is the mean of its clip values (plus eps).
    video 0 (3 clips 2.0, 1.5, 2.6): (1,1) 1.5, (0,1) 1.75, (0,0) 2.0, (0,2) 2.033, (1,2) 2.05, (2,2) 2.6
    video 1 (4 clips 0.1, 0.32, 0.9, 0.2): (0,0) .1, (3,3) .2, (0,1) .21, (1,1) .32, (0,3) .38, (0,2) .44, (1,3) .473,
    (2,3) .55, (1,2) .61, (2,2) .9.  nms_iou = 0.4: (0,1) has IoU 1/2 with (0,0); (0,2), (1,3) 3/4, (2,3), (1,2) 1/2 with
    (0,3); in video 0 (0,1) 1/2 with (1,1), (1,2) 2/3 with (0,2)."""
    from vfr_amd import engine
    counts = np.array([3, 4], np.int64)
    V = np.array([[2.0], [1.5], [2.6], [0.1], [0.32], [0.9], [0.2]], np.float32)
    ops, bank = _cpu_bank(V, counts)
    Q = torch.zeros((1, 1))
    mo = np.array([0, 6, 16], np.int64)
    names = ["three", "four"]
    spans = lambda idx, dist: [(n, s, e) for n, s, e, _ in engine.video_results(idx, dist, names, counts, mo)[0]]
    d, i = ops.score_moment_nms(Q, bank, 10, 0, 0.4)
    assert spans(i, d) == [("four", 0, 0), ("four", 3, 3), ("four", 1, 1), ("four", 0, 3), ("four", 2, 2),
                           ("three", 1, 1), ("three", 0, 0), ("three", 0, 2), ("three", 2, 2)]
    assert i[0, 9] == -1 and d[0, 9] == float("inf")
    d, i = ops.score_moment_nms(Q, bank, 10, 2, 0.4)
    assert spans(i, d) == [("four", 0, 0), ("four", 3, 3), ("three", 1, 1), ("three", 0, 0)]
    d, i = ops.score_moment_nms(Q, bank, 3, 0, 0.0)             # disjoint spans only
    assert spans(i, d) == [("four", 0, 0), ("four", 3, 3), ("four", 1, 1)]
    d, i = ops.score_moment_nms(Q, bank, 4, 0, 1.0)             # no suppression: the moment ranking
    assert spans(i, d) == [("four", 0, 0), ("four", 3, 3), ("four", 0, 1), ("four", 1, 1)]


def _ragged(seed, nv=40, nq=9, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 12, nv).astype(np.int64)
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    V[:counts[0]] = V[0]                                      # a repeated-clip video
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    Q[0] = V[0]                                               # a query that sits on it
    return Q, V, counts


@pytest.mark.parametrize("seed", [1, 2])
def test_cpu_provider_matches_statement(seed):
    Q, V, counts = _ragged(seed)
    ops, bank = _cpu_bank(V, counts, id_base=1000)
    S = ops._dense(torch.from_numpy(Q), bank).numpy()
    for k, per_video, thr in itertools.product((1, 7, 30), (0, 1, 2, 5), (0.0, 0.5, 1 / 3, 1.0)):
        d, i = ops.score_moment_nms(torch.from_numpy(Q), bank, k, per_video, thr)
        wd, wi, wv = expected_nms(S, counts, k, per_video, thr, id_base=1000)
        assert np.array_equal(i.numpy(), wi), (k, per_video, thr)
        assert np.array_equal(d.numpy(), wd), (k, per_video, thr)
        for q in range(len(Q)):                               # the cap holds
            vv = wv[q][wv[q] >= 0]
            assert per_video == 0 or np.bincount(vv).max(initial=0) <= per_video


def test_cpu_identities():
    Q, V, counts = _ragged(3, nv=25)
    ops, bank = _cpu_bank(V, counts)
    q = torch.from_numpy(Q)
    for k in (1, 5, 40):
        vd, vi, _ = ops.score_video_topk(q, bank, k)
        d, i = ops.score_moment_nms(q, bank, k, 1, 0.5)       # identity A (any nms_iou)
        assert torch.equal(i, vi) and torch.equal(d, vd)
        td, ti, _ = ops.score_topk(q, bank, k, None, None)
        for pv in (0, k, k + 3):                              # identity B
            for thr in (1.0, 1.5):
                d, i = ops.score_moment_nms(q, bank, k, pv, thr)
                assert torch.equal(i, ti) and torch.equal(d, td), (k, pv, thr)


def _positive_statement(p, per_video, nms_iou, ks=(1, 10, 100), thresholds=(0.5, 0.7)):
    """evaluate_moments_nms' numbers from the statement on the CPU device's own embeddings and scores."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    from vfr_amd.utils import generate_moments, get_iou
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16)
    ops = engine.TorchCpuOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, "cpu", ops)
    tokens, q_videos, annot_ids = vevaluate._drain_queries(li)
    Q = engine.encode_queries(model, torch.cat(tokens), "cpu", ops)
    S = ops._dense(Q.float(), shard.bank).numpy()
    own = np.asarray([names.index(x) for x in q_videos], np.int64)
    K = max(ks)
    wd, wi, wv = expected_nms(S, shard.counts_all, K, per_video, nms_iou)
    mo = np.asarray(shard.mom_off_all, np.int64)
    out = {}
    for thr in thresholds:
        first = np.full(len(own), K)
        for q in range(len(own)):
            times = ds.annotations[annot_ids[q]]["times"]
            for j in range(K):
                if wv[q, j] != own[q]:
                    continue
                s, e = generate_moments(int(shard.counts_all[own[q]]))[wi[q, j] - mo[own[q]]]
                if (get_iou(times, s, e) > thr).sum() >= 2:
                    first[q] = j
                    break
        out[f"model, IoU={thr}"] = vevaluate.get_metrics({k: (first < k).astype(int) for k in ks})
    return out, wd, wi, wv


@pytest.mark.parametrize("per_video,nms_iou", [(0, 0.5), (2, 0.3), (0, 1.0)])
def test_evaluate_moments_nms_cpu(per_video, nms_iou):
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        model.train()
        vi, li = ds.iterators()
        metrics, (d, i, v) = vevaluate.evaluate_moments_nms(model, vi, li, ds.annotations, "cpu", per_video=per_video,
                                                            nms_iou=nms_iou, return_topk=True)
        assert model.training
        want, wd, wi, wv = _positive_statement(p, per_video, nms_iou)
        if per_video == 0 and nms_iou >= 1:                   # the plain moment ranking: evaluate's R@k
            vi, li = ds.iterators()
            plain = vevaluate.evaluate(model, vi, li, ds.annotations, "cpu")
            for key, m in plain.items():
                assert metrics[key] == {n: x for n, x in m.items() if n != "MR"}
    finally:
        torch.set_num_threads(threads)
    assert metrics == want
    assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd) and np.array_equal(v.numpy(), wv)


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
        metrics, (d, i, v) = vevaluate.evaluate_moments_nms(model, vi, li, ds.annotations, "cpu", per_video=2, nms_iou=0.5,
                                                            rank=rank, world=world, return_topk=True)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), metrics=repr(metrics), d=d.numpy(), i=i.numpy(), v=v.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_moment_nms_equals_single_process(tmp_path):
    from vfr_amd import evaluate as vevaluate
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        vi, li = ds.iterators()
        ref, (rd, ri, rv) = vevaluate.evaluate_moments_nms(make_model(p["sd"], feat_dim=64, hidden=16), vi, li, ds.annotations,
                                                           "cpu", per_video=2, nms_iou=0.5, return_topk=True)
    finally:
        torch.set_num_threads(threads)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npz")
        assert str(got["metrics"]) == repr(ref)
        assert np.array_equal(got["i"], ri.numpy()) and np.array_equal(got["d"], rd.numpy())
        assert np.array_equal(got["v"], rv.numpy())
