"""Sentence retrieval for moments without a GPU: the CPU provider and engine.corpus_sentence_topk against the numpy statement of
tests/sentences_reference.py, the probe selection of evaluate_sentences, evaluate_sentences end to end on CPU tensors, argument
errors, a gloo world of 2, and the C entry point's host-side argument checks and workspace-size properties."""
import ctypes
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import MemoryDataset, make_model, problem
from sentences_reference import dense_blocks, probe_keys, rank_keys_for, split_keys, statement

CPU_THREADS = 1


def _ragged(seed, nv=20, ns=41, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 9, nv).astype(np.int64)
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    a = int(counts[:4].sum())
    V[a:a + counts[4]] = V[a]                                 # a video of repeated clips
    S = (rs.randn(ns, D) * 0.3).astype(np.float32)
    S[10:14] = S[3]                                           # duplicated sentences: the sentence id decides
    return S, V, counts


def _bank(ops, V, counts, id_base=0):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)


def _probes(rs, counts, nm, base=0):
    v = rs.randint(0, len(counts), nm)
    n = counts[v]
    s = (rs.rand(nm) * n).astype(np.int64)
    e = s + (rs.rand(nm) * (n - s)).astype(np.int64)
    return np.stack([v + base, s, e], axis=1).astype(np.int64)


@pytest.mark.parametrize("seed", [0, 1])
def test_cpu_provider_matches_statement(seed):
    from vfr_amd import engine
    S, V, counts = _ragged(seed)
    ops = engine.TorchCpuOps()
    rs = np.random.RandomState(50 + seed)
    lo, hi = 5, 16                                            # a shard: global videos [5, 16)
    sub = counts[lo:hi]
    c0 = int(counts[:lo].sum())
    bank = _bank(ops, V[c0:c0 + int(sub.sum())], sub)
    Sc = ops._dense(torch.from_numpy(S), bank).numpy()
    block = dense_blocks(Sc, sub)
    probes = np.concatenate([_probes(rs, counts, 40), [[lo, 0, 0], [lo, 0, 0], [-1, 0, 0], [lo + 1, 2, 1], [lo + 2, 0, 99]]])
    keys, _ = probe_keys(block, sub, probes, len(S), lo, 7)
    for R in range(5):
        rk = rank_keys_for(keys, rs, R) if R else None
        for k in (0, 1, 7, 41, 100):
            if k == 0 and R == 0:
                continue
            rd, ri = split_keys(rk) if R else (None, None)
            bad = torch.zeros(1, dtype=torch.int32)
            d, i, c = ops.score_sentences(torch.from_numpy(S), bank, torch.from_numpy(probes), k, lo, 7, rd, ri, bad=bad)
            wd, wi, wc, wbad = statement(block, sub, probes, len(S), k, lo, 7, rk)
            assert int(bad) == wbad == 1
            if k:
                assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd), (R, k)
            if R:
                assert np.array_equal(c.numpy(), wc), (R, k)
            else:
                assert c is None


def test_cpu_counts_are_added_and_shards_chain():
    from vfr_amd import engine
    S, V, counts = _ragged(3)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts)
    rs = np.random.RandomState(4)
    probes = _probes(rs, counts, 25)
    block = dense_blocks(ops._dense(torch.from_numpy(S), bank).numpy(), counts)
    keys, _ = probe_keys(block, counts, probes, len(S))
    rd, ri = split_keys(rank_keys_for(keys, rs, 2))
    St, pt = torch.from_numpy(S), torch.from_numpy(probes)
    d1, i1, c1 = ops.score_sentences(St, bank, pt, 9, 0, 0, rd, ri)
    da, ia, cc = ops.score_sentences(St[:17], bank, pt, 9, 0, 0, rd, ri)
    db, ib, cc = ops.score_sentences(St[17:], bank, pt, 9, 0, 17, rd, ri, count_lt=cc)
    dm, im = ops.topk_merge(torch.stack([da, db]), torch.stack([ia, ib]))
    assert torch.equal(dm, d1) and torch.equal(im, i1) and torch.equal(cc, c1)


def test_corpus_sentence_topk_own_ranks_cpu():
    from vfr_amd import engine
    S, V, counts = _ragged(5)
    ops = engine.TorchCpuOps()
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    rs = np.random.RandomState(6)
    probes = np.concatenate([_probes(rs, counts, 30), [[2, 0, 50]]])          # the last span leaves its video: padding, rank 0
    own = rs.randint(0, len(S), len(probes))
    block = dense_blocks(ops._dense(torch.from_numpy(S), shard.bank).numpy(), counts)
    keys, _ = probe_keys(block, counts, probes, len(S))
    rk = np.asarray([0 if kk is None else kk[own[m]] for m, kk in enumerate(keys)], np.uint64)[None]
    d, i, ranks = engine.corpus_sentence_topk(shard, torch.from_numpy(S), probes, 8, own, ops)
    wd, wi, wc, _ = statement(block, counts, probes, len(S), 8, rank_keys=rk)
    assert np.array_equal(d.numpy(), wd) and np.array_equal(i.numpy(), wi) and np.array_equal(ranks.numpy(), wc[0])
    assert ranks.dtype == torch.int64 and int(ranks[-1]) == 0 and np.all(i[-1].numpy() == -1)
    d, i, ranks = engine.corpus_sentence_topk(shard, torch.from_numpy(S), probes, 8, None, ops)
    assert ranks is None and np.array_equal(i.numpy(), wi)
    _, _, ranks = engine.corpus_sentence_topk(shard, torch.from_numpy(S), probes, 0, own, ops)
    assert np.array_equal(ranks.numpy(), wc[0])
    with pytest.raises(ValueError):
        engine.corpus_sentence_topk(shard, torch.from_numpy(S), probes, 8, own[:-1], ops)
    with pytest.raises(ValueError):
        engine.corpus_sentence_topk(shard, torch.from_numpy(S), probes, 8, np.full(len(probes), len(S)), ops)


def test_sentence_probes_selection():
    from vfr_amd import evaluate as vevaluate
    ann = {
        "a": {"times": [[1, 2], [0, 0], [1, 2], [0, 0]]},             # tie 2 : 2 -> the first seen, (1, 2)
        "b": {"times": [[0, 9], [0, 9], [3, 3]]},                     # (0, 9) leaves a 5-clip video: dropped, (3, 3) is left
        "c": {"times": [[4, 7], [-1, 2], [3, 2]]},                    # nothing inside the video: no probe
        "d": {"times": [[2, 4], [0, 1], [2, 4], [0, 1], [0, 1]]},     # the most common, (0, 1)
    }
    counts = np.asarray([5, 5, 4, 6])
    probes, rows = vevaluate.sentence_probes(ann, ["a", "b", "c", "d"], np.asarray([0, 1, 2, 3]), counts)
    assert probes.tolist() == [[0, 1, 2], [1, 3, 3], [3, 0, 1]] and rows.tolist() == [0, 1, 3]
    probes, rows = vevaluate.sentence_probes(ann, ["c"], np.asarray([2]), counts)
    assert probes.shape == (0, 3) and rows.shape == (0,)


def _statement_metrics(p, model, ds):
    """The numpy statement on the CPU provider's own embeddings and dense scores."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    ops = engine.TorchCpuOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, "cpu", ops)
    tokens, q_videos, annot_ids = vevaluate._drain_queries(li)
    Se = engine.encode_queries(model, torch.cat(tokens), "cpu", ops)
    own = np.asarray([names.index(v) for v in q_videos])
    probes, rows = vevaluate.sentence_probes(ds.annotations, annot_ids, own, p["counts"])
    block = dense_blocks(ops._dense(Se, shard.bank).numpy(), p["counts"])
    keys, _ = probe_keys(block, p["counts"], probes, len(Se))
    rk = np.asarray([keys[m][rows[m]] for m in range(len(rows))], np.uint64)[None]
    wd, wi, wc, _ = statement(block, p["counts"], probes, len(Se), 12, rank_keys=rk)
    want = vevaluate.get_metrics({1: (wc[0] < 1).astype(int), 10: (wc[0] < 10).astype(int), 100: (wc[0] < 100).astype(int), "MR": wc[0]})
    if len(rows) < len(annot_ids):
        want["skipped"] = len(annot_ids) - len(rows)
    return {"sentence": want}, wd, wi, rows


def _evaluate(p, rank=0, world=1):
    from vfr_amd import evaluate as vevaluate
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16)
    vi, li = ds.iterators()
    return vevaluate.evaluate_sentences(model, vi, li, ds.annotations, "cpu", rank=rank, world=world, return_topk=12), ds, model


def test_evaluate_sentences_cpu_end_to_end():
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        (got, (d, i, rows)), ds, model = _evaluate(p)
        want, wd, wi, wrows = _statement_metrics(p, model, ds)
        assert got == want and set(got["sentence"]) >= {"R@1", "R@10", "R@100", "MR"}
        assert np.array_equal(rows, wrows) and np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd)
        vi, li = ds.iterators()
        assert vevaluate.evaluate_sentences(model, vi, li, ds.annotations, "cpu") == got
        # an annotation whose spans all leave its video is skipped and counted
        times = [list(t) for t in p["times"]]
        times[4] = [[90, 95]] * len(times[4])
        ds2 = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], times)
        vi, li = ds2.iterators()
        out = vevaluate.evaluate_sentences(model, vi, li, ds2.annotations, "cpu")
        assert out["sentence"]["skipped"] == 1 + got["sentence"].get("skipped", 0)
        # empty query iterator: the metrics of empty lists, as evaluate_videos
        vi, _ = ds.iterators()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # mean / median of an empty list
            empty = vevaluate.evaluate_sentences(model, vi, iter(()), ds.annotations, "cpu")
        assert set(empty["sentence"]) == {"R@1", "R@10", "R@100", "MR"}
    finally:
        torch.set_num_threads(threads)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(CPU_THREADS)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        (metrics, (d, i, rows)), _, _ = _evaluate(p, rank, world)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), m=repr(metrics), d=d.numpy(), i=i.numpy(), rows=rows)
    finally:
        dist.destroy_process_group()


def test_two_rank_sentences_equal_single_process(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        (metrics, (d, i, rows)), _, _ = _evaluate(p)
    finally:
        torch.set_num_threads(threads)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npz")
        assert str(got["m"]) == repr(metrics)
        assert np.array_equal(got["d"], d.numpy()) and np.array_equal(got["i"], i.numpy()) and np.array_equal(got["rows"], rows)


def test_wrapper_refuses_cpu_tensors():
    from vfr_amd import _vfr
    with pytest.raises(RuntimeError):
        _vfr.score_sentences(torch.zeros((3, 100)), None, torch.zeros((1, 3), dtype=torch.int32), 1)


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 20)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def call(S=dummy, Ns=64, V=dummy, off=dummy, Nv=10, max_clips=21, D=100, probes=dummy, Nm=4, vid_base=0, sent_base=0, k=10,
             od=dummy, oi=dummy, num_rank=0, wsb=1 << 20):
        return lib.vfr_score_sentences_f32(S, Ns, V, off, Nv, 210, max_clips, D, 1e-6, probes, Nm, vid_base, sent_base, k, od, oi,
                                           num_rank, None, None, None, None, dummy, wsb, None)
    assert call(k=449) == -1 and call(k=-1) == -1
    assert call(max_clips=65) == -1
    assert call(probes=None) == -1 and call(S=None) == -1 and call(off=None) == -1 and call(od=None) == -1
    assert call(Ns=-1) == -1 and call(Nm=-1) == -1 and call(Nv=-1) == -1 and call(D=0) == -1
    assert call(vid_base=-1) == -1 and call(sent_base=-1) == -1
    assert call(num_rank=5) == -1 and call(num_rank=1) == -1      # rank keys without their arrays
    assert call(Ns=1 << 32) == -1 and call(sent_base=(1 << 32) - 64) == -1
    assert call(Nm=1 << 30, k=2) == -1
    assert b"vfr_score_sentences_f32" in lib.vfr_last_error()
    assert call(wsb=8) == -4
    size = lib.vfr_score_sentences_workspace_bytes
    assert size(4, 64, 449) == 0 and size(-1, 64, 10) == 0 and size(4, -1, 10) == 0 and size(4, 64, -1) == 0
    assert size(1 << 30, 64, 2) == 0
    assert size(4, 64, 10) >= 4 * 10 * 8 and size(4, 64, 0) > 0 and size(0, 0, 0) > 0
    # no Nm x Ns term: the number of sentence chunks is capped, so the size stops growing with Ns and is at most linear in Nm
    for Nm in (1, 8, 100, 5000, 33000):
        for k in (1, 100, 448):
            assert size(Nm, 1 << 24, k) == size(Nm, 1 << 25, k)
            assert size(2 * Nm, 1 << 24, k) <= 2 * size(Nm, 1 << 24, k)
            assert size(2 * Nm, 5000, k) <= 2 * size(Nm, 5000, k)
