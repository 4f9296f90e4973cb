"""Paragraph-to-video retrieval without a GPU: the CPU provider against the numpy statement of tests/paragraph_reference.py on the
oracle's dense scores of the golden embeddings, engine.corpus_paragraph_topk with grounding, evaluate_paragraphs on CPU tensors,
the length-1 identity with score_video_topk, a gloo world of 2, and the C entry points' host-side argument checks."""
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
from paragraph_reference import cycle_lengths, pair_statement, statement
from vfr_amd import synth

CPU_THREADS = 1


def _bank(ops, V, counts, id_base=0):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ops.make_bank(torch.from_numpy(np.ascontiguousarray(V)), torch.from_numpy(off), id_base)


def _own_keys(sc, own):
    return torch.from_numpy(sc[np.arange(len(own)), own].copy()), torch.from_numpy(own.copy())


@pytest.mark.parametrize("tag", ["n6", "ragged", "n21"])
def test_cpu_provider_matches_reference_on_golden(oracle, golden, tag):
    from vfr_amd import engine
    g = golden(f"g2_scoring_{tag}.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    lengths = cycle_lengths(len(Q))
    groups = engine.paragraph_groups(lengths=lengths)
    assert groups.max_len == 8 and groups.num_groups == len(lengths) and groups.num_sentences == len(Q)
    own = (np.arange(len(lengths)) * 7) % len(counts)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts)
    Qt, off = torch.from_numpy(Q), torch.from_numpy(groups.off)
    pairs = np.stack([np.arange(len(lengths)), own], axis=1)
    ps, pm = ops.score_paragraph_pairs(Qt, bank, off, groups.max_len, torch.from_numpy(pairs))
    ws, wm = pair_statement(S, counts, lengths, pairs, groups.max_len)
    assert np.array_equal(ps.numpy(), ws) and np.array_equal(pm.numpy(), wm)
    for k in (1, 10, len(counts) + 5, 0):
        wd, wv, wr, sc = statement(S, counts, lengths, k, own)
        bad = torch.zeros(1, dtype=torch.int32)
        d, v, c = ops.score_paragraphs(Qt, bank, off, groups.max_len, k, 0, *_own_keys(sc, own), bad=bad)
        assert int(bad) == 0 and np.array_equal(c.numpy(), wr), k
        if k:
            assert np.array_equal(v.numpy(), wv) and np.array_equal(d.numpy(), wd), k
        else:
            assert d is None and v is None


def _ragged(seed=2, nv=23, nq=31, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(0, 9, nv).astype(np.int64)            # some videos have no clips
    counts[3] = 0
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    a = int(counts[:5].sum())
    V[a:a + counts[5]] = V[a]                                 # a video of repeated clips
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    Q[7:11] = Q[2]                                            # repeated sentences
    return Q, V, counts


def test_length_one_groups_are_the_video_topk(golden):
    """Paragraphs of one sentence against ``score_video_topk`` of the same provider: the distances bit for bit, the videos = the
    videos of its moment ids, in its order (on a ragged bank with empty videos and on the golden embeddings)."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    cases = [_ragged() + (40, 100)]
    for tag in ("n6", "ragged", "n21"):
        g = golden(f"g2_scoring_{tag}.npz")
        cases.append((g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64), 0, 0))
    for Q, V, counts, id_base, vid_base in cases:
        bank = _bank(ops, V, counts, id_base=id_base)
        Qt = torch.from_numpy(Q)
        groups = engine.paragraph_groups(lengths=np.ones(len(Q), np.int64))
        mom = torch.from_numpy(id_base + np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)]))
        for k in (1, 10, len(counts) + 2):
            d, v, _ = ops.score_paragraphs(Qt, bank, torch.from_numpy(groups.off), 1, k, vid_base)
            wd, wi, _ = ops.score_video_topk(Qt, bank, k)
            assert torch.equal(d, wd)
            wv = torch.where(wi >= 0, torch.searchsorted(mom, wi.clamp(min=0), right=True) - 1 + vid_base, torch.full_like(wi, -1))
            assert torch.equal(v, wv)


def test_corpus_paragraph_topk_grounding_and_edges(oracle):
    from vfr_amd import engine
    Q, V, counts = _ragged()
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    ops = engine.TorchCpuOps()
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    lengths = np.asarray([3, 0, 1, 8, 5, 0, 14], np.int64)   # empty paragraphs included
    groups = engine.paragraph_groups(lengths=lengths)
    own = np.asarray([0, 1, 2, 4, 5, 6, 7], np.int64)
    k = 6
    d, v, ranks, mom = engine.corpus_paragraph_topk(shard, torch.from_numpy(Q), groups, k, own, ground=True, ops=ops)
    wd, wv, wr, sc = statement(S, counts, lengths, k, own)
    wr[lengths == 0] = 0
    assert np.array_equal(d.numpy(), wd) and np.array_equal(v.numpy(), wv) and np.array_equal(ranks.numpy(), wr)
    assert np.all(v.numpy()[lengths == 0] == -1) and np.all(np.isinf(d.numpy()[lengths == 0]))
    pairs = np.stack([np.repeat(np.arange(len(lengths)), k), wv.reshape(-1)], axis=1)
    _, wm = pair_statement(S, counts, lengths, pairs, groups.max_len)
    assert mom.shape == (len(lengths), k, 14) and np.array_equal(mom.numpy().reshape(-1, 14), wm)
    _, _, ranks0, none = engine.corpus_paragraph_topk(shard, torch.from_numpy(Q), groups, 0, own, ops=ops)
    assert none is None and np.array_equal(ranks0.numpy(), wr)
    with pytest.raises(ValueError):
        engine.corpus_paragraph_topk(shard, torch.from_numpy(Q[:-1]), groups, k, ops=ops)
    with pytest.raises(ValueError):
        engine.corpus_paragraph_topk(shard, torch.from_numpy(Q), groups, k, own[:-1], ops=ops)
    # counts are ADDED and shards chain; out-of-shard pairs are left untouched
    Qt, off = torch.from_numpy(Q), torch.from_numpy(groups.off)
    od = torch.from_numpy(sc[np.arange(len(own)), own].copy())
    oi = torch.from_numpy(own.copy())
    half = 11
    parts, cnt = [], None
    for v0, v1 in ((0, half), (half, len(counts))):
        sb = ops.slice_bank(shard.bank, counts, v0, v1)
        pd, pv, cnt = ops.score_paragraphs(Qt, sb, off, 14, k, v0, od, oi, count=cnt)
        parts.append((pd, pv))
    md, mv = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(md.numpy(), wd) and np.array_equal(mv.numpy(), wv) and np.array_equal(cnt.numpy(), wr)


def test_paragraph_groups_and_bad_flag():
    from vfr_amd import engine
    g = engine.paragraph_groups(labels=["a", "a", "b", "c", "c", "c"])
    assert g.off.tolist() == [0, 2, 3, 6] and g.max_len == 3 and g.num_groups == 3
    assert engine.paragraph_groups(lengths=[]).num_groups == 0
    with pytest.raises(ValueError):
        engine.paragraph_groups(lengths=[65])
    with pytest.raises(ValueError):
        engine.paragraph_groups()
    Q, V, counts = _ragged()
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts)
    for off, max_len, want in (([0, 5, 3, 31], 30, 1), ([0, 5, 31], 8, 1), ([0, 5, 30], 30, 1), ([0, 5, 31], 26, 0)):
        bad = torch.zeros(1, dtype=torch.int32)
        ops.score_paragraphs(torch.from_numpy(Q), bank, torch.tensor(off), max_len, 3, bad=bad)
        assert int(bad) == want, off


def _reference_metrics(p, model, ds, oracle, k):
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    ops = engine.TorchCpuOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, "cpu", ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Qe = engine.encode_queries(model, torch.cat(tokens), "cpu", ops).numpy()
    own = np.asarray([names.index(x) for x in q_videos], np.int64)
    order = np.argsort(own, kind="stable")
    videos, lengths = np.unique(own, return_counts=True)
    S = oracle.score_moments(np.ascontiguousarray(Qe[order]), shard.bank.emb.numpy(), synth.clip_offsets(p["counts"]))
    wd, wv, wr, _ = statement(S, p["counts"], lengths, k, videos)
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 5: (wr < 5).astype(int), 10: (wr < 10).astype(int),
                                  50: (wr < 50).astype(int), "MR": wr})
    return {"paragraph": want}, wd, wv, videos


def _evaluate(p, rank=0, world=1):
    from vfr_amd import evaluate as vevaluate
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16)
    vi, li = ds.iterators()
    return vevaluate.evaluate_paragraphs(model, vi, li, ds.annotations, "cpu", rank=rank, world=world, return_topk=9), ds, model


def test_evaluate_paragraphs_cpu_end_to_end(oracle):
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        model.train()
        vi, li = ds.iterators()
        got, (d, v, videos) = vevaluate.evaluate_paragraphs(model, vi, li, ds.annotations, "cpu", return_topk=9)
        assert model.training
        model.eval()
        want, wd, wv, wvideos = _reference_metrics(p, model, ds, oracle, 9)
        assert got == want and set(got["paragraph"]) == {"R@1", "R@5", "R@10", "R@50", "MR"}
        assert np.array_equal(videos, wvideos) and np.array_equal(v.numpy(), wv) and np.array_equal(d.numpy(), wd)
        vi, li = ds.iterators()
        assert vevaluate.evaluate_paragraphs(model, vi, li, ds.annotations, "cpu") == got
        vi, _ = ds.iterators()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # mean / median of an empty list
            empty = vevaluate.evaluate_paragraphs(model, vi, iter(()), ds.annotations, "cpu")
        assert set(empty["paragraph"]) == {"R@1", "R@5", "R@10", "R@50", "MR"}
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
        from vfr_amd import engine
        from vfr_amd import evaluate as vevaluate
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        (metrics, (d, v, videos)), ds, model = _evaluate(p, rank, world)
        # grounding over the sharded corpus as well
        ops = engine.TorchCpuOps()
        vi, li = ds.iterators()
        shard, names = vevaluate.embed_corpus(model.eval(), vi, "cpu", ops, rank, world)
        tokens, q_videos, _ = vevaluate._drain_queries(li)
        Q = engine.encode_queries(model, torch.cat(tokens), "cpu", ops, rank, world)
        groups = engine.paragraph_groups(lengths=cycle_lengths(Q.shape[0]))
        own = np.arange(groups.num_groups) % len(names)
        gd, gv, gr, gm = engine.corpus_paragraph_topk(shard, Q, groups, 5, own, ground=True, ops=ops, world=world)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), m=repr(metrics), d=d.numpy(), v=v.numpy(), gd=gd.numpy(), gv=gv.numpy(),
                 gr=gr.numpy(), gm=gm.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_paragraphs_equal_single_process(tmp_path):
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        (metrics, (d, v, videos)), ds, model = _evaluate(p)
        ops = engine.TorchCpuOps()
        vi, li = ds.iterators()
        shard, names = vevaluate.embed_corpus(model.eval(), vi, "cpu", ops)
        tokens, _, _ = vevaluate._drain_queries(li)
        Q = engine.encode_queries(model, torch.cat(tokens), "cpu", ops)
        groups = engine.paragraph_groups(lengths=cycle_lengths(Q.shape[0]))
        own = np.arange(groups.num_groups) % len(names)
        gd, gv, gr, gm = engine.corpus_paragraph_topk(shard, Q, groups, 5, own, ground=True, ops=ops)
    finally:
        torch.set_num_threads(threads)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npz")
        assert str(got["m"]) == repr(metrics)
        assert np.array_equal(got["d"], d.numpy()) and np.array_equal(got["v"], v.numpy())
        assert np.array_equal(got["gd"], gd.numpy()) and np.array_equal(got["gv"], gv.numpy())
        assert np.array_equal(got["gr"], gr.numpy()) and np.array_equal(got["gm"], gm.numpy())


def test_wrappers_refuse_cpu_tensors():
    from vfr_amd import _vfr
    with pytest.raises(RuntimeError):
        _vfr.score_paragraphs(torch.zeros((3, 100)), None, torch.zeros(2, dtype=torch.int64), 3, 1)
    with pytest.raises(RuntimeError):
        _vfr.score_paragraph_pairs(torch.zeros((3, 100)), None, torch.zeros(2, dtype=torch.int64), 3, torch.zeros((1, 2), dtype=torch.int32))


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    size = lib.vfr_score_paragraphs_workspace_bytes
    assert size(64, 16, 10, 210, 10) > 0 and size(0, 0, 0, 0, 0) > 0
    assert size(-1, 16, 10, 210, 10) == 0 and size(64, -1, 10, 210, 10) == 0 and size(64, 16, -1, 210, 10) == 0
    assert size(64, 16, 10, -1, 10) == 0 and size(64, 16, 10, 210, -1) == 0
    assert size(64, 32, 10, 210, 10) > size(64, 16, 10, 210, 10)
    nb = size(64, 16, 10, 210, 10)
    ws = ctypes.create_string_buffer(nb)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks
    eps = ctypes.c_float(1e-6)

    def call(Q=dummy, Nq=64, off=dummy, Ng=16, max_len=8, V=dummy, co=dummy, mo=dummy, Nv=10, max_clips=21, D=100, vid_base=0, k=10,
             od=dummy, oi=dummy, own=(None, None, None), dtype=2, work=dummy, wsb=nb):
        return lib.vfr_score_paragraphs_f32(Q, Nq, off, Ng, max_len, V, co, mo, Nv, 210, 1, max_clips, D, eps, vid_base, k, od, oi,
                                            own[0], own[1], own[2], dtype, None, work, wsb, None)
    assert call(Q=None) == -1 and call(off=None) == -1 and call(V=None) == -1 and call(co=None) == -1 and call(mo=None) == -1
    assert call(od=None) == -1 and call(oi=None) == -1
    assert call(k=449) == -1 and call(k=-1) == -1 and call(max_clips=65) == -1 and call(max_len=65) == -1 and call(max_len=-1) == -1
    assert call(Nq=-1) == -1 and call(Ng=-1) == -1 and call(Nv=-1) == -1 and call(D=0) == -1 and call(vid_base=-1) == -1
    assert call(own=(dummy, None, None)) == -1 and call(own=(dummy, dummy, None)) == -1
    assert call(dtype=1) == -1 and call(Ng=1 << 30, k=2) == -1
    assert b"vfr_score_paragraphs_f32" in lib.vfr_last_error()
    assert call(work=None) == -4 and call(wsb=8) == -4

    def pairs(Q=dummy, Nq=64, off=dummy, Ng=16, max_len=8, V=dummy, co=dummy, mo=dummy, Nv=10, max_clips=21, D=100, id_base=0, vid_base=0,
              pr=dummy, Np=4, sc=dummy):
        return lib.vfr_score_paragraph_pairs_f32(Q, Nq, off, Ng, max_len, V, co, mo, Nv, 210, 1, max_clips, D, eps, id_base, vid_base,
                                                 pr, Np, sc, None, None, None)
    assert pairs(Q=None) == -1 and pairs(off=None) == -1 and pairs(V=None) == -1 and pairs(pr=None) == -1 and pairs(sc=None) == -1
    assert pairs(max_len=65) == -1 and pairs(max_clips=65) == -1 and pairs(Np=-1) == -1 and pairs(id_base=-1) == -1
    assert pairs(vid_base=-1) == -1 and pairs(D=0) == -1 and pairs(id_base=1 << 32) == -1
    assert b"vfr_score_paragraph_pairs_f32" in lib.vfr_last_error()
