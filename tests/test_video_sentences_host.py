"""Video-to-sentence retrieval without a GPU: the CPU provider and engine.corpus_video_sentence_topk against the numpy statement of
tests/video_sentences_reference.py on the oracle's dense moment scores (ranks from a CSR of own rows, a probe without own rows,
repeated and unsorted probes, grounding, two shards as thread ranks), evaluate_video_sentences end to end on CPU tensors, and the C
entry point's host-side argument checks and workspace-size properties."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, ThreadRanks, make_model, problem
from video_sentences_reference import dense_blocks, own_ranks, probe_keys, rank_keys_for, split_keys, statement
from vfr_amd import synth

CPU_THREADS = 1


def _ragged(seed, nv=20, ns=41, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 9, nv).astype(np.int64)
    counts[7] = 0                                             # a video without clips
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    a = int(counts[:4].sum())
    V[a:a + counts[4]] = V[a]                                 # a video of repeated clips: all its moments tie
    S = (rs.randn(ns, D) * 0.3).astype(np.float32)
    S[10:14] = S[3]                                           # duplicated sentences: the sentence id decides
    S[5] = V[0]                                               # a sentence ON a clip
    return S, V, counts


def _bank(ops, V, counts, id_base=0):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ops.make_bank(torch.from_numpy(np.ascontiguousarray(V)), torch.from_numpy(off), id_base)


@pytest.mark.parametrize("seed", [0, 1])
def test_cpu_provider_matches_statement(oracle, seed):
    from vfr_amd import engine
    S, V, counts = _ragged(seed)
    ops = engine.TorchCpuOps()
    rs = np.random.RandomState(50 + seed)
    lo, hi = 3, 16                                            # a shard: global videos [3, 16)
    sub = counts[lo:hi]
    c0 = int(counts[:lo].sum())
    Vs = np.ascontiguousarray(V[c0:c0 + int(sub.sum())])
    bank = _bank(ops, Vs, sub)
    block = dense_blocks(oracle.score_moments(S, Vs, synth.clip_offsets(sub)), sub)
    videos = np.concatenate([rs.randint(0, len(counts), 30), [4, 4, 7, -1, lo, hi - 1, hi, 99]]).astype(np.int64)
    keys, _, _ = probe_keys(block, sub, videos, len(S), lo, 7)
    assert keys[32] is None and keys[30] is not None          # the clip-less video is skipped, the all-ties video is not
    for R in range(5):
        rk = rank_keys_for(keys, rs, R) if R else None
        for k in (0, 1, 7, 41, 100):
            if k == 0 and R == 0:
                continue
            rd, ri = split_keys(rk) if R else (None, None)
            bad = torch.zeros(1, dtype=torch.int32)
            d, i, c = ops.score_video_sentences(torch.from_numpy(S), bank, torch.from_numpy(videos), k, lo, 7, rd, ri, bad=bad)
            wd, wi, wc, wbad = statement(block, sub, videos, len(S), k, lo, 7, rk)
            assert int(bad) == wbad == 1
            if k:
                assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd), (R, k)
            else:
                assert d is None and i is None
            if R:
                assert np.array_equal(c.numpy(), wc), (R, k)
            else:
                assert c is None
    bad = torch.zeros(1, dtype=torch.int32)
    ops.score_video_sentences(torch.from_numpy(S), bank, torch.from_numpy(videos[:30]), 3, lo, 7, bad=bad)
    assert int(bad) == 0                                       # other shards' videos and the clip-less video are not bad


def test_cpu_counts_are_added_and_sentence_shards_chain(oracle):
    from vfr_amd import engine
    S, V, counts = _ragged(3)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, counts)
    rs = np.random.RandomState(4)
    videos = rs.randint(0, len(counts), 25).astype(np.int64)
    block = dense_blocks(oracle.score_moments(S, V, synth.clip_offsets(counts)), counts)
    keys, _, _ = probe_keys(block, counts, videos, len(S))
    rd, ri = split_keys(rank_keys_for(keys, rs, 2))
    St, vt = torch.from_numpy(S), torch.from_numpy(videos)
    d1, i1, c1 = ops.score_video_sentences(St, bank, vt, 9, 0, 0, rd, ri)
    da, ia, cc = ops.score_video_sentences(St[:17], bank, vt, 9, 0, 0, rd, ri)
    db, ib, cc = ops.score_video_sentences(St[17:], bank, vt, 9, 0, 17, rd, ri, count_lt=cc)
    dm, im = ops.topk_merge(torch.stack([da, db]), torch.stack([ia, ib]))
    assert torch.equal(dm, d1) and torch.equal(im, i1) and torch.equal(cc, c1)


def _own_csr(rs, videos, ns, empty=()):
    """A CSR of own bank rows per probe: 0..4 random rows each, none for the probes in ``empty``."""
    lens = rs.randint(1, 5, len(videos))
    lens[list(empty)] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, rs.randint(0, ns, int(off[-1])).astype(np.int64)


def test_corpus_video_sentence_topk_ranks_and_grounding_cpu(oracle):
    from vfr_amd import engine
    S, V, counts = _ragged(5)
    ops = engine.TorchCpuOps()
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    rs = np.random.RandomState(6)
    videos = np.concatenate([rs.randint(0, len(counts), 30), [4, 7, 7, 2, 2]]).astype(np.int64)    # unsorted, repeated, clip-less
    off, rows = _own_csr(rs, videos, len(S), empty=(3, 31))
    block = dense_blocks(oracle.score_moments(S, V, synth.clip_offsets(counts)), counts)
    keys, _, _ = probe_keys(block, counts, videos, len(S))
    want_ranks = own_ranks(keys, off, rows)
    assert want_ranks[3] == -1 and want_ranks[31] == -1 and want_ranks[32] == 0 and (want_ranks > 0).any()
    St = torch.from_numpy(S)
    k = 8
    d, i, ranks, mom = engine.corpus_video_sentence_topk(shard, St, videos, k, off, rows, ground=True, ops=ops)
    wd, wi, _, _, wm = statement(block, counts, videos, len(S), k, ground=True)
    assert np.array_equal(d.numpy(), wd) and np.array_equal(i.numpy(), wi)
    assert ranks.dtype == torch.int64 and np.array_equal(ranks.numpy(), want_ranks)
    assert mom.shape == (len(videos), k) and np.array_equal(mom.numpy(), wm)
    assert np.all(i.numpy()[31] == -1) and np.all(mom.numpy()[31] == -1)
    # the video of repeated clips: its one-clip moments tie (a mean of several equal distances may round elsewhere), and where
    # the minimum is theirs the first moment of the video is reported
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    b4 = block(4)[i.numpy()[30]]
    first = b4[:, 0] == b4.min(axis=1)
    assert counts[4] > 1 and first.any() and np.all(mom.numpy()[30][first] == mo[4])
    d, i, ranks, mom = engine.corpus_video_sentence_topk(shard, St, videos, k, ops=ops)
    assert ranks is None and mom is None and np.array_equal(i.numpy(), wi)
    d, i, ranks, mom = engine.corpus_video_sentence_topk(shard, St, videos, 0, off, rows, ground=True, ops=ops)
    assert d is None and i is None and mom is None and np.array_equal(ranks.numpy(), want_ranks)
    none = np.zeros(0, np.int64)                              # no probes: empty lists, ranks and moments
    d, i, ranks, mom = engine.corpus_video_sentence_topk(shard, St, none, k, np.zeros(1, np.int64), none, ground=True, ops=ops)
    assert tuple(d.shape) == (0, k) and tuple(i.shape) == (0, k) and tuple(ranks.shape) == (0,) and tuple(mom.shape) == (0, k)
    with pytest.raises(ValueError):
        engine.corpus_video_sentence_topk(shard, St, videos, k, off[:-1], rows, ops=ops)
    with pytest.raises(ValueError):
        engine.corpus_video_sentence_topk(shard, St, videos, k, off, None, ops=ops)
    with pytest.raises(ValueError):
        engine.corpus_video_sentence_topk(shard, St, videos, k, off, np.full(len(rows), len(S)), ops=ops)


@pytest.mark.parametrize("world", [2, 3])
def test_thread_rank_shards_equal_one_shard(world):
    """The clip bank sharded by video over thread ranks (lists merged, counts summed, own keys MIN- and moments MAX-reduced) =
    the one-shard result."""
    from vfr_amd import engine
    S, V, counts = _ragged(8, nv=23, ns=50)
    ops = engine.TorchCpuOps()
    rs = np.random.RandomState(9)
    videos = np.concatenate([rs.randint(0, len(counts), 20), [7, 0, 22, 22]]).astype(np.int64)
    off, rows = _own_csr(rs, videos, len(S), empty=(5,))
    St, Vt = torch.from_numpy(S), torch.from_numpy(V)
    want = engine.corpus_video_sentence_topk(engine.corpus_from_embeddings(Vt, counts, "cpu", ops), St, videos, 9, off, rows,
                                             ground=True, ops=ops)
    group = ThreadRanks(world)
    old = engine._dist
    engine._dist = lambda: group
    try:
        def body(rank, n):
            shard = engine.corpus_from_embeddings(Vt, counts, "cpu", ops, rank, n)
            return engine.corpus_video_sentence_topk(shard, St, videos, 9, off, rows, ground=True, ops=ops, world=n)
        outs = group.run(body)
    finally:
        engine._dist = old
    for got in outs:
        for g, w in zip(got, want):
            assert torch.equal(g, w)


def _statement_metrics(p, model, ds, oracle, k):
    """Ranks and lists computed from the oracle's dense scores of the CPU provider's own embeddings."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    ops = engine.TorchCpuOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, "cpu", ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Se = engine.encode_queries(model, torch.cat(tokens), "cpu", ops).numpy()
    own = np.asarray([names.index(v) for v in q_videos], np.int64)
    videos = np.unique(own)
    rows = np.argsort(own, kind="stable")
    off = np.concatenate([[0], np.cumsum([(own == v).sum() for v in videos])]).astype(np.int64)
    block = dense_blocks(oracle.score_moments(Se, shard.bank.emb.numpy(), synth.clip_offsets(p["counts"])), p["counts"])
    keys, _, _ = probe_keys(block, p["counts"], videos, len(Se))
    wr = own_ranks(keys, off, rows)
    wd, wi, _, _ = statement(block, p["counts"], videos, len(Se), k)
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 5: (wr < 5).astype(int), 10: (wr < 10).astype(int),
                                  50: (wr < 50).astype(int), "MR": wr})
    return {"video_sentence": want}, wd, wi, videos


def test_evaluate_video_sentences_cpu_end_to_end(oracle):
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(37, 23, "didemo", feat_dim=64, hidden=16)
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        model.train()
        vi, li = ds.iterators()
        got, (d, i, videos) = vevaluate.evaluate_video_sentences(model, vi, li, ds.annotations, "cpu", return_topk=9)
        assert model.training
        model.eval()
        want, wd, wi, wvideos = _statement_metrics(p, model, ds, oracle, 9)
        assert got == want and set(got["video_sentence"]) == {"R@1", "R@5", "R@10", "R@50", "MR"}
        assert np.array_equal(videos, wvideos) and np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd)
        vi, li = ds.iterators()
        assert vevaluate.evaluate_video_sentences(model, vi, li, ds.annotations, "cpu") == got
        vi, _ = ds.iterators()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # mean / median of an empty list
            empty, lists = vevaluate.evaluate_video_sentences(model, vi, iter(()), ds.annotations, "cpu", return_topk=3)
        assert set(empty["video_sentence"]) == {"R@1", "R@5", "R@10", "R@50", "MR"} and lists == (None, None, None)
    finally:
        torch.set_num_threads(threads)


def test_wrapper_refuses_cpu_tensors():
    from vfr_amd import _vfr
    with pytest.raises(RuntimeError):
        _vfr.score_video_sentences(torch.zeros((3, 100)), None, torch.zeros((1,), dtype=torch.int32), 1)


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 20)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def call(S=dummy, Ns=64, V=dummy, off=dummy, Nv=10, max_clips=21, D=100, videos=dummy, Np=4, vid_base=0, sent_base=0, k=10,
             od=dummy, oi=dummy, num_rank=0, work=dummy, wsb=1 << 20):
        return lib.vfr_score_video_sentences_f32(S, Ns, V, off, Nv, 210, max_clips, D, 1e-6, videos, Np, vid_base, sent_base, k, od,
                                                 oi, num_rank, None, None, None, None, work, wsb, None)
    assert call(k=449) == -1 and call(k=-1) == -1
    assert call(max_clips=65) == -1 and call(max_clips=-1) == -1
    assert call(videos=None) == -1 and call(S=None) == -1 and call(off=None) == -1 and call(V=None) == -1
    assert call(od=None) == -1 and call(oi=None) == -1
    assert call(Ns=-1) == -1 and call(Np=-1) == -1 and call(Nv=-1) == -1 and call(D=0) == -1
    assert call(vid_base=-1) == -1 and call(sent_base=-1) == -1
    assert call(num_rank=5) == -1 and call(num_rank=-1) == -1 and call(num_rank=1) == -1      # rank keys without their arrays
    assert call(Ns=1 << 32) == -1 and call(sent_base=(1 << 32) - 64) == -1
    assert call(Np=1 << 30, k=2) == -1
    assert b"vfr_score_video_sentences_f32" in lib.vfr_last_error()
    assert call(wsb=8) == -4 and call(work=None) == -4
    # nothing to do: no probes, or neither lists nor counts nor a bad flag asked for -- VFR_OK without touching the (dummy) buffers
    assert call(Np=0) == 0 and call(k=0) == 0
    size = lib.vfr_score_video_sentences_workspace_bytes
    assert size(4, 64, 449) == 0 and size(-1, 64, 10) == 0 and size(4, -1, 10) == 0 and size(4, 64, -1) == 0
    assert size(1 << 30, 64, 2) == 0
    assert size(4, 64, 10) >= 4 * 10 * 8 and size(4, 64, 0) > 0 and size(0, 0, 0) > 0
    # 256 + 8 k Np C with C = min(ceil(2048 / Np), ceil(Ns / 64), 256), rounded up to 256 bytes
    for Np, Ns, k in ((1, 5000, 100), (1000, 5000, 100), (64, 5000, 100), (300, 130, 7), (1, 1 << 24, 448), (5000, 1 << 24, 1)):
        C = max(1, min(-(-2048 // Np), -(-Ns // 64), 256))
        assert size(Np, Ns, k) == -(-(256 + 8 * k * Np * C) // 256) * 256, (Np, Ns, k)
    # no Np x Ns term: the number of sentence chunks is capped, so the size stops growing with Ns and is at most linear in Np
    for Np in (1, 8, 100, 5000, 33000):
        for k in (1, 100, 448):
            assert size(Np, 1 << 24, k) == size(Np, 1 << 25, k)
            assert size(2 * Np, 1 << 24, k) <= 2 * size(Np, 1 << 24, k)
            assert size(2 * Np, 5000, k) <= 2 * size(Np, 5000, k)
