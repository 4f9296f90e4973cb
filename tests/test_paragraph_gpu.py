"""Paragraph-to-video retrieval on the GPU (vfr_score_paragraphs_f32, vfr_score_paragraph_pairs_f32, engine.corpus_paragraph_topk,
evaluate.evaluate_paragraphs) against the numpy statement of tests/paragraph_reference.py on the oracle's dense moment scores.
Bit for bit, in both scoring modes."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from paragraph_reference import cycle_lengths, pair_statement, statement
from test_video_retrieval_gpu import planted_bank
from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


@pytest.fixture(params=["exact", "mfma"])
def score_mode(request, vfr):
    old, old_min = vfr.DEFAULT_SCORE_MODE, vfr.get_option("score_mfma_min")
    vfr.DEFAULT_SCORE_MODE = request.param
    vfr.set_option("score_mfma_min", 0)              # small banks must reach the fast kernels too
    yield request.param
    vfr.DEFAULT_SCORE_MODE = old
    vfr.set_option("score_mfma_min", old_min)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def check(vfr, oracle, Q, V, counts, lengths, ks, own=None, S=None, pairs=True):
    """Lists, ranks and (optionally) the pairs call against the statement; returns (S, all reference scores)."""
    counts = np.asarray(counts, np.int64)
    lengths = np.asarray(lengths, np.int64)
    off = synth.clip_offsets(counts)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    if S is None:
        S = oracle.score_moments(Q, V, off)
    max_len = int(lengths.max()) if len(lengths) else 0
    q, go = dev(Q), dev(offsets(lengths))
    sc = None
    for k in ks:
        wd, wv, wr, sc = statement(S, counts, lengths, k, own)
        od = oi = None
        if own is not None:
            od, oi = dev(sc[np.arange(len(own)), own]), dev(own)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        d, v, c = vfr.score_paragraphs(q, bank, go, max_len, k, 0, od, oi, bad=bad)
        assert int(bad) == 0
        if k > 0:
            assert np.array_equal(v.cpu().numpy(), wv), f"paragraph top-{k}: videos differ"
            assert np.array_equal(d.cpu().numpy(), wd), f"paragraph top-{k}: scores differ"
        if own is not None:
            assert np.array_equal(c.cpu().numpy(), wr), f"paragraph ranks differ (k = {k})"
    if pairs and own is not None:
        pr = np.stack([np.arange(len(own)), own], axis=1)
        ps, pm = vfr.score_paragraph_pairs(q, bank, go, max_len, dev(pr, torch.int32))
        ws, wm = pair_statement(S, counts, lengths, pr, max_len)
        assert np.array_equal(ps.cpu().numpy(), ws) and np.array_equal(pm.cpu().numpy(), wm)
    return S, sc


@pytest.mark.parametrize("tag", ["n6", "ragged", "n21"])
def test_paragraphs_reference_embeddings(vfr, oracle, golden, tag, score_mode):
    g = golden(f"g2_scoring_{tag}.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    lengths = cycle_lengths(len(Q))
    own = (np.arange(len(lengths)) * 7) % len(counts)
    check(vfr, oracle, Q, V, counts, lengths, (1, 10, len(counts) + 5, 0), own)


@pytest.mark.parametrize("nv", [1, 31, 33, 65])
def test_edge_shapes(vfr, oracle, nv, score_mode):
    rs = np.random.RandomState(nv)
    counts = rs.randint(1, 22, nv).astype(np.int64)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    lengths = np.asarray([3, 0, 1, 64, 2], np.int64)          # an empty group, one of length 1, one of max_len
    Q = (rs.randn(int(lengths.sum()), 100) * 0.1).astype(np.float32)
    own = rs.randint(0, nv, len(lengths)).astype(np.int64)
    check(vfr, oracle, Q, V, counts, lengths, (1, 448), own)


def test_edge_shape_d36_takes_the_exact_path(vfr, oracle, score_mode):
    rs = np.random.RandomState(36)
    counts = rs.randint(1, 31, 33).astype(np.int64)
    V = (rs.randn(int(counts.sum()), 36) * 0.1).astype(np.float32)
    lengths = np.asarray([3, 0, 1, 64, 2], np.int64)
    Q = (rs.randn(int(lengths.sum()), 36) * 0.1).astype(np.float32)
    own = rs.randint(0, 33, len(lengths)).astype(np.int64)
    check(vfr, oracle, Q, V, counts, lengths, (1, 448), own)


def test_exact_ties_broken_by_video_index(vfr, oracle, score_mode):
    rs = np.random.RandomState(11)
    counts = np.full(160, 6, np.int64)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    V[6 * 80:] = V[:6 * 80]                                  # videos 80.. = videos 0..
    lengths = cycle_lengths(27)                               # 1, 2, 3, 5, 8, 1, 2, 3, 2
    Q = (rs.randn(27, 100) * 0.1).astype(np.float32)
    a, b = offsets(lengths)[2], offsets(lengths)[7]          # groups 2 and 7 (length 3 each): identical paragraphs
    assert lengths[2] == lengths[7] == 3
    Q[b:b + 3] = Q[a:a + 3]
    own = rs.randint(0, 160, len(lengths)).astype(np.int64)
    bank = vfr.VideoBank(dev(V), dev(synth.clip_offsets(counts).astype(np.int32)), 0)
    d, v, _ = vfr.score_paragraphs(dev(Q), bank, dev(offsets(lengths)), 8, 100)
    d, v = d.cpu().numpy(), v.cpu().numpy()
    assert np.array_equal(d[2], d[7]) and np.array_equal(v[2], v[7])
    for g in range(len(lengths)):                             # a video and its copy tie: the smaller index comes first
        pos = {int(x): i for i, x in enumerate(v[g])}
        for x in v[g]:
            if x < 80 and int(x) + 80 in pos:
                assert pos[int(x) + 80] == pos[int(x)] + 1
    check(vfr, oracle, Q, V, counts, lengths, (10, 100, 0), own)


def test_bound_straddling_planted_bank(vfr, oracle, score_mode):
    Qp, V, counts = planted_bank()
    off = synth.clip_offsets(counts)
    # paragraphs of 4 sentences: three clip rows and the mean row of one video (static shots, last-bit variants and exact
    # duplicates among them: many videos tie or nearly tie the k-th score)
    vids = list(range(0, 40)) + list(range(40, 300, 13))
    rows = []
    for v in vids:
        blk = V[off[v]:off[v + 1]]
        rows += [blk[0], blk[len(blk) // 2], blk[-1], blk.mean(0).astype(np.float32)]
    Q = np.ascontiguousarray(np.stack(rows).astype(np.float32))
    lengths = np.full(len(vids), 4, np.int64)
    own = np.asarray(vids, np.int64)
    S = oracle.score_moments(Q, V, off)
    k = 1
    _, _, _, sc = statement(S, counts, lengths, k, own)
    kth = np.sort(sc, axis=1)[:, k - 1:k]
    near = (np.abs(sc - kth) <= kth * np.float32(2.0 ** -20)).sum() - len(vids)      # the k-th video itself is not counted
    print(f"(group, video) scores within 2^-20 relative of the group's k-th score, besides the k-th itself: {near}")
    assert near >= 10, "the fixture does not exercise the undecided branch"
    check(vfr, oracle, Q, V, counts, lengths, (1, 2, 10, 0), own, S)


def test_length_one_identity_with_video_topk(vfr, golden, score_mode):
    g = golden("g2_scoring_ragged.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    off = synth.clip_offsets(counts)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    mom = torch.from_numpy(np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])).to(DEV)
    q = dev(Q)
    go = dev(np.arange(len(Q) + 1, dtype=np.int64))
    for k in (1, 10, len(counts) + 5):
        wd, wi, _ = vfr.score_video_topk(q, bank, k)
        d, v, _ = vfr.score_paragraphs(q, bank, go, 1, k)
        wv = torch.where(wi >= 0, torch.searchsorted(mom, wi.clamp(min=0), right=True) - 1, torch.full_like(wi, -1))
        assert torch.equal(d, wd) and torch.equal(v, wv)


def test_two_shards_equal_unsplit(vfr, oracle, golden, score_mode):
    g = golden("g2_scoring_ragged.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    lengths = cycle_lengths(len(Q))
    own = (np.arange(len(lengths)) * 7) % len(counts)
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    k = 50
    wd, wv, wr, sc = statement(S, counts, lengths, k, own)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    q, go = dev(Q), dev(offsets(lengths))
    od, oi = dev(sc[np.arange(len(own)), own]), dev(own)
    d0, v0, c0 = vfr.score_paragraphs(q, bank, go, 8, k, 0, od, oi)
    half = len(counts) // 2
    parts, cnt = [], torch.zeros(len(lengths), dtype=torch.int64, device=DEV)
    pr = np.stack([np.arange(len(own)), own], axis=1)
    ps = pm = None
    for a, b in ((0, half), (half, len(counts))):
        sb = vfr.slice_bank(bank, counts, a, b)
        d, v, cnt = vfr.score_paragraphs(q, sb, go, 8, k, a, od, oi, count=cnt)
        parts.append((d, v))
        # the pairs call leaves out-of-shard pairs untouched: the second call completes the first one's outputs
        one_s, one_m = vfr.score_paragraph_pairs(q, sb, go, 8, dev(pr, torch.int32), a)
        inside = torch.from_numpy((own >= a) & (own < b)).to(DEV)
        assert bool(torch.isinf(one_s[~inside]).all()) and bool((one_m[~inside] == -1).all())
        ps, pm = vfr.score_paragraph_pairs(q, sb, go, 8, dev(pr, torch.int32), a, out_score=ps, out_moments=pm)
    md, mv = vfr.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mv, v0) and torch.equal(md, d0) and torch.equal(cnt, c0)
    assert np.array_equal(mv.cpu().numpy(), wv) and np.array_equal(md.cpu().numpy(), wd) and np.array_equal(cnt.cpu().numpy(), wr)
    ws, wm = pair_statement(S, counts, lengths, pr, 8)
    assert np.array_equal(ps.cpu().numpy(), ws) and np.array_equal(pm.cpu().numpy(), wm)


def test_pairs_scores_and_moments(vfr, oracle, golden):
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    lengths = cycle_lengths(len(Q))
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(1)
    pr = np.stack([rs.randint(0, len(lengths), 200), rs.randint(0, len(counts), 200)], axis=1)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 1000)
    ps, pm = vfr.score_paragraph_pairs(dev(Q), bank, dev(offsets(lengths)), 8, dev(pr, torch.int32))
    ws, wm = pair_statement(S, counts, lengths, pr, 8, id_base=1000)
    assert np.array_equal(ps.cpu().numpy(), ws) and np.array_equal(pm.cpu().numpy(), wm)
    short = lengths[pr[:, 0]] < 8
    assert short.any() and np.all(pm.cpu().numpy()[short, -1] == -1)
    ps2, none = vfr.score_paragraph_pairs(dev(Q), bank, dev(offsets(lengths)), 8, dev(pr, torch.int32), moments=False)
    assert none is None and torch.equal(ps2, ps)


def test_bad_flag(vfr, golden, score_mode):
    g = golden("g2_scoring_n6.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    bank = vfr.VideoBank(dev(V), dev(synth.clip_offsets(counts).astype(np.int32)), 0)
    q, nq = dev(Q), len(Q)
    pr = dev(np.asarray([[0, 0], [1, 3]]), torch.int32)
    # a decreasing grp_off, a group longer than max_len, a run that stops short of Nq; and a clean call
    for off, max_len, want in (([0, 5, 3, nq], 64, 1), ([0, 5, nq], 8, 1), ([0, 5, nq - 1], 64, 1), ([0, 5, 12, nq], 64, 0)):
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        vfr.score_paragraphs(q, bank, dev(np.asarray(off, np.int64)), max_len, 5, bad=bad)
        assert int(bad) == want, off
        bad.zero_()
        vfr.score_paragraph_pairs(q, bank, dev(np.asarray(off, np.int64)), max_len, pr, bad=bad)
        assert int(bad) == want, off


def test_capi_counts_only(vfr, oracle, golden):
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"].astype(np.int64)
    lengths = cycle_lengths(len(Q))
    own = (np.arange(len(lengths)) * 7) % len(counts)
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    _, _, wr, sc = statement(S, counts, lengths, 1, own)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    q, go, dd, di = dev(Q), dev(offsets(lengths)), dev(sc[np.arange(len(own)), own]), dev(own)
    Ng = len(lengths)
    old_min = vfr.get_option("score_mfma_min")
    vfr.set_option("score_mfma_min", 0)
    try:
        for dtype in (0, 2):                                       # VFR_MFMA_F32, VFR_SCORE_EXACT
            cnt = torch.full((Ng,), 7, dtype=torch.int64, device=DEV)              # counts are ADDED
            nb = vfr.lib().vfr_score_paragraphs_workspace_bytes(len(Q), Ng, bank.num_videos, bank.total_clips, 0)
            ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=DEV)
            rc = vfr.lib().vfr_score_paragraphs_f32(q.data_ptr(), len(Q), go.data_ptr(), Ng, 8, bank.emb.data_ptr(),
                                                    bank.clip_off.data_ptr(), bank.mom_off.data_ptr(), bank.num_videos,
                                                    bank.total_clips, bank.min_clips, bank.max_clips, bank.dim, ctypes.c_float(1e-6),
                                                    0, 0, None, None, dd.data_ptr(), di.data_ptr(), cnt.data_ptr(), dtype, None,
                                                    ws.data_ptr(), nb, None)
            assert rc == 0, vfr.lib().vfr_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(cnt.cpu().numpy(), wr + 7)
    finally:
        vfr.set_option("score_mfma_min", old_min)


def test_full_synthetic_corpus_10000x21(vfr, oracle, score_mode):
    from vfr_amd import engine
    rs = np.random.RandomState(5)
    counts = synth.clip_counts(10000, 21, seed=123)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    off = synth.clip_offsets(counts)
    lengths = np.full(16, 4, np.int64)
    Q = (rs.randn(64, 100) * 0.1).astype(np.float32)
    own = rs.randint(0, len(counts), 16).astype(np.int64)
    for g in range(8):                                        # half of the paragraphs: clip rows of their own video
        blk = V[off[own[g]]:off[own[g] + 1]]
        Q[4 * g:4 * g + 4] = blk[rs.randint(0, len(blk), 4)]
    S = oracle.score_moments(Q, V, off)
    wd, wv, wr, _ = statement(S, counts, lengths, 100, own)
    shard = engine.corpus_from_embeddings(dev(V), counts, DEV, engine.HipOps())
    groups = engine.paragraph_groups(lengths=lengths, device=DEV)
    d, v, ranks, mom = engine.corpus_paragraph_topk(shard, dev(Q), groups, 100, own, ground=True)
    assert np.array_equal(v.cpu().numpy(), wv) and np.array_equal(d.cpu().numpy(), wd) and np.array_equal(ranks.cpu().numpy(), wr)
    assert np.all(wr[:8] == 0)
    pairs = np.stack([np.repeat(np.arange(16), 100), wv.reshape(-1)], axis=1)
    _, wm = pair_statement(S, counts, lengths, pairs, 4)
    assert np.array_equal(mom.cpu().numpy().reshape(-1, 4), wm)


def test_evaluate_paragraphs_memory_dataset(vfr, oracle, score_mode):
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(60, 40, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
    model.train()
    vi, li = ds.iterators()
    metrics, (d, v, videos) = vevaluate.evaluate_paragraphs(model, vi, li, ds.annotations, DEV, return_topk=20)
    assert model.training
    model.eval()
    ops = engine.ops_for(DEV)
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Qe = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu().numpy()
    own = np.asarray([names.index(x) for x in q_videos], np.int64)
    order = np.argsort(own, kind="stable")
    wvideos, lengths = np.unique(own, return_counts=True)
    S = oracle.score_moments(np.ascontiguousarray(Qe[order]), shard.bank.emb.cpu().numpy(), synth.clip_offsets(shard.counts_all))
    wd, wv, wr, _ = statement(S, shard.counts_all, lengths, 20, wvideos)
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 5: (wr < 5).astype(int), 10: (wr < 10).astype(int),
                                  50: (wr < 50).astype(int), "MR": wr})
    assert metrics == {"paragraph": want}
    assert np.array_equal(videos, wvideos) and np.array_equal(v.cpu().numpy(), wv) and np.array_equal(d.cpu().numpy(), wd)
