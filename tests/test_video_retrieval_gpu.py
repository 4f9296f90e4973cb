"""Video-level retrieval on the GPU (vfr_score_video_topk_f32, engine.corpus_video_topk, evaluate.evaluate_videos) against a
plain numpy statement of the semantics on the oracle's dense moment scores: a stable (distance, global id) sort of every
moment, the first occurrence of each video, the first k of those, and the number of videos ahead of the query's own video.
Bit for bit, in both scoring modes."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
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


def expected(S, counts, k, own=None, id_base=0):
    """numpy statement: (dist [Nq,k], moment id [Nq,k], video [Nq,k], video rank [Nq] | None) from dense scores S."""
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
        order = np.lexsort((ids, S[q]))                     # stable (distance, id)
        v = vid_of[order]
        _, first = np.unique(v, return_index=True)
        pos = order[np.sort(first)]                         # best moment of every video, in video-ranking order
        n = min(k, len(pos))
        od[q, :n], oi[q, :n], ov[q, :n] = S[q, pos[:n]], ids[pos[:n]], vid_of[pos[:n]]
        if own is not None:
            ranks[q] = int(np.nonzero(vid_of[pos] == own[q])[0][0])
    return od, oi, ov, ranks


def own_keys(S, counts, own, id_base=0):
    counts = np.asarray(counts, np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    d = np.empty(len(own), np.float32)
    i = np.empty(len(own), np.int64)
    for q, v in enumerate(own):
        seg = S[q, mo[v]:mo[v + 1]]
        j = int(np.lexsort((np.arange(len(seg)), seg))[0])
        d[q], i[q] = seg[j], id_base + mo[v] + j
    return d, i


def check(vfr, oracle, Q, V, counts, ks, own=None, S=None):
    off = synth.clip_offsets(counts)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    if S is None:
        S = oracle.score_moments(Q, V, off)
    od_own = oi_own = None
    if own is not None:
        od_own, oi_own = own_keys(S, counts, own)
    for k in ks:
        wd, wi, _, wr = expected(S, counts, k, own)
        d, i, c = vfr.score_video_topk(dev(Q), bank, k, None if own is None else dev(od_own), None if own is None else dev(oi_own))
        if k > 0:
            assert np.array_equal(i.cpu().numpy(), wi), f"video top-{k}: ids differ"
            assert np.array_equal(d.cpu().numpy(), wd), f"video top-{k}: distances differ"
        if own is not None:
            assert np.array_equal(c.cpu().numpy(), wr), f"video ranks differ (k = {k})"
    return S


@pytest.mark.parametrize("tag", ["n6", "ragged", "n21"])
def test_video_topk_reference_embeddings(vfr, oracle, golden, tag, score_mode):
    g = golden(f"g2_scoring_{tag}.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    own = g["own"].astype(np.int64)
    check(vfr, oracle, Q, V, counts, (1, 10, 100, len(counts) + 5, 0), own)


def planted_bank(seed=7, nv=300, nq=48, D=100):
    """Random videos plus videos whose clips are ONE repeated row (static shots) or rows differing in the last bits, placed
    near the queries so that they reach the top-k; plus exact duplicates of some videos (ties broken by id)."""
    rs = np.random.RandomState(seed)
    Q = (rs.randn(nq, D) * 0.1).astype(np.float32)
    counts = rs.randint(1, 22, nv).astype(np.int64)
    rows = []
    for v in range(nv):
        n = int(counts[v])
        kind = v % 5
        if kind in (0, 1):
            base = Q[rs.randint(nq)] + (rs.randn(D) * 0.02).astype(np.float32)
            blk = np.repeat(base[None, :].astype(np.float32), n, axis=0)
            if kind == 1:                                    # rows differing in the last bits
                blk = blk.view(np.uint32) ^ rs.randint(0, 4, blk.shape).astype(np.uint32)
                blk = blk.view(np.float32)
            rows.append(blk)
        else:
            rows.append((rs.randn(n, D) * 0.1).astype(np.float32))
    for d in range(0, 40, 4):                                # exact duplicates: video d + 1 := video d
        rows[d + 1] = rows[d].copy()
        counts[d + 1] = counts[d]
    V = np.ascontiguousarray(np.concatenate(rows).astype(np.float32))
    return Q, V, counts


def test_planted_repeated_clip_videos(vfr, oracle, score_mode):
    Q, V, counts = planted_bank()
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    # the fixture must contain a (query, video) whose best moment is a multi-clip window strictly below the video's dmin
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    hits = 0
    for v in range(len(counts)):
        n = int(counts[v])
        seg = S[:, mo[v]:mo[v + 1]]
        dmin = seg[:, :n].min(axis=1)
        best = seg.min(axis=1)
        arg = seg.argmin(axis=1)
        hits += int(np.sum((best < dmin) & (arg >= n)))
    assert hits > 0, "the planted fixture has no multi-clip best moment below dmin"
    own = np.random.RandomState(3).randint(0, len(counts), Q.shape[0]).astype(np.int64)
    check(vfr, oracle, Q, V, counts, (1, 10, 100, 0), own, S)


def test_exact_ties_broken_by_id(vfr, oracle, score_mode):
    rs = np.random.RandomState(11)
    counts = np.full(160, 6, np.int64)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    V[6 * 80:] = V[:6 * 80]                                  # videos 80.. = videos 0..
    Q = (rs.randn(20, 100) * 0.1).astype(np.float32)
    own = rs.randint(0, 160, 20).astype(np.int64)
    check(vfr, oracle, Q, V, counts, (10, 100, 0), own)


@pytest.mark.parametrize("nq", [1, 8, 64])
def test_small_batches_default_smallq(vfr, oracle, golden, nq, score_mode):
    assert vfr.get_option("score_smallq") == 64               # the library's default
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    Q = np.ascontiguousarray(np.resize(Q, (nq, Q.shape[1])).astype(np.float32))
    own = np.arange(nq, dtype=np.int64) % len(counts)
    check(vfr, oracle, Q, V, counts, (10, 100), own)


def test_full_synthetic_corpus_10000x21(vfr, oracle, score_mode):
    rs = np.random.RandomState(5)
    counts = synth.clip_counts(10000, 21, seed=123)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    # 64 queries: random rows, and the hardest kind -- copies of clip rows and of videos' mean rows (their own video ties
    # the query at distance ~ eps; many videos straddle the bounds)
    Q = (rs.randn(64, 100) * 0.1).astype(np.float32)
    off = synth.clip_offsets(counts)
    pick = rs.randint(0, len(counts), 32)
    Q[:16] = V[off[pick[:16]]]
    Q[16:32] = np.stack([V[off[v]:off[v + 1]].mean(0) for v in pick[16:32]])
    own = rs.randint(0, len(counts), 64).astype(np.int64)
    own[:32] = pick
    check(vfr, oracle, Q, V, counts, (100,), own)


def test_two_shards_equal_unsplit(vfr, oracle, golden, score_mode):
    g = golden("g2_scoring_ragged.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    own = g["own"].astype(np.int64)
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    od_own, oi_own = own_keys(S, counts, own)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    k = 50
    d0, i0, c0 = vfr.score_video_topk(dev(Q), bank, k, dev(od_own), dev(oi_own))
    half = len(counts) // 2
    parts, cnt = [], torch.zeros(Q.shape[0], dtype=torch.int64, device=DEV)
    for v0, v1 in ((0, half), (half, len(counts))):
        sb = vfr.slice_bank(bank, counts, v0, v1)
        d, i, cnt = vfr.score_video_topk(dev(Q), sb, k, dev(od_own), dev(oi_own), count=cnt)
        parts.append((d, i))
    md, mi = vfr.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, i0) and torch.equal(md, d0) and torch.equal(cnt, c0)
    wd, wi, _, wr = expected(S, counts, k, own)
    assert np.array_equal(mi.cpu().numpy(), wi) and np.array_equal(cnt.cpu().numpy(), wr)


def test_evaluate_videos_memory_dataset(vfr, oracle, score_mode):
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(60, 40, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
    model.train()
    vi, li = ds.iterators()
    metrics, (d, i, v) = vevaluate.evaluate_videos(model, vi, li, ds.annotations, DEV, return_topk=20)
    assert model.training
    # the statement on the same embeddings (the device encoders are bit-exact to the oracle elsewhere in the suite)
    model.eval()
    ops = engine.ops_for(DEV)
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Qe = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu().numpy()
    Ve = shard.bank.emb.cpu().numpy()
    counts = shard.counts_all
    own = np.asarray([names.index(x) for x in q_videos], np.int64)
    S = oracle.score_moments(Qe, Ve, synth.clip_offsets(counts))
    wd, wi, wv, wr = expected(S, counts, 20, own)
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 10: (wr < 10).astype(int), 100: (wr < 100).astype(int), "MR": wr})
    assert metrics == {"video": want}
    assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd) and np.array_equal(v.cpu().numpy(), wv)


def test_capi_counts_only(vfr, oracle, golden):
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    own = g["own"].astype(np.int64)
    off = synth.clip_offsets(counts)
    S = oracle.score_moments(Q, V, off)
    od_own, oi_own = own_keys(S, counts, own)
    _, _, _, wr = expected(S, counts, 1, own)
    bank = vfr.VideoBank(dev(V), dev(off.astype(np.int32)), 0)
    q, dd, di = dev(Q), dev(od_own), dev(oi_own)
    for dtype in (0, 2):                                       # VFR_MFMA_F32, VFR_SCORE_EXACT
        cnt = torch.full((Q.shape[0],), 7, dtype=torch.int64, device=DEV)          # counts are ADDED
        nb = vfr.lib().vfr_score_video_topk_workspace_bytes(Q.shape[0], bank.num_videos, bank.total_clips, 0)
        ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=DEV)
        rc = vfr.lib().vfr_score_video_topk_f32(q.data_ptr(), Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                                bank.mom_off.data_ptr(), bank.num_videos, bank.total_clips, bank.min_clips,
                                                bank.max_clips, bank.dim, ctypes.c_float(1e-6), 0, 0, None, None,
                                                dd.data_ptr(), di.data_ptr(), cnt.data_ptr(), dtype, ws.data_ptr(), nb, None)
        assert rc == 0, vfr.lib().vfr_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), wr + 7)
