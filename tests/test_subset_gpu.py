"""Candidate-restricted retrieval on the GPU (vfr_score_subset_f32, engine.corpus_subset_topk, evaluate.evaluate_candidates)
against the numpy statement of tests/subset_reference.py on the oracle's dense moment scores, bit for bit, in both levels; and
the two identities against the full-corpus entry points (every list = every video) and vfr_score_own_f32 (the own video alone)."""
import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from subset_reference import keys_of, split_keys, statement
from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ["moments", "videos"]


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def corpus(counts, D=100, seed=0, repeat_every=0, duplicate=()):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    if repeat_every:
        for v in range(0, len(counts), repeat_every):          # repeated clips: every moment of the video scores alike
            V[off[v]:off[v + 1]] = V[off[v]]
    for a, b in duplicate:                                    # video b = video a (same clip count): ties broken by id
        V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
    return V, counts, off.astype(np.int32)


def lists_of(pools):
    from vfr_amd import engine
    return engine.candidate_lists(pools)


def rank_keys_for(S, rs, R, id_base=0):
    """R rank keys per query: keys of random moments of the bank, and for r = 3 a key between two scores."""
    K = keys_of(S, id_base)
    nq = S.shape[0]
    rk = K[np.arange(nq)[None, :].repeat(R, 0), rs.randint(0, S.shape[1], (R, nq))]
    if R > 3:
        rk[3] = (rk[3] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0x7FFFFFFF)
    return rk


def run(vfr, Q, V, off, cl, k, level, R=0, rk=None, id_base=0, vid_base=0):
    bank = vfr.VideoBank(dev(V), dev(off), id_base)
    o, vv = cl.on(DEV)
    rd = ri = None
    if R:
        rd, ri = split_keys(rk)
        rd, ri = rd.to(DEV), ri.to(DEV)
    d, i, c = vfr.score_subset(dev(Q), bank, o, vv, k, level, vid_base, rd, ri, max_list=cl.max_list)
    torch.cuda.synchronize()
    return (None if d is None else d.cpu().numpy(), None if i is None else i.cpu().numpy(), None if c is None else c.cpu().numpy())


def check(vfr, oracle, Q, V, counts, off, cl, ks, level, Rs=(0, 2), id_base=0, vid_base=0, seed=1):
    S = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(seed)
    for R in Rs:
        rk = rank_keys_for(S, rs, R, id_base) if R else None
        for k in ks:
            if k == 0 and R == 0:
                continue
            d, i, c = run(vfr, Q, V, off, cl, k, level, R, rk, id_base, vid_base)
            wd, wi, wc = statement(S, counts, cl.off, cl.vid, k, level, vid_base, id_base, rk)
            if k:
                assert np.array_equal(i, wi), f"{level} top-{k} ids differ (R = {R})"
                assert np.array_equal(d, wd), f"{level} top-{k} distances differ (R = {R})"
            if R:
                assert np.array_equal(c, wc), f"{level} rank counts differ (R = {R}, k = {k})"


@pytest.mark.parametrize("level", LEVELS)
def test_pool_sizes_and_k(vfr, oracle, level):
    V, counts, off = corpus(synth.clip_counts(1200, "didemo", seed=3), repeat_every=97)
    nv = len(counts)
    rs = np.random.RandomState(4)
    Q = (rs.randn(9, 100) * 0.3).astype(np.float32)
    sizes = [0, 1, 5, 63, 64, 65, 1000, nv, 2]
    cl = lists_of([sorted(rs.choice(nv, s, replace=False).tolist()) for s in sizes])
    check(vfr, oracle, Q, V, counts, off, cl, (1, 10, 100, 448), level, Rs=(0, 1, 2, 3, 4))


@pytest.mark.parametrize("level", LEVELS)
def test_skewed_pools(vfr, oracle, level):
    V, counts, off = corpus(synth.clip_counts(700, 21, seed=5), seed=5)
    nv = len(counts)
    rs = np.random.RandomState(6)
    Q = (rs.randn(40, 100) * 0.3).astype(np.float32)
    pools = [list(range(nv))] + [[int(rs.randint(nv))] for _ in range(39)]
    check(vfr, oracle, Q, V, counts, off, lists_of(pools), (10, 100), level)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("D", [100, 36, 13])
def test_ragged_64_clips_ties(vfr, oracle, level, D):
    rs = np.random.RandomState(7)
    counts = np.concatenate([np.arange(1, 22), rs.randint(1, 65, 60), [64, 64, 63]])
    counts[30] = counts[31]
    V, counts, off = corpus(counts, D=D, seed=8, repeat_every=9, duplicate=[(30, 31), (81, 82)])
    nv = len(counts)
    Q = (rs.randn(12, D) * 0.3).astype(np.float32)
    Q[3] = V[off[30]]                                         # a query ON a clip: distance eps-only
    pools = [sorted(rs.choice(nv, rs.randint(0, nv + 1), replace=False).tolist()) for _ in range(11)] + [[30, 31, 81, 82]]
    check(vfr, oracle, Q, V, counts, off, lists_of(pools), (1, 10, 100, 448), level, Rs=(0, 4))


@pytest.mark.parametrize("level", LEVELS)
def test_shard_id_base_vid_base(vfr, oracle, level):
    """A bank holding global videos [300, 700) of a 1000-video corpus: lists name global indices, the rest are skipped."""
    Vall, call, offall = corpus(synth.clip_counts(1000, "didemo", seed=9), seed=9)
    lo, hi = 300, 700
    sub = call[lo:hi]
    V = Vall[offall[lo]:offall[hi]]
    off = (offall[lo:hi + 1] - offall[lo]).astype(np.int32)
    id_base = int((call[:lo] * (call[:lo] + 1) // 2).sum())
    rs = np.random.RandomState(10)
    Q = (rs.randn(10, 100) * 0.3).astype(np.float32)
    pools = [sorted(rs.choice(1000, s, replace=False).tolist()) for s in (0, 1, 10, 64, 65, 300, 999, 1000, 3, 200)]
    check(vfr, oracle, Q, V, sub, off, lists_of(pools), (1, 100, 448), level, Rs=(0, 2), id_base=id_base, vid_base=lo)


@pytest.mark.parametrize("score_mode", ["exact", "mfma"])
def test_identity_full_lists(vfr, oracle, score_mode):
    V, counts, off = corpus(synth.clip_counts(900, 21, seed=11), seed=11, repeat_every=50)
    nv = len(counts)
    rs = np.random.RandomState(12)
    Q = (rs.randn(70, 100) * 0.3).astype(np.float32)
    bank = vfr.VideoBank(dev(V), dev(off), 17)
    cl = lists_of([range(nv)] * len(Q))
    o, vv = cl.on(DEV)
    S = oracle.score_moments(Q, V, off)
    rd, ri = split_keys(rank_keys_for(S, rs, 2, 17))
    rd, ri = rd.to(DEV), ri.to(DEV)
    old = vfr.get_option("score_mfma_min")
    vfr.set_option("score_mfma_min", 0)
    try:
        for k in (1, 100):
            d, i, c = vfr.score_subset(dev(Q), bank, o, vv, k, "moments", 0, rd, ri, max_list=cl.max_list)
            wd, wi, wc = vfr.score_topk(dev(Q), bank, k, rd, ri, mode=score_mode)
            assert torch.equal(i, wi) and torch.equal(d, wd) and torch.equal(c, wc)
            d, i, c = vfr.score_subset(dev(Q), bank, o, vv, k, "videos", 0, rd[:1], ri[:1], max_list=cl.max_list)
            wd, wi, wc = vfr.score_video_topk(dev(Q), bank, k, rd[0], ri[0], mode=score_mode)
            assert torch.equal(i, wi) and torch.equal(d, wd) and torch.equal(c[0], wc)
    finally:
        vfr.set_option("score_mfma_min", old)


def test_identity_own_video(vfr, oracle):
    V, counts, off = corpus(synth.clip_counts(300, "didemo", seed=13), seed=13)
    rs = np.random.RandomState(14)
    Q = (rs.randn(50, 100) * 0.3).astype(np.float32)
    own = rs.randint(0, len(counts), 50)
    bank = vfr.VideoBank(dev(V), dev(off))
    sc = vfr.score_own(dev(Q), bank, dev(own.astype(np.int32))).cpu().numpy()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    cl = lists_of([[int(v)] for v in own])
    o, vv = cl.on(DEV)
    for k in (1, 10, 448):
        d, i, _ = vfr.score_subset(dev(Q), bank, o, vv, k, "moments", max_list=1)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        for q in range(len(Q)):
            M = int(mo[own[q] + 1] - mo[own[q]])
            order = np.argsort(sc[q, :M], kind="stable")[:k]
            n = len(order)
            assert np.array_equal(d[q, :n], sc[q, order]) and np.array_equal(i[q, :n], mo[own[q]] + order)
            assert np.all(np.isinf(d[q, n:])) and np.all(i[q, n:] == -1)


@pytest.mark.parametrize("level", LEVELS)
def test_bad_flag(vfr, level):
    V, counts, off = corpus([3, 4, 5, 6, 2], D=100, seed=15)
    bank = vfr.VideoBank(dev(V), dev(off))
    Q = dev(np.zeros((2, 100), np.float32))
    cases = {"ok": ([0, 2, 4], 0), "unsorted": ([0, 3, 1], 1), "duplicate": ([1, 1, 2], 1), "negative": ([-1, 2, 3], 1)}
    for name, (second, want) in cases.items():
        off_t = dev(np.array([0, 2, 5], np.int64))
        vid_t = dev(np.array([0, 4] + second, np.int32))
        bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
        vfr.score_subset(Q, bank, off_t, vid_t, 5, level, bad=bad, max_list=3)
        assert int(bad.item()) == want, name


def test_evaluate_candidates_gpu(vfr, oracle):
    """Full pools: evaluate's and evaluate_videos' dicts on the GPU.  Random pools: the ranks of the numpy statement on the
    oracle's scores of the GPU's own embeddings."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(45, 30, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
    nv, nq = len(p["counts"]), len(p["own"])
    vi, li = ds.iterators()
    got = vevaluate.evaluate_candidates(model, vi, li, ds.annotations, DEV, [range(nv)] * nq)
    vi, li = ds.iterators()
    assert got == vevaluate.evaluate(model, vi, li, ds.annotations, DEV)
    vi, li = ds.iterators()
    got = vevaluate.evaluate_candidates(model, vi, li, ds.annotations, DEV, [range(nv)] * nq, level="videos")
    vi, li = ds.iterators()
    assert got == vevaluate.evaluate_videos(model, vi, li, ds.annotations, DEV)
    rs = np.random.RandomState(16)
    pools = [rs.choice(nv, rs.randint(0, 12), replace=False).tolist() for _ in range(nq)]
    vi, li = ds.iterators()
    got = vevaluate.evaluate_candidates(model, vi, li, ds.annotations, DEV, pools)
    # the statement: own video added, labels of evaluate, the best positive key per threshold, moments of the pool before it
    ops = engine.HipOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
    tokens, q_videos, annot_ids = vevaluate._drain_queries(li)
    Qe = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu().numpy()
    Ve = shard.bank.emb.cpu().numpy()
    S = oracle.score_moments(Qe, Ve, p["off"])
    K = keys_of(S)
    own = np.asarray([names.index(v) for v in q_videos])
    lab = engine.gt_label_table([ds.annotations[a]["times"] for a in annot_ids], p["counts"][own], [0.5, 0.7], True)
    mo = np.concatenate([[0], np.cumsum(p["counts"] * (p["counts"] + 1) // 2)])
    cl = engine.candidate_lists([list(pl) + [int(own[q])] for q, pl in enumerate(pools)], num_videos=nv)
    rk = np.zeros((2, nq), np.uint64)
    for r in range(2):
        for q in range(nq):
            M = int(mo[own[q] + 1] - mo[own[q]])
            pos = np.nonzero(lab[r, q, :M])[0]
            rk[r, q] = K[q, mo[own[q]] + pos].min()
    _, _, wc = statement(S, p["counts"], cl.off, cl.vid, 0, "moments", rank_keys=rk)
    for r, thr in enumerate((0.5, 0.7)):
        want = vevaluate.get_metrics({1: (wc[r] < 1).astype(int), 10: (wc[r] < 10).astype(int), 100: (wc[r] < 100).astype(int),
                                      "MR": wc[r]})
        assert got[f"model, IoU={thr}"] == want


@pytest.mark.parametrize("level", LEVELS)
def test_bench_shaped_corpus(vfr, oracle, level):
    """10 000 videos x 21 clips, 64 queries x 1 000 candidates (own video included), k = 100, two rank keys."""
    V, counts, off = corpus(np.full(10000, 21), seed=17)
    nv = len(counts)
    rs = np.random.RandomState(18)
    own = rs.randint(0, nv, 64)
    Q = (V[off[own] + 3] + rs.randn(64, 100).astype(np.float32) * 0.05).astype(np.float32)
    pools = [np.unique(np.concatenate([rs.choice(nv, 999, replace=False), [own[q]]]))[:1000].tolist() for q in range(64)]
    cl = lists_of(pools)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    rk = np.empty((2, 64), np.uint64)
    wd, wi, wc = [], [], []
    for q0 in range(0, 64, 8):                                # the dense scores 8 queries at a time (74 MB)
        S = oracle.score_moments(Q[q0:q0 + 8], V, off)
        K = keys_of(S)
        for j in range(8):
            q = q0 + j
            rk[0, q] = K[j, mo[own[q]]:mo[own[q] + 1]].min()
            rk[1, q] = K[j, rs.randint(0, S.shape[1])]
        sub = type(cl)(cl.off[q0:q0 + 9] - cl.off[q0], cl.vid[cl.off[q0]:cl.off[q0 + 8]], cl.max_list)
        a, b, c = statement(S, counts, sub.off, sub.vid, 100, level, rank_keys=rk[:, q0:q0 + 8])
        wd.append(a), wi.append(b), wc.append(c)
    d, i, c = run(vfr, Q, V, off, cl, 100, level, 2, rk)
    assert np.array_equal(i, np.concatenate(wi)) and np.array_equal(d, np.concatenate(wd))
    assert np.array_equal(c, np.concatenate(wc, axis=1))
