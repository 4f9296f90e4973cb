"""Diversified moment retrieval on the GPU (vfr_score_moment_nms_f32, engine.corpus_moment_nms, evaluate.evaluate_moments_nms)
against the plain statement of tests/nms_reference.py on the oracle's dense moment scores, and against the two calls it
reduces to (per_video = 1: the video top-k; no cap and nms_iou >= 1: the moment top-k).  Bit for bit, in both scoring modes."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from nms_reference import expected_nms
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


def bank_of(vfr, V, counts, id_base=0):
    return vfr.VideoBank(dev(V), dev(synth.clip_offsets(counts).astype(np.int32)), id_base)


def check(vfr, Q, bank, S, counts, ks, per_videos, thresholds):
    """GPU == statement; the statement runs once at the largest k (a top-k is a prefix of a longer one)."""
    K = max(ks)
    for pv, thr in itertools.product(per_videos, thresholds):
        wd, wi, wv = expected_nms(S, counts, K, pv, thr)
        for k in ks:
            d, i = vfr.score_moment_nms(dev(Q), bank, k, pv, thr)
            assert np.array_equal(i.cpu().numpy(), wi[:, :k]), f"k = {k}, per_video = {pv}, nms_iou = {thr}: ids differ"
            assert np.array_equal(d.cpu().numpy(), wd[:, :k]), f"k = {k}, per_video = {pv}, nms_iou = {thr}: distances differ"
    return wv


@pytest.mark.parametrize("tag", ["n6", "ragged", "n21"])
def test_reference_embeddings(vfr, oracle, golden, tag, score_mode):
    g = golden(f"g2_scoring_{tag}.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    check(vfr, Q, bank_of(vfr, V, counts), S, counts, (1, 10, 100), (0, 1, 2, 5), (0.0, 0.5, 1.0))


def test_identities_full_synthetic_corpus_10000x21(vfr, score_mode):
    rs = np.random.RandomState(5)
    counts = synth.clip_counts(10000, 21, seed=123)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    off = synth.clip_offsets(counts)
    Q = (rs.randn(64, 100) * 0.1).astype(np.float32)
    pick = rs.randint(0, len(counts), 32)
    Q[:16] = V[off[pick[:16]]]
    Q[16:32] = np.stack([V[off[v]:off[v + 1]].mean(0) for v in pick[16:32]])
    bank = bank_of(vfr, V, counts)
    q = dev(Q)
    for k in (10, 100):
        vd, vi, _ = vfr.score_video_topk(q, bank, k)
        d, i = vfr.score_moment_nms(q, bank, k, 1, 0.5)                 # identity A
        assert torch.equal(i, vi) and torch.equal(d, vd), f"per_video = 1 != video top-{k}"
        td, ti, _ = vfr.score_topk(q, bank, k)
        for pv in (0, k):                                               # identity B
            d, i = vfr.score_moment_nms(q, bank, k, pv, 1.0)
            assert torch.equal(i, ti) and torch.equal(d, td), f"per_video = {pv}, nms_iou = 1 != moment top-{k}"
        d, i = vfr.score_moment_nms(q, bank, k, 3, 0.5)
        vid = torch.searchsorted(bank.mom_off, i, right=True) - 1
        for r in range(Q.shape[0]):
            assert int(torch.bincount(vid[r]).max()) <= 3


def test_planted_dominant_video(vfr, oracle, score_mode):
    """Queries sitting on one video each: its shifted spans fill the plain moment top-k, the cap and NMS must thin them."""
    rs = np.random.RandomState(8)
    counts = rs.randint(8, 22, 200).astype(np.int64)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    off = synth.clip_offsets(counts)
    hot = rs.choice(len(counts), 12, replace=False)
    for v in hot:                                            # a near-static shot: every span of it is close to the query
        V[off[v]:off[v + 1]] = V[off[v]] + (rs.randn(int(counts[v]), 100) * 0.01).astype(np.float32)
    Q = np.stack([V[off[v]] + (rs.randn(100) * 0.01).astype(np.float32) for v in hot]).astype(np.float32)
    S = oracle.score_moments(Q, V, off)
    bank = bank_of(vfr, V, counts)
    td, ti, _ = vfr.score_topk(dev(Q), bank, 10)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    plain_vid = np.searchsorted(mo, ti.cpu().numpy(), side="right") - 1
    assert max(np.bincount(r).max() for r in plain_vid) > 3, "the fixture does not concentrate the moment ranking"
    for pv, thr in ((1, 1.0), (2, 0.5), (3, 0.0), (0, 0.3)):
        wv = check(vfr, Q, bank, S, counts, (10, 30), (pv,), (thr,))
        if pv:
            assert all(np.bincount(r[r >= 0]).max() <= pv for r in wv)


def test_exact_ties(vfr, oracle, score_mode):
    rs = np.random.RandomState(11)
    counts = np.full(160, 6, np.int64)
    V = (rs.randn(int(counts.sum()), 100) * 0.1).astype(np.float32)
    V[6 * 80:] = V[:6 * 80]                                  # videos 80.. = videos 0..
    V[0:6] = V[0]                                            # one video of six equal clips (equal multi-clip means)
    Q = (rs.randn(20, 100) * 0.1).astype(np.float32)
    Q[0] = V[0]
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    check(vfr, Q, bank_of(vfr, V, counts), S, counts, (10, 100), (0, 2), (0.5, 1.0))


@pytest.mark.parametrize("nq", [1, 8, 64])
def test_small_batches(vfr, oracle, golden, nq, score_mode):
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    Q = np.ascontiguousarray(np.resize(Q, (nq, Q.shape[1])).astype(np.float32))
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    check(vfr, Q, bank_of(vfr, V, counts), S, counts, (10, 100), (0, 3), (0.5,))


def test_two_shards_equal_unsplit(vfr, oracle, golden, score_mode):
    g = golden("g2_scoring_ragged.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    bank = bank_of(vfr, V, counts)
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    k = 50
    for pv, thr in ((0, 0.5), (2, 0.0), (1, 1.0)):
        d0, i0 = vfr.score_moment_nms(dev(Q), bank, k, pv, thr)
        half = len(counts) // 2
        parts = [vfr.score_moment_nms(dev(Q), vfr.slice_bank(bank, counts, v0, v1), k, pv, thr)
                 for v0, v1 in ((0, half), (half, len(counts)))]
        md, mi = vfr.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        assert torch.equal(mi, i0) and torch.equal(md, d0)
        wd, wi, _ = expected_nms(S, counts, k, pv, thr)
        assert np.array_equal(mi.cpu().numpy(), wi) and np.array_equal(md.cpu().numpy(), wd)


def test_workspace_shared_with_moment_topk(vfr, oracle, golden):
    g = golden("g2_scoring_n21.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    S = oracle.score_moments(Q, V, synth.clip_offsets(counts))
    wd, wi, _ = expected_nms(S, counts, 20, 2, 0.5)
    old = vfr.get_option("score_mfma_min")
    vfr.set_option("score_mfma_min", 0)
    try:
        bank = bank_of(vfr, V, counts)
        n = max(vfr.lib().vfr_score_moment_nms_workspace_bytes(Q.shape[0], bank.num_videos, bank.total_clips, 20, 2),
                vfr.lib().vfr_score_topk_mfma_workspace_bytes(Q.shape[0], bank.num_videos, bank.total_clips, 20))
        ws = torch.empty((n,), dtype=torch.uint8, device=DEV)
        vfr.score_topk(dev(Q), bank, 20, mode="mfma", workspace=ws)
        for it in range(3):                                  # the 2nd and 3rd calls claim VFR_MFMA_BANK_READY
            d, i = vfr.score_moment_nms(dev(Q), bank, 20, 2, 0.5, mode="mfma", workspace=ws)
            assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd), it
            if it == 0:
                assert getattr(ws, "_vfr_bank", None) is not None
        vfr.score_topk(dev(Q), bank, 20, mode="mfma", workspace=ws)      # and the moment-level call after it
        d, i = vfr.score_moment_nms(dev(Q), bank, 20, 2, 0.5, mode="mfma", workspace=ws)
        assert np.array_equal(i.cpu().numpy(), wi)
    finally:
        vfr.set_option("score_mfma_min", old)


def test_capi_einval(vfr, golden):
    g = golden("g2_scoring_n6.npz")
    Q, V, counts = g["query_emb"], g["visual_emb"], g["counts"]
    bank = bank_of(vfr, V, counts)
    q = dev(Q)
    Nq = Q.shape[0]
    od = torch.empty((Nq, 448), dtype=torch.float32, device=DEV)
    oi = torch.empty((Nq, 448), dtype=torch.int64, device=DEV)
    nb = vfr.lib().vfr_score_moment_nms_workspace_bytes(Nq, bank.num_videos, bank.total_clips, 448, 0)
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)

    def call(k=10, per_video=0, nms_iou=0.5, max_clips=None, dtype=0, out=True, id_base=0):
        return vfr.lib().vfr_score_moment_nms_f32(q.data_ptr(), Nq, bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                                  bank.mom_off.data_ptr(), bank.num_videos, bank.total_clips, bank.min_clips,
                                                  bank.max_clips if max_clips is None else max_clips, bank.dim,
                                                  ctypes.c_float(1e-6), id_base, k, per_video, nms_iou,
                                                  od.data_ptr() if out else None, oi.data_ptr() if out else None, dtype,
                                                  ws.data_ptr(), nb, None)
    assert call() == 0, vfr.lib().vfr_last_error()
    torch.cuda.synchronize()
    for bad in (dict(per_video=-1), dict(nms_iou=float("nan")), dict(nms_iou=-0.5), dict(k=449), dict(k=-1),
                dict(max_clips=65), dict(dtype=1), dict(out=False), dict(id_base=(1 << 32) - 10)):
        assert call(**bad) == -1, bad
    assert vfr.lib().vfr_score_moment_nms_workspace_bytes(Nq, bank.num_videos, bank.total_clips, 10, -1) == 0
    assert call(k=448, per_video=0, nms_iou=2.0) == 0                    # k = 448, nms_iou > 1: valid
    torch.cuda.synchronize()


def test_evaluate_moments_nms_gpu_equals_cpu(vfr, oracle, score_mode):
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(60, 40, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    for pv, thr in ((0, 0.5), (2, 0.3), (0, 1.0)):
        model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
        model.train()
        vi, li = ds.iterators()
        m_gpu, (d, i, v) = vevaluate.evaluate_moments_nms(model, vi, li, ds.annotations, DEV, per_video=pv, nms_iou=thr,
                                                          return_topk=True)
        assert model.training
        vi, li = ds.iterators()
        m_cpu = vevaluate.evaluate_moments_nms(make_model(p["sd"], feat_dim=64, hidden=16), vi, li, ds.annotations, "cpu",
                                               per_video=pv, nms_iou=thr)
        assert m_gpu == m_cpu, (pv, thr)
        # the list itself: the statement on the device's own embeddings
        model.eval()
        ops = engine.ops_for(DEV)
        vi, li = ds.iterators()
        shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
        tokens, _, _ = vevaluate._drain_queries(li)
        Qe = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu().numpy()
        S = oracle.score_moments(Qe, shard.bank.emb.cpu().numpy(), synth.clip_offsets(shard.counts_all))
        wd, wi, wv = expected_nms(S, shard.counts_all, 100, pv, thr)
        assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd)
        assert np.array_equal(v.cpu().numpy(), wv)
