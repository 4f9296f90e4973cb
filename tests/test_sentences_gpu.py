"""Sentence retrieval for moments on the GPU (vfr_score_sentences_f32, engine.corpus_sentence_topk, evaluate.evaluate_sentences)
against the numpy statement of tests/sentences_reference.py on the oracle's dense moment scores, bit for bit; and the identity with
the device's own dense path (vfr_score_moments_f32 with the sentences as the queries)."""
import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from sentences_reference import (all_moments, dense_blocks, local_id, probe_keys, rank_keys_for, sliced_blocks, split_keys,
                                 statement)
from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def corpus(counts, D=100, seed=0, repeat=()):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    for v in repeat:                                          # a video of repeated clips: all its moments score alike
        V[off[v]:off[v + 1]] = V[off[v]]
    return V, counts, off.astype(np.int32)


def sentences(ns, D=100, seed=1):
    return (np.random.RandomState(seed).randn(ns, D) * 0.3).astype(np.float32)


def random_probes(rs, counts, nm, vid_base=0, max_len=None):
    v = rs.randint(0, len(counts), nm)
    n = np.asarray(counts)[v]
    s = (rs.rand(nm) * n).astype(np.int64)
    room = n - s if max_len is None else np.minimum(n - s, max_len)
    e = s + (rs.rand(nm) * room).astype(np.int64)
    return np.stack([v + vid_base, s, e], axis=1).astype(np.int64)


def run(vfr, S, V, off, probes, k, rk=None, vid_base=0, sent_base=0, want_bad=False):
    bank = vfr.VideoBank(dev(V), dev(off))
    rd = ri = None
    if rk is not None and len(rk):
        rd, ri = split_keys(rk)
        rd, ri = rd.to(DEV), ri.to(DEV)
    bad = torch.zeros((1,), dtype=torch.int32, device=DEV) if want_bad else None
    d, i, c = vfr.score_sentences(dev(S), bank, dev(probes, torch.int32), k, vid_base, sent_base, rd, ri, bad=bad)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return cpu(d), cpu(i), cpu(c), (int(bad.item()) if want_bad else None)


def check(vfr, block, S, V, counts, off, probes, ks, Rs=(0, 2), vid_base=0, sent_base=0, seed=1):
    rs = np.random.RandomState(seed)
    keys, _ = probe_keys(block, counts, probes, len(S), vid_base, sent_base)
    for R in Rs:
        rk = rank_keys_for(keys, rs, R) if R else None
        for k in ks:
            if k == 0 and R == 0:
                continue
            d, i, c, _ = run(vfr, S, V, off, probes, k, rk, vid_base, sent_base)
            wd, wi, wc, _ = statement(block, counts, probes, len(S), k, vid_base, sent_base, rk)
            if k:
                assert np.array_equal(i, wi), f"top-{k} sentence ids differ (R = {R})"
                assert np.array_equal(d, wd), f"top-{k} distances differ (R = {R})"
            if R:
                assert np.array_equal(c, wc), f"rank counts differ (R = {R}, k = {k})"


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 5000])
def test_bank_sizes_and_k(vfr, oracle, ns):
    """Ns in {1, 63, 64, 65, 5000} x k in {0, 1, 10, 100, 448} (k > Ns pads) x 0..4 rank keys.  Ns = 65 also takes k on both sides
    of the list capacities (128 | 256 slots at k = 64 | 65, 256 | 512 at k = 192 | 193)."""
    V, counts, off = corpus(synth.clip_counts(40, "didemo", seed=3), seed=3)
    S = sentences(ns, seed=4)
    probes = random_probes(np.random.RandomState(5), counts, 37)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    ks = (0, 1, 10, 100, 448) + ((64, 65, 192, 193) if ns == 65 else ())
    check(vfr, block, S, V, counts, off, probes, ks, Rs=(0, 1, 2, 3, 4))


def test_all_moments_of_shared_videos(vfr, oracle):
    """Every one of the 231 moments of several 21-clip videos: the probes of a video share its clip distances."""
    V, counts, off = corpus(np.full(6, 21), seed=6)
    S = sentences(700, seed=7)
    probes = np.asarray([(v, s, e) for v in (4, 0, 2) for s, e in all_moments(21)], np.int64)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    check(vfr, block, S, V, counts, off, probes, (10, 100), Rs=(0, 2))


def test_didemo_counts_repeated_and_unsorted_probes(vfr, oracle):
    V, counts, off = corpus(synth.clip_counts(300, "didemo", seed=8), seed=8)
    S = sentences(900, seed=9)
    rs = np.random.RandomState(10)
    probes = random_probes(rs, counts, 400)
    probes = np.concatenate([probes, probes[:50], probes[rs.permutation(100)]])       # repeated, unsorted
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    check(vfr, block, S, V, counts, off, probes, (1, 100), Rs=(0, 4))


@pytest.mark.parametrize("D", [100, 36, 13])
def test_ragged_64_clips_and_ties(vfr, oracle, D):
    """Ragged banks with 1..64 clips and 64-clip spans; duplicated sentence rows (the sentence id decides), a video of repeated
    clips, a sentence lying ON a clip (eps-only distance)."""
    rs = np.random.RandomState(11)
    counts = np.concatenate([np.arange(1, 22), rs.randint(1, 65, 30), [64, 64, 63]])
    V, counts, off = corpus(counts, D=D, seed=12, repeat=(9, 52))
    S = sentences(333, D=D, seed=13)
    S[100:140] = S[17]                                        # duplicated sentences: ties broken by sentence id
    S[200] = S[5]
    S[7] = V[off[30]]                                         # a sentence ON a clip
    nv = len(counts)
    probes = random_probes(rs, counts, 150)
    full = [(v, 0, int(counts[v]) - 1) for v in (nv - 1, nv - 2, nv - 3, 9, 52, 0)]          # whole-video spans (64 clips)
    probes = np.concatenate([probes, np.asarray(full, np.int64), np.asarray([(30, 0, 0), (9, 2, 7), (52, 0, 3)], np.int64)])
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    check(vfr, block, S, V, counts, off, probes, (1, 10, 100, 448), Rs=(0, 4))


def test_identity_with_device_dense_path(vfr):
    """vfr_score_moments_f32 with S as the queries, columns gathered and stably sorted on the host = the new output, bit for bit."""
    V, counts, off = corpus(synth.clip_counts(60, "didemo", seed=14), seed=14)
    S = sentences(1500, seed=15)
    probes = random_probes(np.random.RandomState(16), counts, 200)
    bank = vfr.VideoBank(dev(V), dev(off))
    Sc = vfr.score_moments(dev(S), bank).cpu().numpy()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    d, i, _, _ = run(vfr, S, V, off, probes, 100)
    for m, (v, s, e) in enumerate(probes.tolist()):
        col = Sc[:, mo[v] + local_id(int(counts[v]), s, e)]
        order = np.argsort(col, kind="stable")[:100]
        assert np.array_equal(i[m], order) and np.array_equal(d[m], col[order]), m


def test_sentence_shards_and_video_shards(vfr, oracle):
    """Two sentence-bank halves with sent_base, lists merged by vfr_topk_merge_f32 and counts chained = one call; a clip bank
    holding global videos [300, 700) of 1000 with vid_base = 300 skips the rest (padding, +0)."""
    Vall, call, offall = corpus(synth.clip_counts(1000, "didemo", seed=17), seed=17)
    S = sentences(1001, seed=18)
    rs = np.random.RandomState(19)
    probes = random_probes(rs, call, 300)
    lo, hi = 300, 700
    V = Vall[offall[lo]:offall[hi]]
    off = (offall[lo:hi + 1] - offall[lo]).astype(np.int32)
    sub = call[lo:hi]
    block = sliced_blocks(oracle.score_moments, S, V, off)
    check(vfr, block, S, V, sub, off, probes, (1, 100), Rs=(0, 2), vid_base=lo)
    outside = (probes[:, 0] < lo) | (probes[:, 0] >= hi)
    huge = np.full((1, len(probes)), np.uint64(0x7F000000) << np.uint64(32), np.uint64)      # every real key sorts before it
    d, i, c, _ = run(vfr, S, V, off, probes, 10, huge, lo)
    assert outside.any() and np.all(i[outside] == -1) and np.all(np.isinf(d[outside])) and np.all(c[0, outside] == 0)
    assert np.all(c[0, ~outside] == len(S))
    # sentence shards
    keys, _ = probe_keys(block, sub, probes, len(S), lo)
    rk = rank_keys_for(keys, rs, 2)
    rd, ri = split_keys(rk)
    rd, ri = rd.to(DEV), ri.to(DEV)
    bank = vfr.VideoBank(dev(V), dev(off))
    pt = dev(probes, torch.int32)
    k, half = 100, 480
    d1, i1, c1 = vfr.score_sentences(dev(S), bank, pt, k, lo, 0, rd, ri)
    da, ia, cc = vfr.score_sentences(dev(S[:half]), bank, pt, k, lo, 0, rd, ri)
    db, ib, cc = vfr.score_sentences(dev(S[half:]), bank, pt, k, lo, half, rd, ri, count_lt=cc)
    dm, im = vfr.topk_merge(torch.stack([da, db]), torch.stack([ia, ib]))
    assert torch.equal(dm, d1) and torch.equal(im, i1) and torch.equal(cc, c1)


def test_bad_flag(vfr, oracle):
    V, counts, off = corpus([3, 4, 5, 6, 2], seed=20)
    S = sentences(90, seed=21)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    good = [(0, 0, 2), (3, 1, 4), (4, 1, 1)]
    cases = {"ok": ((2, 0, 4), 0), "negative video": ((-1, 0, 0), 1), "end < start": ((1, 2, 1), 1), "end >= n": ((1, 0, 4), 1),
             "negative start": ((2, -1, 1), 1)}
    for name, (extra, want) in cases.items():
        probes = np.asarray(good[:2] + [extra] + good[2:], np.int64)
        d, i, _, bad = run(vfr, S, V, off, probes, 7, want_bad=True)
        wd, wi, _, wbad = statement(block, counts, probes, len(S), 7)
        assert bad == want == wbad, name
        assert np.array_equal(i, wi) and np.array_equal(d, wd), name
        if want:
            assert np.all(i[2] == -1), name


def test_evaluate_sentences_gpu(vfr, oracle):
    """evaluate_sentences equals the numpy statement applied to the oracle's scores of the GPU's own embeddings."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(45, 30, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
    vi, li = ds.iterators()
    got, (d, i, rows) = vevaluate.evaluate_sentences(model, vi, li, ds.annotations, DEV, return_topk=10)
    ops = engine.HipOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
    tokens, q_videos, annot_ids = vevaluate._drain_queries(li)
    Se = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu().numpy()
    Ve = shard.bank.emb.cpu().numpy()
    own = np.asarray([names.index(v) for v in q_videos])
    probes, prow = vevaluate.sentence_probes(ds.annotations, annot_ids, own, p["counts"])
    assert np.array_equal(rows, prow) and len(prow) > 0
    block = dense_blocks(oracle.score_moments(Se, Ve, p["off"]), p["counts"])
    keys, _ = probe_keys(block, p["counts"], probes, len(Se))
    rk = np.asarray([keys[m][prow[m]] for m in range(len(prow))], np.uint64)[None]
    wd, wi, wc, _ = statement(block, p["counts"], probes, len(Se), 10, rank_keys=rk)
    assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd)
    want = vevaluate.get_metrics({1: (wc[0] < 1).astype(int), 10: (wc[0] < 10).astype(int), 100: (wc[0] < 100).astype(int), "MR": wc[0]})
    if len(prow) < len(annot_ids):
        want["skipped"] = len(annot_ids) - len(prow)
    assert got == {"sentence": want}


def test_bench_shaped_corpus(vfr, oracle):
    """10 000 videos x 21 clips, 5 000 sentences, 512 probes (half of them all moments of two videos), k = 100, one rank key."""
    V, counts, off = corpus(np.full(10000, 21), seed=22)
    S = sentences(5000, seed=23)
    rs = np.random.RandomState(24)
    shared = [(v, s, e) for v in (1234, 9999) for s, e in all_moments(21)][:256]
    probes = np.concatenate([random_probes(rs, counts, 256), np.asarray(shared, np.int64)])
    block = sliced_blocks(oracle.score_moments, S, V, off)
    check(vfr, block, S, V, counts, off, probes, (100,), Rs=(1,))
