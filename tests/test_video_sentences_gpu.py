"""Video-to-sentence retrieval on the GPU (vfr_score_video_sentences_f32, engine.corpus_video_sentence_topk,
evaluate.evaluate_video_sentences) against the numpy statement of tests/video_sentences_reference.py on the oracle's dense moment
scores, bit for bit; and the identities with the device's own paths (score_video_topk with the sentences as the queries,
score_paragraph_pairs with groups of length 1)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, ThreadRanks, make_model, problem
from video_sentences_reference import (dense_blocks, own_ranks, probe_keys, rank_keys_for, sliced_blocks, split_keys, statement)
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
    for v in repeat:                                          # a video of repeated clips: its one-clip moments all tie
        V[off[v]:off[v + 1]] = V[off[v]]
    return V, counts, off.astype(np.int32)


def sentences(ns, D=100, seed=1):
    return (np.random.RandomState(seed).randn(ns, D) * 0.3).astype(np.float32)


def run(vfr, S, bank, videos, k, rk=None, vid_base=0, sent_base=0, want_bad=False):
    rd = ri = None
    if rk is not None and len(rk):
        rd, ri = split_keys(rk)
        rd, ri = rd.to(DEV), ri.to(DEV)
    bad = torch.zeros((1,), dtype=torch.int32, device=DEV) if want_bad else None
    St = S if isinstance(S, torch.Tensor) else dev(S)
    d, i, c = vfr.score_video_sentences(St, bank, dev(videos, torch.int32), k, vid_base, sent_base, rd, ri, bad=bad)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return cpu(d), cpu(i), cpu(c), (int(bad.item()) if want_bad else None)


def check(vfr, block, S, V, counts, off, videos, ks, Rs=(0, 2), vid_base=0, sent_base=0, seed=1, bank=None):
    rs = np.random.RandomState(seed)
    bank = bank or vfr.VideoBank(dev(V), dev(off))
    keys, _, _ = probe_keys(block, counts, videos, len(S), vid_base, sent_base)
    for R in Rs:
        rk = rank_keys_for(keys, rs, R) if R else None
        for k in ks:
            if k == 0 and R == 0:
                continue
            d, i, c, _ = run(vfr, S, bank, videos, k, rk, vid_base, sent_base)
            wd, wi, wc, _ = statement(block, counts, videos, len(S), k, vid_base, sent_base, rk)
            if k:
                assert np.array_equal(i, wi), f"top-{k} sentence ids differ (R = {R})"
                assert np.array_equal(d, wd), f"top-{k} distances differ (R = {R})"
            if R:
                assert np.array_equal(c, wc), f"rank counts differ (R = {R}, k = {k})"


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 700])
def test_bank_sizes_and_k(vfr, oracle, ns):
    """Ns in {1, 63, 64, 65, 700} x k in {0, 1, 10, 100, 448} (k > Ns pads) x 0..4 rank keys.  Ns = 65 also takes k on both sides
    of the list capacities (128 | 256 slots at k = 64 | 65, 256 | 512 at k = 192 | 193)."""
    V, counts, off = corpus(synth.clip_counts(40, "didemo", seed=3), seed=3)
    S = sentences(ns, seed=4)
    videos = np.random.RandomState(5).randint(0, 40, 37).astype(np.int64)        # unsorted, with repeats
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    ks = (0, 1, 10, 100, 448) + ((64, 65, 192, 193) if ns == 65 else ())
    check(vfr, block, S, V, counts, off, videos, ks, Rs=(0, 1, 2, 3, 4))


@pytest.mark.parametrize("D", [100, 36, 13])
def test_ragged_64_clips_and_ties(vfr, oracle, D):
    """Ragged banks with 1..64 clips; duplicated sentence rows (the sentence id decides), videos of repeated clips (ground reports
    the first of the tying moments), a sentence lying ON a clip (eps-only distance)."""
    from vfr_amd import engine
    rs = np.random.RandomState(11)
    counts = np.concatenate([np.arange(1, 22), rs.randint(1, 65, 30), [64, 64, 63]])
    V, counts, off = corpus(counts, D=D, seed=12, repeat=(9, 52))
    S = sentences(333, D=D, seed=13)
    S[100:140] = S[17]                                        # duplicated sentences: ties broken by sentence id
    S[200] = S[5]
    S[7] = V[off[30]]                                         # a sentence ON a clip
    nv = len(counts)
    videos = np.concatenate([rs.permutation(nv), [9, 52, 30, nv - 1, 9]]).astype(np.int64)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    check(vfr, block, S, V, counts, off, videos, (1, 10, 100, 448), Rs=(0, 4))
    # grounding: the first argmin in generate_moments order, through the pairs call
    shard = engine.corpus_from_embeddings(dev(V), counts, DEV, engine.HipOps())
    d, i, _, mom = engine.corpus_video_sentence_topk(shard, dev(S), videos, 10, ground=True)
    wd, wi, _, _, wm = statement(block, counts, videos, len(S), 10, ground=True)
    assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd) and np.array_equal(mom.cpu().numpy(), wm)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    for p in (nv, nv + 1):                                    # the probes on videos 9 and 52: all spans of one length tie
        n = int(counts[videos[p]])                            # (equal clips, the same sum), so the best moment starts at clip 0:
        local = mom.cpu().numpy()[p] - mo[videos[p]]          # local id 0, or n + e - 1 for the span (0, e)
        assert n > 1 and np.all((local == 0) | ((local >= n) & (local <= 2 * n - 2)))
    p30 = nv + 2
    assert wi[p30, 0] == 7 and wm[p30, 0] == mo[30]           # the sentence on video 30's first clip lands on that clip


def _shifted(a):
    """The rows of ``a`` on the device starting one float past a 16-byte boundary."""
    buf = torch.empty((a.size + 4,), dtype=torch.float32, device=DEV)
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def test_unaligned_rows_take_the_generic_path(vfr, oracle):
    """S and V offset by one float at D = 100 (the generic loop) against the aligned run (the register-resident path)."""
    V, counts, off = corpus(synth.clip_counts(30, "didemo", seed=21), seed=21)
    S = sentences(200, seed=22)
    videos = np.arange(30, dtype=np.int64)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    keys, _, _ = probe_keys(block, counts, videos, len(S))
    rk = rank_keys_for(keys, np.random.RandomState(23), 2)
    aligned = run(vfr, S, vfr.VideoBank(dev(V), dev(off)), videos, 50, rk)
    wd, wi, wc, _ = statement(block, counts, videos, len(S), 50, rank_keys=rk)
    for Sx, Vx in ((_shifted(S), dev(V)), (dev(S), _shifted(V)), (_shifted(S), _shifted(V))):
        d, i, c, _ = run(vfr, Sx, vfr.VideoBank(Vx, dev(off)), videos, 50, rk)
        assert np.array_equal(d, aligned[0]) and np.array_equal(i, aligned[1]) and np.array_equal(c, aligned[2])
    assert np.array_equal(aligned[0], wd) and np.array_equal(aligned[1], wi) and np.array_equal(aligned[2], wc)


@pytest.mark.parametrize("shape", [(1, 5000), (300, 130)])
def test_chunk_edges(vfr, oracle, shape):
    """1 probe x 5 000 sentences (the sentence axis cut into many chunks) and 300 probes x 130 sentences (a few chunks, the last
    one holding two sentences)."""
    npr, ns = shape
    V, counts, off = corpus(synth.clip_counts(50, "didemo", seed=31), seed=31)
    S = sentences(ns, seed=32)
    videos = np.random.RandomState(33).randint(0, 50, npr).astype(np.int64)
    block = sliced_blocks(oracle.score_moments, S, V, off)
    check(vfr, block, S, V, counts, off, videos, (1, 100), Rs=(0, 4))


def test_zero_clip_videos_and_a_larger_max_clips(vfr, oracle):
    """Videos without clips give padding, add nothing and are not bad; max_clips passed larger than the bank's real maximum."""
    counts = np.asarray([3, 0, 5, 0, 0, 8, 1, 0], np.int64)
    V, counts, off = corpus(counts, seed=41)
    S = sentences(150, seed=42)
    videos = np.asarray([1, 0, 3, 5, 7, 2, 4, 6, 1], np.int64)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    for max_clips in (8, 21, 64):
        bank = vfr.VideoBank(dev(V), dev(off), max_clips=max_clips, total_moments=int((counts * (counts + 1) // 2).sum()), min_clips=0)
        check(vfr, block, S, V, counts, off, videos, (0, 7, 100), Rs=(0, 2), bank=bank)
        huge = np.full((1, len(videos)), np.uint64(0x7F000000) << np.uint64(32), np.uint64)    # every real key sorts before it
        d, i, c, bad = run(vfr, S, bank, videos, 5, huge, want_bad=True)
        empty = counts[videos] == 0
        assert bad == 0 and np.all(i[empty] == -1) and np.all(np.isinf(d[empty])) and np.all(c[0, empty] == 0)
        assert np.all(c[0, ~empty] == len(S))


def test_shards_and_bad_probes(vfr, oracle):
    """A clip bank holding global videos [300, 700) of 1000 with vid_base = 300 and sent_base > 0: probes on both sides are
    skipped (padding, +0); video < 0 sets bad and leaves the good probes' outputs alone; sentence-bank halves chain."""
    Vall, call, offall = corpus(synth.clip_counts(1000, "didemo", seed=17), seed=17)
    S = sentences(301, seed=18)
    rs = np.random.RandomState(19)
    videos = rs.randint(0, 1000, 200).astype(np.int64)
    lo, hi = 300, 700
    V = Vall[offall[lo]:offall[hi]]
    off = (offall[lo:hi + 1] - offall[lo]).astype(np.int32)
    sub = call[lo:hi]
    block = sliced_blocks(oracle.score_moments, S, V, off)
    check(vfr, block, S, V, sub, off, videos, (1, 100), Rs=(0, 2), vid_base=lo, sent_base=1000)
    bank = vfr.VideoBank(dev(V), dev(off))
    outside = (videos < lo) | (videos >= hi)
    assert (videos < lo).any() and (videos >= hi).any()
    huge = np.full((1, len(videos)), np.uint64(0x7F000000) << np.uint64(32), np.uint64)
    d, i, c, bad = run(vfr, S, bank, videos, 10, huge, lo, 1000, want_bad=True)
    assert bad == 0 and np.all(i[outside] == -1) and np.all(np.isinf(d[outside])) and np.all(c[0, outside] == 0)
    assert np.all(c[0, ~outside] == len(S)) and i[~outside].min() >= 1000
    # video < 0
    withbad = np.concatenate([videos[:50], [-1], videos[50:], [-7]])
    hb = np.full((1, len(withbad)), huge[0, 0], np.uint64)
    db, ib, cb, bad = run(vfr, S, bank, withbad, 10, hb, lo, 1000, want_bad=True)
    good = np.ones(len(withbad), bool)
    good[[50, len(withbad) - 1]] = False
    assert bad == 1 and np.all(ib[~good] == -1) and np.all(np.isinf(db[~good])) and np.all(cb[0, ~good] == 0)
    assert np.array_equal(db[good], d) and np.array_equal(ib[good], i) and np.array_equal(cb[0, good], c[0])
    wd, wi, wc, wbad = statement(block, sub, withbad, len(S), 10, lo, 1000, hb)
    assert wbad == 1 and np.array_equal(db, wd) and np.array_equal(ib, wi) and np.array_equal(cb, wc)
    # sentence shards: counts chain through count_lt, lists merge with vfr_topk_merge_f32
    keys, _, _ = probe_keys(block, sub, videos, len(S), lo)
    rd, ri = split_keys(rank_keys_for(keys, rs, 2))
    rd, ri = rd.to(DEV), ri.to(DEV)
    vt = dev(videos, torch.int32)
    k, half = 100, 130
    d1, i1, c1 = vfr.score_video_sentences(dev(S), bank, vt, k, lo, 0, rd, ri)
    da, ia, cc = vfr.score_video_sentences(dev(S[:half]), bank, vt, k, lo, 0, rd, ri)
    db, ib, cc = vfr.score_video_sentences(dev(S[half:]), bank, vt, k, lo, half, rd, ri, count_lt=cc)
    dm, im = vfr.topk_merge(torch.stack([da, db]), torch.stack([ia, ib]))
    assert torch.equal(dm, d1) and torch.equal(im, i1) and torch.equal(cc, c1)


@pytest.mark.parametrize("world", [2, 3])
def test_two_shard_bank_through_the_engine(vfr, oracle, world):
    """engine.corpus_video_sentence_topk over a video-sharded bank (thread ranks on the one device: lists merged, counts summed,
    own keys MIN- and moments MAX-reduced) = the one-shard result = the statement."""
    from vfr_amd import engine
    V, counts, off = corpus(synth.clip_counts(90, "didemo", seed=51), seed=51)
    counts[13] = 0
    V, counts, off = corpus(counts, seed=51)
    S = sentences(400, seed=52)
    rs = np.random.RandomState(53)
    videos = np.concatenate([rs.randint(0, 90, 60), [13, 0, 89, 89]]).astype(np.int64)
    lens = rs.randint(0, 4, len(videos))
    own_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    own_rows = rs.randint(0, len(S), int(own_off[-1])).astype(np.int64)
    ops = engine.HipOps()
    St, Vt = dev(S), dev(V)
    one = engine.corpus_video_sentence_topk(engine.corpus_from_embeddings(Vt, counts, DEV, ops), St, videos, 20, own_off, own_rows,
                                            ground=True, ops=ops)
    block = dense_blocks(oracle.score_moments(S, V, off), counts)
    keys, _, _ = probe_keys(block, counts, videos, len(S))
    wd, wi, _, _, wm = statement(block, counts, videos, len(S), 20, ground=True)
    assert np.array_equal(one[0].cpu().numpy(), wd) and np.array_equal(one[1].cpu().numpy(), wi)
    assert np.array_equal(one[2].cpu().numpy(), own_ranks(keys, own_off, own_rows)) and (lens == 0).any()
    assert np.array_equal(one[3].cpu().numpy(), wm)
    group = ThreadRanks(world)
    old = engine._dist
    engine._dist = lambda: group
    try:
        def body(rank, n):
            torch.cuda.set_device(0)
            shard = engine.corpus_from_embeddings(Vt, counts, DEV, ops, rank, n)
            return [t.cpu() for t in engine.corpus_video_sentence_topk(shard, St, videos, 20, own_off, own_rows, ground=True,
                                                                       ops=ops, world=n)]
        outs = group.run(body)
    finally:
        engine._dist = old
    for got in outs:
        for g, w in zip(got, one):
            assert torch.equal(g, w.cpu())


def test_identities_on_the_device_paths(vfr):
    """With Q = S, score_video_topk(k = Nv) lists every b(j, v) with the moment that attains it: entry (p, r) of the new call
    carries the bits of b(out_idx[p, r], v_p); score_paragraph_pairs with groups of length 1 on the returned pairs gives the same
    scores and the moments ground=True reports."""
    from vfr_amd import engine
    V, counts, off = corpus(synth.clip_counts(60, "didemo", seed=14), seed=14)
    S = sentences(500, seed=15)
    nv, ns, k = len(counts), len(S), 100
    videos = np.random.RandomState(16).permutation(nv)[:45].astype(np.int64)
    ops = engine.HipOps()
    shard = engine.corpus_from_embeddings(dev(V), counts, DEV, ops)
    St = dev(S)
    d, i, _, mom = engine.corpus_video_sentence_topk(shard, St, videos, k, ground=True, ops=ops)
    d, i, mom = d.cpu().numpy(), i.cpu().numpy(), mom.cpu().numpy()
    assert (i >= 0).all()
    vd, vi, _ = vfr.score_video_topk(St, shard.bank, nv)                       # [Ns, Nv]: every video's best key per sentence
    vd, vi = vd.cpu().numpy(), vi.cpu().numpy()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    vid = np.searchsorted(mo, vi, side="right") - 1
    b = np.empty((ns, nv), np.float32)
    m = np.empty((ns, nv), np.int64)
    rows = np.arange(ns)[:, None]
    b[rows, vid] = vd
    m[rows, vid] = vi
    assert np.array_equal(d.view(np.uint32), b[i, videos[:, None]].view(np.uint32))
    assert np.array_equal(mom, m[i, videos[:, None]])
    # the k smallest of column v_p, in (bits, sentence) order
    for p, v in enumerate(videos.tolist()):
        order = np.argsort(b[:, v], kind="stable")[:k]
        assert np.array_equal(i[p], order)
    pairs = np.stack([np.arange(len(videos) * k), np.repeat(videos, k)], axis=1).astype(np.int32)
    one = torch.arange(len(pairs) + 1, dtype=torch.int64, device=DEV)
    ps, pm = vfr.score_paragraph_pairs(St[dev(i.reshape(-1))].contiguous(), shard.bank, one, 1, dev(pairs))
    assert np.array_equal(ps.cpu().numpy().view(np.uint32), d.reshape(-1).view(np.uint32))
    assert np.array_equal(pm.cpu().numpy().reshape(-1), mom.reshape(-1))


def test_nothing_to_do(vfr):
    """Np = 0, Ns = 0, and k = 0 without rank keys."""
    V, counts, off = corpus([3, 4, 5], seed=61)
    S = sentences(20, seed=62)
    bank = vfr.VideoBank(dev(V), dev(off))
    none = torch.zeros((0,), dtype=torch.int32, device=DEV)
    d, i, c = vfr.score_video_sentences(dev(S), bank, none, 5)
    assert tuple(d.shape) == (0, 5) and tuple(i.shape) == (0, 5) and c is None
    videos = dev(np.asarray([2, 0, 1]), torch.int32)
    assert vfr.score_video_sentences(dev(S), bank, videos, 0) == (None, None, None)
    rd, ri = torch.full((1, 3), float("inf"), device=DEV), torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    d, i, c = vfr.score_video_sentences(torch.zeros((0, 100), device=DEV), bank, videos, 4, rank_dist=rd, rank_idx=ri)
    torch.cuda.synchronize()
    assert torch.isinf(d).all() and (i == -1).all() and (c == 0).all()


def test_host_argument_errors_enqueue_nothing(vfr):
    """Bad host arguments give VFR_EINVAL and a short workspace VFR_EWORKSPACE; the outputs stay as they were."""
    V, counts, off = corpus([3, 4, 5], seed=71)
    S = dev(sentences(70, seed=72))
    bank = vfr.VideoBank(dev(V), dev(off))
    videos = dev(np.asarray([2, 0, 1]), torch.int32)
    k = 4
    od = torch.full((3, k), 123.0, device=DEV)
    oi = torch.full((3, k), 77, dtype=torch.int64, device=DEV)
    cnt = torch.full((1, 3), 5, dtype=torch.int64, device=DEV)
    rd, ri = torch.full((1, 3), float("inf"), device=DEV), torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    lib = vfr.lib()
    nb = lib.vfr_score_video_sentences_workspace_bytes(3, 70, k)
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)

    def call(Ns=70, max_clips=bank.max_clips, D=100, Np=3, vid_base=0, sent_base=0, kk=k, num_rank=1, wsb=nb, vp=videos.data_ptr()):
        return lib.vfr_score_video_sentences_f32(S.data_ptr(), Ns, bank.emb.data_ptr(), bank.clip_off.data_ptr(), 3, bank.total_clips,
                                                 max_clips, D, ctypes.c_float(1e-6), vp, Np, vid_base, sent_base, kk, od.data_ptr(),
                                                 oi.data_ptr(), num_rank, rd.data_ptr(), ri.data_ptr(), cnt.data_ptr(), None,
                                                 ws.data_ptr(), wsb, None)
    for bad in (dict(kk=449), dict(kk=-1), dict(max_clips=65), dict(D=0), dict(Ns=-1), dict(Np=-1), dict(vid_base=-1),
                dict(sent_base=-1), dict(num_rank=5), dict(sent_base=(1 << 32) - 70), dict(vp=None)):
        assert call(**bad) == -1, bad
    assert call(wsb=nb - 256) == -4
    torch.cuda.synchronize()
    assert (od == 123.0).all() and (oi == 77).all() and (cnt == 5).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (oi >= 0).all() and (cnt == 5 + 70).all()              # counts are ADDED: every key sorts before (+inf, 0)


def test_evaluate_video_sentences_device_equals_cpu_provider(vfr):
    """evaluate_video_sentences on the device = the CPU provider (engine.TorchCpuOps) on the device's own embeddings: identical
    metric dicts and top-k lists."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(45, 30, "didemo", feat_dim=64, hidden=16)
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)
    vi, li = ds.iterators()
    got, (d, i, videos) = vevaluate.evaluate_video_sentences(model, vi, li, ds.annotations, DEV, return_topk=10)
    ops = engine.HipOps()
    vi, li = ds.iterators()
    shard, names = vevaluate.embed_corpus(model, vi, DEV, ops)
    tokens, q_videos, _ = vevaluate._drain_queries(li)
    Se = engine.encode_queries(model, torch.cat(tokens), DEV, ops).cpu()
    own = np.asarray([names.index(v) for v in q_videos], np.int64)
    wvideos, lengths = np.unique(own, return_counts=True)
    cpu = engine.TorchCpuOps()
    cshard = engine.corpus_from_embeddings(shard.bank.emb.cpu(), p["counts"], "cpu", cpu)
    wd, wi, wr, _ = engine.corpus_video_sentence_topk(cshard, Se, wvideos, 10, np.concatenate([[0], np.cumsum(lengths)]),
                                                      np.argsort(own, kind="stable"), ops=cpu)
    wr = wr.numpy()
    want = vevaluate.get_metrics({1: (wr < 1).astype(int), 5: (wr < 5).astype(int), 10: (wr < 10).astype(int),
                                  50: (wr < 50).astype(int), "MR": wr})
    assert got == {"video_sentence": want} and (wr >= 0).all()
    assert np.array_equal(videos, wvideos) and torch.equal(i.cpu(), wi) and torch.equal(d.cpu(), wd)
