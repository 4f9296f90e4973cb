"""Hard-negative mining on the GPU (vfr_score_spans_f32, vfr_mine_negatives_f32, engine.corpus_mine_negatives,
training.HardNegativeSampler) against the numpy statement of tests/mining_reference.py on the oracle's dense moment scores, bit
for bit; the identity of vfr_score_spans_f32 with the device's own dense path; and one training epoch on mined triplets."""
import random

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from mining_reference import eligible, local_id, moment_offsets, span_scores, statement
from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("inter_dist", "inter_vid", "intra_dist", "intra_idx", "count_inter", "count_intra")


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def corpus(counts, D=100, seed=0, nq=11, same=(), repeat=()):
    """Random clip rows and queries; ``same`` = pairs of equally long videos given identical rows (tied scores), ``repeat`` =
    videos whose clips are all alike (ties inside a video)."""
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    for a, b in same:
        assert counts[a] == counts[b]
        V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
    for v in repeat:
        V[off[v]:off[v + 1]] = V[off[v]]
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, off.astype(np.int32)


def random_items(rs, counts, nm, nq, vids=None, base=0):
    v = rs.randint(0, len(counts), nm) if vids is None else np.asarray(vids)[rs.randint(0, len(vids), nm)]
    n = np.asarray(counts)[v]
    s = (rs.rand(nm) * n).astype(np.int64)
    e = s + (rs.rand(nm) * (n - s)).astype(np.int64)
    return np.stack([rs.randint(0, nq, nm), v + base, s, e], axis=1).astype(np.int64)


def run(vfr, Q, V, off, items, h, mode="same_length", excl=None, floor=None, thr=None, vid_base=0, id_base=0):
    bank = vfr.VideoBank(dev(V), dev(off), id_base)
    bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
    got = vfr.mine_negatives(dev(Q), bank, dev(items, torch.int32), h, vid_base, mode, dev(excl, torch.int32), dev(floor), dev(thr),
                             bad=bad)
    torch.cuda.synchronize()
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in zip(KEYS, got)}
    out["bad"] = int(bad.item())
    return out


def check(vfr, Sc, Q, V, counts, off, items, hs, mode="same_length", excl=None, floor=None, thr=None, vid_base=0, id_base=0, what=""):
    for h in hs:
        if h == 0 and thr is None:
            continue
        got = run(vfr, Q, V, off, items, h, mode, excl, floor, thr, vid_base, id_base)
        want = statement(Sc, counts, items, h, vid_base, id_base, mode, excl, floor, thr)
        assert got["bad"] == want["bad"], (what, h)
        for k in KEYS[:4] if h else ():
            assert np.array_equal(got[k], want[k]), f"{what}: {k} differs (h = {h}, {mode})"
        for k in KEYS[4:] if thr is not None else ():
            assert np.array_equal(got[k], want[k]), f"{what}: {k} differs (h = {h}, {mode})"
    return want


def mixed_counts(nv, seed):
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = 21
    c[-1] = 21
    return c


@pytest.mark.parametrize("nv", [1, 2, 63, 64, 65, 130])
def test_chunk_edges_and_own_video_positions(vfr, oracle, nv):
    """Banks that end before, on and after a chunk of 64 videos, clip counts mixed 1..21 (many videos shorter than e + 1), the own
    video first, at both sides of a chunk edge and last.  Nv = 130 also takes h on both sides of the inter list's capacities (128 |
    256 slots at h = 64 | 65, 256 | 512 at h = 192 | 193)."""
    counts = mixed_counts(nv, nv)
    for v in (63, 64):
        if v < nv:
            counts[v] = 15
    Q, V, counts, off = corpus(counts, seed=nv)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(100 + nv)
    owns = sorted({v for v in (0, 63, 64, nv - 1) if v < nv})
    items = np.concatenate([random_items(rs, counts, 12, len(Q), vids=owns), random_items(rs, counts, 20, len(Q))])
    pos, _ = span_scores(Sc, counts, items)
    thr = (pos + np.float32(0.1)).astype(np.float32)
    hs = (0, 1, 16) + ((64, 65, 192, 193) if nv == 130 else ())
    for mode in ("same_length", "any"):
        check(vfr, Sc, Q, V, counts, off, items, hs, mode, thr=thr, what=f"Nv = {nv}")


@pytest.mark.parametrize("nm", [0, 1, 65])
def test_item_counts(vfr, oracle, nm):
    Q, V, counts, off = corpus(mixed_counts(130, 7), seed=7)
    Sc = oracle.score_moments(Q, V, off)
    items = random_items(np.random.RandomState(8), counts, nm, len(Q))
    thr = np.full(nm, 3.0, np.float32)
    check(vfr, Sc, Q, V, counts, off, items, (0, 16), thr=thr, what=f"Nm = {nm}")
    got = run(vfr, Q, V, off, items, 16)
    assert got["inter_dist"].shape == (nm, 16) and got["count_inter"] is None


@pytest.mark.parametrize("mode", ["same_length", "any"])
def test_long_videos_full_spans_and_h(vfr, oracle, mode):
    """max_clips = 64; spans of one clip, of the full video, (0, 0) of a 1-clip video (no intra negative at all: padding);
    h in {0, 1, 16, 448} with fewer eligible videos than h."""
    counts = np.concatenate([[1, 64, 64, 2, 1, 40], np.random.RandomState(9).randint(1, 65, 24)])
    Q, V, counts, off = corpus(counts, seed=9)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(10)
    fixed = [(0, 0, 0, 0), (1, 4, 0, 0), (2, 1, 0, 63), (3, 2, 0, 63), (4, 1, 17, 17), (5, 3, 0, 1), (6, 5, 0, 39), (7, 1, 3, 60)]
    items = np.concatenate([np.asarray(fixed, np.int64), random_items(rs, counts, 25, len(Q))])
    pos, _ = span_scores(Sc, counts, items)
    thr = (pos + np.float32(0.1)).astype(np.float32)
    want = check(vfr, Sc, Q, V, counts, off, items, (0, 1, 16, 448), mode, thr=thr, what="long videos")
    assert np.all(want["intra_idx"][[0, 1]] == -1)                           # 1-clip videos
    if mode == "same_length":
        assert np.all(want["intra_idx"][[2, 3, 5, 6]] == -1)                 # full-video spans
        assert want["inter_vid"][2, 0] == 2 and np.all(want["inter_vid"][2, 1:] == -1)    # one other video has 64 clips
    else:
        assert (want["intra_idx"][2] >= 0).all()                             # 2079 other moments, the 448 hardest listed


def test_streams_of_several_blocks_per_wave(vfr, oracle):
    """2 100 items against 1 100 videos: the video axis is cut into 2 chunks of 576 and 524 videos, so one wave streams 9 blocks of
    64 videos under its running threshold -- the list fills and is sorted and cut back to h inside the loop (h = 1 and 16 after two
    blocks, h = 448 after eight), later keys are tested against the threshold, and the last block of a chunk is partial.  Tied
    videos sit in different blocks of one chunk and in different chunks.  h = 64 | 65 and 192 | 193 sit on both sides of the list
    capacities (128 | 256 and 256 | 512 slots): here, unlike at Nv = 130, each of those lists fills and is cut back."""
    lib = vfr.lib()
    nv, distinct, rep = 1100, 60, 35
    assert lib.vfr_mine_negatives_workspace_bytes(distinct * rep, nv, 448) == 256 + 2 * distinct * rep * 448 * 8      # 2 chunks
    counts = np.random.RandomState(27).randint(4, 22, nv).astype(np.int64)
    same = ((3, 130), (70, 500), (130, 575), (600, 1000), (20, 640))
    for a, b in same:
        counts[b] = counts[a]
    Q, V, counts, off = corpus(counts, seed=27, same=same)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(28)
    short = random_items(rs, np.full(nv, 4), distinct // 2, len(Q))          # spans inside the first 4 clips: every video eligible
    short[:5, 1] = (3, 130, 70, 600, 1000)
    base = np.concatenate([short, random_items(rs, counts, distinct - len(short), len(Q))])
    pick = np.concatenate([np.arange(distinct), rs.randint(0, distinct, distinct * (rep - 1))])
    items = base[pick]
    pos, _ = span_scores(Sc, counts, base)
    floor = np.where(np.arange(distinct) % 2 == 0, pos, np.float32(0)).astype(np.float32)
    thr = (pos + np.float32(0.1)).astype(np.float32)
    for h in (1, 16, 64, 65, 192, 193, 448):
        want = statement(Sc, counts, base, h, floor=floor, thr=thr)
        got = run(vfr, Q, V, off, items, h, floor=floor[pick], thr=thr[pick])
        assert got["bad"] == 0
        for k in KEYS:
            assert np.array_equal(got[k], want[k][pick]), f"{k} differs (h = {h})"
    assert np.all(want["inter_vid"][1:distinct // 2:2, -1] >= 0)             # 1 099 eligible videos, no floor: the cut happened
    d, i = want["inter_dist"], want["inter_vid"]
    tied = (d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])
    assert tied.any() and np.all(i[:, 1:][tied] > i[:, :-1][tied])


def test_ties_are_ordered_by_id(vfr, oracle):
    """Videos with identical clip rows on both sides of a chunk edge and far apart, and an own video of repeated clips: tied
    scores are ordered by the global video index / the moment id."""
    counts = np.full(130, 6, np.int64)
    Q, V, counts, off = corpus(counts, seed=11, same=((63, 64), (63, 5), (10, 100), (10, 129)), repeat=(20, 64))
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(12)
    items = np.concatenate([random_items(rs, counts, 30, len(Q)), random_items(rs, counts, 12, len(Q), vids=(20, 64, 63, 10))])
    for mode in ("same_length", "any"):
        want = check(vfr, Sc, Q, V, counts, off, items, (1, 16, 448), mode, what="ties")
    d, i = want["inter_dist"], want["inter_vid"]
    tied = (d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])
    assert tied.any() and np.all(i[:, 1:][tied] > i[:, :-1][tied])
    d, i = want["intra_dist"], want["intra_idx"]
    tied = (d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])
    assert tied.any() and np.all(i[:, 1:][tied] > i[:, :-1][tied])


def test_floor_and_threshold_edges(vfr, oracle):
    """A floor equal to a real key's score (that key is not listed: strict >), a floor above everything (all padding), a threshold
    between two scores and one equal to a score (strict <)."""
    Q, V, counts, off = corpus(mixed_counts(70, 13), seed=13)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(14)
    items = random_items(rs, counts, 40, len(Q), vids=np.flatnonzero(counts >= 4))
    Nm = len(items)
    floor, thr = np.zeros(Nm, np.float32), np.zeros(Nm, np.float32)
    for m, it in enumerate(items):
        sc, _, isc, _ = eligible(Sc, counts, it, mode="any")
        srt = np.sort(np.concatenate([sc, isc]))
        if m % 4 == 0:
            floor[m], thr[m] = srt[2], srt[4]                                # equal to real scores
        elif m % 4 == 1:
            floor[m], thr[m] = srt[-1], np.nextafter(srt[3], np.float32(np.inf))     # above everything / between two scores
        elif m % 4 == 2:
            floor[m], thr[m] = np.float32(np.inf), np.float32(np.inf)
        else:
            floor[m], thr[m] = np.float32(0), np.float32(0)
    for mode in ("same_length", "any"):
        want = check(vfr, Sc, Q, V, counts, off, items, (0, 3, 16), mode, floor=floor, thr=thr, what="floor / thr")
        assert np.all(want["inter_vid"][1::4] == -1) and np.all(want["intra_idx"][1::4] == -1)
        assert np.all(want["inter_vid"][2::4] == -1) and np.all(want["count_inter"][3::4] == 0)
        assert np.all(want["inter_dist"][0::4, 0] > floor[0::4]) and want["count_inter"].sum() > 0


@pytest.mark.parametrize("X", [1, 4, 8])
def test_any_mode_exclusions(vfr, oracle, X):
    """VFR_MINE_ANY with X excluded spans per item: the positive itself, duplicates, spans outside the video, padded rows."""
    Q, V, counts, off = corpus(mixed_counts(40, 15), seed=15)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(16 + X)
    items = random_items(rs, counts, 50, len(Q))
    excl = np.full((len(items), X, 2), -1, np.int64)
    for m, (_, v, s, e) in enumerate(items):
        n = int(counts[v])
        for j in range(rs.randint(0, X + 1)):
            a = rs.randint(0, n)
            excl[m, j] = (a, rs.randint(a, n + 2)) if j % 3 else (excl[m, j - 1] if j else (s, e))
    check(vfr, Sc, Q, V, counts, off, items, (5, 448), "any", excl=excl, thr=np.full(len(items), 2.0, np.float32), what=f"X = {X}")


@pytest.mark.parametrize("D", [100, 96, 33])
def test_dimensions(vfr, oracle, D):
    Q, V, counts, off = corpus(mixed_counts(90, 17), D=D, seed=17)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(18)
    items = random_items(rs, counts, 60, len(Q))
    items = np.concatenate([items, items[:10], items[rs.permutation(30)]])          # repeated, unsorted, shared query rows
    pos, bad = span_scores(Sc, counts, items)
    for mode in ("same_length", "any"):
        check(vfr, Sc, Q, V, counts, off, items, (1, 16), mode, floor=pos, thr=(pos + np.float32(0.1)).astype(np.float32), what=f"D = {D}")
    bank = vfr.VideoBank(dev(V), dev(off))
    got = vfr.score_spans(dev(Q), bank, dev(items, torch.int32)).cpu().numpy()
    assert bad == 0 and np.array_equal(got, pos)


def test_bad_items(vfr, oracle):
    """bad is set and the item padded for a query row out of range, a negative video, e >= n, e < s, s < 0; good neighbours are
    unaffected.  Nothing here faults: the kernels check before they read."""
    Q, V, counts, off = corpus([3, 4, 5, 6, 2, 7], seed=19)
    Sc = oracle.score_moments(Q, V, off)
    good = [(0, 0, 0, 2), (1, 3, 1, 4), (2, 4, 1, 1)]
    cases = {"ok": ((3, 2, 0, 4), 0), "query row too large": ((len(Q), 1, 0, 0), 1), "negative query row": ((-1, 1, 0, 0), 1),
             "negative video": ((0, -1, 0, 0), 1), "end < start": ((0, 1, 2, 1), 1), "end >= n": ((0, 1, 0, 4), 1),
             "negative start": ((0, 2, -1, 1), 1), "video of no shard": ((0, 99, 0, 1), 0)}
    bank = vfr.VideoBank(dev(V), dev(off))
    for name, (extra, want_bad) in cases.items():
        items = np.asarray(good[:2] + [extra] + good[2:], np.int64)
        thr = np.full(len(items), 9.0, np.float32)
        for mode in ("same_length", "any"):
            got = run(vfr, Q, V, off, items, 4, mode, thr=thr)
            want = statement(Sc, counts, items, 4, mode=mode, thr=thr)
            assert got["bad"] == want_bad == want["bad"], name
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (name, k)
            if want_bad:
                assert np.all(got["inter_vid"][2] == -1) and np.all(got["intra_idx"][2] == -1) and got["count_inter"][2] == 0, name
        bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
        sp = vfr.score_spans(dev(Q), bank, dev(items, torch.int32), bad=bad).cpu().numpy()
        wp, wb = span_scores(Sc, counts, items)
        assert np.array_equal(sp, wp) and int(bad.item()) == wb == want_bad, name


def test_shards_with_bases(vfr, oracle):
    """A bank that holds global videos [40, 110) of 150 (vid_base = 40, id_base = its first moment id): items whose own video
    belongs to another shard get their complete inter list and an untouched intra list; two shards chain to the one-bank result."""
    Qa, Va, ca, offa = corpus(mixed_counts(150, 21), seed=21)
    rs = np.random.RandomState(22)
    items = random_items(rs, ca, 80, len(Qa))
    lo, hi = 40, 110
    mo = moment_offsets(ca)
    V, off, sub = Va[offa[lo]:offa[hi]], (offa[lo:hi + 1] - offa[lo]).astype(np.int32), ca[lo:hi]
    Sc = oracle.score_moments(Qa, V, off)
    outside = (items[:, 1] < lo) | (items[:, 1] >= hi)
    assert outside.any() and (~outside).any()
    thr = np.full(len(items), 2.5, np.float32)
    for mode in ("same_length", "any"):
        want = check(vfr, Sc, Qa, V, sub, off, items, (0, 16), mode, thr=thr, vid_base=lo, id_base=int(mo[lo]), what="shard")
        assert np.all(want["intra_idx"][outside] == -1) and np.all(want["count_intra"][outside] == 0)
        assert np.all(want["inter_vid"][outside][:, 0] >= lo) and want["intra_idx"][~outside].max() >= mo[lo]
    # three shards chained on the device = the whole bank
    whole = vfr.VideoBank(dev(Va), dev(offa))
    Qd, it, td = dev(Qa), dev(items, torch.int32), dev(thr)
    one = vfr.mine_negatives(Qd, whole, it, 16, thr=td)
    parts, intra, ci, ca_ = [], None, None, None
    pos = None
    for a, b in ((0, lo), (lo, hi), (hi, 150)):
        sh = vfr.slice_bank(whole, ca, a, b)
        r = vfr.mine_negatives(Qd, sh, it, 16, a, thr=td, intra_out=intra, count_inter=ci, count_intra=ca_)
        parts.append((r[0], r[1]))
        intra, ci, ca_ = (r[2], r[3]), r[4], r[5]
        pos = vfr.score_spans(Qd, sh, it, a, out=pos)
    md, mi = vfr.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(md, one[0]) and torch.equal(mi, one[1]) and torch.equal(intra[0], one[2]) and torch.equal(intra[1], one[3])
    assert torch.equal(ci, one[4]) and torch.equal(ca_, one[5])
    assert torch.equal(pos, vfr.score_spans(Qd, whole, it))


def test_score_spans_equals_device_dense_path(vfr):
    """vfr_score_spans_f32 = the entry of vfr_score_moments_f32 at [query row, moment id], bit for bit."""
    Q, V, counts, off = corpus(synth.clip_counts(200, "didemo", seed=23), seed=23, nq=50)
    items = random_items(np.random.RandomState(24), counts, 300, len(Q))
    bank = vfr.VideoBank(dev(V), dev(off))
    Sc = vfr.score_moments(dev(Q), bank).cpu().numpy()
    got = vfr.score_spans(dev(Q), bank, dev(items, torch.int32)).cpu().numpy()
    mo = moment_offsets(counts)
    want = np.asarray([Sc[q, mo[v] + local_id(int(counts[v]), s, e)] for q, v, s, e in items.tolist()], np.float32)
    assert np.array_equal(got, want)


def test_corpus_mine_negatives_gpu(vfr, oracle):
    from vfr_amd import engine
    Q, V, counts, off = corpus(synth.clip_counts(300, "didemo", seed=25), seed=25, nq=40)
    Sc = oracle.score_moments(Q, V, off)
    items = random_items(np.random.RandomState(26), counts, 300, len(Q))
    shard = engine.corpus_from_embeddings(dev(V), counts, DEV, engine.HipOps())
    res = engine.corpus_mine_negatives(shard, dev(Q), items, 16, "same_length", None, True, 0.1)
    pos, _ = span_scores(Sc, counts, items)
    want = statement(Sc, counts, items, 16, floor=pos, thr=(pos + np.float32(0.1)).astype(np.float32))
    assert np.array_equal(res.pos.cpu().numpy(), pos)
    for k in KEYS:
        assert np.array_equal(getattr(res, k).cpu().numpy(), want[k]), k
    spans = res.intra_spans()
    real = want["intra_idx"] >= 0
    assert real.any() and np.all((spans[..., 1] - spans[..., 0])[real] == np.broadcast_to((items[:, 3] - items[:, 2])[:, None], real.shape)[real])
    assert want["count_inter"].sum() > 0                                    # a margin of 0.1 finds violators on random embeddings


def test_sampler_refresh_device_equals_cpu_and_trains(vfr):
    """HardNegativeSampler.refresh on the device = the TorchCpuOps refresh on the same embeddings (encoded once on the device and
    copied); then one Trainer.train_epoch over the mined triplets runs to a finite loss."""
    from vfr_amd import engine, training
    p = problem(40, 60, "didemo", feat_dim=64, hidden=16)
    counts = p["counts"]
    times = [[[s, e - 1 if s == 0 and e == counts[p["own"][q]] - 1 and e > 0 else e] for s, e in t] for q, t in enumerate(p["times"])]
    keep = [q for q, t in enumerate(times) if counts[p["own"][q]] >= 2]
    ds = MemoryDataset(p["seg"], p["ctx"], counts, p["tokens"][keep], p["own"][keep], [times[q] for q in keep])
    model = make_model(p["sd"], feat_dim=64, hidden=16).to(DEV)

    class CopiedEmbeddings(engine.TorchCpuOps):
        def encode_clips(self, model, seg, ctx, clip_off):
            return model.encode_clips(seg.to(DEV), ctx.to(DEV), clip_off.to(DEV)).cpu()

        def encode_queries(self, model, tokens):
            return model.encode_queries(tokens.to(DEV)).cpu()

    args = (32, ds.annotations, ds.num_segments_info)
    on_dev = training.HardNegativeSampler(*args, h=8).refresh(model, ds, DEV, semi_hard=True, margin=0.1)
    on_cpu = training.HardNegativeSampler(*args, h=8).refresh(model, ds, "cpu", CopiedEmbeddings(), semi_hard=True, margin=0.1)
    assert on_dev.mined == on_cpu.mined and len(on_dev.mined) >= len(keep)
    assert on_dev.last_stats == on_cpu.last_stats and on_dev.last_stats["violators_inter"] > 0
    random.seed(3)
    loader = training.TripletLoader(ds, on_dev, DEV)
    model.train()
    torch.manual_seed(0)
    opt = training.Adam(model.parameters(), lr=5e-4, weight_decay=5e-3)
    loss = training.Trainer(device=DEV).train_epoch(model, loader, opt)
    assert np.isfinite(loss) and on_dev.last_stats["mined_draws"] > 0
