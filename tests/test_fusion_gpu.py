"""Late-fusion retrieval on the GPU (vfr_score_fusion_f32, vfr_score_fusion_own_f32, engine.corpus_fusion_topk,
evaluate.evaluate_fusion) against the numpy statement of tests/fusion_reference.py on the oracle's dense moment scores, bit for bit
in distances, ids and counts; the two identities against the device's own single-stream entry points."""
import numpy as np
import pytest
import torch

from fusion_reference import all_moments, fused_scores, level_keys, moment_offsets, own_rows, split_keys, statement
from helpers import MemoryDataset, make_model, problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ("moments", "videos")
DIMS4 = (100, 37, 4, 100)
W4 = (0.5, 0.25, 0.125, 2.0)


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


def streams(counts, dims=(100, 100), seed=0, nq=11, same=(), repeat=()):
    """Random clip rows and queries per stream; ``same`` = pairs of equally long videos given identical rows in EVERY stream (tied
    fused scores), ``repeat`` = videos whose clips are all alike (ties inside a video)."""
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    Qs, Vs = [], []
    for D in dims:
        V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
        for a, b in same:
            assert counts[a] == counts[b]
            V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
        for v in repeat:
            V[off[v]:off[v + 1]] = V[off[v]]
        Vs.append(V)
        Qs.append((rs.randn(nq, D) * 0.3).astype(np.float32))
    return Qs, Vs, counts, off.astype(np.int32)


def mixed_counts(nv, seed):
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = 21
    c[-1] = 21
    return c


def dense(oracle, Qs, Vs, off):
    return [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]


def banks_of(vfr, Vs, off, id_base=0):
    off_t = dev(off)
    return [vfr.VideoBank(dev(V), off_t, id_base) for V in Vs]


def rank_keys(Scs, counts, w, level, id_base=0):
    """Two rank keys per query from the reference's own keys: one present in the bank, one strictly between two keys."""
    K = level_keys(fused_scores(Scs, counts, w), counts, level, id_base)
    nq = K.shape[0]
    if K.shape[1] == 0:
        return np.stack([np.full(nq, 5, np.uint64), np.full(nq, (0x3F800000 << 32) | 7, np.uint64)])
    srt = np.sort(K, axis=1)
    m = srt.shape[1]
    return np.stack([srt[np.arange(nq), (np.arange(nq) * 7) % m], srt[np.arange(nq), (np.arange(nq) * 5 + 2) % m] + np.uint64(1)])


def run(vfr, Qs, banks, w, k, level, rk=None):
    rd = ri = None
    if rk is not None:
        rd, ri = (dev(x) for x in split_keys(rk))
    d, i, c = vfr.score_fusion([dev(Q) for Q in Qs], banks, w, k, level, rd, ri)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d, i, c))


def check(vfr, Scs, Qs, Vs, counts, off, w, ks, levels=LEVELS, id_base=0, what=""):
    banks = banks_of(vfr, Vs, off, id_base)
    for level in levels:
        rk = rank_keys(Scs, counts, w, level, id_base) if len(Qs[0]) else None      # no queries: no rank keys either
        for k in ks:
            if k == 0 and rk is None:
                continue
            d, i, c = run(vfr, Qs, banks, w, k, level, rk)
            wd, wi, wc = statement(Scs, counts, w, k, level, id_base, rk)
            if k:
                assert np.array_equal(i, wi), f"{what}: ids differ ({level}, k = {k})"
                assert np.array_equal(d, wd), f"{what}: distances differ ({level}, k = {k})"
            assert (c is None and wc is None) or np.array_equal(c, wc), f"{what}: counts differ ({level}, k = {k})"


@pytest.mark.parametrize("nv", [1, 2, 63, 64, 65, 130])
def test_chunk_edges(vfr, oracle, nv):
    """Banks that end before, on and after a chunk of 64 videos; clip counts mixed 1..21 with 21 first and last; S = 2.
    Nv = 130 also takes k on both sides of the list capacities (128 | 256 slots at k = 64 | 65, 256 | 512 at k = 192 | 193): a block
    of 64 videos emits over a thousand keys, so the list fills and is cut back at every capacity."""
    Qs, Vs, counts, off = streams(mixed_counts(nv, nv), seed=nv)
    ks = (0, 1, 16, 448) + ((64, 65, 192, 193) if nv == 130 else ())
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, (0.7, 0.3), ks, what=f"Nv = {nv}")


def test_long_videos(vfr, oracle):
    """max_clips = 64: 64 rows of clip distances per lane, triangles of 2080 moments."""
    counts = np.concatenate([[64, 3, 21, 64, 1, 40], np.random.RandomState(9).randint(1, 65, 10)])
    Qs, Vs, counts, off = streams(counts, seed=9)
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, (0.7, 0.3), (1, 16, 448), what="long videos")


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_stream_shapes(vfr, oracle, S):
    """1..4 streams of widths 100 (16-byte loads), 37 (scalar loop), 4, 100 with dyadic and non-dyadic weights."""
    Qs, Vs, counts, off = streams(mixed_counts(70, 40 + S), DIMS4[:S], seed=40 + S)
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, W4[:S], (1, 16), what=f"S = {S}")


def test_identities_on_the_device(vfr, oracle):
    """S = 1, w = (1) and w = (1, 0) are vfr_score_topk_f32 / vfr_score_video_topk_f32 (VFR_SCORE_EXACT) on stream 0; all-zero
    weights give score 0 and ids in ascending order."""
    Qs, Vs, counts, off = streams(mixed_counts(130, 3), (100, 37), seed=3)
    banks = banks_of(vfr, Vs, off, 9)
    Scs = dense(oracle, Qs, Vs, off)
    Q0 = dev(Qs[0])
    for level in LEVELS:
        rk = rank_keys(Scs[:1], counts, (1.0,), level, 9)
        rd, ri = (dev(x) for x in split_keys(rk))
        for k in (1, 16, 448):
            if level == "moments":
                wd, wi, wc = vfr.score_topk(Q0, banks[0], k, rd, ri, mode="exact")
            else:
                wd, wi, wc0 = vfr.score_video_topk(Q0, banks[0], k, rd[0].contiguous(), ri[0].contiguous(), mode="exact")
                _, _, wc1 = vfr.score_video_topk(Q0, banks[0], 0, rd[1].contiguous(), ri[1].contiguous(), mode="exact")
                wc = torch.stack([wc0, wc1])
            torch.cuda.synchronize()
            for Qx, bx, w in (([Qs[0]], banks[:1], (1.0,)), (Qs, banks, (1.0, 0.0))):
                d, i, c = run(vfr, Qx, bx, w, k, level, rk)
                assert np.array_equal(i, wi.cpu().numpy()) and np.array_equal(d, wd.cpu().numpy()), (level, k, w)
                assert np.array_equal(c, wc.cpu().numpy()), (level, k, w)
    mo = moment_offsets(counts)
    d, i, _ = run(vfr, Qs, banks, (0.0, 0.0), 16, "moments")
    assert np.all(d == 0) and np.array_equal(i, np.tile(9 + np.arange(16), (len(Qs[0]), 1)))
    d, i, _ = run(vfr, Qs, banks, (0.0, 0.0), 16, "videos")
    assert np.all(d == 0) and np.array_equal(i, np.tile(9 + mo[:16], (len(Qs[0]), 1)))


def test_ties_are_broken_by_id(vfr, oracle):
    counts = mixed_counts(70, 12)
    counts[[5, 6, 63, 64]] = (8, 8, 13, 13)
    Qs, Vs, counts, off = streams(counts, seed=12, same=((5, 6), (63, 64)), repeat=(0, 20, 69))
    Scs = dense(oracle, Qs, Vs, off)
    w = (0.7, 0.3)
    check(vfr, Scs, Qs, Vs, counts, off, w, (16, 448), what="ties")
    F = fused_scores(Scs, counts, w)
    mo = moment_offsets(counts)
    assert np.array_equal(F[:, mo[5]:mo[6]], F[:, mo[6]:mo[7]]) and np.array_equal(F[:, mo[63]:mo[64]], F[:, mo[64]:mo[65]])
    assert np.all(F[:, mo[20]:mo[20] + counts[20]] == F[:, mo[20]:mo[20] + 1])               # equal clips: equal single-clip scores


@pytest.mark.parametrize("nq", [0, 1, 65])
def test_query_counts_and_padding(vfr, oracle, nq):
    """k larger than the number of moments and of videos (padding), Nq in {0, 1, 65}."""
    Qs, Vs, counts, off = streams([3, 1, 2, 4], seed=nq, nq=nq)
    Scs = dense(oracle, Qs, Vs, off) if nq else [np.zeros((0, 20), np.float32)] * 2
    check(vfr, Scs, Qs, Vs, counts, off, (0.7, 0.3), (0, 16, 448), what=f"Nq = {nq}")
    banks = banks_of(vfr, Vs, off)
    d, i, _ = run(vfr, Qs, banks, (0.7, 0.3), 448, "moments")
    assert d.shape == (nq, 448) and np.all(i[:, 20:] == -1) and np.all(np.isinf(d[:, 20:])) and np.all(i[:, :20] >= 0)
    d, i, _ = run(vfr, Qs, banks, (0.7, 0.3), 16, "videos")
    assert np.all(i[:, 4:] == -1) and np.all(np.isinf(d[:, 4:])) and np.all(i[:, :4] >= 0)


def test_empty_bank(vfr):
    Qs = [np.random.RandomState(1).randn(11, D).astype(np.float32) for D in (100, 37)]
    off_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    banks = [vfr.VideoBank(torch.zeros((0, D), dtype=torch.float32, device=DEV), off_t, 4) for D in (100, 37)]
    rk = np.stack([np.full(11, (0x3F800000 << 32) | 7, np.uint64)] * 2)
    for level in LEVELS:
        d, i, c = run(vfr, Qs, banks, (0.7, 0.3), 16, level, rk)
        assert np.all(np.isinf(d)) and np.all(i == -1) and np.all(c == 0)


# the plan of csrc/fusion.hip at 70 queries x 1 100 videos, k = 100: ceil(4096 / 70) = 59 chunks wanted, 18 blocks of 64 videos
# there are -> 18 chunks of 64 videos (the last holds 12), a list of 256 slots that is cut back to k once more than 192 are in use
CUT_NQ, CUT_NV, CUT_K, CUT_PER, CUT_SLOTS = 70, 1100, 100, 64, 256


def test_in_loop_cut_and_chunk_merge(vfr, oracle):
    """A wave's list fills and is cut back to k several times (a block of 64 videos emits thousands of keys into 256 slots), and
    the per-query select merges 18 chunk lists.  That the running threshold is really at work is asserted on the REFERENCE: in the
    last chunk, the threshold a wave holds after its first cut (the k-th smallest of the keys emitted up to then, in the kernel's
    order: start clip, then end clip, all lanes of a step together) still has at least k of the chunk's keys below it."""
    counts = mixed_counts(CUT_NV, 77)
    counts[-12:] = np.maximum(counts[-12:], 12)                 # the last chunk alone emits well over k keys
    Qs, Vs, counts, off = streams(counts, seed=77, nq=CUT_NQ)
    Scs = dense(oracle, Qs, Vs, off)
    w = (0.7, 0.3)
    K = level_keys(fused_scores(Scs, counts, w), counts, "moments")
    mo = moment_offsets(counts)
    v0 = (CUT_NV - 1) // CUT_PER * CUT_PER
    assert CUT_NV // CUT_PER + 1 > 1 and CUT_NV - v0 <= 64
    nmax = int(counts[v0:].max())
    seen, first = [], None
    for s in range(nmax):
        for e in range(s, nmax):
            seen += [mo[v] + all_moments(int(counts[v])).index((s, e)) for v in range(v0, CUT_NV) if e < counts[v]]
            if first is None and len(seen) > CUT_SLOTS - 64:
                first = list(seen)
    assert first is not None and len(first) >= CUT_K
    thr = np.sort(K[:, first], axis=1)[:, CUT_K - 1]
    below = (K[:, mo[v0]:mo[CUT_NV]] < thr[:, None]).sum(axis=1)
    assert np.all(below >= CUT_K), "the reference does not exercise the running threshold at this shape"
    check(vfr, Scs, Qs, Vs, counts, off, w, (CUT_K,), what="in-loop cut")


# the plan at 1 100 queries x 1 100 videos: ceil(4096 / 1100) = 4 chunks wanted of the 18 blocks of 64 videos -> 4 chunks of
# 5 blocks = 320 videos (the last holds 140); k = 100: a list of 256 slots, cut back to k once more than 192 are in use
LONG_NQ, LONG_NV, LONG_K, LONG_PER, LONG_CHUNKS, LONG_SLOTS = 1100, 1100, 100, 320, 4, 256


def test_chunks_of_several_blocks(vfr, oracle):
    """A wave walks FIVE blocks of 64 videos (the shape of the benchmark, where one wave streams the whole bank): the threshold is
    carried from block to block, the lanes' LDS columns of clip distances are reused, and at the video level -- one key per lane
    and block -- the list is cut only because a chunk holds more than 192 videos.  Short videos (1..6 clips, widths 100 and 37)
    keep the dense reference small.  On the REFERENCE: the workspace is that of 4 chunks, and in chunk 0 the video-level threshold
    after the first cut (the k-th smallest best key of the first 256 videos) both lets videos of the fifth block through and
    keeps others out."""
    rs = np.random.RandomState(88)
    counts = rs.randint(1, 7, LONG_NV).astype(np.int64)
    counts[[0, 319, 320, -1]] = 6
    Qs, Vs, counts, off = streams(counts, (100, 37), seed=88, nq=LONG_NQ)
    assert vfr.lib().vfr_score_fusion_workspace_bytes(LONG_NQ, LONG_NV, LONG_K) == LONG_CHUNKS * LONG_NQ * LONG_K * 8 + 256
    assert -(-LONG_NV // LONG_PER) == LONG_CHUNKS and LONG_PER > LONG_SLOTS - 64
    Scs = dense(oracle, Qs, Vs, off)
    w = (0.7, 0.3)
    B = level_keys(fused_scores(Scs, counts, w), counts, "videos")
    thr = np.sort(B[:, :LONG_SLOTS], axis=1)[:, LONG_K - 1]
    late = B[:, LONG_SLOTS:LONG_PER] < thr[:, None]
    assert late.any() and not late.all(), "the reference does not exercise the carried threshold at this shape"
    check(vfr, Scs, Qs, Vs, counts, off, w, (LONG_K,), what="chunks of several blocks")


def test_own_rows_feed_the_rank_keys(vfr, oracle):
    """score_fusion_own for own videos first, last and at both sides of a chunk edge; its rows go through gt_rank_keys into
    score_fusion and reproduce the ranks of the reference's dense argsort."""
    counts = mixed_counts(130, 31)
    counts[[63, 64]] = (15, 9)
    Qs, Vs, counts, off = streams(counts, seed=31)
    Scs = dense(oracle, Qs, Vs, off)
    w = (0.7, 0.3)
    nq = len(Qs[0])
    own = np.asarray([0, 129, 63, 64, 1, 128, 62, 65, 17, 99, 64], np.int64)[:nq]
    banks = banks_of(vfr, Vs, off, 6)
    Qd = [dev(Q) for Q in Qs]
    rows = vfr.score_fusion_own(Qd, banks, w, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    want = own_rows(Scs, counts, w, own)
    assert np.array_equal(rows.cpu().numpy(), want)
    rs = np.random.RandomState(32)
    labels = np.zeros((2, nq, want.shape[1]), bool)
    for q in range(nq):
        M = int(counts[own[q]] * (counts[own[q]] + 1) // 2)
        labels[0, q, rs.randint(0, M, 3)] = True
        labels[1, q, rs.randint(0, M)] = True
    mo = moment_offsets(counts)
    _keys, rd, ri, cnt0, missing = vfr.gt_rank_keys(rows, dev(labels), dev(6 + mo[own]), dev(np.arange(nq, dtype=np.int64)), nq)
    _, _, cnt = vfr.score_fusion(Qd, banks, w, 0, "moments", rd, ri, count_lt=cnt0)
    torch.cuda.synchronize()
    assert int(missing.item()) == 0
    F = fused_scores(Scs, counts, w)
    for q in range(nq):
        order = np.argsort(F[q], kind="stable")                              # the dense (score, id) order
        where = np.empty_like(order)
        where[order] = np.arange(len(order))
        for r in range(2):
            assert int(cnt[r, q]) == int(where[mo[own[q]] + np.nonzero(labels[r, q])[0]].min()), (r, q)


def test_id_base_and_two_shards(vfr, oracle):
    """id_base > 0, and the bank sliced into two shards whose merged lists and summed counts equal the unsharded call."""
    Qs, Vs, counts, off = streams(mixed_counts(130, 51), (100, 37), seed=51)
    Scs = dense(oracle, Qs, Vs, off)
    w = (0.7, 0.3)
    check(vfr, Scs, Qs, Vs, counts, off, w, (16,), id_base=1000, what="id_base")
    banks = banks_of(vfr, Vs, off, 1000)
    Qd = [dev(Q) for Q in Qs]
    cut = 70
    parts = [[vfr.slice_bank(b, counts, a, z) for b in banks] for a, z in ((0, cut), (cut, 130))]
    for level in LEVELS:
        rk = rank_keys(Scs, counts, w, level, 1000)
        rd, ri = (dev(x) for x in split_keys(rk))
        wd, wi, wc = vfr.score_fusion(Qd, banks, w, 16, level, rd, ri)
        cnt, lists = None, []
        for sub in parts:
            d, i, cnt = vfr.score_fusion(Qd, sub, w, 16, level, rd, ri, count_lt=cnt)
            lists.append((d, i))
        md, mi = vfr.topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]))
        torch.cuda.synchronize()
        assert torch.equal(md, wd) and torch.equal(mi, wi) and torch.equal(cnt, wc), level


def test_evaluate_fusion_gpu_equals_cpu():
    """Two differently seeded models, weights (0.6, 0.4): the metric dicts and the top-10 ids of cuda:0 equal the CPU device's."""
    from vfr_amd import evaluate as vevaluate
    ps = [problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=123)]
    ps.append(dict(ps[0], sd=problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=321)["sd"]))
    res = {}
    for device in ("cpu", DEV):
        for level in LEVELS:
            dss = [MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"]) for p in ps]
            models = [make_model(p["sd"], feat_dim=64, hidden=16).to(device) for p in ps]
            its = [d.iterators() for d in dss]
            out, (d, i, v) = vevaluate.evaluate_fusion(models, [x[0] for x in its], [x[1] for x in its], dss[0].annotations, device,
                                                       (0.6, 0.4), level=level, return_topk=10)
            res[(device, level)] = (out, None, i.cpu().numpy(), v.cpu().numpy())
    for level in LEVELS:
        a, b = res[("cpu", level)], res[(DEV, level)]
        assert a[0] == b[0], level
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), level
