"""Prior-aware retrieval on the GPU (vfr_score_prior_f32, vfr_score_prior_own_f32, engine.corpus_prior_topk,
evaluate.evaluate_prior) against the numpy statement of tests/prior_reference.py on the oracle's dense moment scores, bit for bit in
distances, ids and counts; the zero-table identity against the device's own plain entry points."""
import numpy as np
import pytest
import torch

from fusion_reference import all_moments, moment_offsets, split_keys
from helpers import MemoryDataset, make_model, problem
from prior_reference import biased_scores, own_rows, rank_keys, span_mask, statement, table_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ("moments", "videos")


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


def case(counts, D=100, seed=0, nq=11, same=()):
    """Random clip rows and queries; ``same`` = pairs of equally long videos given identical rows (tied scores)."""
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    for a, b in same:
        assert counts[a] == counts[b]
        V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, off.astype(np.int32)


def mixed_counts(nv, seed):
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = 21
    c[-1] = 21
    return c


def random_values(max_clips, seed, excluded=0.2):
    """Biases drawn from multiples of 2^-4 (ties across moments and videos occur), a share of the entries excluded."""
    rs = np.random.RandomState(seed)
    v = (rs.randint(0, 8, int(table_offsets(max_clips)[-1])) / 16.0).astype(np.float32)
    v[rs.rand(len(v)) < excluded] = np.inf
    return v


def table_of(values, max_clips):
    """The device table of raw entries (no host-side validation: the bad-flag test plants a NaN)."""
    from vfr_amd import engine
    values = np.ascontiguousarray(values, np.float32)
    return engine.MomentTable(max_clips, values, dev(table_offsets(max_clips).astype(np.int32)), dev(values))


def run(vfr, Q, bank, table, k, level, rk=None, count_lt=None, bad=None):
    rd = ri = None
    if rk is not None:
        rd, ri = (dev(x) for x in split_keys(rk))
    d, i, c = vfr.score_prior(dev(Q), bank, table, k, level, rd, ri, count_lt=count_lt, bad=bad)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d, i, c))


def check(vfr, Sc, Q, V, counts, off, values, max_clips, ks, levels=LEVELS, id_base=0, what=""):
    bank = vfr.VideoBank(dev(V), dev(off), id_base)
    table = table_of(values, max_clips)
    for level in levels:
        rk = rank_keys(Sc, counts, values, level, id_base)
        for k in ks:
            d, i, c = run(vfr, Q, bank, table, k, level, rk)
            wd, wi, wc = statement(Sc, counts, values, k, level, id_base, rk)
            if k:
                assert np.array_equal(i, wi), f"{what}: ids differ ({level}, k = {k})"
                assert np.array_equal(d, wd), f"{what}: distances differ ({level}, k = {k})"
            assert np.array_equal(c, wc), f"{what}: counts differ ({level}, k = {k})"


@pytest.mark.parametrize("nv", [1, 2, 63, 64, 65, 130])
def test_chunk_edges(vfr, oracle, nv):
    """Banks that end before, on and after a chunk of 64 videos; clip counts mixed 1..21 with 21 first and last; a random table.
    Nv = 130 also takes k on both sides of the list capacities (128 | 256 slots at k = 64 | 65, 256 | 512 at k = 192 | 193): a block
    of 64 videos emits over a thousand keys, so the list fills and is cut back at every capacity."""
    Q, V, counts, off = case(mixed_counts(nv, nv), seed=nv)
    ks = (0, 1, 16, 448) + ((64, 65, 192, 193) if nv == 130 else ())
    check(vfr, oracle.score_moments(Q, V, off), Q, V, counts, off, random_values(21, 100 + nv), 21, ks, what=f"Nv = {nv}")


@pytest.fixture(scope="module")
def bank65(oracle):
    """65 videos, two of them identical (videos 5, 6 and 63, 64), and their dense scores: shared by the table cases."""
    counts = mixed_counts(65, 12)
    counts[[5, 6, 63, 64]] = (8, 8, 13, 13)
    Q, V, counts, off = case(counts, seed=12, same=((5, 6), (63, 64)))
    Sc = oracle.score_moments(Q, V, off)
    Sc.setflags(write=False)
    return Q, V, counts, off, Sc


def test_zero_table_is_the_plain_retrieval(vfr, bank65):
    """Zeros: the reference, and the device's own score_topk / score_video_topk (exact kernels), bit for bit."""
    Q, V, counts, off, Sc = bank65
    values = np.zeros(int(table_offsets(21)[-1]), np.float32)
    check(vfr, Sc, Q, V, counts, off, values, 21, (1, 16, 448), id_base=9, what="zeros")
    bank = vfr.VideoBank(dev(V), dev(off), 9)
    table = table_of(values, 21)
    Qd = dev(Q)
    for level in LEVELS:
        rk = rank_keys(Sc, counts, values, level, 9)
        rd, ri = (dev(x) for x in split_keys(rk))
        for k in (1, 16, 448):
            if level == "moments":
                wd, wi, wc = vfr.score_topk(Qd, bank, k, rd, ri, mode="exact")
            else:
                wd, wi, wc0 = vfr.score_video_topk(Qd, bank, k, rd[0].contiguous(), ri[0].contiguous(), mode="exact")
                _, _, wc1 = vfr.score_video_topk(Qd, bank, 0, rd[1].contiguous(), ri[1].contiguous(), mode="exact")
                wc = torch.stack([wc0, wc1])
            torch.cuda.synchronize()
            d, i, c = run(vfr, Q, bank, table, k, level, rk)
            assert np.array_equal(i, wi.cpu().numpy()) and np.array_equal(d, wd.cpu().numpy()), (level, k)
            assert np.array_equal(c, wc.cpu().numpy()), (level, k)


def test_random_biases_with_ties(vfr, bank65):
    """Biases from multiples of 2^-4 and two pairs of identical videos: equal biased scores inside and across videos, broken by id."""
    Q, V, counts, off, Sc = bank65
    values = random_values(21, 13, excluded=0.1)
    G = biased_scores(Sc, counts, values)
    mo = moment_offsets(counts)
    assert np.array_equal(G[:, mo[5]:mo[6]], G[:, mo[6]:mo[7]]) and np.array_equal(G[:, mo[63]:mo[64]], G[:, mo[64]:mo[65]])
    check(vfr, Sc, Q, V, counts, off, values, 21, (16, 448), what="random biases")


def test_lengths_mask(vfr, bank65):
    from vfr_amd import engine
    Q, V, counts, off, Sc = bank65
    t = engine.moment_table(21, lengths=(1, 2))
    assert np.array_equal(t.values, span_mask(21, lambda n, s, e: e - s + 1 <= 2))
    check(vfr, Sc, Q, V, counts, off, t.values, 21, (0, 16, 448), what="lengths = (1, 2)")
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    _, i, _ = run(vfr, Q, bank, t.on(DEV), 448, "moments")
    mo = moment_offsets(counts)
    vids = np.searchsorted(mo, i, side="right") - 1
    for j, v in zip((i - mo[vids]).ravel(), vids.ravel()):                    # every listed moment is one or two clips long
        s, e = all_moments(int(counts[v]))[int(j)]
        assert e - s + 1 <= 2


def test_one_clip_count_excluded(vfr, bank65):
    """Every moment of 21-clip videos excluded: they never appear, and the video list is padded when k > ranked videos."""
    Q, V, counts, off, Sc = bank65
    values = random_values(21, 14, excluded=0.0)
    to = table_offsets(21)
    values[to[21]:to[22]] = np.inf
    check(vfr, Sc, Q, V, counts, off, values, 21, (16, 448), what="one clip count excluded")
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    ranked = int((counts != 21).sum())
    assert 0 < ranked < 65
    for level in LEVELS:
        d, i, _ = run(vfr, Q, bank, table_of(values, 21), 448, level)
        vids = np.searchsorted(moment_offsets(counts), i[i >= 0], side="right") - 1
        assert not np.isin(vids, np.nonzero(counts == 21)[0]).any(), level
    assert np.all(i[:, :ranked] >= 0) and np.all(i[:, ranked:] == -1) and np.all(np.isinf(d[:, ranked:])) and np.all(np.isfinite(d[:, :ranked]))


def test_everything_excluded(vfr, bank65):
    """All padding, and the counts stay what they were."""
    Q, V, counts, off, Sc = bank65
    values = np.full(int(table_offsets(21)[-1]), np.inf, np.float32)
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    rk = np.stack([np.full(len(Q), np.uint64(0x7F800000FFFFFFFF)), np.full(len(Q), np.uint64((0x41000000 << 32) | 7))])
    for level in LEVELS:
        before = torch.full((2, len(Q)), 5, dtype=torch.int64, device=DEV)
        d, i, c = run(vfr, Q, bank, table_of(values, 21), 16, level, rk, count_lt=before)
        assert np.all(np.isinf(d)) and np.all(i == -1) and np.all(c == 5), level
        wd, wi, wc = statement(Sc, counts, values, 16, level, 0, rk)
        assert np.array_equal(d, wd) and np.array_equal(i, wi) and not wc.any()
    # the rank key (+inf, -1) counts every candidate: with zeros, all moments / all videos
    zeros = np.zeros_like(values)
    _, _, c = run(vfr, Q, bank, table_of(zeros, 21), 0, "moments", rk)
    assert np.all(c[0] == int(moment_offsets(counts)[-1]))
    _, _, c = run(vfr, Q, bank, table_of(zeros, 21), 0, "videos", rk)
    assert np.all(c[0] == 65)


def test_long_videos(vfr, oracle):
    """One 64-clip video beside 1-clip videos, max_clips = 64: stride-4 windows of lengths (4, 8, 16), and a full random table."""
    from vfr_amd import engine
    counts = np.ones(70, np.int64)
    counts[3] = 64
    Q, V, counts, off = case(counts, seed=9)
    Sc = oracle.score_moments(Q, V, off)
    t = engine.moment_table(64, lengths=(4, 8, 16), stride=4)
    assert np.array_equal(t.values, span_mask(64, lambda n, s, e: e - s + 1 in (4, 8, 16) and s % 4 == 0))
    assert int(t.enabled(64).sum()) == 16 + 15 + 13 and not t.enabled(1).any()
    check(vfr, Sc, Q, V, counts, off, t.values, 64, (0, 16, 448), what="sliding windows")
    check(vfr, Sc, Q, V, counts, off, random_values(64, 15), 64, (1, 448), what="long videos, random table")


@pytest.mark.parametrize("D", [100, 37, 4])
def test_widths(vfr, oracle, D):
    """The fast path (D = 100, aligned rows), the generic path and the smallest width a 16-byte row has."""
    Q, V, counts, off = case(mixed_counts(70, 40 + D), D, seed=40 + D)
    check(vfr, oracle.score_moments(Q, V, off), Q, V, counts, off, random_values(21, D), 21, (1, 16), what=f"D = {D}")


def test_unaligned_rows_take_the_generic_path(vfr, oracle):
    """D = 100 with a bank that starts 4 bytes past a 16-byte boundary: no 16-byte loads, the same bits."""
    Q, V, counts, off = case(mixed_counts(20, 5), seed=5)
    Sc = oracle.score_moments(Q, V, off)
    values = random_values(21, 6)
    pad = torch.zeros(V.size + 1, dtype=torch.float32, device=DEV)
    pad[1:] = dev(V).reshape(-1)
    bank = vfr.VideoBank(pad[1:].view(V.shape), dev(off), 0)
    assert bank.emb.data_ptr() % 16 == 4
    rk = rank_keys(Sc, counts, values, "moments")
    d, i, c = run(vfr, Q, bank, table_of(values, 21), 16, "moments", rk)
    wd, wi, wc = statement(Sc, counts, values, 16, "moments", 0, rk)
    assert np.array_equal(d, wd) and np.array_equal(i, wi) and np.array_equal(c, wc)


def test_empty_shapes(vfr):
    """Nq = 0 and Nv = 0: VFR_OK; nothing to write without queries, padding and untouched counts without videos."""
    values = np.zeros(int(table_offsets(21)[-1]), np.float32)
    table = table_of(values, 21)
    Q, V, counts, off = case([3, 1, 2, 4], seed=1, nq=0)
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    empty = vfr.VideoBank(torch.zeros((0, 100), dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 4)
    for level in LEVELS:
        for b in (bank, empty):
            d, i, c = run(vfr, Q, b, table, 16, level)
            assert d.shape == (0, 16) and i.shape == (0, 16) and c is None
        Q11 = np.random.RandomState(1).randn(11, 100).astype(np.float32)
        rk = np.stack([np.full(11, (0x3F800000 << 32) | 7, np.uint64)] * 2)
        before = torch.full((2, 11), 3, dtype=torch.int64, device=DEV)
        d, i, c = run(vfr, Q11, empty, table, 16, level, rk, count_lt=before)
        assert np.all(np.isinf(d)) and np.all(i == -1) and np.all(c == 3)
        _, _, c = run(vfr, Q11, empty, table, 0, level, rk, count_lt=before)
        assert np.all(c == 3)
    rows = vfr.score_prior_own(dev(Q), bank, table, torch.zeros(0, dtype=torch.int32, device=DEV))
    assert rows.shape == (0, 10)


def test_own_path(vfr, oracle):
    """score_prior_own equals the reference rows (own videos first, last, at both sides of a chunk edge, outside [0, Nv): all +inf);
    its rows go through gt_rank_keys into score_prior and reproduce the ranks of the reference's dense order."""
    counts = mixed_counts(130, 31)
    counts[[63, 64]] = (15, 9)
    Q, V, counts, off = case(counts, seed=31)
    Sc = oracle.score_moments(Q, V, off)
    values = random_values(21, 32)
    table = table_of(values, 21)
    own = np.asarray([0, 129, 63, 64, 1, 128, 62, 65, 17, -1, 130], np.int64)
    bank = vfr.VideoBank(dev(V), dev(off), 6)
    rows = vfr.score_prior_own(dev(Q), bank, table, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    want = own_rows(Sc, counts, values, own)
    assert np.array_equal(rows.cpu().numpy(), want) and np.all(np.isinf(want[9:]))
    Q37, V37, _, _ = case(counts, 37, seed=33)
    rows = vfr.score_prior_own(dev(Q37), vfr.VideoBank(dev(V37), dev(off), 6), table, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), own_rows(oracle.score_moments(Q37, V37, off), counts, values, own))
    # ranks: positives drawn among the CANDIDATES of the first nine queries' own videos
    own9, nq9 = own[:9], 9
    rs = np.random.RandomState(34)
    G = biased_scores(Sc, counts, values)
    mo = moment_offsets(counts)
    labels = np.zeros((2, nq9, want.shape[1]), bool)
    for q in range(nq9):
        cand = np.nonzero(np.isfinite(G[q, mo[own9[q]]:mo[own9[q] + 1]]))[0]
        labels[0, q, rs.choice(cand, min(3, len(cand)), replace=False)] = True
        labels[1, q, rs.choice(cand)] = True
    Q9 = dev(Q[:nq9])
    rows9 = vfr.score_prior_own(Q9, bank, table, dev(own9.astype(np.int32)))
    _keys, rd, ri, cnt0, missing = vfr.gt_rank_keys(rows9, dev(labels), dev(6 + mo[own9]), dev(np.arange(nq9, dtype=np.int64)), nq9)
    _, _, cnt = vfr.score_prior(Q9, bank, table, 0, "moments", rd, ri, count_lt=cnt0)
    torch.cuda.synchronize()
    assert int(missing.item()) == 0
    for q in range(nq9):
        order = np.argsort(G[q], kind="stable")                              # the dense (biased score, id) order; +inf last
        where = np.empty_like(order)
        where[order] = np.arange(len(order))
        for r in range(2):
            assert int(cnt[r, q]) == int(where[mo[own9[q]] + np.nonzero(labels[r, q])[0]].min()), (r, q)


def test_bad_flag(vfr, oracle):
    """A NaN and a negative entry set the flag and exclude their moments; every other moment is what the clean table gives."""
    counts = mixed_counts(65, 21)
    counts[10] = 8
    Q, V, counts, off = case(counts, seed=21)
    Sc = oracle.score_moments(Q, V, off)
    clean = random_values(21, 22, excluded=0.0)
    to = table_offsets(21)
    broken = clean.copy()
    broken[to[21] + 7] = np.nan
    broken[to[8] + 2] = -0.5
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    for level in LEVELS:
        rk = rank_keys(Sc, counts, broken, level)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        d, i, c = run(vfr, Q, bank, table_of(broken, 21), 448, level, rk, bad=bad)
        assert int(bad.item()) == 1, level
        wd, wi, wc = statement(Sc, counts, broken, 448, level, 0, rk)       # the reference treats both entries as excluded
        assert np.array_equal(d, wd) and np.array_equal(i, wi) and np.array_equal(c, wc), level
        bad.zero_()
        run(vfr, Q, bank, table_of(clean, 21), 16, level, rk, bad=bad)
        assert int(bad.item()) == 0, level
    excluded = clean.copy()
    excluded[[to[21] + 7, to[8] + 2]] = np.inf
    assert np.array_equal(biased_scores(Sc, counts, broken), biased_scores(Sc, counts, excluded))       # neighbours are unaffected
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    own = np.asarray([0, 64, 10, 1, 2, 3, 4, 5, 6, 7, 8], np.int64)          # the 21-clip and the 8-clip videos among them
    rows = vfr.score_prior_own(dev(Q), bank, table_of(broken, 21), dev(own.astype(np.int32)), bad=bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 1 and np.array_equal(rows.cpu().numpy(), own_rows(Sc, counts, broken, own))


def test_id_base_and_two_shards(vfr, oracle):
    """id_base > 0, and the bank sliced into two shards whose merged lists and chained counts equal the unsharded call."""
    Q, V, counts, off = case(mixed_counts(130, 51), 37, seed=51)
    Sc = oracle.score_moments(Q, V, off)
    values = random_values(21, 52)
    check(vfr, Sc, Q, V, counts, off, values, 21, (16,), id_base=1000, what="id_base")
    bank = vfr.VideoBank(dev(V), dev(off), 1000)
    table = table_of(values, 21)
    Qd = dev(Q)
    parts = [vfr.slice_bank(bank, counts, a, z) for a, z in ((0, 70), (70, 130))]
    for level in LEVELS:
        rk = rank_keys(Sc, counts, values, level, 1000)
        rd, ri = (dev(x) for x in split_keys(rk))
        wd, wi, wc = vfr.score_prior(Qd, bank, table, 16, level, rd, ri)
        cnt, lists = None, []
        for sub in parts:
            d, i, cnt = vfr.score_prior(Qd, sub, table, 16, level, rd, ri, count_lt=cnt)
            lists.append((d, i))
        md, mi = vfr.topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]))
        torch.cuda.synchronize()
        assert torch.equal(md, wd) and torch.equal(mi, wi) and torch.equal(cnt, wc), level


def test_evaluate_prior_gpu_equals_cpu():
    """A training-frequency prior with a length limit: the metric dicts, the unreachable shares and the top-10 ids of cuda:0 equal
    the CPU device's."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    p = problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=123)
    nmax = int(p["counts"].max())
    prior = engine.prior_table(p["times"], p["counts"][p["own"]], lam=0.25, alpha=0.5, max_clips=nmax)
    mask = engine.moment_table(nmax, max_len=3)
    table = engine.moment_table(nmax, bias={n: prior.row(n) for n in range(nmax + 1)}, max_len=3)
    assert np.array_equal(np.isinf(table.values), np.isinf(mask.values)) and table.values[np.isfinite(table.values)].any()
    res = {}
    for device in ("cpu", DEV):
        for level in LEVELS:
            ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
            model = make_model(p["sd"], feat_dim=64, hidden=16).to(device)
            out, (d, i, v) = vevaluate.evaluate_prior(model, *ds.iterators(), ds.annotations, device, table, level=level, k=10)
            res[(device, level)] = (out, i.cpu().numpy(), v.cpu().numpy())
    for level in LEVELS:
        a, b = res[("cpu", level)], res[(DEV, level)]
        assert a[0] == b[0], level
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), level
