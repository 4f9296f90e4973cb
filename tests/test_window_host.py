"""Windowed retrieval without a GPU: the CPU provider against the numpy statement of tests/window_reference.py on the oracle's dense
moment scores (lists, rank counts, span keys), window_positives against its brute force and against gt_label_table, decode_moments
on every id of a bank with long videos, corpus_window_topk against corpus_ranks / corpus_topk, evaluate_windowed against evaluate,
and a bank sliced in two."""
import numpy as np
import pytest
import torch

from fusion_reference import moment_offsets, split_keys
from helpers import MemoryDataset, make_model, problem
from window_reference import KEY_EMPTY, bank_spans, positives_brute, rank_keys, span_keys, spans_of, statement

LENGTHS = (1, 2, 7, 64)


def _case(seed, counts, nq=5, D=37, same=()):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    for a, b in same:
        V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, off.astype(np.int32)


def _signed(keys):
    return torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64).copy())


@pytest.fixture(scope="module")
def mixed(oracle):
    """Empty, one-clip, tile-sized and long videos, two identical pairs (exact ties across videos), and the dense scores."""
    Q, V, counts, off = _case(1, [5, 0, 1, 63, 64, 65, 2, 129, 5, 2, 7], same=((0, 8), (6, 9)))
    Sc = oracle.score_moments(Q, V, off)
    Sc.setflags(write=False)
    return Q, V, counts, off, Sc


def test_spans_table_is_generate_moments_order():
    from vfr_amd.utils import generate_moments
    for n in (0, 1, 2, 7, 21):
        assert spans_of(n).tolist() == [list(m) for m in generate_moments(n)]


def test_cpu_score_window_matches_reference(mixed):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off, Sc = mixed
    id_base = 11
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)
    Qt = torch.from_numpy(Q)
    for L in LENGTHS:
        rk = rank_keys(Sc, counts, L, id_base)
        rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
        for k in (0, 1, 100, 448):
            d, i, c = ops.score_window(Qt, bank, L, k, rd, ri)
            wd, wi, wc = statement(Sc, counts, L, k, id_base, rk)
            if k:
                assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd), (L, k)
            else:
                assert d is None and i is None
            assert np.array_equal(c.numpy(), wc), (L, k)
        before = torch.full((4, len(Q)), 3, dtype=torch.int64)
        _, _, c = ops.score_window(Qt, bank, L, 0, rd, ri, count_lt=before)
        assert np.array_equal(c.numpy(), statement(Sc, counts, L, 0, id_base, rk)[2] + 3), L
    d, i, c = ops.score_window(Qt, bank, 3, 5)
    assert c is None and d.shape == (len(Q), 5)
    for bad_len in (0, 65):
        with pytest.raises(ValueError):
            ops.score_window(Qt, bank, bad_len, 5)


def test_cpu_score_window_long_video(oracle):
    """A 300-clip video between short ones: nothing in the provider is sized by its 45 150 moments."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off = _case(2, [3, 300, 4], nq=3, D=12)
    Sc = oracle.score_moments(Q, V, off)
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), 0)
    for L in (1, 16, 64):
        rk = rank_keys(Sc, counts, L)
        rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
        d, i, c = ops.score_window(torch.from_numpy(Q), bank, L, 100, rd, ri)
        wd, wi, wc = statement(Sc, counts, L, 100, 0, rk)
        assert np.array_equal(i.numpy(), wi) and np.array_equal(d.numpy(), wd) and np.array_equal(c.numpy(), wc), L


def test_cpu_span_keys_match_reference(mixed):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off, Sc = mixed
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), 9)
    good = [(0, 3, 0, 62), (1, 7, 60, 123), (2, 7, 65, 128), (4, 2, 0, 0), (4, 2, 0, 0), (3, 0, 1, 3), (0, 10, 6, 6), (1, 5, 1, 64)]
    other = [(0, 11, 0, 0), (1, 40, 2, 3), (2, -1, 0, 0)]                             # videos outside the bank: untouched, not bad
    items = np.asarray(good + other, np.int32)
    out = ops.window_span_keys(torch.from_numpy(Q), bank, torch.from_numpy(items))
    want, bad = span_keys(Sc, counts, items, 9)
    assert bad == 0 and np.array_equal(out.numpy().view(np.uint64), want)
    assert (want[:len(good)] != KEY_EMPTY).all() and (want[len(good):] == KEY_EMPTY).all()
    for wrong in [(5, 3, 0, 1), (-1, 3, 0, 1), (0, 3, -1, 1), (0, 3, 4, 3), (0, 3, 0, 63), (0, 7, 0, 64), (0, 1, 0, 0)]:
        mixed_items = np.asarray(good[:2] + [wrong] + good[2:4], np.int32)
        flag = torch.zeros(1, dtype=torch.int32)
        out = ops.window_span_keys(torch.from_numpy(Q), bank, torch.from_numpy(mixed_items), bad=flag)
        want, bad = span_keys(Sc, counts, mixed_items, 9)
        assert bad == 1 and int(flag) == 1 and want[2] == KEY_EMPTY, wrong
        assert np.array_equal(out.numpy().view(np.uint64), want), wrong
    # a shard that starts at corpus video 100
    out = ops.window_span_keys(torch.from_numpy(Q), bank, torch.from_numpy(np.asarray([(0, 103, 0, 5), (0, 3, 0, 5)], np.int32)), vid_base=100)
    want, _ = span_keys(Sc, counts, [(0, 103, 0, 5), (0, 3, 0, 5)], 9, vid_base=100)
    assert np.array_equal(out.numpy().view(np.uint64), want) and want[0] != KEY_EMPTY and want[1] == KEY_EMPTY


def test_window_positives_against_brute_force():
    from vfr_amd import engine
    rs = np.random.RandomState(3)
    counts_own = np.asarray([6, 5, 21, 1, 30, 6, 21, 70], np.int64)
    times = []
    for n in counts_own:
        spans = []
        for _ in range(int(rs.randint(2, 5))):
            s = int(rs.randint(0, n))
            spans.append([s, int(rs.randint(s, min(n, s + 12)))])
        spans.append(list(spans[0]))
        times.append(spans)
    thresholds = (0.3, 0.5, 0.7)
    for L, strict, agree in ((1, True, 2), (3, True, 2), (64, True, 2), (8, False, 2), (8, True, 1), (8, True, 3)):
        got = engine.window_positives(times, counts_own, thresholds, L, strict=strict, agree=agree)
        want = positives_brute(times, counts_own, thresholds, L, strict=strict, agree=agree)
        assert len(got) == len(thresholds)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), (L, strict, agree)
    for bad_len in (0, 65):
        with pytest.raises(ValueError):
            engine.window_positives(times, counts_own, thresholds, bad_len)


def test_window_positives_select_the_label_table():
    """n <= 21 and L >= n: exactly the moments gt_label_table labels 1."""
    from vfr_amd import engine
    from vfr_amd.utils import moment_index
    p = problem(30, 40, 21, feat_dim=8, hidden=4, seed=5)
    p2 = problem(30, 40, "didemo", feat_dim=8, hidden=4, seed=6)
    for prob in (p, p2):
        n_own = np.asarray(prob["counts"], np.int64)[prob["own"]]
        for strict in (True, False):
            labels = engine.gt_label_table(prob["times"], n_own, [0.5, 0.7], strict)
            pos = engine.window_positives(prob["times"], n_own, [0.5, 0.7], 21, strict=strict)
            for r in range(2):
                sel = np.zeros_like(labels[r])
                for q, s, e in pos[r].tolist():
                    assert not sel[q, moment_index(int(n_own[q]), s, e)]
                    sel[q, moment_index(int(n_own[q]), s, e)] = True
                assert np.array_equal(sel, labels[r]), (strict, r)


def test_decode_moments_round_trips_every_id():
    from vfr_amd import engine
    counts = np.asarray([0, 1, 64, 65, 0, 300, 1024, 3], np.int64)
    mom = moment_offsets(counts)
    shard = engine.CorpusShard(None, 0, len(counts), counts, mom, torch.device("cpu"))
    ids = torch.arange(int(mom[-1]), dtype=torch.int64)
    v, s, e = engine.decode_moments(shard, ids)
    want = bank_spans(counts)
    assert np.array_equal(torch.stack([v, s, e], 1).numpy(), want)
    v, s, e = engine.decode_moments(shard, torch.tensor([[-1, 0], [int(mom[-1]) - 1, -1]]))
    assert v.tolist() == [[-1, 1], [7, -1]] and s.tolist() == [[-1, 0], [1, -1]] and e.tolist() == [[-1, 0], [2, -1]]


def _window_problem(seed, nv=20, nq=15, clips="didemo", D=37):
    p = problem(nv, nq, clips, feat_dim=8, hidden=4, seed=seed)
    Q, V, counts, off = _case(seed, p["counts"], nq=nq, D=D)
    return p, Q, V, counts


def test_corpus_window_topk_equals_the_plain_corpus_pass():
    """L = 64 over a corpus of videos of up to 21 clips: the ranks of corpus_ranks and the lists of corpus_topk."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    for clips, seed in (("didemo", 7), (21, 8)):
        p, Q, V, counts = _window_problem(seed, clips=clips)
        shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
        Qt = torch.from_numpy(Q)
        n_own = counts[p["own"]]
        labels = engine.gt_label_table(p["times"], n_own, [0.5, 0.7], True)
        ranks, wd, wi = engine.corpus_ranks(shard, Qt, p["own"], labels, ops, k=100)
        td, ti = engine.corpus_topk(shard, Qt, 100, ops)
        pos = engine.window_positives(p["times"], n_own, [0.5, 0.7], 64)
        d, i, vid, r, unreach = engine.corpus_window_topk(shard, Qt, 64, 100, own_global=p["own"], positives=pos, ops=ops)
        assert torch.equal(r, ranks) and not bool(unreach.any())
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(d, td) and torch.equal(i, ti)
        v2, s2, e2 = engine.decode_moments(shard, i)
        assert torch.equal(v2, vid) and bool(((e2 - s2 + 1 <= 21) & (s2 >= 0)).all())
        d, i, vid, r, unreach = engine.corpus_window_topk(shard, Qt, 64, 0, own_global=p["own"], positives=pos, ops=ops)
        assert d is None and i is None and vid is None and torch.equal(r, ranks)
        d, i, vid, r, unreach = engine.corpus_window_topk(shard, Qt, 2, 10, ops=ops)
        assert r is None and unreach is None and bool((engine.decode_moments(shard, i)[2] - engine.decode_moments(shard, i)[1] <= 1).all())
    with pytest.raises(ValueError):
        engine.corpus_window_topk(shard, Qt, 65, 10, ops=ops)
    with pytest.raises(ValueError, match="inside"):
        engine.corpus_window_topk(shard, Qt, 4, 0, own_global=p["own"], positives=[np.asarray([[0, 0, 21]])], ops=ops)


def test_unreachable_queries_rank_behind_every_candidate():
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    p, Q, V, counts = _window_problem(9, clips=21)
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    n_own = counts[p["own"]]
    full = engine.window_positives(p["times"], n_own, [0.5], 64)[0]
    shortest = np.full(len(Q), 99)
    np.minimum.at(shortest, full[:, 0], full[:, 2] - full[:, 1] + 1)
    L = int(shortest.max()) - 1
    assert 1 <= L < 64
    pos = engine.window_positives(p["times"], n_own, [0.5], L)
    _, _, _, r, unreach = engine.corpus_window_topk(shard, torch.from_numpy(Q), L, 0, own_global=p["own"], positives=pos, ops=ops)
    assert np.array_equal(unreach[0].numpy(), shortest > L) and bool(unreach.any()) and not bool(unreach.all())
    candidates = int(sum(min(L, n - s) for n in counts.tolist() for s in range(n)))
    assert bool((r[0][unreach[0]] == candidates).all()) and bool((r[0][~unreach[0]] < candidates).all())
    # positives longer than the window are no candidates: passing the full set changes nothing
    _, _, _, r2, u2 = engine.corpus_window_topk(shard, torch.from_numpy(Q), L, 0, own_global=p["own"], positives=[full], ops=ops)
    assert torch.equal(r2, r) and torch.equal(u2, unreach)


def test_evaluate_windowed_equals_evaluate():
    from vfr_amd import evaluate as vevaluate
    from vfr_amd.dropin import evaluate as dropin_evaluate
    assert dropin_evaluate.evaluate_windowed is vevaluate.evaluate_windowed
    p = problem(12, 14, "didemo", feat_dim=64, hidden=16, seed=123)

    def run(fn, *args, **kw):
        ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        return fn(model, *ds.iterators(), ds.annotations, "cpu", *args, **kw)
    want = run(vevaluate.evaluate, preliminary=0)
    got = run(vevaluate.evaluate_windowed, 6)
    assert {k: v for k, v in got.items() if k != "unreachable"} == want
    assert got["unreachable"] == {"IoU=0.5": 0.0, "IoU=0.7": 0.0}
    assert run(vevaluate.evaluate_windowed, 64) == got
    from vfr_amd import engine
    n_own = np.asarray(p["counts"], np.int64)[p["own"]]
    full = engine.window_positives(p["times"], n_own, [0.5], 64)[0]
    shortest = np.full(len(n_own), 99)
    np.minimum.at(shortest, full[:, 0], full[:, 2] - full[:, 1] + 1)
    L = int(shortest.max()) - 1
    assert L >= 1
    short = run(vevaluate.evaluate_windowed, L)
    assert short["unreachable"]["IoU=0.5"] == pytest.approx(100.0 * float((shortest > L).mean())) and short["unreachable"]["IoU=0.5"] > 0
    # an empty query batch
    ds = MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"][:0], p["own"][:0], [])
    empty = vevaluate.evaluate_windowed(make_model(p["sd"], feat_dim=64, hidden=16), *ds.iterators(), ds.annotations, "cpu", 4)
    assert set(empty) == {"model, IoU=0.5", "model, IoU=0.7", "unreachable"}


def test_sliced_bank_reproduces_the_single_shard(mixed):
    """Two slices with id_base, chained counts, merged lists and MIN-reduced span keys equal the whole bank."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off, Sc = mixed
    id_base = 1000
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)
    Qt = torch.from_numpy(Q)
    cut = 7                                                                        # the 129-clip video opens the second slice
    parts = [ops.slice_bank(bank, counts, a, z) for a, z in ((0, cut), (cut, len(counts)))]
    assert parts[1].id_base == id_base + int(moment_offsets(counts)[cut])
    for L in (2, 64):
        rk = rank_keys(Sc, counts, L, id_base)
        rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
        wd, wi, wc = ops.score_window(Qt, bank, L, 100, rd, ri)
        cnt, lists = None, []
        for sub in parts:
            d, i, cnt = ops.score_window(Qt, sub, L, 100, rd, ri, count_lt=cnt)
            lists.append((d, i))
        md, mi = ops.topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]))
        assert torch.equal(md, wd) and torch.equal(mi, wi) and torch.equal(cnt, wc), L
    items = torch.from_numpy(np.asarray([(0, 3, 0, 62), (1, 7, 60, 123), (2, 10, 0, 6), (3, 0, 0, 0)], np.int32))
    whole = ops.window_span_keys(Qt, bank, items)
    red = torch.minimum(ops.window_span_keys(Qt, parts[0], items, vid_base=0), ops.window_span_keys(Qt, parts[1], items, vid_base=cut))
    assert torch.equal(red, whole) and bool((whole != _signed([KEY_EMPTY])[0]).all())


def test_two_thread_ranks_reproduce_the_single_shard(monkeypatch):
    from helpers import ThreadRanks
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    p, Q, V, counts = _window_problem(11, nv=9, nq=8, clips=21)
    counts = counts.copy()
    Qt, Vt = torch.from_numpy(Q), torch.from_numpy(V)
    n_own = counts[p["own"]]
    pos = engine.window_positives(p["times"], n_own, [0.5, 0.7], 5)
    whole = engine.corpus_from_embeddings(Vt, counts, "cpu", ops)
    want = engine.corpus_window_topk(whole, Qt, 5, 20, own_global=p["own"], positives=pos, ops=ops)
    ranks = ThreadRanks(2)
    monkeypatch.setattr(engine, "_dist", lambda: ranks)

    def body(rank, world):
        shard = engine.corpus_from_embeddings(Vt, counts, "cpu", ops, rank, world)
        return engine.corpus_window_topk(shard, Qt, 5, 20, own_global=p["own"], positives=pos, ops=ops, world=world)
    for got in ranks.run(body):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
