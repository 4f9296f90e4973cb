"""Prior-aware retrieval without a GPU: the CPU provider against the numpy statement of tests/prior_reference.py on the oracle's dense
moment scores (both levels, rank counts, own rows), the zero-table identities against the plain entry points, the table builders
against brute-force enumerations and direct counts, the unreachable semantics, evaluate_prior against evaluate, a bank split in two,
a dominating prior against evaluate_single's "prior" ordering, and the C entry points' host-side argument checks."""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

from fusion_reference import all_moments, moment_offsets, split_keys
from helpers import MemoryDataset, make_model, problem
from prior_reference import KEY_EMPTY, biased_scores, level_keys, own_rows, rank_keys, span_mask, statement, table_offsets

LEVELS = ("moments", "videos")


def _case(seed, counts, nq=7, D=37):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    V = (rs.randn(int(counts.sum()), D) * 0.3).astype(np.float32)
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _mixed_counts(nv, seed):
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = c[-1] = 21
    return c


def _random_values(max_clips, seed, excluded=0.2):
    """Biases drawn from multiples of 2^-4 (ties across moments and videos), a share of the entries excluded."""
    rs = np.random.RandomState(seed)
    v = (rs.randint(0, 8, int(table_offsets(max_clips)[-1])) / 16.0).astype(np.float32)
    v[rs.rand(len(v)) < excluded] = np.inf
    return v


def _table(engine, values, max_clips):
    off = table_offsets(max_clips)
    return engine.moment_table(max_clips, bias={n: values[off[n]:off[n + 1]] for n in range(max_clips + 1)})


def test_cpu_provider_matches_reference(oracle):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off = _case(1, _mixed_counts(9, 1))
    id_base = 11
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)
    Sc = oracle.score_moments(Q, V, off)
    values = _random_values(21, 2)
    table = _table(engine, values, 21)
    assert np.array_equal(table.values, values)
    nq = len(Q)
    for level in LEVELS:
        rk = rank_keys(Sc, counts, values, level, id_base)
        rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
        for k in (0, 1, 16, 448):
            d, i, c = ops.score_prior(torch.from_numpy(Q), bank, table, k, level, rd, ri)
            wd, wi, wc = statement(Sc, counts, values, k, level, id_base, rk)
            if k:
                assert np.array_equal(d.numpy(), wd) and np.array_equal(i.numpy(), wi), (level, k)
            assert np.array_equal(c.numpy(), wc), (level, k)
        assert wc[0].tolist() == [(q * 7) % int((level_keys(biased_scores(Sc, counts, values), counts, level)[0] != KEY_EMPTY).sum())
                                  for q in range(nq)]
    own = np.asarray([0, 8, 3, -1, 9, 4, 5], np.int64)                       # two of them outside the bank
    got = ops.score_prior_own(torch.from_numpy(Q), bank, table, torch.from_numpy(own.astype(np.int32)))
    assert np.array_equal(got.numpy(), own_rows(Sc, counts, values, own))


def test_zero_table_is_the_plain_retrieval():
    """A table of zeros: corpus_topk, corpus_video_topk and corpus_ranks, bit for bit."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off = _case(5, _mixed_counts(8, 5))
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    Qt = torch.from_numpy(Q)
    table = engine.moment_table(21)
    assert not table.values.any() and table.table_off.dtype == torch.int32 and table.table.dtype == torch.float32
    rs = np.random.RandomState(6)
    own = rs.randint(0, len(counts), len(Q))
    Mmax = int(counts[own].max() * (counts[own].max() + 1) // 2)
    labels = np.zeros((2, len(Q), Mmax), bool)
    for q in range(len(Q)):
        M = int(counts[own[q]] * (counts[own[q]] + 1) // 2)
        labels[0, q, rs.randint(0, M, 3)] = True
        labels[1, q, rs.randint(0, M)] = True
    labels = torch.from_numpy(labels)
    for k in (1, 10, 100):
        d, i, v, r, u = engine.corpus_prior_topk(shard, Qt, table, k, "moments", own_global=own, labels=labels, ops=ops)
        wd, wi = engine.corpus_topk(shard, Qt, k, ops)
        wr, _, _ = engine.corpus_ranks(shard, Qt, own, labels, ops)
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(r, wr) and not u.any()
        d, i, v, r, u = engine.corpus_prior_topk(shard, Qt, table, k, "videos", own_global=own, ops=ops)
        wd, wi, wv, wr = engine.corpus_video_topk(shard, Qt, k, own, ops)
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(v, wv) and torch.equal(r, wr) and not u.any()
    # lists only, no ground truth
    d, i, v, r, u = engine.corpus_prior_topk(shard, Qt, table, 5, ops=ops)
    assert torch.equal(i, engine.corpus_topk(shard, Qt, 5, ops)[1]) and r is None and u is None


@pytest.mark.parametrize("nmax", [8, 21])
def test_moment_table_masks_against_enumeration(nmax):
    from vfr_amd import engine
    from vfr_amd.utils import generate_moments
    for n in range(nmax + 1):
        assert [tuple(m) for m in generate_moments(n)] == all_moments(n)
    cases = [(dict(), lambda n, s, e: True),
             (dict(max_len=3), lambda n, s, e: e - s + 1 <= 3),
             (dict(min_len=2), lambda n, s, e: e - s + 1 >= 2),
             (dict(lengths=(1, 2, 3)), lambda n, s, e: e - s + 1 in (1, 2, 3)),
             (dict(lengths=(4, 8, 16), stride=4), lambda n, s, e: e - s + 1 in (4, 8, 16) and s % 4 == 0),
             (dict(min_len=2, max_len=5, lengths=(1, 3, 5, 7), stride=2), lambda n, s, e: e - s + 1 in (3, 5) and s % 2 == 0)]
    for kw, keep in cases:
        t = engine.moment_table(nmax, **kw)
        assert np.array_equal(t.values, span_mask(nmax, keep)), kw
        assert t.max_clips == nmax and t.table_off.tolist() == table_offsets(nmax).tolist() and np.array_equal(t.table.numpy(), t.values)
        for n in (0, 1, nmax):
            assert np.array_equal(t.enabled(n), np.asarray([keep(n, s, e) for s, e in all_moments(n)], bool))
    # a callable bias, and a dict bias with a clip count it does not name; masks win over finite biases
    t = engine.moment_table(nmax, bias=lambda n, s, e: 0.25 * (e - s), max_len=2)
    want = np.asarray([0.25 * (e - s) if e - s + 1 <= 2 else np.inf for n in range(nmax + 1) for s, e in all_moments(n)], np.float32)
    assert np.array_equal(t.values, want)
    t = engine.moment_table(nmax, bias={2: [1.0, 2.0, 3.0]})
    off = table_offsets(nmax)
    assert t.row(2).tolist() == [1.0, 2.0, 3.0] and t.values.sum() == 6.0 and len(t.values) == off[-1]


def test_moment_table_refusals():
    from vfr_amd import engine
    for bad in (float("nan"), -1.0, float("-inf")):
        with pytest.raises(ValueError):
            engine.moment_table(4, bias=lambda n, s, e: bad if (n, s, e) == (3, 0, 2) else 0.0)
        with pytest.raises(ValueError):
            engine.moment_table(4, bias={3: [0, 0, 0, 0, bad, 0]})
        with pytest.raises(ValueError):
            engine.moment_table(4, bias={3: [0, 0, 0, 0, bad, 0]}, max_len=1)      # also under the mask
    with pytest.raises(ValueError):
        engine.moment_table(4, bias={3: [0, 0, 0]})                                # a row of the wrong length
    with pytest.raises(ValueError):
        engine.moment_table(4, bias=lambda n, s, e: 1e39)                          # finite, but not in fp32
    for kw in (dict(max_clips=65), dict(max_clips=-1), dict(max_clips=4, stride=0)):
        with pytest.raises(ValueError):
            engine.moment_table(**kw)
    assert np.isinf(engine.moment_table(4, bias=lambda n, s, e: float("inf")).values).all()     # +inf is the exclusion, no error
    with pytest.raises(ValueError):
        engine.prior_table([[(0, 0)]], [3, 3])
    with pytest.raises(ValueError):
        engine.prior_table([[(0, 0)]], [3], lam=-1.0)
    with pytest.raises(ValueError):
        engine.prior_table([[(0, 0)]], [3], alpha=float("nan"))
    # a table built for shorter videos than the corpus holds
    ops = engine.TorchCpuOps()
    Q, V, counts, off = _case(3, [3, 5, 2])
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    with pytest.raises(ValueError, match="up to 4 clips"):
        engine.corpus_prior_topk(shard, torch.from_numpy(Q), engine.moment_table(4), 3, ops=ops)
    with pytest.raises(ValueError):
        engine.corpus_prior_topk(shard, torch.from_numpy(Q), engine.moment_table(5), 3, level="clips", ops=ops)


def test_prior_table_against_a_direct_count():
    """Every annotator span of every annotation is counted, per clip count of the annotation's own video (a small hand-made
    training set: 40 annotations of four spans each on videos of 3, 5 and 6 clips)."""
    from vfr_amd import engine
    rs = np.random.RandomState(4)
    counts = rs.choice([3, 5, 6], 40)
    times = [[(int(s), int(min(n - 1, s + rs.randint(0, 3)))) for s in rs.randint(0, n, 4)] for n in counts]
    times[0] = times[0] + [(1, 7), (2, 1)]                                   # outside the video / reversed: ignored
    lam, alpha = 0.5, 1.0
    t = engine.prior_table(times, counts, lam=lam, alpha=alpha, max_clips=8)
    assert t.max_clips == 8
    for n in range(9):
        c = Counter(tuple(x) for tt, m in zip(times, counts) if m == n for x in tt if 0 <= x[0] <= x[1] < n)
        if not c:
            assert not t.row(n).any(), n                                      # a clip count never seen in training: zeros
            continue
        total, M = sum(c.values()), n * (n + 1) // 2
        want = np.asarray([lam * -np.log((c.get(m, 0) + alpha) / (total + alpha * M)) for m in all_moments(n)]).astype(np.float32)
        assert np.array_equal(t.row(n), want), n
        assert (t.row(n) >= 0).all()
    # alpha = 0: a moment nobody annotated is never proposed
    t0 = engine.prior_table(times, counts, alpha=0.0)
    assert t0.max_clips == 6
    for n in (3, 5, 6):
        c = Counter(tuple(x) for tt, m in zip(times, counts) if m == n for x in tt if 0 <= x[0] <= x[1] < n)
        seen = np.asarray([m in c for m in all_moments(n)])
        assert np.array_equal(np.isinf(t0.row(n)), ~seen) and np.array_equal(t0.enabled(n), seen), n
        total = sum(c.values())
        assert np.array_equal(t0.row(n)[seen], np.asarray([-np.log(c[m] / total) for m in all_moments(n) if m in c]).astype(np.float32))
    assert not t0.row(4).any()
    # lam = 0 keeps the exclusions (0 x inf is not formed)
    tz = engine.prior_table(times, counts, lam=0.0, alpha=0.0)
    assert np.array_equal(np.isinf(tz.values), np.isinf(t0.values)) and not tz.values[np.isfinite(tz.values)].any()


def test_unreachable_queries():
    """Every positive of some queries is masked: no IndexError, rank = the number of candidates, flagged."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    counts = np.asarray([6, 4, 6, 5, 3, 6], np.int64)
    Q, V, counts, off = _case(8, counts, nq=6)
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    Qt = torch.from_numpy(Q)
    table = engine.moment_table(6, lengths=(1, 2))
    own = np.asarray([0, 1, 2, 3, 4, 5])
    Mmax = 21
    labels = np.zeros((2, 6, Mmax), bool)
    for q in range(6):
        spans = all_moments(int(counts[own[q]]))
        labels[0, q, spans.index((0, 2))] = True                             # length 3: masked for every query
        labels[1, q, spans.index((0, 2))] = True
        if q % 2:
            labels[1, q, spans.index((1, 2))] = True                         # length 2: reachable
    candidates = int(sum(n + (n - 1) for n in counts))
    d, i, v, r, u = engine.corpus_prior_topk(shard, Qt, table, 448, "moments", own_global=own, labels=torch.from_numpy(labels), ops=ops)
    assert u[0].all() and u[1].tolist() == [True, False, True, False, True, False]
    assert (r[0] == candidates).all() and (r[1][u[1]] == candidates).all() and (r[1][~u[1]] < candidates).all()
    assert int((i[0] >= 0).sum()) == candidates and (r.max() >= int((i[0] >= 0).sum()))       # no k finds an unreachable query
    # a query without any positive, masked or not, still raises
    labels[0, 3] = False
    with pytest.raises(IndexError):
        engine.corpus_prior_topk(shard, Qt, table, 0, "moments", own_global=own, labels=torch.from_numpy(labels), ops=ops)
    # video level: the own video has no candidate at all
    t6 = engine.moment_table(6, bias={n: (np.full(n * (n + 1) // 2, np.inf) if n == 4 else np.zeros(n * (n + 1) // 2)) for n in range(7)})
    d, i, v, r, u = engine.corpus_prior_topk(shard, Qt, t6, 6, "videos", own_global=own, ops=ops)
    assert u.tolist() == [False, True, False, False, False, False] and int(r[1]) == 5 and (v[:, 5] == -1).all() and (v[:, :5] != 1).all()


def _dataset(p):
    return MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])


def test_evaluate_prior_zero_table_is_evaluate():
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = problem(23, 17, "didemo", feat_dim=64, hidden=16)
        ds = _dataset(p)
        model = make_model(p["sd"], feat_dim=64, hidden=16)
        table = engine.moment_table(int(p["counts"].max()))
        want, (wd, wi) = vevaluate.evaluate(model, *ds.iterators(), ds.annotations, "cpu", return_topk=10)
        got, (d, i, v) = vevaluate.evaluate_prior(model, *ds.iterators(), ds.annotations, "cpu", table, k=10)
        assert got.pop("unreachable") == {"IoU=0.5": 0.0, "IoU=0.7": 0.0}
        assert got == want and torch.equal(d, wd) and torch.equal(i, wi)
        got = vevaluate.evaluate_prior(model, *ds.iterators(), ds.annotations, "cpu", table, level="videos")
        assert got.pop("unreachable") == {"video": 0.0}
        assert got == vevaluate.evaluate_videos(model, *ds.iterators(), ds.annotations, "cpu")
        # a proposal set: the share of unreachable queries is reported, the metrics keep their format
        got = vevaluate.evaluate_prior(model, *ds.iterators(), ds.annotations, "cpu", engine.moment_table(int(p["counts"].max()), lengths=(1,)))
        assert set(got) == set(want) | {"unreachable"} and set(got["model, IoU=0.5"]) == set(want["model, IoU=0.5"])
        assert all(0.0 <= x <= 100.0 for x in got["unreachable"].values())
        with pytest.raises(ValueError):
            vevaluate.evaluate_prior(model, *ds.iterators(), ds.annotations, "cpu", table, level="clips")
    finally:
        torch.set_num_threads(threads)


def test_two_shards_chain_and_merge(oracle):
    """The bank split in two with id_base and chained counts, merged with the top-k merge, equals the single bank."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Q, V, counts, off = _case(9, _mixed_counts(13, 9), nq=9)
    id_base = 1000
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)
    values = _random_values(21, 10)
    table = _table(engine, values, 21)
    Sc = oracle.score_moments(Q, V, off)
    Qt = torch.from_numpy(Q)
    parts = [ops.slice_bank(bank, counts, a, z) for a, z in ((0, 6), (6, 13))]
    assert parts[1].id_base == id_base + int(moment_offsets(counts)[6])
    for level in LEVELS:
        rk = rank_keys(Sc, counts, values, level, id_base)
        rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
        wd, wi, wc = ops.score_prior(Qt, bank, table, 16, level, rd, ri)
        sd, si, sc_ = statement(Sc, counts, values, 16, level, id_base, rk)
        assert np.array_equal(wd.numpy(), sd) and np.array_equal(wi.numpy(), si) and np.array_equal(wc.numpy(), sc_)
        cnt, lists = None, []
        for sub in parts:
            d, i, cnt = ops.score_prior(Qt, sub, table, 16, level, rd, ri, count_lt=cnt)
            lists.append((d, i))
        md, mi = ops.topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]))
        assert torch.equal(md, wd) and torch.equal(mi, wi) and torch.equal(cnt, wc), level


def test_dominating_prior_orders_like_evaluate_single():
    """bias = 1e6 x position in the training-frequency order: each query's own video is ordered exactly as the "prior" list
    evaluate_single consumes (moments by falling training frequency, ties by id)."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    rs = np.random.RandomState(12)
    counts = np.asarray([6, 6, 5, 6, 5, 4], np.int64)
    Q, V, counts, off = _case(12, counts, nq=6)
    train_counts = rs.choice([4, 5, 6], 60)
    train_times = [[(int(s), int(min(n - 1, s + rs.randint(0, 2)))) for s in rs.randint(0, n, 4)] for n in train_counts]
    prior, bias = {}, {}
    for n in (4, 5, 6):
        c = Counter(x for tt, m in zip(train_times, train_counts) if m == n for x in tt)
        spans = all_moments(n)
        order = sorted(range(len(spans)), key=lambda j: (-c.get(spans[j], 0), j))       # falling frequency, ties by id
        prior[n] = [spans[j] for j in order]                                          # evaluate_single's prior[num_segments]
        pos = np.empty(len(spans), np.int64)
        pos[order] = np.arange(len(spans))
        bias[n] = 1e6 * pos
    table = engine.moment_table(6, bias=bias)
    bank = ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), 0)
    own = np.arange(6)
    rows = ops.score_prior_own(torch.from_numpy(Q), bank, table, torch.from_numpy(own.astype(np.int32))).numpy()
    for q in range(6):
        n = int(counts[own[q]])
        spans = all_moments(n)
        got = [spans[j] for j in np.argsort(rows[q, :len(spans)], kind="stable")]
        assert got == prior[n], q
    # and through the corpus pass: a video's moments appear in the prior's order among the k best of its own query
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    d, i, v, _, _ = engine.corpus_prior_topk(shard, torch.from_numpy(Q), table, 448, ops=ops)      # the corpus has 103 moments
    mo = moment_offsets(counts)
    for q in range(6):
        mine = i[q][v[q] == own[q]].numpy() - mo[own[q]]
        spans = all_moments(int(counts[own[q]]))
        assert [spans[j] for j in mine] == prior[int(counts[own[q]])], q


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 16)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def call(Q=dummy, k=10, level=0, max_clips=21, D=100, num_rank=0, nbytes=1 << 16, wsp=dummy, table_off=dummy, table=dummy,
             id_base=0, out=dummy):
        return lib.vfr_score_prior_f32(Q, 4, dummy, dummy, dummy, 10, 210, 21, max_clips, D, 1e-6, id_base, level, k, out, out,
                                       num_rank, None, None, None, table_off, table, None, wsp, nbytes, None)

    def own(max_clips=21, Mmax=231, D=100, table_off=dummy, table=dummy, own_=dummy):
        return lib.vfr_score_prior_own_f32(dummy, 4, dummy, dummy, own_, 10, max_clips, D, 1e-6, Mmax, table_off, table, dummy, None,
                                           None)

    assert call(k=449) == -1 and call(level=2) == -1 and call(num_rank=5) == -1 and call(num_rank=1) == -1
    assert b"vfr_score_prior_f32" in lib.vfr_last_error()
    assert call(max_clips=65) == -1 and call(D=0) == -1 and call(id_base=-1) == -1 and call(id_base=1 << 32) == -1
    assert call(table=None) == -1 and b"table" in lib.vfr_last_error() and call(table_off=None) == -1
    assert call(Q=None) == -1 and call(out=None) == -1
    assert call(wsp=None) == -4 and call(nbytes=16) == -4                      # VFR_EWORKSPACE
    assert own(Mmax=230) == -1 and own(max_clips=65) == -1 and own(D=0) == -1 and own(table=None) == -1 and own(own_=None) == -1
    assert b"vfr_score_prior_own_f32" in lib.vfr_last_error()
    wsb = lib.vfr_score_prior_workspace_bytes
    assert wsb(5000, 10000, 100) == 5000 * 100 * 8 + 256 == wsb(5000, 10_000_000, 100)     # O(Nq k): no Nq x Nv term
    assert wsb(1, 64 * 256, 100) == wsb(1, 1 << 30, 100) == 256 * 100 * 8 + 256
    assert wsb(5000, 10000, 449) == 0 and wsb(-1, 10, 1) == 0 and wsb(1 << 31, 10, 1) == 0
