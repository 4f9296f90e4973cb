"""Hard-negative mining without a GPU: the CPU provider and engine.corpus_mine_negatives against the numpy statement of
tests/mining_reference.py on the oracle's dense moment scores (bit for bit), shards cut with slice_bank, the C entry points'
host-side argument checks, and training.HardNegativeSampler."""
import ctypes
import random

import numpy as np
import pytest
import torch

from helpers import MemoryDataset, make_model, problem
from mining_reference import all_moments, eligible, span_scores, statement

KEYS = ("inter_dist", "inter_vid", "intra_dist", "intra_idx")


def _ragged(seed, nv=23, nq=9, D=12):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 9, nv).astype(np.int64)
    counts[:3] = (1, 8, 8)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    V[off[2]:off[3]] = V[off[1]:off[2]]                       # videos 1 and 2 alike: tied scores, the id decides
    V[off[5]:off[6]] = V[off[5]]                              # a video of repeated clips: ties inside the own video
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, off


def _items(rs, counts, nm, nq, base=0):
    v = rs.randint(0, len(counts), nm)
    n = np.asarray(counts)[v]
    s = (rs.rand(nm) * n).astype(np.int64)
    e = s + (rs.rand(nm) * (n - s)).astype(np.int64)
    return np.stack([rs.randint(0, nq, nm), v + base, s, e], axis=1).astype(np.int64)


def _excl(rs, items, X):
    ex = np.full((len(items), X, 2), -1, np.int64)
    for m, (_, _, s, e) in enumerate(items):
        ex[m, 0] = (s, e)                                     # the positive itself, as the sampler passes it
        for j in range(1, rs.randint(1, X + 1)):
            a = rs.randint(0, 8)
            ex[m, j] = (a, rs.randint(a, 8))
    return ex


def _bank(ops, V, off, id_base=0):
    return ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base)


def _same(got, want, h, what=""):
    ind, inv, itd, iti, ci, ca = got
    if h:
        for name, t in zip(KEYS, (ind, inv, itd, iti)):
            assert np.array_equal(t.numpy(), want[name]), (what, name)
    if ci is not None:
        assert np.array_equal(ci.numpy(), want["count_inter"]) and np.array_equal(ca.numpy(), want["count_intra"]), what


@pytest.mark.parametrize("mode", ["same_length", "any"])
def test_cpu_provider_matches_statement(oracle, mode):
    from vfr_amd import engine
    Q, V, counts, off = _ragged(0)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, off)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(1)
    items = np.concatenate([_items(rs, counts, 40, len(Q)), [[0, 0, 0, 0], [1, 1, 0, 7], [2, 2, 0, 7], [3, 5, 1, 2], [3, 5, 1, 2]],
                            [[9, 1, 0, 0], [-1, 1, 0, 0], [0, -1, 0, 0], [0, 1, 2, 1], [0, 1, -1, 0], [0, 3, 0, 99]]])
    excl = _excl(rs, items, 4) if mode == "any" else None
    pos, pbad = span_scores(Sc, counts, items)
    got_pos = ops.score_spans(torch.from_numpy(Q), bank, torch.from_numpy(items))
    assert pbad == 1 and np.array_equal(got_pos.numpy(), pos)
    thr = (pos + np.float32(0.1)).astype(np.float32)
    for floor, th in ((None, None), (pos, None), (None, thr), (pos, thr)):
        for h in (0, 1, 5, 40):
            if h == 0 and th is None:
                continue
            bad = torch.zeros(1, dtype=torch.int32)
            got = ops.mine_negatives(torch.from_numpy(Q), bank, torch.from_numpy(items), h, 0, mode,
                                     None if excl is None else torch.from_numpy(excl), None if floor is None else torch.from_numpy(floor),
                                     None if th is None else torch.from_numpy(th), bad=bad)
            want = statement(Sc, counts, items, h, 0, 0, mode, excl, floor, th)
            assert int(bad) == want["bad"] == 1
            _same(got, want, h, (floor is not None, th is not None, h))
            assert (got[4] is None) == (th is None)
    # the hardest semi-hard negative scores above the positive, and a whole-video span has no same-length neighbour
    want = statement(Sc, counts, items, 1, 0, 0, mode, excl, pos, None)
    ok = np.isfinite(want["inter_dist"][:, 0])
    assert ok.any() and np.all(want["inter_dist"][ok, 0] > pos[ok])
    if mode == "same_length":
        assert np.all(want["intra_idx"][[41, 42]] == -1)


def test_two_shards_merge_to_one(oracle):
    """The bank cut in two by slice_bank (vid_base / id_base != 0): merged inter lists, MIN / MAX-merged intra lists and summed
    counts equal the one-shard result; for some items the own video sits on the other shard."""
    from vfr_amd import engine
    Q, V, counts, off = _ragged(2)
    ops = engine.TorchCpuOps()
    bank = _bank(ops, V, off)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(3)
    items = _items(rs, counts, 50, len(Q))
    cut = 10
    assert (items[:, 1] < cut).any() and (items[:, 1] >= cut).any()
    pos, _ = span_scores(Sc, counts, items)
    thr = (pos + np.float32(0.1)).astype(np.float32)
    Qt, it, tt = torch.from_numpy(Q), torch.from_numpy(items), torch.from_numpy(thr)
    for mode in ("same_length", "any"):
        h = 6
        one = ops.mine_negatives(Qt, bank, it, h, 0, mode, None, None, tt)
        _same(one, statement(Sc, counts, items, h, 0, 0, mode, None, None, thr), h, mode)
        lo = ops.slice_bank(bank, counts, 0, cut)
        hi = ops.slice_bank(bank, counts, cut, len(counts))
        assert hi.id_base > 0
        a = ops.mine_negatives(Qt, lo, it, h, 0, mode, None, None, tt)
        # the statement holds per shard as well
        mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
        Sc_hi = Sc[:, mo[cut]:]
        _same(ops.mine_negatives(Qt, hi, it, h, cut, mode, None, None, tt),
              statement(Sc_hi, counts[cut:], items, h, cut, int(mo[cut]), mode, None, None, thr), h, mode + " upper shard")
        b = ops.mine_negatives(Qt, hi, it, h, cut, mode, None, None, tt, intra_out=(a[2], a[3]), count_inter=a[4], count_intra=a[5])
        md, mi = ops.topk_merge(torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]]))
        assert torch.equal(md, one[0]) and torch.equal(mi, one[1])
        assert torch.equal(b[2], one[2]) and torch.equal(b[3], one[3])
        assert torch.equal(b[4], one[4]) and torch.equal(b[5], one[5])
        p = ops.score_spans(Qt, hi, it, cut, out=ops.score_spans(Qt, lo, it, 0))
        assert np.array_equal(p.numpy(), pos)


def test_corpus_mine_negatives_cpu(oracle):
    from vfr_amd import engine
    Q, V, counts, off = _ragged(4)
    ops = engine.TorchCpuOps()
    shard = engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops)
    Sc = oracle.score_moments(Q, V, off)
    rs = np.random.RandomState(5)
    items = _items(rs, counts, 30, len(Q))
    pos, _ = span_scores(Sc, counts, items)
    thr = pos + np.float32(0.1)
    res = engine.corpus_mine_negatives(shard, torch.from_numpy(Q), items, 4, "same_length", None, True, 0.1, ops)
    want = statement(Sc, counts, items, 4, 0, 0, "same_length", None, pos, thr)
    assert np.array_equal(res.pos.numpy(), pos) and not res.malformed()
    broken = np.concatenate([items[:3], [[0, 1, 0, 99]]])
    assert engine.corpus_mine_negatives(shard, torch.from_numpy(Q), broken, 2, ops=ops).malformed()
    _same((res.inter_dist, res.inter_vid, res.intra_dist, res.intra_idx, res.count_inter, res.count_intra), want, 4)
    spans = res.intra_spans()
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    for m, (_, v, s, e) in enumerate(items):
        for j in range(4):
            i = want["intra_idx"][m, j]
            if i < 0:
                assert tuple(spans[m, j]) == (-1, -1)
            else:
                assert tuple(spans[m, j]) == all_moments(int(counts[v]))[i - mo[v]] and spans[m, j, 1] - spans[m, j, 0] == e - s
    res = engine.corpus_mine_negatives(shard, torch.from_numpy(Q), items, 0, margin=0.1, ops=ops)
    assert res.inter_dist is None and np.array_equal(res.count_inter.numpy(), want["count_inter"])
    with pytest.raises(ValueError):
        engine.corpus_mine_negatives(shard, torch.from_numpy(Q), items, 4, "longest", ops=ops)


def test_wrappers_refuse_cpu_tensors():
    from vfr_amd import _vfr
    with pytest.raises(RuntimeError):
        _vfr.mine_negatives(torch.zeros((3, 100)), None, torch.zeros((1, 4), dtype=torch.int32), 1)
    with pytest.raises(RuntimeError):
        _vfr.score_spans(torch.zeros((3, 100)), None, torch.zeros((1, 4), dtype=torch.int32))


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 20)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def mine(Q=dummy, Nq=8, V=dummy, off=dummy, mom=dummy, Nv=10, max_clips=21, D=100, id_base=0, vid_base=0, items=dummy, Nm=4, h=10,
             mode=0, excl=None, X=0, thr=None, ind=dummy, inv=dummy, itd=dummy, iti=dummy, ci=None, ca=None, wsb=1 << 20):
        return lib.vfr_mine_negatives_f32(Q, Nq, V, off, mom, Nv, 210, max_clips, D, 1e-6, id_base, vid_base, items, Nm, h, mode, excl,
                                          X, None, thr, ind, inv, itd, iti, ci, ca, None, dummy, wsb, None)
    assert mine(h=449) == -1 and mine(h=-1) == -1
    assert mine(mode=1, X=9, excl=dummy) == -1 and mine(mode=1, X=-1) == -1 and mine(mode=1, X=2) == -1 and mine(mode=2) == -1
    assert mine(max_clips=65) == -1
    assert mine(items=None) == -1 and mine(Q=None) == -1 and mine(off=None) == -1 and mine(mom=None) == -1 and mine(V=None) == -1
    assert mine(ind=None) == -1 and mine(iti=None) == -1                       # half a list
    assert mine(thr=dummy) == -1 and mine(ci=dummy) == -1                      # a threshold without counts, counts without one
    assert mine(Nq=-1) == -1 and mine(Nm=-1) == -1 and mine(Nv=-1) == -1 and mine(D=0) == -1
    assert mine(vid_base=-1) == -1 and mine(id_base=-1) == -1
    assert mine(vid_base=(1 << 32) - 5) == -1 and mine(id_base=1 << 32) == -1
    assert mine(Nm=1 << 30, h=2) == -1
    assert b"vfr_mine_negatives_f32" in lib.vfr_last_error()
    assert mine(wsb=8) == -4

    def spans(Q=dummy, Nq=8, V=dummy, off=dummy, Nv=10, max_clips=21, D=100, vid_base=0, items=dummy, Np=4, out=dummy):
        return lib.vfr_score_spans_f32(Q, Nq, V, off, Nv, 210, max_clips, D, 1e-6, vid_base, items, Np, out, None, None)
    assert spans(items=None) == -1 and spans(out=None) == -1 and spans(Q=None) == -1 and spans(off=None) == -1 and spans(V=None) == -1
    assert spans(Np=-1) == -1 and spans(Nq=-1) == -1 and spans(Nv=-1) == -1 and spans(D=0) == -1 and spans(max_clips=65) == -1
    assert spans(vid_base=-1) == -1 and spans(vid_base=(1 << 32) - 5) == -1
    assert b"vfr_score_spans_f32" in lib.vfr_last_error()
    size = lib.vfr_mine_negatives_workspace_bytes
    assert size(4, 10, 449) == 0 and size(-1, 10, 10) == 0 and size(4, -1, 10) == 0 and size(4, 10, -1) == 0 and size(1 << 30, 10, 2) == 0
    assert size(4, 10, 10) >= 4 * 10 * 8 and size(4, 10, 0) > 0 and size(0, 0, 0) > 0
    # no Nm x Nv term: the number of video chunks is capped, so the size stops growing with Nv and is at most linear in Nm
    for Nm in (1, 64, 100, 5000, 33000):
        for h in (1, 16, 448):
            assert size(Nm, 1 << 24, h) == size(Nm, 1 << 25, h)
            assert size(2 * Nm, 1 << 24, h) <= 2 * size(Nm, 1 << 24, h)
            assert size(2 * Nm, 10000, h) <= 2 * size(Nm, 10000, h)


def test_chunk_plan_of_the_benchmark_shapes():
    """The video axis is cut into C = min(ceil(4096 / Nm), ceil(Nv / 64), 256) chunks; the workspace is 256 + 8 h Nm C bytes rounded
    up to 256: 5 000 items stream the whole bank in one chunk, 64 items take 64 chunks, one item one chunk per block of 64 videos."""
    from vfr_amd import _vfr
    size = _vfr.lib().vfr_mine_negatives_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256
    for Nm, Nv, h, C in ((5000, 10000, 16, 1), (64, 10000, 16, 64), (1, 10000, 16, 157), (1, 100000, 16, 256), (2100, 1100, 448, 2),
                         (300, 300, 16, 5), (4096, 10000, 448, 1), (4095, 10000, 1, 2)):
        assert size(Nm, Nv, h) == up(256 + 8 * h * Nm * C), (Nm, Nv, h)


# ------------------------------------------------------------------------------------------------ the sampler
def _dataset(whole_video=False):
    """A small corpus whose annotations stay inside their videos and never cover one (unless asked for)."""
    p = problem(17, 26, "didemo", feat_dim=64, hidden=16)
    counts = p["counts"]
    rs = np.random.RandomState(11)
    long_enough = np.flatnonzero(counts >= 3)
    own = long_enough[rs.randint(0, len(long_enough), len(p["tokens"]))]
    times = []
    for q, v in enumerate(own):
        n = int(counts[v])
        spans = []
        for _ in range(3):
            s = int(rs.randint(0, n - 1))
            e = int(rs.randint(s, min(n - 1, s + n - 2)))      # never the whole video
            spans.append([s, e])
        times.append(spans + [list(spans[0])])
    if whole_video:
        times[3] = [[0, int(counts[own[3]]) - 1]] * 4
    ds = MemoryDataset(p["seg"], p["ctx"], counts, p["tokens"], own, times)
    return p, ds, make_model(p["sd"], feat_dim=64, hidden=16)


def _batches(sampler, seed):
    random.seed(seed)
    return [list(b) for b in sampler]


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("same_length", [True, False])
def test_sampler_before_refresh_is_the_parent(train, same_length):
    from vfr_amd import training
    _, ds, _ = _dataset()
    parent = training.TripletBatchSampler(24, ds.annotations, ds.num_segments_info, train=train, same_length=same_length)
    hard = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, train=train, same_length=same_length, h=4)
    assert _batches(hard, 5) == _batches(parent, 5) and len(_batches(parent, 5)) > 1


def _statement_tables(ds, model, same_length, h, semi_hard=False):
    """Per (annotation, span) the statement's hardest inter videos and intra spans, on the CPU provider's own embeddings."""
    from oracle import oracle as orc
    from vfr_amd import engine
    orc.build()
    ops = engine.TorchCpuOps()
    bank = ds.feature_bank()
    shard = engine.build_corpus(model, bank, "cpu", ops)
    counts = shard.counts_all
    ids = list(ds.annotations)
    Q = engine.encode_queries(model, torch.cat([ds.lang_features[a] for a in ids]), "cpu", ops)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    Sc = orc.score_moments(Q.numpy(), shard.bank.emb.numpy(), off)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    out = {}
    for r, a in enumerate(ids):
        v = bank.videos.index(ds.annotations[a]["video"])
        named = sorted({(int(s), int(e)) for s, e in ds.annotations[a]["times"]})
        for s, e in named:
            item = (r, v, s, e)
            sc, vs, isc, iid = eligible(Sc, counts, item, 0, 0, "same_length" if same_length else "any", named)
            fl = Sc[r, mo[v] + (s if s == e else counts[v] + (s * (2 * counts[v] - s - 1)) // 2 + (e - s - 1))]
            if semi_hard:
                vs, sc = vs[sc > fl], sc[sc > fl]
                iid, isc = iid[isc > fl], isc[isc > fl]
            vo = vs[np.lexsort((vs, sc))][:h]
            io = iid[np.lexsort((iid, isc))][:h]
            n = int(counts[v])
            out[(a, s, e)] = ([bank.videos[i] for i in vo], [all_moments(n)[i - mo[v]] for i in io])
    return out


@pytest.mark.parametrize("same_length", [True, False])
def test_sampler_after_refresh_draws_the_hardest(same_length):
    from vfr_amd import engine, training
    _, ds, model = _dataset()
    model.train()
    hard = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, train=False, same_length=same_length, h=1)
    hard.refresh(model, ds, "cpu", engine.TorchCpuOps(), margin=0.1)
    assert model.training                                        # the caller's mode came back
    want = _statement_tables(ds, model.eval(), same_length, 1)
    loader = training.TripletLoader(ds, hard, "cpu")
    seen = 0
    for batch in hard:
        for t in batch:
            vids, spans = want[(t["annotation_id"], t["start_t"], t["end_t"])]
            assert t["video_neg"] == vids[0] and (t["start_tn"], t["end_tn"]) == spans[0], t
            n = ds.num_segments_info
            assert t["end_t"] < n[t["video_neg"]] and t["end_tn"] < n[t["video_pos"]] and t["video_neg"] != t["video_pos"]
            seen += 1
        assert loader.collate(batch)["n_samples"] == len(batch)
    st = hard.last_stats
    assert seen == len(ds.annotations) and st["mined_draws"] == 2 * seen and st["parent_draws"] == 0
    assert st["violators_inter"] >= 0 and st["violators_intra"] >= 0 and st["items"] >= seen
    # train=True: every draw comes from the mined lists, and a seeded `random` repeats the batches
    hard5 = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, train=True, same_length=same_length, h=5)
    hard5.refresh(model, ds, "cpu", engine.TorchCpuOps(), semi_hard=True)
    want5 = _statement_tables(ds, model.eval(), same_length, 5, semi_hard=True)
    first = _batches(hard5, 9)
    assert first == _batches(hard5, 9) and first != _batches(hard5, 10)
    for t in (t for b in first for t in b):
        vids, spans = want5[(t["annotation_id"], t["start_t"], t["end_t"])]
        assert (t["video_neg"] in vids or not vids) and ((t["start_tn"], t["end_tn"]) in spans or not spans)


def test_sampler_hard_fraction_zero_never_uses_the_lists():
    from vfr_amd import engine, training
    _, ds, model = _dataset()
    for train in (True, False):
        parent = training.TripletBatchSampler(24, ds.annotations, ds.num_segments_info, train=train)
        hard = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, train=train, h=2, hard_fraction=0.0)
        hard.refresh(model, ds, "cpu", engine.TorchCpuOps())
        assert hard.mined and _batches(hard, 3) == _batches(parent, 3)
        assert hard.last_stats["mined_draws"] == 0 and hard.last_stats["parent_draws"] == 2 * len(ds.annotations)
    mixed = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, h=2, hard_fraction=0.5)
    mixed.refresh(model, ds, "cpu", engine.TorchCpuOps())
    assert _batches(mixed, 4) == _batches(mixed, 4)
    assert 0 < mixed.last_stats["mined_draws"] < 2 * len(ds.annotations)


def test_sampler_whole_video_span_falls_back():
    """An annotation whose span covers its whole video has no same-length neighbour: the mined intra list is empty, the draw falls
    back (to the any-length candidates, the parent having none) and the triplet still passes TripletLoader's span check."""
    from vfr_amd import engine, training
    _, ds, model = _dataset(whole_video=True)
    n = ds.num_segments_info
    for train in (True, False):
        hard = training.HardNegativeSampler(24, ds.annotations, ds.num_segments_info, train=train, h=3)
        hard.refresh(model, ds, "cpu", engine.TorchCpuOps())
        video = ds.annotations[3]["video"]
        assert hard.mined[(3, 0, n[video] - 1)][1] == [] and len(hard.mined[(3, 0, n[video] - 1)][0]) > 0
        loader = training.TripletLoader(ds, hard, "cpu")
        random.seed(2)
        got = [t for b in hard for t in b if loader.collate(b) is not None]
        mine = [t for t in got if t["annotation_id"] == 3]
        assert len(got) == len(ds.annotations) and len(mine) == 1
        t = mine[0]
        assert (t["start_t"], t["end_t"]) == (0, n[video] - 1) and (t["start_tn"], t["end_tn"]) != (0, n[video] - 1)
        assert t["end_tn"] < n[video] and t["end_t"] < n[t["video_neg"]]
        assert hard.last_stats["parent_draws"] >= 1 and hard.last_stats["skipped"] == 0
