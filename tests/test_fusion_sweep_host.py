"""The fusion weight sweep without a GPU: the CPU provider against the numpy statement of tests/fusion_reference.py per row of the
grid (counts at both levels, own rows), engine.simplex_grid, the split of a 17-row grid, evaluate.sweep_fusion against
evaluate_fusion row by row with the selection rule, and the C entry points' host-side refusals."""
import ctypes

import numpy as np
import pytest
import torch

from fusion_sweep_reference import GRID5, fused_grid, grid_keys, mixed_counts, rank_keys, split_keys, streams, sweep_own_rows, sweep_statement
from helpers import MemoryDataset, make_model, problem

CPU_THREADS = 1
LEVELS = ("moments", "videos")


def _t(arrs):
    return [torch.from_numpy(a) for a in arrs]


def _banks(ops, Vs, off, id_base=0):
    return [ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base) for V in Vs]


def _rank_tensors(rk):
    rd, ri = split_keys(rk)
    return torch.from_numpy(rd.reshape(rk.shape)), torch.from_numpy(ri.reshape(rk.shape))


@pytest.mark.parametrize("dims", [(100, 37), (100, 37, 4)])
def test_cpu_provider_matches_the_statement_per_row(oracle, dims):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    S = len(dims)
    grid = GRID5 if S == 2 else ((0.5, 0.25, 2.0), (0.0, 1.0, 0.0), (0.2, 0.3, 0.5))
    Qs, Vs, counts, off = streams(mixed_counts(9, S), dims, seed=S, nq=7)
    id_base = 11
    banks = _banks(ops, Vs, off, id_base)
    Scs = [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]
    for level in LEVELS:
        rk = rank_keys(grid_keys(fused_grid(Scs, counts, grid), counts, level, id_base))
        want = sweep_statement(Scs, counts, grid, level, id_base, rk)
        rd, ri = _rank_tensors(rk)
        got = ops.score_fusion_sweep(_t(Qs), banks, grid, level, rd, ri)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want), level
        assert want.any()
        # counts are ADDED onto a preset tensor
        preset = torch.arange(want.size, dtype=torch.int64).reshape(want.shape)
        assert np.array_equal(ops.score_fusion_sweep(_t(Qs), banks, grid, level, rd, ri, count_lt=preset).numpy(), want + preset.numpy())
    own = (np.arange(7) * 4) % len(counts)
    got = ops.score_fusion_sweep_own(_t(Qs), banks, grid, torch.from_numpy(own.astype(np.int32)))
    assert np.array_equal(got.numpy(), sweep_own_rows(Scs, counts, grid, own))


def test_simplex_grid():
    from math import comb

    from vfr_amd import engine
    g = engine.simplex_grid(2, 10)
    assert g.dtype == np.float32 and g.shape == (11, 2)
    assert np.array_equal(g, (np.stack([np.arange(11), 10 - np.arange(11)], axis=1) / 10).astype(np.float32))
    for S, steps in ((1, 5), (2, 1), (3, 4), (4, 3)):
        g = engine.simplex_grid(S, steps)
        assert g.dtype == np.float32 and g.shape == (comb(steps + S - 1, S - 1), S)
        ints = np.rint(g.astype(np.float64) * steps).astype(np.int64)
        assert np.array_equal((ints / steps).astype(np.float32), g) and np.all(ints >= 0) and np.all(ints.sum(axis=1) == steps)
        rows = [tuple(r) for r in ints]
        assert rows == sorted(set(rows)), "lexicographic, no duplicates"
    assert engine.simplex_grid(1, 7).tolist() == [[1.0]]
    for bad in ((0, 3), (2, 0)):
        with pytest.raises(ValueError):
            engine.simplex_grid(*bad)


def test_weight_grid_validation():
    from vfr_amd import _vfr
    g = _vfr.fusion_weight_grid([[0.5, 0.5], [1, 0]], 2)
    assert g.dtype == np.float32 and g.shape == (2, 2) and g.flags["C_CONTIGUOUS"]
    for bad, S in (([[0.5, -0.1]], 2), ([[0.5, float("nan")]], 2), ([[float("inf"), 1.0]], 2), ([[1.0]], 2), ([0.5, 0.5], 2),
                   (np.zeros((0, 2)), 2), ([[1.0] * 5], 5)):
        with pytest.raises(ValueError):
            _vfr.fusion_weight_grid(bad, S)
    with pytest.raises(ValueError, match="row 3"):
        _vfr.fusion_weight_grid([[1, 0]] * 3 + [[0.5, -1]], 2)


def test_a_17_row_grid_equals_its_two_slices(oracle):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    grid = engine.simplex_grid(2, 16)
    assert len(grid) == 17
    Qs, Vs, counts, off = streams(mixed_counts(6, 3), (100, 37), seed=3, nq=5)
    banks = _banks(ops, Vs, off, 4)
    Scs = [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]
    rk = rank_keys(grid_keys(fused_grid(Scs, counts, grid), counts, "moments", 4))
    rd, ri = _rank_tensors(rk)
    whole = ops.score_fusion_sweep(_t(Qs), banks, grid, "moments", rd, ri)
    parts = [ops.score_fusion_sweep(_t(Qs), banks, grid[a:z], "moments", rd[a:z], ri[a:z]) for a, z in ((0, 16), (16, 17))]
    assert torch.equal(whole, torch.cat(parts))
    assert np.array_equal(whole.numpy(), sweep_statement(Scs, counts, grid, "moments", 4, rk))
    own = torch.from_numpy((np.arange(5) % len(counts)).astype(np.int32))
    whole = ops.score_fusion_sweep_own(_t(Qs), banks, grid, own)
    assert whole.shape[0] == 17
    assert torch.equal(whole, torch.cat([ops.score_fusion_sweep_own(_t(Qs), banks, grid[a:z], own) for a, z in ((0, 16), (16, 17))]))


def _dataset(p):
    return MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])


def _two_stream_problem():
    ps = [problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=123)]
    ps.append(dict(ps[0], sd=problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=321)["sd"]))
    return ps


def test_sweep_fusion_equals_evaluate_fusion_per_row():
    """The 40-video, 30-query problem of the fusion tests, two differently seeded models."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        ps = _two_stream_problem()
        models = [make_model(p["sd"], feat_dim=64, hidden=16) for p in ps]
        dss = [_dataset(p) for p in ps]
        grid = engine.simplex_grid(2, 4)

        def its():
            x = [d.iterators() for d in dss]
            return [i[0] for i in x], [i[1] for i in x]
        for level, select in (("moments", ("model, IoU=0.5", "R@10")), ("moments", ("model, IoU=0.7", "MR")), ("videos", ("video", "MR")),
                              ("videos", None)):
            vi, li = its()
            metrics, best = vevaluate.sweep_fusion(models, vi, li, dss[0].annotations, "cpu", grid, level=level, select=select)
            assert len(metrics) == len(grid)
            for w, m in zip(grid, metrics):
                vi, li = its()
                assert m == vevaluate.evaluate_fusion(models, vi, li, dss[0].annotations, "cpu", w, level=level), (level, w)
            if select is None:
                assert best is None
            else:
                vals = [m[select[0]][select[1]] for m in metrics]
                target = min(vals) if select[1] == "MR" else max(vals)
                assert best == vals.index(target), (level, select, vals)
        # a tie goes to the lowest index: one weight vector three times behind another one
        tie = np.asarray([(0.5, 0.5), (0.25, 0.75), (0.25, 0.75), (0.25, 0.75)], np.float32)
        for select in (("model, IoU=0.5", "R@1"), ("model, IoU=0.5", "MR")):
            vi, li = its()
            metrics, best = vevaluate.sweep_fusion(models, vi, li, dss[0].annotations, "cpu", tie, select=select)
            assert metrics[1] == metrics[2] == metrics[3]
            vals = [m[select[0]][select[1]] for m in metrics]
            target = min(vals) if select[1] == "MR" else max(vals)
            assert best == vals.index(target) and best in (0, 1)
            vi, li = its()
            assert vevaluate.sweep_fusion(models, vi, li, dss[0].annotations, "cpu", tie[1:], select=select)[1] == 0
        # refusals: those of evaluate_fusion
        vi, li = its()
        with pytest.raises(ValueError):
            vevaluate.sweep_fusion(models, vi, li, dss[0].annotations, "cpu", [(0.5, -0.5)])
        with pytest.raises(ValueError):
            vevaluate.sweep_fusion(models, vi, li, dss[0].annotations, "cpu", grid, level="clips")
        with pytest.raises(ValueError):
            vevaluate.sweep_fusion(models, vi[:1], li, dss[0].annotations, "cpu", grid)
    finally:
        torch.set_num_threads(threads)


def test_capi_rejects_bad_sweep_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    dummy = ctypes.cast(buf, ctypes.c_void_p).value      # never dereferenced: every call below ends in its host-side checks

    def hosts(S, W, D=(100, 37, 4, 100), neg=None):
        w = [0.25] * (max(W, 1) * S)
        if neg is not None:
            w[neg[0] * S + neg[1]] = -0.5
        return ((ctypes.c_void_p * S)(*[dummy] * S), (ctypes.c_void_p * S)(*[dummy] * S), (ctypes.c_int * S)(*D[:S]),
                (ctypes.c_float * len(w))(*w))

    def scan(S=2, W=3, max_clips=21, num_rank=0, neg=None, level=0, h=None):
        Qh, Vh, Dh, wh = h if h is not None else hosts(S, W, neg=neg)
        return lib.vfr_score_fusion_sweep_f32(Qh, Vh, Dh, wh, W, S, 4, dummy, dummy, 10, 10 * max_clips, max_clips, 1e-6, 0, level,
                                              num_rank, None, None, None, None)

    def own(S=2, W=3, max_clips=21, neg=None, Mmax=None, h=None, nq=0):
        Qh, Vh, Dh, wh = h if h is not None else hosts(S, W, neg=neg)
        Mmax = max_clips * (max_clips + 1) // 2 if Mmax is None else Mmax
        return lib.vfr_score_fusion_sweep_own_f32(Qh, Vh, Dh, wh, W, S, nq, dummy, dummy, 10, max_clips, 1e-6, Mmax, dummy, None)

    for fn in (scan, own):
        assert fn(W=0) == -1 and b"W = 0" in lib.vfr_last_error()
        assert fn(W=17) == -1 and b"W = 17" in lib.vfr_last_error() and b"VFR_FUSION_MAX_SWEEP" in lib.vfr_last_error()
        assert fn(W=16, neg=(7, 1)) == -1
        err = lib.vfr_last_error()
        assert b"row 7" in err and b"weight -0.5" in err, err
        assert fn(W=1, neg=(0, 0)) == -1 and b"row 0" in lib.vfr_last_error()
        assert fn(S=0) == -1 and b"S = 0" in lib.vfr_last_error()
        Qh, Vh, Dh, wh = hosts(2, 3)
        assert fn(h=(Qh, Vh, Dh, None)) == -1 and fn(h=(None, Vh, Dh, wh)) == -1 and b"null stream array" in lib.vfr_last_error()
        assert fn(max_clips=65) == -1
        assert fn() == 0                                    # num_rank = 0 / Nq = 0: VFR_OK, nothing enqueued
    for nan in (float("nan"), float("inf")):
        Qh, Vh, Dh, wh = hosts(2, 3)
        wh[5] = nan
        assert scan(h=(Qh, Vh, Dh, wh)) == -1 and b"row 2" in lib.vfr_last_error()
    assert scan(level=2) == -1 and scan(num_rank=5) == -1 and scan(num_rank=1) == -1
    assert b"vfr_score_fusion_sweep_f32" in lib.vfr_last_error()
    assert own(Mmax=230, nq=4) == -1 and own(nq=4, h=hosts(2, 3)[:3] + (None,)) == -1
    # the LDS plan: 4 x (100 + 40 + 4 + 100) of query rows + 256 x 64 x (4 + 1) of distances = 82 896 bytes > 65 536
    assert scan(S=4, W=1, max_clips=64) == -2
    err = lib.vfr_last_error()
    assert b"82896 bytes" in err and b"65536" in err, err
    # S = 2 at 64 clips fits with the widest grid: 4 x 140 + 256 x 64 x 3 (+ 16 x 16 x 4 with four rank keys) = 49 712 (50 736)
    assert scan(S=2, W=16, max_clips=64) == 0
    assert scan(S=3, W=1, max_clips=51) == 0 and scan(S=3, W=1, max_clips=64) == -2
    assert lib.vfr_version() == 100
