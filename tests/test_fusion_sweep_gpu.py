"""The fusion weight sweep on the GPU (vfr_score_fusion_sweep_f32, vfr_score_fusion_sweep_own_f32, engine.corpus_fusion_sweep,
evaluate.sweep_fusion): per row of the grid bit for bit the numpy statement of tests/fusion_reference.py on the oracle's dense
moment scores AND the device's own single-weight calls."""
import numpy as np
import pytest
import torch

from fusion_reference import fused_scores, moment_offsets
from fusion_sweep_reference import GRID5, counts_of, fused_grid, grid_keys, mixed_counts, rank_keys, split_keys, streams, sweep_own_rows
from helpers import MemoryDataset, make_model, problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ("moments", "videos")
DIMS4 = (100, 37, 4, 100)


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def dense(oracle, Qs, Vs, off):
    return [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]


def banks_of(vfr, Vs, off, id_base=0):
    off_t = dev(off)
    return [vfr.VideoBank(dev(V), off_t, id_base) for V in Vs]


def rank_tensors(rk):
    rd, ri = split_keys(rk)
    return dev(rd.reshape(rk.shape)), dev(ri.reshape(rk.shape))


def check(vfr, Scs, Qs, Vs, counts, off, grid=GRID5, levels=LEVELS, id_base=0, num_rank=2, single=True, what=""):
    """Sweep counts == statement per row == (``single``) the device's score_fusion(k = 0) per row."""
    banks = banks_of(vfr, Vs, off, id_base)
    Qd = [dev(Q) for Q in Qs]
    Fs = fused_grid(Scs, counts, grid)
    for level in levels:
        keys = grid_keys(Fs, counts, level, id_base)
        rk = rank_keys(keys, num_rank)
        want = counts_of(keys, rk)
        rd, ri = rank_tensors(rk)
        got = vfr.score_fusion_sweep(Qd, banks, grid, level, rd, ri)
        torch.cuda.synchronize()
        assert got.shape == want.shape and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want), f"{what}: counts differ from the statement ({level})"
        if single:
            for w in range(len(grid)):
                one = vfr.score_fusion(Qd, banks, grid[w], 0, level, rd[w].contiguous(), ri[w].contiguous())[2]
                assert torch.equal(got[w], one), f"{what}: counts differ from score_fusion at row {w} ({level})"
    return banks, Qd


@pytest.mark.parametrize("nv", [1, 64, 65, 130])
def test_block_edges(vfr, oracle, nv):
    """Banks that end on, before and after a block of 64 videos; clip counts mixed 1..21 with 21 first and last; two rank keys."""
    Qs, Vs, counts, off = streams(mixed_counts(nv, nv), seed=nv)
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, what=f"Nv = {nv}")


@pytest.mark.parametrize("W", [1, 16, 17])
def test_grid_sizes(vfr, oracle, W):
    """One row, a full launch of 16 rows, and 17 rows through the wrapper's split into 16 + 1."""
    from vfr_amd import engine
    grid = np.asarray([(0.7, 0.3)], np.float32) if W == 1 else engine.simplex_grid(2, W - 1)
    assert len(grid) == W
    Qs, Vs, counts, off = streams(mixed_counts(70, 20 + W), (100, 37), seed=20 + W)
    Scs = dense(oracle, Qs, Vs, off)
    banks, Qd = check(vfr, Scs, Qs, Vs, counts, off, grid, what=f"W = {W}")
    own = (np.arange(len(Qs[0])) * 13) % len(counts)
    rows = vfr.score_fusion_sweep_own(Qd, banks, grid, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), sweep_own_rows(Scs, counts, grid, own))


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_stream_shapes(vfr, oracle, S):
    """1..4 streams of widths 100 (16-byte loads), 37 (scalar loop), 4, 100."""
    grid = np.asarray([(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (0.7, 0.3, 0.125, 2.0), (0.3, 0.7, 0.6, 0.4)], np.float32)[:, :S]
    Qs, Vs, counts, off = streams(mixed_counts(70, 40 + S), DIMS4[:S], seed=40 + S)
    Scs = dense(oracle, Qs, Vs, off)
    banks, Qd = check(vfr, Scs, Qs, Vs, counts, off, grid, what=f"S = {S}")
    own = (np.arange(len(Qs[0])) * 7) % len(counts)
    rows = vfr.score_fusion_sweep_own(Qd, banks, grid, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), sweep_own_rows(Scs, counts, grid, own))
    for w in range(len(grid)):
        assert torch.equal(rows[w], vfr.score_fusion_own(Qd, banks, grid[w], dev(own.astype(np.int32))))


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_rank_key_counts(vfr, oracle, R):
    Qs, Vs, counts, off = streams(mixed_counts(70, 50), (100, 37), seed=50)
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, num_rank=R, what=f"num_rank = {R}")


def test_counts_are_added_and_shards_chain(vfr, oracle):
    """Counts go ON TOP of a preset tensor; the bank sliced at video 70 into two shards (id_base = 1000) chains to the unsharded
    call's counts."""
    Qs, Vs, counts, off = streams(mixed_counts(130, 51), (100, 37), seed=51)
    Scs = dense(oracle, Qs, Vs, off)
    banks, Qd = check(vfr, Scs, Qs, Vs, counts, off, id_base=1000, what="id_base")
    parts = [[vfr.slice_bank(b, counts, a, z) for b in banks] for a, z in ((0, 70), (70, 130))]
    Fs = fused_grid(Scs, counts, GRID5)
    for level in LEVELS:
        keys = grid_keys(Fs, counts, level, 1000)
        rk = rank_keys(keys)
        want = counts_of(keys, rk)
        rd, ri = rank_tensors(rk)
        preset = torch.arange(want.size, dtype=torch.int64, device=DEV).reshape(want.shape) * 3 + 1
        got = vfr.score_fusion_sweep(Qd, banks, GRID5, level, rd, ri, count_lt=preset.clone())
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want + preset.cpu().numpy()), level
        cnt = None
        for sub in parts:
            cnt = vfr.score_fusion_sweep(Qd, sub, GRID5, level, rd, ri, count_lt=cnt)
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), want), level


def test_long_videos(vfr, oracle):
    """64-clip videos among short ones at S = 2: 64 rows per column block, triangles of 2080 moments."""
    counts = np.concatenate([[64, 3, 21, 64, 1, 40], np.random.RandomState(9).randint(1, 65, 10)])
    Qs, Vs, counts, off = streams(counts, seed=9)
    Scs = dense(oracle, Qs, Vs, off)
    banks, Qd = check(vfr, Scs, Qs, Vs, counts, off, what="long videos")
    own = np.asarray([0, 3, 1, 4, 5, 2, 15, 0, 3, 9, 10], np.int64)
    rows = vfr.score_fusion_sweep_own(Qd, banks, GRID5, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), sweep_own_rows(Scs, counts, GRID5, own))


def test_chunks_of_several_blocks(vfr, oracle):
    """1 100 queries x 1 100 videos of 1..6 clips (the shape of test_fusion_gpu.py::test_chunks_of_several_blocks): the plan cuts the
    video axis into 4 chunks of 5 blocks, so a wave carries its per-(weight, rank) totals over five blocks."""
    rs = np.random.RandomState(88)
    counts = rs.randint(1, 7, 1100).astype(np.int64)
    counts[[0, 319, 320, -1]] = 6
    Qs, Vs, counts, off = streams(counts, (100, 37), seed=88, nq=1100)
    assert vfr.lib().vfr_score_fusion_workspace_bytes(1100, 1100, 100) == 4 * 1100 * 100 * 8 + 256      # 4 chunks: 320 videos each
    check(vfr, dense(oracle, Qs, Vs, off), Qs, Vs, counts, off, what="chunks of several blocks")


def test_ties(vfr, oracle):
    """Two pairs of identical videos and videos of identical clips; rank keys 0 and 2 equal a present key (of a tied moment for
    some queries): 'strictly before' and the id order decide."""
    counts = mixed_counts(70, 12)
    counts[[5, 6, 63, 64]] = (8, 8, 13, 13)
    Qs, Vs, counts, off = streams(counts, seed=12, same=((5, 6), (63, 64)), repeat=(0, 20, 69))
    Scs = dense(oracle, Qs, Vs, off)
    mo = moment_offsets(counts)
    F = fused_scores(Scs, counts, GRID5[3])
    assert np.array_equal(F[:, mo[5]:mo[6]], F[:, mo[6]:mo[7]]) and np.array_equal(F[:, mo[63]:mo[64]], F[:, mo[64]:mo[65]])
    check(vfr, Scs, Qs, Vs, counts, off, num_rank=4, what="ties")
    # rank keys that ARE tied keys: both copies of a moment of videos 5 / 6 and one of the all-alike video 20, for every query
    banks, Qd = banks_of(vfr, Vs, off), [dev(Q) for Q in Qs]
    Fs = fused_grid(Scs, counts, GRID5)
    for level in LEVELS:
        keys = grid_keys(Fs, counts, level)
        cols = (mo[5] + 3, mo[6] + 3, mo[20] + 1) if level == "moments" else (5, 6, 20)
        rk = np.stack([np.stack([K[:, c] for c in cols]) for K in keys])
        got = vfr.score_fusion_sweep(Qd, banks, GRID5, level, *rank_tensors(rk))
        torch.cuda.synchronize()
        want = counts_of(keys, rk)
        assert np.array_equal(got.cpu().numpy(), want), level
        if level == "moments":
            assert np.all(want[:, 1] > want[:, 0])           # the copy with the higher id sorts after its twin


@pytest.mark.parametrize("nq", [0, 1, 65])
def test_query_counts(vfr, oracle, nq):
    Qs, Vs, counts, off = streams([3, 1, 2, 4], seed=nq, nq=nq)
    banks, Qd = banks_of(vfr, Vs, off), [dev(Q) for Q in Qs]
    own = dev((np.arange(nq) % 4).astype(np.int32))
    if nq == 0:
        z = torch.zeros((5, 2, 0), device=DEV)
        assert vfr.score_fusion_sweep(Qd, banks, GRID5, "moments", z, z.long()).shape == (5, 2, 0)
        assert vfr.score_fusion_sweep_own(Qd, banks, GRID5, own).shape == (5, 0, 10)
        return
    Scs = dense(oracle, Qs, Vs, off)
    check(vfr, Scs, Qs, Vs, counts, off, what=f"Nq = {nq}")
    rows = vfr.score_fusion_sweep_own(Qd, banks, GRID5, own)
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), sweep_own_rows(Scs, counts, GRID5, own.cpu().numpy()))


def test_empty_bank_and_own_outside(vfr, oracle):
    Qn = [np.random.RandomState(1).randn(11, D).astype(np.float32) for D in (100, 37)]
    off_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    banks = [vfr.VideoBank(torch.zeros((0, D), dtype=torch.float32, device=DEV), off_t, 4) for D in (100, 37)]
    rk = np.tile(np.asarray((0x3F800000 << 32) | 7, np.uint64), (5, 2, 11))
    for level in LEVELS:
        preset = torch.full((5, 2, 11), 9, dtype=torch.int64, device=DEV)
        got = vfr.score_fusion_sweep([dev(Q) for Q in Qn], banks, GRID5, level, *rank_tensors(rk), count_lt=preset)
        torch.cuda.synchronize()
        assert torch.all(got == 9)
    # an own video outside [0, Nv): the row is all +inf, for every weight; the others are the statement's
    Qs, Vs, counts, off = streams([3, 1, 2, 4], seed=5, nq=6)
    Scs = dense(oracle, Qs, Vs, off)
    own = np.asarray([0, -1, 3, 4, 2, 1000], np.int64)
    rows = vfr.score_fusion_sweep_own([dev(Q) for Q in Qs], banks_of(vfr, Vs, off), GRID5, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    inside = (own >= 0) & (own < 4)
    assert rows.shape == (5, 6, 10) and np.all(np.isinf(rows[:, ~inside])) and np.all(rows[:, ~inside] > 0)
    assert np.array_equal(rows[:, inside], sweep_own_rows([Sc[inside] for Sc in Scs], counts, GRID5, own[inside]))


def test_own_rows_feed_the_rank_keys(vfr, oracle):
    """sweep_own rows -> gt_rank_keys -> sweep reproduce, per row of the grid, the rank of the best positive moment in the dense
    (score, id) argsort."""
    counts = mixed_counts(130, 31)
    counts[[63, 64]] = (15, 9)
    Qs, Vs, counts, off = streams(counts, seed=31)
    Scs = dense(oracle, Qs, Vs, off)
    nq = len(Qs[0])
    own = np.asarray([0, 129, 63, 64, 1, 128, 62, 65, 17, 99, 64], np.int64)[:nq]
    banks = banks_of(vfr, Vs, off, 6)
    Qd = [dev(Q) for Q in Qs]
    rows = vfr.score_fusion_sweep_own(Qd, banks, GRID5, dev(own.astype(np.int32)))
    torch.cuda.synchronize()
    want = sweep_own_rows(Scs, counts, GRID5, own)
    assert np.array_equal(rows.cpu().numpy(), want)
    rs = np.random.RandomState(32)
    labels = np.zeros((2, nq, want.shape[2]), bool)
    for q in range(nq):
        M = int(counts[own[q]] * (counts[own[q]] + 1) // 2)
        labels[0, q, rs.randint(0, M, 3)] = True
        labels[1, q, rs.randint(0, M)] = True
    mo = moment_offsets(counts)
    keys = [vfr.gt_rank_keys(rows[w], dev(labels), dev(6 + mo[own]), dev(np.arange(nq, dtype=np.int64)), nq) for w in range(len(GRID5))]
    assert all(int(k[4].item()) == 0 for k in keys)
    rd, ri, cnt0 = (torch.stack([k[i] for k in keys]) for i in (1, 2, 3))
    cnt = vfr.score_fusion_sweep(Qd, banks, GRID5, "moments", rd, ri, count_lt=cnt0).cpu().numpy()
    for w, wv in enumerate(GRID5):
        F = fused_scores(Scs, counts, wv)
        for q in range(nq):
            order = np.argsort(F[q], kind="stable")                          # the dense (score, id) order
            where = np.empty_like(order)
            where[order] = np.arange(len(order))
            for r in range(2):
                assert int(cnt[w, r, q]) == int(where[mo[own[q]] + np.nonzero(labels[r, q])[0]].min()), (w, r, q)


def test_sweep_fusion_gpu_equals_cpu():
    """Two differently seeded models on the 40-video, 30-query problem: the metric dicts and ``best`` of cuda:0 equal the CPU
    device's."""
    from vfr_amd import engine
    from vfr_amd import evaluate as vevaluate
    ps = [problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=123)]
    ps.append(dict(ps[0], sd=problem(40, 30, "didemo", feat_dim=64, hidden=16, seed=321)["sd"]))
    grid = engine.simplex_grid(2, 5)
    res = {}
    for device in ("cpu", DEV):
        for level, select in (("moments", ("model, IoU=0.5", "R@10")), ("videos", ("video", "MR"))):
            dss = [MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"]) for p in ps]
            models = [make_model(p["sd"], feat_dim=64, hidden=16).to(device) for p in ps]
            its = [d.iterators() for d in dss]
            res[(device, level)] = vevaluate.sweep_fusion(models, [x[0] for x in its], [x[1] for x in its], dss[0].annotations, device,
                                                          grid, level=level, select=select)
    for level in LEVELS:
        assert res[("cpu", level)] == res[(DEV, level)], level
        assert res[(DEV, level)][1] is not None and len(res[(DEV, level)][0]) == len(grid)
