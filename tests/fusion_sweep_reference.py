"""The contract of the fusion weight sweep (include/vfr.h vfr_score_fusion_sweep_f32 / vfr_score_fusion_sweep_own_f32) on top of
tests/fusion_reference.py: per row w of the grid the sweep's numbers are those of the single-weight statement at w.  Shared by the
host and the GPU tests: stream generators, per-weight rank keys and the per-row statement."""
import numpy as np

from fusion_reference import fused_scores, level_keys, own_rows, split_keys, statement

GRID5 = ((1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.7, 0.3), (0.3, 0.7))
# (column multiplier, column offset, added to the key): keys 0 and 2 are present in the bank; keys 1 and 3 are a present key + 1 =
# the same score with the next id, which sorts strictly after that key and at or before every later one
_PICKS = ((7, 0, 0), (5, 2, 1), (11, 3, 0), (13, 5, 1))


def streams(counts, dims=(100, 100), seed=0, nq=11, same=(), repeat=()):
    """Random clip rows and queries per stream (as tests/test_fusion_gpu.py builds them); ``same`` = pairs of equally long videos
    given identical rows in EVERY stream, ``repeat`` = videos whose clips are all alike."""
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
    """Clip counts 1 .. 21 with 21 first and last."""
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = 21
    c[-1] = 21
    return c


def fused_grid(Scs, counts, grid):
    """The fused moment scores [Nq, sum M] of the single-weight statement, one per row of the grid (the expensive part: once
    for both levels)."""
    return [fused_scores(Scs, counts, w) for w in grid]


def grid_keys(Fs, counts, level, id_base=0):
    """Per row of the grid (``fused_grid``) the keys [Nq, M] (moments) or best keys [Nq, videos] of the statement."""
    return [level_keys(F, counts, level, id_base) for F in Fs]


def rank_keys(keys, num_rank=2):
    """Per-weight rank keys [W, num_rank, Nq] uint64 from the reference's own keys (``grid_keys``): a key present in the bank, a key
    strictly after a present one, and the same again from other columns."""
    out = []
    for K in keys:
        nq, m = K.shape
        q = np.arange(nq)
        if m == 0:
            rows = [np.full(nq, 5, np.uint64), np.full(nq, (0x3F800000 << 32) | 7, np.uint64)] * 2
        else:
            rows = [K[q, (q * a + b) % m] + np.uint64(plus) for a, b, plus in _PICKS]
        out.append(np.stack(rows[:num_rank]))
    return np.stack(out)


def counts_of(keys, rk):
    """[W, R, Nq] int64: the keys that sort strictly before each rank key -- the count of ``fusion_reference.statement``."""
    return np.stack([(K[None, :, :] < np.asarray(r, np.uint64)[:, :, None]).sum(-1).astype(np.int64) for K, r in zip(keys, rk)])


def sweep_statement(Scs, counts, grid, level, id_base, rk):
    """[W, R, Nq]: ``fusion_reference.statement`` (k = 0) row by row."""
    return np.stack([statement(Scs, counts, w, 0, level, id_base, rk[i])[2] for i, w in enumerate(grid)])


def sweep_own_rows(Scs, counts, grid, own):
    """[W, Nq, Mmax]: ``fusion_reference.own_rows`` row by row."""
    return np.stack([own_rows(Scs, counts, w, own) for w in grid])


__all__ = ["GRID5", "streams", "mixed_counts", "fused_grid", "grid_keys", "rank_keys", "counts_of", "sweep_statement", "sweep_own_rows", "split_keys"]
