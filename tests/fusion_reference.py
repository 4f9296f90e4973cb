"""The contract of late-fusion retrieval (include/vfr.h vfr_score_fusion_f32 / vfr_score_fusion_own_f32) as a plain numpy statement
on the oracle's dense moment scores, shared by the host and the GPU tests.  Per stream ``Sc_s = oracle.score_moments(Q_s, V_s, off)``;
the stream's clip distances are the single-clip columns of ``Sc_s`` (moment (c, c) of an n-clip video is column c of its block);
they are fused with separate float32 multiplies and adds, and the moment chain -- sequential float32 sum s -> e, one float32
division -- is rebuilt on the fused distances."""
import numpy as np

LEVELS = ("moments", "videos")
KEY_EMPTY = np.uint64(0x7F800000FFFFFFFF)


def all_moments(n):
    """Every (s, e) of an n-clip video in utils.generate_moments order."""
    return [(s, s) for s in range(n)] + [(s, e) for s in range(n) for e in range(s + 1, n)]


def moment_offsets(counts):
    counts = np.asarray(counts, np.int64)
    return np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])


def clip_distances(Sc, counts):
    """[Nq, total_clips] clip distances of one stream: the single-clip columns of its dense moment scores."""
    counts = np.asarray(counts, np.int64)
    mo = moment_offsets(counts)
    cols = np.concatenate([mo[v] + np.arange(counts[v]) for v in range(len(counts))]) if len(counts) else np.zeros(0, np.int64)
    return np.ascontiguousarray(np.asarray(Sc, np.float32)[:, cols.astype(np.int64)])


def fuse(dists, weights):
    """f = fl(w_0 d_0); f = fl(f + fl(w_s d_s)): float32, every operation rounded."""
    f = None
    for d, w in zip(dists, weights):
        t = np.multiply(np.float32(w), np.asarray(d, np.float32), dtype=np.float32)
        f = t if f is None else np.add(f, t, dtype=np.float32)
    return f


def fused_scores(Scs, counts, weights):
    """[Nq, sum M] fused moment scores in global moment order."""
    counts = np.asarray(counts, np.int64)
    f = fuse([clip_distances(Sc, counts) for Sc in Scs], weights)
    off = np.concatenate([[0], np.cumsum(counts)])
    mo = moment_offsets(counts)
    out = np.empty((f.shape[0], int(mo[-1])), np.float32)
    for n in np.unique(counts):                               # the videos of one length together: the same chain, element-wise
        vids = np.nonzero(counts == n)[0]
        fv = f[:, off[vids][:, None] + np.arange(n)[None, :]]                     # [Nq, videos, n]
        for j, (s, e) in enumerate(all_moments(int(n))):
            acc = fv[:, :, s].copy()
            for c in range(s + 1, e + 1):
                acc = np.add(acc, fv[:, :, c], dtype=np.float32)
            out[:, mo[vids] + j] = np.divide(acc, np.float32(e - s + 1), dtype=np.float32)
    return out


def keys_of(sc, ids):
    return (np.ascontiguousarray(sc, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def split_keys(keys):
    """packed keys -> (float32 scores, int64 ids)."""
    keys = np.asarray(keys, np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def level_keys(F, counts, level, id_base=0):
    """[Nq, M] keys of every moment, or [Nq, videos with clips] best keys of the videos."""
    assert level in LEVELS
    K = keys_of(F, id_base + np.arange(F.shape[1], dtype=np.int64)[None, :].repeat(F.shape[0], 0))
    if level == "moments":
        return K
    mo = moment_offsets(counts)
    best = [K[:, mo[v]:mo[v + 1]].min(axis=1) for v in range(len(counts)) if mo[v + 1] > mo[v]]
    return np.stack(best, axis=1) if best else np.zeros((F.shape[0], 0), np.uint64)


def statement(Scs, counts, weights, k, level="moments", id_base=0, rank_keys=None):
    """vfr_score_fusion_f32 on one shard: (dist [Nq, k], idx [Nq, k], counts [R, Nq] | None = what the call ADDS)."""
    F = fused_scores(Scs, counts, weights)
    K = level_keys(F, counts, level, id_base)
    Nq = F.shape[0]
    srt = np.sort(K, axis=1)[:, :k]
    d, i = np.full((Nq, k), np.inf, np.float32), np.full((Nq, k), -1, np.int64)
    if srt.shape[1]:
        d[:, :srt.shape[1]], i[:, :srt.shape[1]] = split_keys(srt)
    cnt = None
    if rank_keys is not None:
        rk = np.asarray(rank_keys, np.uint64).reshape(-1, Nq)
        cnt = (K[None, :, :] < rk[:, :, None]).sum(-1).astype(np.int64)
    return d, i, cnt


def own_rows(Scs, counts, weights, own):
    """vfr_score_fusion_own_f32: [Nq, Mmax] fused scores of each query's own (local) video, tail +inf."""
    counts = np.asarray(counts, np.int64)
    F = fused_scores(Scs, counts, weights)
    mo = moment_offsets(counts)
    nmax = int(counts.max()) if len(counts) else 0
    out = np.full((F.shape[0], nmax * (nmax + 1) // 2), np.inf, np.float32)
    for q, v in enumerate(np.asarray(own, np.int64)):
        out[q, :mo[v + 1] - mo[v]] = F[q, mo[v]:mo[v + 1]]
    return out
