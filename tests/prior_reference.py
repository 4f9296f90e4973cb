"""The contract of prior-aware retrieval (include/vfr.h vfr_score_prior_f32 / vfr_score_prior_own_f32) as a plain numpy statement on
the oracle's dense moment scores ``Sc = oracle.score_moments(Q, V, off)``, shared by the host and the GPU tests.  A moment table is
the flat float32 array of its entries: for n = 0 .. max_clips the n (n + 1) / 2 entries of an n-clip video in
utils.generate_moments order.  g = Sc + entry is ONE float32 addition; a moment is a candidate iff g < +inf; an entry that is NaN or
negative excludes its moment."""
import numpy as np

from fusion_reference import all_moments, keys_of, moment_offsets, split_keys

LEVELS = ("moments", "videos")
KEY_EMPTY = np.uint64(0x7F800000FFFFFFFF)


def table_offsets(max_clips):
    """[max_clips + 2]: where the row of n-clip videos starts; the last entry is the number of entries."""
    n = np.arange(max_clips + 1, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(n * (n + 1) // 2)])


def table_row(table, n):
    off = table_offsets(n)
    return np.asarray(table, np.float32)[off[n]:off[n + 1]]


def span_mask(max_clips, keep):
    """A table of zeros where ``keep(n, s, e)`` holds and +inf elsewhere, by brute-force enumeration."""
    return np.asarray([0.0 if keep(n, s, e) else np.inf for n in range(max_clips + 1) for s, e in all_moments(n)], np.float32)


def bias_columns(table, counts):
    """[sum M] the table entry of every moment of the bank, in global moment order."""
    rows = [table_row(table, int(n)) for n in counts]
    return np.concatenate(rows) if rows else np.zeros(0, np.float32)


def biased_scores(Sc, counts, table):
    """[Nq, sum M] g = fl(Sc + entry); +inf where the entry is NaN or < 0."""
    b = bias_columns(table, counts)
    b = np.where(b >= 0, b, np.float32(np.inf)).astype(np.float32)
    return np.add(np.asarray(Sc, np.float32), b[None, :], dtype=np.float32)


def level_keys(G, counts, level, id_base=0):
    """[Nq, M] keys of the moments, or [Nq, videos with clips] best keys of the videos; KEY_EMPTY where there is no candidate."""
    assert level in LEVELS
    K = keys_of(G, id_base + np.arange(G.shape[1], dtype=np.int64)[None, :].repeat(G.shape[0], 0))
    K = np.where(G < np.inf, K, KEY_EMPTY)
    if level == "moments":
        return K
    mo = moment_offsets(counts)
    best = [K[:, mo[v]:mo[v + 1]].min(axis=1) for v in range(len(counts)) if mo[v + 1] > mo[v]]
    return np.stack(best, axis=1) if best else np.zeros((G.shape[0], 0), np.uint64)


def statement(Sc, counts, table, k, level="moments", id_base=0, rank_keys=None):
    """vfr_score_prior_f32 on one shard: (dist [Nq, k], idx [Nq, k], counts [R, Nq] | None = what the call ADDS)."""
    K = level_keys(biased_scores(Sc, counts, table), counts, level, id_base)
    Nq = K.shape[0]
    srt = np.sort(K, axis=1)[:, :k]
    d, i = np.full((Nq, k), np.inf, np.float32), np.full((Nq, k), -1, np.int64)
    if srt.shape[1]:
        sd, si = split_keys(srt)
        real = srt != KEY_EMPTY
        d[:, :srt.shape[1]], i[:, :srt.shape[1]] = np.where(real, sd, np.float32(np.inf)), np.where(real, si, -1)
    cnt = None
    if rank_keys is not None:
        rk = np.asarray(rank_keys, np.uint64).reshape(-1, Nq)
        cnt = ((K[None, :, :] < rk[:, :, None]) & (K != KEY_EMPTY)[None]).sum(-1).astype(np.int64)
    return d, i, cnt


def own_rows(Sc, counts, table, own):
    """vfr_score_prior_own_f32: [Nq, Mmax] biased scores of each query's own (local) video; +inf at excluded moments, in the tail and
    for an own video outside [0, Nv)."""
    counts = np.asarray(counts, np.int64)
    G = biased_scores(Sc, counts, table)
    mo = moment_offsets(counts)
    nmax = int(counts.max()) if len(counts) else 0
    out = np.full((G.shape[0], nmax * (nmax + 1) // 2), np.inf, np.float32)
    for q, v in enumerate(np.asarray(own, np.int64)):
        if 0 <= v < len(counts):
            out[q, :mo[v + 1] - mo[v]] = G[q, mo[v]:mo[v + 1]]
    return out


def rank_keys(Sc, counts, table, level, id_base=0):
    """Two rank keys per query from the reference's own candidate keys: one present in the bank, one strictly between two keys."""
    K = np.sort(level_keys(biased_scores(Sc, counts, table), counts, level, id_base), axis=1)
    nq = K.shape[0]
    m = int((K[0] != KEY_EMPTY).sum()) if nq and K.shape[1] else 0       # the table decides the candidates: the same for every query
    if m == 0:
        return np.stack([np.full(nq, 5, np.uint64), np.full(nq, (0x3F800000 << 32) | 7, np.uint64)])
    return np.stack([K[np.arange(nq), (np.arange(nq) * 7) % m], K[np.arange(nq), (np.arange(nq) * 5 + 2) % m] + np.uint64(1)])
