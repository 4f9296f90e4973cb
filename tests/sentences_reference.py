"""The contract of sentence retrieval for moments (include/vfr.h vfr_score_sentences_f32) as a plain numpy statement on dense
moment scores, shared by the host and the GPU tests: column ``moment_offsets[v] + local id(s, e)`` of the [Ns, sum M] matrix
``score_moments(S, V, off)`` (the sentences as the queries) is the probe's score vector."""
import numpy as np
import torch


def local_id(n, s, e):
    """Position of span (s, e) in utils.generate_moments(n) order."""
    return s if s == e else n + (s * (2 * n - s - 1)) // 2 + (e - s - 1)


def dense_blocks(Sc, counts):
    """Dense [Ns, sum M] scores -> block(v) = the [Ns, M_v] columns of local video v."""
    counts = np.asarray(counts, np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    return lambda v: Sc[:, mo[v]:mo[v + 1]]


def sliced_blocks(score_moments, S, V, off):
    """The same columns without the whole matrix: one video's [Ns, M_v] block per call of the dense scorer (cached)."""
    off = np.asarray(off, np.int64)
    cache = {}

    def block(v):
        if v not in cache:
            cache[v] = score_moments(S, V[off[v]:off[v + 1]], np.asarray([0, off[v + 1] - off[v]], np.int32))
        return cache[v]
    return block


def probe_keys(block, counts, probes, Ns, vid_base=0, sent_base=0):
    """Per probe its uint64 keys over the sentences ((fp32 bits << 32) | sentence id), or None for a probe that is skipped
    (video of another shard) or bad; and the bad flag."""
    counts = np.asarray(counts, np.int64)
    ids = np.uint64(sent_base) + np.arange(Ns, dtype=np.uint64)
    out, bad = [], 0
    for gv, s, e in np.asarray(probes, np.int64).reshape(-1, 3).tolist():
        wrong = gv < 0 or s < 0 or e < s
        lv = gv - vid_base
        owned = gv >= 0 and 0 <= lv < len(counts)
        if owned and e >= counts[lv]:
            wrong = True
        bad |= int(wrong)
        if wrong or not owned:
            out.append(None)
            continue
        col = np.ascontiguousarray(block(lv)[:, local_id(int(counts[lv]), s, e)], np.float32)
        out.append((col.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids)
    return out, bad


def statement(block, counts, probes, Ns, k, vid_base=0, sent_base=0, rank_keys=None):
    """The contract in numpy: per probe the k smallest keys padded with (+inf, -1), the keys strictly below each rank key, and
    whether any probe is malformed."""
    keys, bad = probe_keys(block, counts, probes, Ns, vid_base, sent_base)
    Nm = len(keys)
    od = np.full((Nm, k), np.inf, np.float32)
    oi = np.full((Nm, k), -1, np.int64)
    R = 0 if rank_keys is None else rank_keys.shape[0]
    cnt = np.zeros((R, Nm), np.int64)
    for m, kk in enumerate(keys):
        if kk is None:
            continue
        for r in range(R):
            cnt[r, m] = int((kk < np.uint64(rank_keys[r, m])).sum())
        srt = np.sort(kk)[:k]
        od[m, :len(srt)] = (srt >> np.uint64(32)).astype(np.uint32).view(np.float32)
        oi[m, :len(srt)] = (srt & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return od, oi, cnt, bad


def rank_keys_for(keys, rs, R):
    """R rank keys per probe taken from real (probe, sentence) keys; for r = 3 a key that falls between two scores (id part
    0x7FFFFFFF).  Probes without keys get (+inf, 0)."""
    Nm = len(keys)
    rk = np.full((R, Nm), np.uint64(0x7F800000) << np.uint64(32), np.uint64)
    for m, kk in enumerate(keys):
        if kk is None or len(kk) == 0:
            continue
        rk[:, m] = kk[rs.randint(0, len(kk), R)]
    if R > 3:
        rk[3] = (rk[3] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0x7FFFFFFF)
    return rk


def split_keys(rk):
    """uint64 rank keys [R, Nm] -> (rank_dist fp32, rank_idx int64) tensors."""
    d = (rk >> np.uint64(32)).astype(np.uint32).view(np.float32)
    i = (rk & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return torch.from_numpy(d.copy()), torch.from_numpy(i)


def all_moments(n):
    """Every (s, e) of an n-clip video in utils.generate_moments order."""
    return [(s, s) for s in range(n)] + [(s, e) for s in range(n) for e in range(s + 1, n)]
