"""The contract of windowed retrieval (include/vfr.h vfr_score_window_f32 / vfr_score_window_span_keys_f32) as a plain numpy statement
on the oracle's dense moment scores ``Sc = oracle.score_moments(Q, V, off)`` (canonical ids: column m of ``Sc`` is global moment m),
shared by the host and the GPU tests.  The candidates of a window ``max_len = L`` are the columns whose span is at most L clips long;
the span of every column comes from a table in utils.generate_moments order that is built arithmetically."""
import numpy as np

from fusion_reference import keys_of, moment_offsets, split_keys

KEY_EMPTY = np.uint64(0x7F800000FFFFFFFF)


def spans_of(n):
    """int64 [n (n + 1) / 2, 2]: (start, end) of an n-clip video in utils.generate_moments order -- the n single clips, then per
    start the ends after it."""
    s, e = np.triu_indices(int(n), 1)
    one = np.arange(int(n), dtype=np.int64)
    return np.concatenate([np.stack([one, one], 1), np.stack([s, e], 1).astype(np.int64)])


def bank_spans(counts):
    """int64 [sum M, 3]: (video, start, end) of every global moment of the bank."""
    rows = [np.concatenate([np.full((int(n) * (int(n) + 1) // 2, 1), v, np.int64), spans_of(n)], axis=1) for v, n in enumerate(counts)]
    return np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)


def moment_index(n, s, e):
    return s if s == e else n + (s * (2 * n - s - 1)) // 2 + (e - s - 1)


def window_keys(Sc, counts, L, id_base=0):
    """uint64 [Nq, candidates]: the keys (score, id_base + column) of the columns whose span has at most L clips."""
    sp = bank_spans(counts)
    cols = np.nonzero(sp[:, 2] - sp[:, 1] + 1 <= L)[0]
    Sc = np.asarray(Sc, np.float32)
    return keys_of(Sc[:, cols], (id_base + cols)[None, :].repeat(Sc.shape[0], 0))


def statement(Sc, counts, L, k, id_base=0, rank_keys=None):
    """vfr_score_window_f32 on one shard: (dist [Nq, k], idx [Nq, k], counts [R, Nq] | None = what the call ADDS)."""
    K = window_keys(Sc, counts, L, id_base)
    Nq = K.shape[0]
    srt = np.sort(K, axis=1)[:, :k]
    d, i = np.full((Nq, k), np.inf, np.float32), np.full((Nq, k), -1, np.int64)
    if srt.shape[1]:
        d[:, :srt.shape[1]], i[:, :srt.shape[1]] = split_keys(srt)
    cnt = None
    if rank_keys is not None:
        rk = np.asarray(rank_keys, np.uint64).reshape(-1, Nq)
        cnt = (K[None, :, :] < rk[:, :, None]).sum(-1).astype(np.int64)
    return d, i, cnt


def rank_keys(Sc, counts, L, id_base=0):
    """Four rank keys per query from the reference's own candidate keys: the first, a middle one, the last, and one absent key (a
    present key + 1: strictly between two keys).  Without candidates: arbitrary keys."""
    K = np.sort(window_keys(Sc, counts, L, id_base), axis=1)
    nq, m = K.shape
    if m == 0:
        return np.stack([np.full(nq, 5, np.uint64), np.full(nq, (0x3F800000 << 32) | 7, np.uint64)] * 2)
    q = np.arange(nq)
    return np.stack([K[:, 0], K[q, (q * 7 + m // 2) % m], K[:, m - 1], K[q, (q * 5 + 2) % m] + np.uint64(1)])


def span_keys(Sc, counts, items, id_base=0, vid_base=0):
    """vfr_score_window_span_keys_f32 on one shard (``Sc`` / ``counts`` of the shard's videos, which are the corpus's videos
    vid_base ..): (keys uint64 [Np] with KEY_EMPTY where the call leaves the slot untouched, bad flag)."""
    counts = np.asarray(counts, np.int64)
    mo = moment_offsets(counts)
    nq = Sc.shape[0]
    out = np.full(len(items), KEY_EMPTY, np.uint64)
    bad = 0
    for p, (q, gv, s, e) in enumerate(np.asarray(items, np.int64).reshape(-1, 4).tolist()):
        lv = gv - vid_base
        owned = 0 <= lv < len(counts)
        wrong = q < 0 or q >= nq or s < 0 or e < s or e - s + 1 > 64 or (owned and e >= counts[lv])
        if wrong:
            bad = 1
        if wrong or not owned:
            continue
        col = int(mo[lv]) + moment_index(int(counts[lv]), s, e)
        out[p] = keys_of(np.asarray(Sc[q, col], np.float32).reshape(1), np.asarray([id_base + col]))[0]
    return out, bad


def positives_brute(times, counts_own, thresholds, L, strict=True, agree=2):
    """engine.window_positives by the reference's own loop: utils.get_iou of every window with every annotator span."""
    from vfr_amd.utils import get_iou
    out = []
    for thr in thresholds:
        rows = []
        for q, (spans, n) in enumerate(zip(times, counts_own)):
            for s in range(int(n)):
                for e in range(s, min(int(n), s + L)):
                    ious = get_iou(spans, s, e)
                    if int(((ious > thr) if strict else (ious >= thr)).sum()) >= agree:
                        rows.append((q, s, e))
        out.append(np.asarray(rows, np.int32).reshape(-1, 3))
    return out
