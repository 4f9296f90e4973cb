"""The contract of video-to-sentence retrieval (include/vfr.h vfr_score_video_sentences_f32) as a plain numpy statement on dense
moment scores, shared by the host and the GPU tests: score(p, j) is the minimum of row j over the block of video v_p of the
[Ns, sum M] matrix ``score_moments(S, V, off)`` (the sentences as the queries), and m(j, v_p) is the first column that attains it
(columns are in utils.generate_moments order, so the first one is the smallest moment id)."""
import numpy as np

from sentences_reference import dense_blocks, sliced_blocks, split_keys  # noqa: F401  (re-exported for the tests)


def video_best(block, lv):
    """Local video lv -> (best [Ns] fp32 = the row-wise minimum of its block, arg [Ns] = its first argmin)."""
    b = np.ascontiguousarray(block(lv), np.float32)
    arg = b.argmin(axis=1)
    return b[np.arange(b.shape[0]), arg], arg


def probe_keys(block, counts, videos, Ns, vid_base=0, sent_base=0):
    """Per probe its uint64 keys over the sentences ((fp32 bits of b(j, v) << 32) | sentence id) and the local position of
    m(j, v) per sentence, or (None, None) for a probe that is skipped (video of another shard, video without clips) or bad (video
    < 0); and the bad flag."""
    counts = np.asarray(counts, np.int64)
    ids = np.uint64(sent_base) + np.arange(Ns, dtype=np.uint64)
    keys, args, bad, cache = [], [], 0, {}
    for gv in np.asarray(videos, np.int64).reshape(-1).tolist():
        lv = gv - vid_base
        if gv < 0:
            bad = 1
        if gv < 0 or lv < 0 or lv >= len(counts) or counts[lv] == 0 or Ns == 0:
            keys.append(None)
            args.append(None)
            continue
        if lv not in cache:
            cache[lv] = video_best(block, lv)
        best, arg = cache[lv]
        keys.append((best.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids)
        args.append(arg)
    return keys, args, bad


def statement(block, counts, videos, Ns, k, vid_base=0, sent_base=0, rank_keys=None, ground=False, id_base=0):
    """The contract in numpy: per probe the k smallest keys padded with (+inf, -1), the keys strictly below each rank key, whether
    any probe is malformed, and (``ground``) the global moment id m(j, v_p) of every listed sentence (-1 for padding):
    ``id_base`` + the video's moment offset + the first argmin of its block."""
    counts = np.asarray(counts, np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    keys, args, bad = probe_keys(block, counts, videos, Ns, vid_base, sent_base)
    vids = np.asarray(videos, np.int64).reshape(-1)
    Np = len(keys)
    od = np.full((Np, k), np.inf, np.float32)
    oi = np.full((Np, k), -1, np.int64)
    om = np.full((Np, k), -1, np.int64)
    R = 0 if rank_keys is None else rank_keys.shape[0]
    cnt = np.zeros((R, Np), np.int64)
    for p, kk in enumerate(keys):
        if kk is None:
            continue
        for r in range(R):
            cnt[r, p] = int((kk < np.uint64(rank_keys[r, p])).sum())
        order = np.argsort(kk, kind="stable")[:k]
        srt = kk[order]
        od[p, :len(srt)] = (srt >> np.uint64(32)).astype(np.uint32).view(np.float32)
        oi[p, :len(srt)] = (srt & np.uint64(0xFFFFFFFF)).astype(np.int64)
        om[p, :len(srt)] = id_base + mo[vids[p] - vid_base] + args[p][order]
    if ground:
        return od, oi, cnt, bad, om
    return od, oi, cnt, bad


def rank_keys_for(keys, rs, R):
    """R rank keys per probe taken from real (probe, sentence) keys; for r = 3 a key that falls between two scores (id part
    0x7FFFFFFF).  Probes without keys get (+inf, 0)."""
    Np = len(keys)
    rk = np.full((R, Np), np.uint64(0x7F800000) << np.uint64(32), np.uint64)
    for p, kk in enumerate(keys):
        if kk is None or len(kk) == 0:
            continue
        rk[:, p] = kk[rs.randint(0, len(kk), R)]
    if R > 3:
        rk[3] = (rk[3] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0x7FFFFFFF)
    return rk


def own_ranks(keys, own_off, own_rows):
    """0-based rank per probe of its best-ranked own sentence: the keys strictly before the smallest own key; -1 without own rows,
    0 for a probe without keys."""
    out = np.zeros(len(keys), np.int64)
    for p, kk in enumerate(keys):
        rows = np.asarray(own_rows[own_off[p]:own_off[p + 1]], np.int64)
        if len(rows) == 0:
            out[p] = -1
        elif kk is not None:
            out[p] = int((kk < kk[rows].min()).sum())
    return out
