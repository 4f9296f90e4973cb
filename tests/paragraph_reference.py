"""The contract of paragraph-to-video retrieval (include/vfr.h vfr_score_paragraphs_f32 / vfr_score_paragraph_pairs_f32) as a plain
numpy statement on dense moment scores ``S`` [Nq, sum M] (the oracle's ``score_moments`` with the sentences as the queries), shared
by the host and the GPU tests:

  1. per (sentence, video) the lexicographic minimum of (score, moment id) over the video's segment of ``S``;
  2. per (paragraph, video) the float32 chain of those minima in sentence order, starting from the first, then one float32 division
     by the number of sentences (numpy float32 arithmetic, one video per element: every operation is a single rounded fp32 one);
  3. ``np.lexsort((video, score))``; the rank of a paragraph is the position of its own video."""
import numpy as np


def cycle_lengths(nq, cycle=(1, 2, 3, 5, 8)):
    """Group lengths cycling through ``cycle`` until they cover ``nq`` rows (the last one is cut to fit)."""
    out, left, i = [], nq, 0
    while left > 0:
        n = min(cycle[i % len(cycle)], left)
        out.append(n)
        left -= n
        i += 1
    return np.asarray(out, np.int64)


def best_per_video(S, counts, id_base=0):
    """(b [Nq, Nv] float32, m [Nq, Nv] int64): the lexicographic min of (score, global moment id) per video; (+inf, -1) for a
    video without clips."""
    counts = np.asarray(counts, np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    Nq, Nv = S.shape[0], len(counts)
    b = np.full((Nq, Nv), np.inf, np.float32)
    m = np.full((Nq, Nv), -1, np.int64)
    for v in range(Nv):
        seg = S[:, mo[v]:mo[v + 1]]
        if seg.shape[1] == 0:
            continue
        j = np.argmin(seg, axis=1)                          # the first of equal scores: the smallest id
        b[:, v] = seg[np.arange(Nq), j]
        m[:, v] = id_base + mo[v] + j
    return b, m


def group_scores(b, lengths):
    """[Ng, Nv] float32: the chain b[j0] + b[j0+1] + .. in sentence order and one division by float32(L); +inf for an empty group."""
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)])
    out = np.full((len(lengths), b.shape[1]), np.inf, np.float32)
    for g, L in enumerate(lengths):
        if L == 0:
            continue
        acc = b[off[g]].astype(np.float32)
        for j in range(off[g] + 1, off[g + 1]):
            acc = (acc + b[j]).astype(np.float32)
        out[g] = (acc / np.float32(L)).astype(np.float32)
    return out


def statement(S, counts, lengths, k, own=None, vid_base=0):
    """(score [Ng, k] padded with +inf, global video [Ng, k] padded with -1, ranks [Ng] | None, all scores [Ng, Nv]); ``own`` =
    the GLOBAL index of each paragraph's own video, a video with clips of this bank; an empty paragraph keeps padding and rank 0."""
    counts = np.asarray(counts, np.int64)
    lengths = np.asarray(lengths, np.int64)
    b, _ = best_per_video(S, counts)
    sc = group_scores(b, lengths)
    Ng, Nv = sc.shape
    live = counts > 0
    vids = np.arange(Nv, dtype=np.int64)
    od = np.full((Ng, k), np.inf, np.float32)
    ov = np.full((Ng, k), -1, np.int64)
    ranks = np.zeros(Ng, np.int64) if own is not None else None
    for g in range(Ng):
        if lengths[g] == 0:
            continue
        order = np.lexsort((vids, sc[g]))
        order = order[live[order]]
        n = min(k, len(order))
        od[g, :n], ov[g, :n] = sc[g, order[:n]], vid_base + order[:n]
        if own is not None:
            ranks[g] = int(np.nonzero(order == own[g] - vid_base)[0][0])
    return od, ov, ranks, sc


def pair_statement(S, counts, lengths, pairs, max_len, vid_base=0, id_base=0):
    """(score [Np], moments [Np, max_len]) of the (group, global video) pairs; pairs of other banks keep (+inf, -1)."""
    counts = np.asarray(counts, np.int64)
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)])
    b, m = best_per_video(S, counts, id_base)
    sc = group_scores(b, lengths)
    ps = np.full(len(pairs), np.inf, np.float32)
    pm = np.full((len(pairs), max_len), -1, np.int64)
    for p, (g, gv) in enumerate(np.asarray(pairs, np.int64).tolist()):
        lv = gv - vid_base
        if not 0 <= lv < len(counts) or counts[lv] == 0 or lengths[g] == 0:
            continue
        ps[p] = sc[g, lv]
        pm[p, :lengths[g]] = m[off[g]:off[g + 1], lv]
    return ps, pm
