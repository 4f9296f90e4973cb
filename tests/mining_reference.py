"""The contract of hard-negative mining (include/vfr.h vfr_score_spans_f32 / vfr_mine_negatives_f32) as a plain numpy statement on
dense moment scores, shared by the host and the GPU tests: ``Sc = score_moments(Q, V, off)`` [Nq, sum M] of the bank's own videos;
the score of (query row q, local video v, span (s, e)) is ``Sc[q, moment_offsets[v] + local_id(n_v, s, e)]``."""
import numpy as np

MODES = ("same_length", "any")


def local_id(n, s, e):
    """Position of span (s, e) in utils.generate_moments(n) order."""
    return s if s == e else n + (s * (2 * n - s - 1)) // 2 + (e - s - 1)


def all_moments(n):
    """Every (s, e) of an n-clip video in utils.generate_moments order."""
    return [(s, s) for s in range(n)] + [(s, e) for s in range(n) for e in range(s + 1, n)]


def moment_offsets(counts):
    counts = np.asarray(counts, np.int64)
    return np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])


def check_item(item, counts, Nq, vid_base):
    """(malformed, own local video or -1) of one item on the shard that holds global videos [vid_base, vid_base + len(counts))."""
    q, gv, s, e = (int(x) for x in item)
    wrong = q < 0 or q >= Nq or gv < 0 or s < 0 or e < s
    lv = gv - vid_base
    owned = gv >= 0 and 0 <= lv < len(counts)
    if owned and e >= counts[lv]:
        wrong = True
    return wrong, (lv if owned else -1)


def span_scores(Sc, counts, items, vid_base=0):
    """vfr_score_spans_f32: out [Np] (+inf where the call leaves the pre-filled value) and the bad flag."""
    counts = np.asarray(counts, np.int64)
    mo = moment_offsets(counts)
    items = np.asarray(items, np.int64).reshape(-1, 4)
    out, bad = np.full(len(items), np.inf, np.float32), 0
    for p, it in enumerate(items):
        wrong, lv = check_item(it, counts, Sc.shape[0], vid_base)
        bad |= int(wrong)
        if not wrong and lv >= 0:
            out[p] = Sc[it[0], mo[lv] + local_id(int(counts[lv]), int(it[2]), int(it[3]))]
    return out, bad


def _keys(sc, ids):
    return (np.ascontiguousarray(sc, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def eligible(Sc, counts, item, vid_base=0, id_base=0, mode="same_length", excl=None):
    """(inter scores, inter global videos, intra scores | None, intra global moment ids | None) of a well-formed item: the eligible
    negatives of both kinds on this shard (intra None when the own video lives elsewhere)."""
    counts = np.asarray(counts, np.int64)
    mo = moment_offsets(counts)
    q, gv, s, e = (int(x) for x in item)
    lv = gv - vid_base
    vs = np.asarray([v for v in range(len(counts)) if v != lv and counts[v] >= e + 1], np.int64)
    cols = np.asarray([mo[v] + local_id(int(counts[v]), s, e) for v in vs], np.int64)
    inter = (Sc[q, cols].astype(np.float32), vs + vid_base)
    if not 0 <= lv < len(counts):
        return inter + (None, None)
    n = int(counts[lv])
    gone = {(s, e)}
    if mode == "any" and excl is not None:
        gone |= {(int(a), int(b)) for a, b in np.asarray(excl).reshape(-1, 2)}
    if mode == "same_length":
        loc = [j for j, (s1, e1) in enumerate(all_moments(n)) if e1 - s1 == e - s and (s1, e1) != (s, e)]
    else:
        loc = [j for j, m in enumerate(all_moments(n)) if m not in gone]
    loc = np.asarray(loc, np.int64)
    return inter + (Sc[q, mo[lv] + loc].astype(np.float32), id_base + mo[lv] + loc)


def _select(sc, ids, h, floor, thr):
    """The h smallest (score, id) keys above the floor, padded with (+inf, -1); the eligible scores below thr."""
    below = 0 if thr is None else int((sc < np.float32(thr)).sum())
    if floor is not None:
        keep = ~(sc <= np.float32(floor))
        sc, ids = sc[keep], ids[keep]
    srt = np.sort(_keys(sc, ids))[:h]
    d, i = np.full(h, np.inf, np.float32), np.full(h, -1, np.int64)
    d[:len(srt)] = (srt >> np.uint64(32)).astype(np.uint32).view(np.float32)
    i[:len(srt)] = (srt & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return d, i, below


def statement(Sc, counts, items, h, vid_base=0, id_base=0, mode="same_length", excl=None, floor=None, thr=None):
    """vfr_mine_negatives_f32 on one shard: dict of inter_dist / inter_vid / intra_dist / intra_idx [Nm, h], count_inter /
    count_intra [Nm] (what the call ADDS) and bad.  Intra rows the call leaves untouched hold the pre-filled (+inf, -1)."""
    assert mode in MODES
    counts = np.asarray(counts, np.int64)
    items = np.asarray(items, np.int64).reshape(-1, 4)
    Nm = len(items)
    out = dict(inter_dist=np.full((Nm, h), np.inf, np.float32), inter_vid=np.full((Nm, h), -1, np.int64),
               intra_dist=np.full((Nm, h), np.inf, np.float32), intra_idx=np.full((Nm, h), -1, np.int64),
               count_inter=np.zeros(Nm, np.int64), count_intra=np.zeros(Nm, np.int64), bad=0)
    for m, it in enumerate(items):
        wrong, lv = check_item(it, counts, Sc.shape[0], vid_base)
        out["bad"] |= int(wrong)
        if wrong:
            continue
        fl = None if floor is None else floor[m]
        th = None if thr is None else thr[m]
        sc, vs, isc, iid = eligible(Sc, counts, it, vid_base, id_base, mode, None if excl is None else excl[m])
        out["inter_dist"][m], out["inter_vid"][m], out["count_inter"][m] = _select(sc, vs, h, fl, th)
        if isc is not None:
            out["intra_dist"][m], out["intra_idx"][m], out["count_intra"][m] = _select(isc, iid, h, fl, th)
    return out
