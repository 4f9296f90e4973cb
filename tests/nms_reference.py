"""Plain statement of diversified moment retrieval on dense moment scores, shared by the moment-NMS tests: a stable
(distance, global id) sort of every moment, then one sweep in that order that accepts a moment unless its video already
holds ``per_video`` accepted moments (0 = no cap) or an accepted moment of its video has IoU > ``nms_iou`` with it (IoU of
inclusive clip spans in float64, as ``utils.get_iou``), stopping at k.  Per-video decisions only see that video's earlier
moments, so the sweep is the per-video greedy followed by the merge."""
import numpy as np

from vfr_amd.utils import generate_moments


def expected_nms(S, counts, k, per_video=0, nms_iou=1.0, id_base=0):
    """(dist [Nq,k] f32, id [Nq,k] i64, video [Nq,k] i64), padded with (+inf, -1, -1)."""
    counts = np.asarray(counts, np.int64)
    M = counts * (counts + 1) // 2
    vid_of = np.repeat(np.arange(len(counts)), M)
    spans = np.concatenate([np.asarray(generate_moments(int(n)), np.int64).reshape(-1, 2) for n in counts])
    ids = id_base + np.arange(S.shape[1], dtype=np.int64)
    Nq = S.shape[0]
    od = np.full((Nq, k), np.inf, np.float32)
    oi = np.full((Nq, k), -1, np.int64)
    ov = np.full((Nq, k), -1, np.int64)
    vl, sl, el = vid_of.tolist(), spans[:, 0].tolist(), spans[:, 1].tolist()
    for q in range(Nq):
        if k == 0:
            break
        order = np.lexsort((ids, S[q])).tolist()              # stable (distance, id)
        acc = {}
        out = []
        for m in order:
            v = vl[m]
            a = acc.setdefault(v, [])
            if per_video and len(a) >= per_video:
                continue
            s, e = sl[m], el[m]
            if any((max(min(e, ea) + 1 - max(s, sa), 0) / (max(e, ea) + 1 - min(s, sa))) > nms_iou for sa, ea in a):
                continue
            a.append((s, e))
            out.append(m)
            if len(out) == k:
                break
        n = len(out)
        od[q, :n], oi[q, :n], ov[q, :n] = S[q, out], ids[out], vid_of[out]
    return od, oi, ov
