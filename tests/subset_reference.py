"""The contract of candidate-restricted retrieval (include/vfr.h vfr_score_subset_f32) as a plain numpy statement on dense
moment scores, shared by the host and the GPU tests."""
import numpy as np
import torch


def keys_of(S, id_base=0):
    """[Nq, M] scores -> uint64 keys (fp32 bits << 32 | global moment id): their order is the (distance, id) order."""
    ids = np.uint64(id_base) + np.arange(S.shape[1], dtype=np.uint64)
    return (S.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]


def statement(S, counts, off, vid, k, level, vid_base=0, id_base=0, rank_keys=None):
    """The contract in numpy: per query the keys of its listed videos of this bank (all their moments, or each one's smallest
    key), the k smallest padded with (+inf, -1), and the keys strictly below each rank key."""
    counts = np.asarray(counts, np.int64)
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    K = keys_of(S, id_base)
    Nq = S.shape[0]
    od = np.full((Nq, k), np.inf, np.float32)
    oi = np.full((Nq, k), -1, np.int64)
    R = 0 if rank_keys is None else rank_keys.shape[0]
    cnt = np.zeros((R, Nq), np.int64)
    for q in range(Nq):
        sel = [v - vid_base for v in vid[off[q]:off[q + 1]] if 0 <= v - vid_base < len(counts) and counts[v - vid_base] > 0]
        if level == "moments":
            kk = np.concatenate([K[q, mo[v]:mo[v + 1]] for v in sel]) if sel else np.zeros(0, np.uint64)
        else:
            kk = np.asarray([K[q, mo[v]:mo[v + 1]].min() for v in sel], np.uint64)
        for r in range(R):
            cnt[r, q] = int((kk < np.uint64(rank_keys[r, q])).sum())
        srt = np.sort(kk)[:k]
        od[q, :len(srt)] = (srt >> np.uint64(32)).astype(np.uint32).view(np.float32)
        oi[q, :len(srt)] = (srt & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return od, oi, cnt


def split_keys(rk):
    """uint64 rank keys [R, Nq] -> (rank_dist fp32, rank_idx int64) tensors."""
    d = (rk >> np.uint64(32)).astype(np.uint32).view(np.float32)
    i = (rk & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return torch.from_numpy(d.copy()), torch.from_numpy(i)
