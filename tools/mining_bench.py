#!/usr/bin/env python3
"""Hard-negative mining (vfr_mine_negatives_f32) against the only route the library had before it, same process (GPU box).

    python tools/mining_bench.py [--videos 10000] [--reps 20] [--items 5000,64] [--chunk 64]

Seeded random embeddings (D = 100, the model's width) on a bank of --videos x 21 clips; items = (query row, own video, span) with
DiDeMo-shaped spans (1..6 clips), h = 16, same-length intra negatives.  Two routes, ALTERNATED rep by rep after warm-up, device
events around synchronised work:
  new    _vfr.mine_negatives (sort of the items by span + vfr_mine_negatives_f32 + the caller's order restored): inter and intra lists
  dense  what a caller could do without it: vfr_score_moments_f32 for --chunk query rows at a time (the [chunk, sum M] matrix), the
         span's column of every video gathered, the own video masked, torch.topk on the packed (score, video) keys; the intra list
         from the own video's block of the same matrix under the same-length mask.
Both routes must give identical bits (asserted per shape before timing).  Per shape: median and interquartile range of both routes,
the factor, and whether the new route's median is below the dense route's by more than the sum of the two interquartile ranges.
One JSON line per shape and one at the end."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr  # noqa: E402

D, H, N = 100, 16, 21
KEY_MAX = torch.iinfo(torch.int64).max


def timed_pair(fa, fb, reps, warm=2):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            acc.append(s.elapsed_time(e))
    return ta, tb


def stats(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(t)), 4), "reps": len(t)}


def all_moments(n):
    return [(s, s) for s in range(n)] + [(s, e) for s in range(n) for e in range(s + 1, n)]


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--reps": "20", "--items": "5000,64", "--chunk": "64"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, reps, chunk = int(opt["--videos"]), int(opt["--reps"]), int(opt["--chunk"])
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    V = torch.randn((Nv * N, D), generator=gen, device=dev) * 0.3
    Qall = torch.randn((5000, D), generator=gen, device=dev) * 0.3
    clip_off = torch.arange(0, Nv * N + 1, N, dtype=torch.int32, device=dev)
    M = N * (N + 1) // 2
    bank = _vfr.VideoBank(V, clip_off, 0, max_clips=N, total_moments=Nv * M, min_clips=N)
    spans = all_moments(N)
    lid = {m: j for j, m in enumerate(spans)}
    same = torch.tensor([[a[1] - a[0] == b[1] - b[0] and a != b for b in spans] for a in spans], device=dev)     # [M, M]
    rs = np.random.RandomState(7)
    out = {"videos": Nv, "clips": N, "D": D, "h": H, "dense_chunk_rows": chunk, "rows": []}

    for Nm in (int(x) for x in opt["--items"].split(",")):
        Q = Qall[:Nm].contiguous()
        ln = rs.randint(1, 7, Nm)
        s = (rs.rand(Nm) * (N - ln + 1)).astype(np.int64)
        own_h = rs.randint(0, Nv, Nm)
        items_h = np.stack([np.arange(Nm), own_h, s, s + ln - 1], axis=1).astype(np.int32)
        items = torch.from_numpy(items_h).to(dev)
        col = torch.tensor([lid[(int(a), int(b))] for a, b in items_h[:, 2:]], device=dev)
        own = torch.from_numpy(own_h).to(dev)
        vids = torch.arange(Nv, device=dev, dtype=torch.int64)
        mids = torch.arange(M, device=dev, dtype=torch.int64)
        ws = torch.empty((_vfr.lib().vfr_mine_negatives_workspace_bytes(Nm, Nv, H),), dtype=torch.uint8, device=dev)

        def new():
            return _vfr.mine_negatives(Q, bank, items, H, workspace=ws)[:4]

        def lists(keys):
            top = torch.topk(keys, H, dim=1, largest=False, sorted=True).values
            pad = top == KEY_MAX
            d = (top >> 32).to(torch.int32).view(torch.float32).masked_fill(pad, float("inf"))
            return d, (top & 0xFFFFFFFF).masked_fill(pad, -1)

        def dense():
            parts = []
            for a in range(0, Nm, chunk):
                b = min(a + chunk, Nm)
                sc = _vfr.score_moments(Q[a:b], bank).view(b - a, Nv, M)                       # the [rows, sum M] matrix
                rows = torch.arange(b - a, device=dev)
                inter = sc[rows, :, col[a:b]]                                                  # the span's column of every video
                keys = (inter.contiguous().view(torch.int32).long() << 32) | vids[None, :]
                keys[rows, own[a:b]] = KEY_MAX                                                 # not the own video
                blk = sc[rows, own[a:b]]                                                       # the own video's [rows, M] block
                ikeys = (blk.contiguous().view(torch.int32).long() << 32) | (own[a:b, None] * M + mids[None, :])
                ikeys = torch.where(same[col[a:b]], ikeys, torch.full_like(ikeys, KEY_MAX))
                parts.append(lists(keys) + lists(ikeys))
            return tuple(torch.cat([p[j] for p in parts]) for j in range(4))

        got, want = new(), dense()
        torch.cuda.synchronize()
        same_bits = all(torch.equal(g, w) for g, w in zip(got, want))
        assert same_bits, f"{Nm} items: the mining call and the dense route differ"
        tn, td = timed_pair(new, dense, reps)
        row = {"items": Nm, "identical_bits": same_bits, "new": stats(tn), "dense": stats(td)}
        row["factor"] = round(row["dense"]["median_ms"] / row["new"]["median_ms"], 2)
        row["goal_median_gap_exceeds_sum_of_iqr"] = bool(row["dense"]["median_ms"] - row["new"]["median_ms"] >
                                                         row["dense"]["iqr_ms"] + row["new"]["iqr_ms"])
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
