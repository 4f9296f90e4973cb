#!/usr/bin/env python3
"""Late-fusion retrieval (vfr_score_fusion_f32) against the only route the library had before it, same process (GPU box).

    python tools/fusion_bench.py [--queries 5000] [--videos 10000] [--reps 5] [--slice 64] [--k 100]

Seeded random embeddings (D = 100, the model's width) for S = 2 streams on a bank of --videos x 21 clips, weights (0.6, 0.4),
k = 100, two rank keys per query.  Two routes, ALTERNATED rep by rep after warm-up, device events around synchronised work:
  new    _vfr.score_fusion: one call, lists and both rank counts, O(Nq k) workspace
  dense  what a caller could do without it: for --slice query rows at a time, vfr_score_moments_f32 once per stream (S dense
         [slice, sum M] matrices), a torch weighted sum, torch.topk on the sum, and comparisons against the rank scores for the
         counts.
The dense route fuses at the MOMENT level (the weighted sum of the streams' moment scores); the new route fuses at the clip and
runs the moment chain once.  The two agree in real arithmetic and may differ in the last bits, so the dense route is a TIMING
baseline only, not a parity check: the tool reports how many of the top-k ids agree and asserts nothing about it (the bit-for-bit
checks are tests/test_fusion_gpu.py).  One JSON line at the end: median and interquartile range of both routes and the factor."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr  # noqa: E402

D, N, S = 100, 21, 2
WEIGHTS = (0.6, 0.4)


def timed_pair(fa, fb, reps, warm=1):
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


def main():
    args = sys.argv[1:]
    opt = {"--queries": "5000", "--videos": "10000", "--reps": "5", "--slice": "64", "--k": "100"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nq, Nv, reps, rows, k = (int(opt[x]) for x in ("--queries", "--videos", "--reps", "--slice", "--k"))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    clip_off = torch.arange(0, Nv * N + 1, N, dtype=torch.int32, device=dev)
    M = N * (N + 1) // 2
    banks = [_vfr.VideoBank(torch.randn((Nv * N, D), generator=gen, device=dev) * 0.3, clip_off, 0, max_clips=N, total_moments=Nv * M,
                            min_clips=N) for _ in range(S)]
    Qs = [torch.randn((Nq, D), generator=gen, device=dev) * 0.3 for _ in range(S)]
    w = torch.tensor(WEIGHTS, dtype=torch.float32, device=dev)
    # rank keys: the fused scores of two fixed moments of each query's "own" video, by the new route's own-video call
    own = torch.randint(0, Nv, (Nq,), generator=gen, device=dev).to(torch.int32)
    sc = _vfr.score_fusion_own(Qs, banks, WEIGHTS, own)
    rd = torch.stack([sc[:, 3], sc[:, 40]]).contiguous()
    ri = torch.stack([own.long() * M + 3, own.long() * M + 40]).contiguous()
    ws = torch.empty((_vfr.lib().vfr_score_fusion_workspace_bytes(Nq, Nv, k),), dtype=torch.uint8, device=dev)

    def new():
        return _vfr.score_fusion(Qs, banks, WEIGHTS, k, "moments", rd, ri, workspace=ws)

    def dense():
        ds, is_, cs = [], [], []
        for a in range(0, Nq, rows):
            b = min(a + rows, Nq)
            fused = None
            for s in range(S):
                t = _vfr.score_moments(Qs[s][a:b].contiguous(), banks[s]) * w[s]             # one dense [slice, sum M] matrix per stream
                fused = t if fused is None else fused + t
            top = torch.topk(fused, k, dim=1, largest=False, sorted=True)
            ds.append(top.values)
            is_.append(top.indices)
            cs.append(torch.stack([(fused < rd[r, a:b, None]).sum(dim=1) for r in range(2)]))   # (ties by id left out: a baseline)
        return torch.cat(ds), torch.cat(is_), torch.cat(cs, dim=1)

    got, want = new(), dense()
    torch.cuda.synchronize()
    agree = float((got[1] == want[1]).float().mean())
    tn, td = timed_pair(new, dense, reps)
    out = {"queries": Nq, "videos": Nv, "clips": N, "D": D, "streams": S, "weights": WEIGHTS, "k": k, "rank_keys": 2,
           "dense_slice_rows": rows, "workspace_bytes_new": int(ws.numel()), "dense_bytes_per_slice": int(S * rows * Nv * M * 4),
           "topk_ids_agreeing_with_moment_level_fusion": round(agree, 6), "new": stats(tn), "dense": stats(td)}
    out["factor"] = round(out["dense"]["median_ms"] / out["new"]["median_ms"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
