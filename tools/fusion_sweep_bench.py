#!/usr/bin/env python3
"""Fusion weight sweep (vfr_score_fusion_sweep_f32 / _sweep_own_f32) against the route a caller had before it, same process (GPU box).

    python tools/fusion_sweep_bench.py [--queries 5000] [--videos 10000] [--reps 20] [--steps 10]

Seeded random embeddings (D = 100, the model's width) for S = 2 streams on a bank of --videos x 21 clips, the weight grid
engine.simplex_grid(2, --steps) (11 rows), two ground-truth label rows per query, moment level.  Two routes to the ranks [W, 2, Nq],
ALTERNATED rep by rep after a warm-up of both, device events around synchronised work:
  sweep   score_fusion_sweep_own -> gt_best_keys per row -> score_fusion_sweep: the stream clip distances once
  loop    per row of the grid: score_fusion_own -> gt_best_keys -> score_fusion(k = 0): W passes over the bank
The two must give IDENTICAL ranks (asserted before anything is timed).  One JSON line at the end: median and interquartile range of
both routes, their ratio, and whether the sweep's median lies below the loop's by more than the sum of the two ranges."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr, engine  # noqa: E402

D, N, S = 100, 21, 2


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
    opt = {"--queries": "5000", "--videos": "10000", "--reps": "20", "--steps": "10"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nq, Nv, reps, steps = (int(opt[x]) for x in ("--queries", "--videos", "--reps", "--steps"))
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    clip_off = torch.arange(0, Nv * N + 1, N, dtype=torch.int32, device=dev)
    M = N * (N + 1) // 2
    banks = [_vfr.VideoBank(torch.randn((Nv * N, D), generator=gen, device=dev) * 0.3, clip_off, 0, max_clips=N, total_moments=Nv * M,
                            min_clips=N) for _ in range(S)]
    Qs = [torch.randn((Nq, D), generator=gen, device=dev) * 0.3 for _ in range(S)]
    grid = engine.simplex_grid(S, steps)
    W = len(grid)
    own = torch.randint(0, Nv, (Nq,), generator=gen, device=dev).to(torch.int32)
    labels = torch.rand((2, Nq, M), generator=gen, device=dev) < 0.02            # two label rows (IoU thresholds) per query ...
    labels[:, :, 3] = True                                                       # ... none of them empty
    base = own.long() * M
    sel = torch.arange(Nq, dtype=torch.int64, device=dev)
    ops = engine.HipOps()

    def sweep():
        sc = _vfr.score_fusion_sweep_own(Qs, banks, grid, own)
        keys = torch.stack([ops.gt_best_keys(sc[w], labels, base, sel, Nq) for w in range(W)])
        rd, ri = engine._unpack_key(keys)
        return _vfr.score_fusion_sweep(Qs, banks, grid, "moments", rd.contiguous(), ri.contiguous())

    def loop():
        out = []
        for w in range(W):
            sc = _vfr.score_fusion_own(Qs, banks, grid[w], own)
            rd, ri = engine._unpack_key(ops.gt_best_keys(sc, labels, base, sel, Nq))
            out.append(_vfr.score_fusion(Qs, banks, grid[w], 0, "moments", rd.contiguous(), ri.contiguous())[2])
        return torch.stack(out)

    got, want = sweep(), loop()
    torch.cuda.synchronize()
    assert got.shape == (W, 2, Nq) and torch.equal(got, want), "the sweep's ranks differ from the per-row route's"
    ts, tl = timed_pair(sweep, loop, reps)
    out = {"queries": Nq, "videos": Nv, "clips": N, "D": D, "streams": S, "grid_rows": W, "rank_keys": 2, "level": "moments",
           "ranks_identical": True, "sweep": stats(ts), "loop": stats(tl)}
    out["loop_over_sweep"] = round(out["loop"]["median_ms"] / out["sweep"]["median_ms"], 2)
    out["sweep_faster_beyond_noise"] = bool(out["sweep"]["median_ms"] + out["sweep"]["iqr_ms"] + out["loop"]["iqr_ms"] < out["loop"]["median_ms"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
