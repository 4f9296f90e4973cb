#!/usr/bin/env python3
"""Prior-aware retrieval (vfr_score_prior_f32) against the routes the library had before it, same process (GPU box).

    python tools/prior_bench.py [--queries 5000] [--videos 10000] [--reps 7] [--slice 64] [--k 100] [--out FILE]

Seeded random embeddings (D = 100, the model's width) on a bank of --videos x 21 clips, k = 100, two rank keys per query.  Five
routes, ALTERNATED rep by rep after a warm-up of every route, device events around synchronised work:
  prior_zero     _vfr.score_prior with a table of zeros (the results of score_topk)
  prior_table    ... with an engine.prior_table built from seeded training spans (finite biases, nothing excluded)
  prior_lengths  ... with engine.moment_table(lengths=(1, 2, 3)): 60 of a video's 231 moments are candidates
  fusion_1       _vfr.score_fusion with ONE stream of weight 1: the kernel of the same structure without a table
  dense          what a caller could do without it: for --slice query rows at a time vfr_score_moments_f32 (a dense [slice, sum M]
                 matrix), a torch add of the table's row, torch.topk, and comparisons against the rank scores for the counts
Parity is tests/test_prior_gpu.py's business; here the tool only asserts that the zero-table lists equal the one-stream fusion's.
One JSON line at the end (also written to --out): median, interquartile range and minimum of every route and the factors."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr, engine  # noqa: E402

D, N = 100, 21


def timed(routes, reps, warm=2):
    for _ in range(warm):
        for f in routes.values():
            f()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, f in routes.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    return times


def stats(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(t)), 4), "reps": len(t)}


def main():
    args = sys.argv[1:]
    opt = {"--queries": "5000", "--videos": "10000", "--reps": "7", "--slice": "64", "--k": "100", "--out": ""}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nq, Nv, reps, rows, k = (int(opt[x]) for x in ("--queries", "--videos", "--reps", "--slice", "--k"))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    clip_off = torch.arange(0, Nv * N + 1, N, dtype=torch.int32, device=dev)
    M = N * (N + 1) // 2
    bank = _vfr.VideoBank(torch.randn((Nv * N, D), generator=gen, device=dev) * 0.3, clip_off, 0, max_clips=N, total_moments=Nv * M,
                          min_clips=N)
    Q = torch.randn((Nq, D), generator=gen, device=dev) * 0.3
    rs = np.random.RandomState(1234)
    starts = rs.randint(0, N, (2000, 4))
    train = [[(int(s), int(min(N - 1, s + rs.randint(0, 4)))) for s in row] for row in starts]
    tables = {"prior_zero": engine.moment_table(N, device=dev),
              "prior_table": engine.prior_table(train, np.full(len(train), N), lam=0.1, alpha=1.0, device=dev),
              "prior_lengths": engine.moment_table(N, lengths=(1, 2, 3), device=dev)}
    own = torch.randint(0, Nv, (Nq,), generator=gen, device=dev).to(torch.int32)
    ws = torch.empty((max(_vfr.lib().vfr_score_prior_workspace_bytes(Nq, Nv, k), _vfr.lib().vfr_score_fusion_workspace_bytes(Nq, Nv, k)),),
                     dtype=torch.uint8, device=dev)
    # rank keys: the biased scores of two fixed single-clip moments of each query's "own" video (candidates under every table)
    keys = {}
    for name, t in tables.items():
        sc = _vfr.score_prior_own(Q, bank, t, own)
        keys[name] = (torch.stack([sc[:, 3], sc[:, 17]]).contiguous(), torch.stack([own.long() * M + 3, own.long() * M + 17]).contiguous())
    routes = {name: (lambda name=name: _vfr.score_prior(Q, bank, tables[name], k, "moments", *keys[name], workspace=ws)) for name in tables}
    routes["fusion_1"] = lambda: _vfr.score_fusion([Q], [bank], (1.0,), k, "moments", *keys["prior_zero"], workspace=ws)
    trow = tables["prior_table"].table[int(tables["prior_table"].table_off[N]):].repeat(Nv)     # the bias of every moment of the bank
    rd = keys["prior_table"][0]

    def dense():
        ds, is_, cs = [], [], []
        for a in range(0, Nq, rows):
            b = min(a + rows, Nq)
            g = _vfr.score_moments(Q[a:b].contiguous(), bank) + trow                          # one dense [slice, sum M] matrix
            top = torch.topk(g, k, dim=1, largest=False, sorted=True)
            ds.append(top.values)
            is_.append(top.indices)
            cs.append(torch.stack([(g < rd[r, a:b, None]).sum(dim=1) for r in range(2)]))     # (ties by id left out: a baseline)
        return torch.cat(ds), torch.cat(is_), torch.cat(cs, dim=1)
    routes["dense"] = dense

    a, b = routes["prior_zero"](), routes["fusion_1"]()
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "zero table != one-stream fusion"
    t = timed(routes, reps)
    out = {"queries": Nq, "videos": Nv, "clips": N, "D": D, "k": k, "rank_keys": 2, "dense_slice_rows": rows,
           "workspace_bytes": int(_vfr.lib().vfr_score_prior_workspace_bytes(Nq, Nv, k)), "dense_bytes_per_slice": int(rows * Nv * M * 4),
           "candidates_per_video": {name: int(tb.enabled(N).sum()) for name, tb in tables.items()}}
    out.update({name: stats(v) for name, v in t.items()})
    out["zero_over_fusion_1"] = round(out["prior_zero"]["median_ms"] / out["fusion_1"]["median_ms"], 3)
    out["dense_over_prior_table"] = round(out["dense"]["median_ms"] / out["prior_table"]["median_ms"], 2)
    line = json.dumps(out)
    if opt["--out"]:
        Path(opt["--out"]).parent.mkdir(parents=True, exist_ok=True)
        Path(opt["--out"]).write_text(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
