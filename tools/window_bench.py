#!/usr/bin/env python3
"""Windowed retrieval (vfr_score_window_f32, engine.corpus_window_topk) on the benchmark bank and on a long-video bank (GPU box).

    python tools/window_bench.py [--reps 7] [--out FILE]

Seeded random embeddings (D = 100, the model's width), k = 100, one rank key per query, device events around synchronised work, a
warm-up of every route, routes ALTERNATED rep by rep, the median of the repeats.
  (a) the benchmark bank: 10 000 videos x 21 clips, 5 000 queries, max_len = 8.  The same request through
      engine.corpus_prior_topk with engine.moment_table(21, max_len=8) -- the route that existed before -- and through
      engine.corpus_window_topk; distances, ids and ranks are ASSERTED identical before anything is timed.  Also the two scan entry
      points alone (_vfr.score_prior / _vfr.score_window on the same rank keys).
  (b) a long shape no other route can score: 2 000 videos x 128 clips, 1 000 queries, max_len = 16: ms and candidate moments / s.
One JSON line at the end (also written to --out)."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr, engine  # noqa: E402
from vfr_amd.utils import moment_index  # noqa: E402

D, K = 100, 100


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


def corpus(Nv, n, Nq, seed, dev):
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    counts = np.full(Nv, n, np.int64)
    emb = torch.randn((Nv * n, D), generator=gen, device=dev) * 0.3
    shard = engine.corpus_from_embeddings(emb, counts, dev, engine.HipOps())
    Q = torch.randn((Nq, D), generator=gen, device=dev) * 0.3
    own = np.random.RandomState(seed).randint(0, Nv, Nq)
    return shard, Q, own


def candidates(Nv, n, L):
    return Nv * sum(min(L, n - s) for s in range(n))


def main():
    args = sys.argv[1:]
    opt = {"--reps": "7", "--out": ""}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    reps = int(opt["--reps"])
    dev = torch.device("cuda", 0)
    ops = engine.HipOps()
    out = {"D": D, "k": K, "rank_keys": 1}

    # ---- (a) the benchmark bank ----
    Nv, n, Nq, L = 10000, 21, 5000, 8
    shard, Q, own = corpus(Nv, n, Nq, 1234, dev)
    table = engine.moment_table(n, max_len=L, device=dev)
    span = (3, 5)                                                # the one positive of every query: clips 3 .. 5 of its own video
    labels = torch.zeros((1, Nq, n * (n + 1) // 2), dtype=torch.bool, device=dev)
    labels[:, :, moment_index(n, *span)] = True
    positives = [np.stack([np.arange(Nq), np.full(Nq, span[0]), np.full(Nq, span[1])], axis=1)]
    ws = torch.empty((max(_vfr.lib().vfr_score_prior_workspace_bytes(Nq, Nv, K),
                          _vfr.lib().vfr_score_window_workspace_bytes(Nq, Nv * n, K)),), dtype=torch.uint8, device=dev)
    prior = lambda: engine.corpus_prior_topk(shard, Q, table, K, "moments", own_global=own, labels=labels, ops=ops, workspace=ws)
    window = lambda: engine.corpus_window_topk(shard, Q, L, K, own_global=own, positives=positives, ops=ops, workspace=ws)
    a, b = prior(), window()
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "window lists != prior lists"
    assert torch.equal(a[3], b[3]) and not bool(b[4].any()), "window ranks != prior ranks"
    rd, ri = a[0][:, K // 2].contiguous(), a[1][:, K // 2].contiguous()
    routes = {"a_prior_request": prior, "a_window_request": window,
              "a_prior_scan": lambda: _vfr.score_prior(Q, shard.bank, table, K, "moments", rd, ri, workspace=ws),
              "a_window_scan": lambda: _vfr.score_window(Q, shard.bank, L, K, rd, ri, workspace=ws)}
    x, y = routes["a_prior_scan"](), routes["a_window_scan"]()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(x, y)), "window scan != prior scan"
    t = timed(routes, reps)
    cand = candidates(Nv, n, L)
    out["a"] = {"videos": Nv, "clips": n, "queries": Nq, "max_len": L, "candidates_per_query": cand, "identical_to_prior": True}
    out["a"].update({name[2:]: stats(v) for name, v in t.items()})
    out["a"]["window_over_prior_request"] = round(out["a"]["window_request"]["median_ms"] / out["a"]["prior_request"]["median_ms"], 3)
    out["a"]["window_over_prior_scan"] = round(out["a"]["window_scan"]["median_ms"] / out["a"]["prior_scan"]["median_ms"], 3)
    out["a"]["window_scan_moments_per_s"] = round(Nq * cand / (out["a"]["window_scan"]["median_ms"] * 1e-3), 0)
    del shard, Q, labels, ws, a, b, x, y

    # ---- (b) long videos ----
    Nv, n, Nq, L = 2000, 128, 1000, 16
    shard, Q, own = corpus(Nv, n, Nq, 4321, dev)
    positives = [np.stack([np.arange(Nq), np.full(Nq, 40), np.full(Nq, 47)], axis=1)]
    ws = torch.empty((_vfr.lib().vfr_score_window_workspace_bytes(Nq, Nv * n, K),), dtype=torch.uint8, device=dev)
    window = lambda: engine.corpus_window_topk(shard, Q, L, K, own_global=own, positives=positives, ops=ops, workspace=ws)
    d, i, vid, ranks, unreach = window()
    torch.cuda.synchronize()
    v2, s2, e2 = engine.decode_moments(shard, i)
    assert torch.equal(v2, vid) and bool((e2 - s2 < L).all()) and not bool(unreach.any())
    rd, ri = d[:, K // 2].contiguous(), i[:, K // 2].contiguous()
    t = timed({"b_window_request": window,
               "b_window_scan": lambda: _vfr.score_window(Q, shard.bank, L, K, rd, ri, workspace=ws)}, reps)
    cand = candidates(Nv, n, L)
    out["b"] = {"videos": Nv, "clips": n, "queries": Nq, "max_len": L, "candidates_per_query": cand}
    out["b"].update({name[2:]: stats(v) for name, v in t.items()})
    out["b"]["window_scan_moments_per_s"] = round(Nq * cand / (out["b"]["window_scan"]["median_ms"] * 1e-3), 0)
    line = json.dumps(out)
    if opt["--out"]:
        Path(opt["--out"]).parent.mkdir(parents=True, exist_ok=True)
        Path(opt["--out"]).write_text(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
