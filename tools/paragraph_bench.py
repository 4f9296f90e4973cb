#!/usr/bin/env python3
"""Paragraph-to-video retrieval (vfr_score_paragraphs_f32) against the only route the library had before it, same process (GPU box).

    python tools/paragraph_bench.py [--videos 10000] [--reps 20] [--groups 1000,64,8,1] [--clips 21,6] [--chunk 256]

Seeded random embeddings (D = 100, the model's width) on banks of --videos x 21 and x 6 clips; paragraphs of 4 sentences, half of
them clip rows of their own video (so the own video ranks first and many bounds have something to decide), k = 100, with ranks.
Three routes, ALTERNATED rep by rep after warm-up, device events around synchronised work:
  fast    _vfr.score_paragraphs(mode="mfma"): bounds GEMM -> group bounds and selection -> exact chain on the listed pairs -> top-k
  exact   _vfr.score_paragraphs(mode="exact"): the exact chain on every (paragraph, video)
  dense   what a caller could do without it: vfr_score_moments_f32 in chunks of --chunk sentences (whole paragraphs) -> per-video
          segment minimum -> the fp32 chain over the sentences and the division -> stable sort by (score, video) -> the first k and
          the rank count.  The 1 000-paragraph dense matrix does not fit in one piece (9.2 GB at 21 clips), hence the chunks.
All three must give identical bits (checked per shape before timing).  Per shape: median and interquartile range of each route,
how many (paragraph, video) pairs the fast path re-scored exactly, and whether the fast path is below both other medians by more
than the sum of the two interquartile ranges.  One JSON line at the end."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr  # noqa: E402

D, K, L = 100, 100, 4


def timed(fns, reps, warm=2):
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for f, a in zip(fns, acc):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            a.append(s.elapsed_time(e))
    return acc


def stats(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(t)), 4), "reps": len(t)}


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--reps": "20", "--groups": "1000,64,8,1", "--clips": "21,6", "--chunk": "256"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, reps, chunk = int(opt["--videos"]), int(opt["--reps"]), int(opt["--chunk"]) // L * L
    dev = torch.device("cuda", 0)
    out = {"videos": Nv, "D": D, "k": K, "sentences_per_paragraph": L, "rows": []}
    for n in [int(x) for x in opt["--clips"].split(",")]:
        gen = torch.Generator(device=dev); gen.manual_seed(1234 + n)
        V = torch.randn((Nv * n, D), generator=gen, device=dev) * 0.3
        clip_off = torch.arange(0, Nv * n + 1, n, dtype=torch.int32, device=dev)
        bank = _vfr.VideoBank(V, clip_off, 0, max_clips=n, total_moments=Nv * n * (n + 1) // 2, min_clips=n)
        M = n * (n + 1) // 2
        vids = torch.arange(Nv, device=dev, dtype=torch.int64)
        for Ng in [int(x) for x in opt["--groups"].split(",")]:
            rs = np.random.RandomState(Ng)
            Nq = Ng * L
            Q = torch.randn((Nq, D), generator=gen, device=dev) * 0.3
            own_h = rs.randint(0, Nv, Ng)
            for g in range(0, Ng, 2):                                             # every second paragraph: rows of its own video
                Q[g * L:(g + 1) * L] = V[int(own_h[g]) * n + torch.from_numpy(rs.randint(0, n, L)).to(dev)]
            own = torch.from_numpy(own_h).to(dev)
            off = torch.arange(0, Nq + 1, L, dtype=torch.int64, device=dev)
            pairs = torch.stack([torch.arange(Ng, device=dev), own], dim=1).to(torch.int32)
            od, _ = _vfr.score_paragraph_pairs(Q, bank, off, L, pairs, moments=False)
            ws = torch.empty((_vfr.lib().vfr_score_paragraphs_workspace_bytes(Nq, Ng, Nv, Nv * n, K),), dtype=torch.uint8, device=dev)
            cnt = torch.zeros(Ng, dtype=torch.int64, device=dev)

            def new(mode):
                cnt.zero_()
                return _vfr.score_paragraphs(Q, bank, off, L, K, 0, od, own, count=cnt, mode=mode, workspace=ws)

            def dense():
                keys = torch.empty((Ng, Nv), dtype=torch.int64, device=dev)
                for a in range(0, Nq, chunk):
                    b = min(Nq, a + chunk)
                    best = _vfr.score_moments(Q[a:b], bank).view(b - a, Nv, M).min(dim=2).values.view((b - a) // L, L, Nv)
                    acc = best[:, 0]
                    for t in range(1, L):
                        acc = acc + best[:, t]
                    sc = acc / float(L)
                    keys[a // L:b // L] = (sc.contiguous().view(torch.int32).long() << 32) | vids[None, :]
                okey = (od.view(torch.int32).long() << 32) | own
                c = (keys < okey[:, None]).sum(dim=1)
                top = keys.sort(dim=1, stable=True).values[:, :K]
                return (top >> 32).to(torch.int32).view(torch.float32), top & 0xFFFFFFFF, c

            fd, fi, fc = new("mfma")
            fc = fc.clone()
            st = _vfr.score_paragraphs_stats(ws, Nq, Ng, bank)
            ed, ei, ec = new("exact")
            ec = ec.clone()
            dd, di, dc = dense()
            torch.cuda.synchronize()
            row = {"clips": n, "paragraphs": Ng, "sentences": Nq,
                   "identical_bits": bool(torch.equal(fd, ed) and torch.equal(fi, ei) and torch.equal(fc, ec) and torch.equal(fd, dd) and
                                          torch.equal(fi, di) and torch.equal(fc, dc)),
                   "fast_rescored_pairs": int(st[:, 0].sum()), "of_pairs": Ng * Nv, "rank_undecided_pairs": int(st[:, 1].sum())}
            del fd, fi, ed, ei, dd, di
            tf, te, td = timed([lambda: new("mfma"), lambda: new("exact"), dense], reps)
            row["fast"], row["exact"], row["dense"] = stats(tf), stats(te), stats(td)
            f, e, d_ = row["fast"], row["exact"], row["dense"]
            row["fast_below_dense"] = bool(d_["median_ms"] - f["median_ms"] > d_["iqr_ms"] + f["iqr_ms"])
            row["fast_below_exact"] = bool(e["median_ms"] - f["median_ms"] > e["iqr_ms"] + f["iqr_ms"])
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
