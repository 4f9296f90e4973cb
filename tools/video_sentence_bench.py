#!/usr/bin/env python3
"""Video-to-sentence retrieval (vfr_score_video_sentences_f32) against the only route the library had before it, same process (GPU
box).

    python tools/video_sentence_bench.py [--videos 10000] [--sentences 5000] [--reps 20] [--probes 1000,64] [--clips 21,6] [--chunk 1000]

Seeded random embeddings (D = 100, the model's width; the timing does not depend on what the encoders would have produced) on a
bank of --videos x 21 clips and on the 6-clip DiDeMo shape.  Two routes, ALTERNATED rep by rep after warm-up, device events
around synchronised work:
  new    _vfr.score_video_sentences, k = 100 with one rank key per probe
  dense  what a caller could do without it: a pseudo-bank of the probe videos' clip rows -> vfr_score_moments_f32 with the
         sentences as the queries, in chunks of --chunk rows, restricted to those blocks -> the minimum of every (sentence, video)
         block -> transpose -> torch.topk on the packed (bits, sentence) keys and the rank count.  Gathering the pseudo-bank is
         part of its time.
Both routes must give identical bits (asserted per shape before timing).
Per shape: median and interquartile range of both routes, the factor, and whether the new call's median lies below the dense
route's by more than the SUM of the two interquartile ranges.  One JSON line at the end."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr  # noqa: E402

D, K = 100, 100


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


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--sentences": "5000", "--reps": "20", "--probes": "1000,64", "--clips": "21,6", "--chunk": "1000"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, Ns, reps, chunk = int(opt["--videos"]), int(opt["--sentences"]), int(opt["--reps"]), int(opt["--chunk"])
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    S = torch.randn((Ns, D), generator=gen, device=dev) * 0.3
    ids = torch.arange(Ns, device=dev, dtype=torch.int64)
    rs = np.random.RandomState(7)
    out = {"videos": Nv, "sentences": Ns, "D": D, "k": K, "rows": []}

    for n in (int(x) for x in opt["--clips"].split(",")):
        V = torch.randn((Nv * n, D), generator=gen, device=dev) * 0.3
        clip_off = torch.arange(0, Nv * n + 1, n, dtype=torch.int32, device=dev)
        M = n * (n + 1) // 2
        bank = _vfr.VideoBank(V, clip_off, 0, max_clips=n, total_moments=Nv * M, min_clips=n)
        for Np in (int(x) for x in opt["--probes"].split(",")):
            videos = torch.from_numpy(rs.choice(Nv, Np, replace=False).astype(np.int32)).to(dev)
            own = torch.from_numpy(rs.randint(0, Ns, Np)).to(dev)
            poff = torch.arange(0, Np * n + 1, n, dtype=torch.int32, device=dev)
            ws = torch.empty((_vfr.lib().vfr_score_video_sentences_workspace_bytes(Np, Ns, K),), dtype=torch.uint8, device=dev)

            def dense_keys():
                rows = (videos.long() * n)[:, None] + torch.arange(n, device=dev)[None, :]
                pb = _vfr.VideoBank(V[rows.reshape(-1)], poff, 0, max_clips=n, total_moments=Np * M, min_clips=n)
                best = torch.empty((Ns, Np), dtype=torch.float32, device=dev)
                for a in range(0, Ns, chunk):
                    sc = _vfr.score_moments(S[a:a + chunk], pb)                  # [rows, Np * M]
                    best[a:a + chunk] = sc.view(-1, Np, M).min(dim=2).values     # the segment minimum of every video's block
                return (best.t().contiguous().view(torch.int32).long() << 32) | ids[None, :]

            def dense():
                keys = dense_keys()
                rkey = keys[torch.arange(Np, device=dev), own]
                cnt = (keys < rkey[:, None]).sum(dim=1)
                top = torch.topk(keys, K, dim=1, largest=False, sorted=True).values
                return (top >> 32).to(torch.int32).view(torch.float32), top & 0xFFFFFFFF, cnt

            bd, bi, bc = dense()
            rkey = dense_keys()[torch.arange(Np, device=dev), own]               # the rank key: the own sentence's key
            rd = (rkey >> 32).to(torch.int32).view(torch.float32).contiguous()
            cnt = torch.zeros((1, Np), dtype=torch.int64, device=dev)

            def new():
                cnt.zero_()
                return _vfr.score_video_sentences(S, bank, videos, K, 0, 0, rd, own, count_lt=cnt, workspace=ws)

            d, i, c = new()
            torch.cuda.synchronize()
            assert torch.equal(d, bd) and torch.equal(i, bi) and torch.equal(c[0], bc), f"routes differ at {Np} probes x {n} clips"
            del bd, bi, bc
            tn, tb = timed_pair(new, dense, reps)
            row = {"clips": n, "probes": Np, "identical_bits": True, "new": stats(tn), "dense": stats(tb)}
            med, b = row["new"]["median_ms"], row["dense"]
            row["factor"] = round(b["median_ms"] / med, 2)
            row["us_per_probe"] = round(1e3 * med / Np, 3)
            row["algorithmic_tflops_over_call_time"] = round(3.0 * D * Np * n * Ns / (med * 1e-3) / 1e12, 3)
            row["faster_by_more_than_the_iqr_sum"] = bool(b["median_ms"] - med > b["iqr_ms"] + row["new"]["iqr_ms"])
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
