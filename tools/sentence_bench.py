#!/usr/bin/env python3
"""Sentence retrieval for moments (vfr_score_sentences_f32) against the only route the library had before it, same process (GPU box).

    python tools/sentence_bench.py [--videos 10000] [--reps 20] [--shapes a,b,c,d] [--reps-d 5]

Seeded random embeddings (D = 100, the model's width; the timing does not depend on what the encoders would have produced) on a
bank of --videos x 21 clips.  Two routes, ALTERNATED rep by rep after warm-up, device events around synchronised work:
  new       _vfr.score_sentences (sort of the probes by video + vfr_score_sentences_f32 + the caller's order restored)
  baseline  what a caller could do without it: a pseudo-bank with one "video" per probe span (gathered clip rows, offsets) ->
            vfr_score_moments_f32 dense [Ns, sum of span triangles] -> the full-span column of every probe -> transpose -> torch
            sort by (distance, id) -> the first k and the rank count.  Building the pseudo-bank is part of its time.
Both routes must give identical bits (checked per shape before timing).
Shapes: a  5 000 sentences x 5 000 probes, span lengths 1..6, k = 100, one rank key          (the headline)
        b  5 000 sentences x all 231 moments of 64 videos (14 784 probes): shared clip distances
        c  1 / 8 / 64 probes x 33 000 sentences: a serving request
        d  33 000 x 33 000 (--reps-d repeats; the baseline only if its matrices fit)
Per shape: median and interquartile range of both routes, the factor, time per probe, and the algorithmic rate
3 x D x (distinct clip, sentence pairs) / time of the new route.  One JSON line at the end."""
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
        if fb:
            fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            if f is None:
                continue
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            acc.append(s.elapsed_time(e))
    return ta, tb


def stats(t):
    if not t:
        return None
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(t)), 4), "reps": len(t)}


def all_moments(n):
    return [(s, s) for s in range(n)] + [(s, e) for s in range(n) for e in range(s + 1, n)]


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--reps": "20", "--shapes": "a,b,c,d", "--reps-d": "5"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, reps, reps_d, shapes = int(opt["--videos"]), int(opt["--reps"]), int(opt["--reps-d"]), opt["--shapes"].split(",")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    n = 21
    V = torch.randn((Nv * n, D), generator=gen, device=dev) * 0.3
    Sall = torch.randn((33000, D), generator=gen, device=dev) * 0.3
    clip_off = torch.arange(0, Nv * n + 1, n, dtype=torch.int32, device=dev)
    bank = _vfr.VideoBank(V, clip_off, 0, max_clips=n, total_moments=Nv * n * (n + 1) // 2, min_clips=n)
    rs = np.random.RandomState(7)
    out = {"videos": Nv, "clips": n, "D": D, "k": K, "rows": []}

    def case(name, Ns, probes_h, reps, baseline=True):
        S = Sall[:Ns].contiguous()
        Nm = len(probes_h)
        probes = torch.from_numpy(probes_h.astype(np.int32)).to(dev)
        own = torch.from_numpy(rs.randint(0, Ns, Nm)).to(dev)
        lens_h = (probes_h[:, 2] - probes_h[:, 1] + 1).astype(np.int64)
        poff_h = np.concatenate([[0], np.cumsum(lens_h)])
        pmom = int((lens_h * (lens_h + 1) // 2).sum())
        ids = torch.arange(Ns, device=dev, dtype=torch.int64)
        ws = torch.empty((_vfr.lib().vfr_score_sentences_workspace_bytes(Nm, Ns, K),), dtype=torch.uint8, device=dev)

        def dense_route():
            # the pseudo-bank: probe m's clips as "video" m
            lens = (probes[:, 2] - probes[:, 1] + 1).long()
            poff = torch.zeros(Nm + 1, dtype=torch.int64, device=dev)
            poff[1:] = lens.cumsum(0)
            owner = torch.repeat_interleave(torch.arange(Nm, device=dev), lens, output_size=int(poff_h[-1]))
            rows = torch.arange(int(poff_h[-1]), device=dev) - poff[owner] + (probes[:, 0].long() * n + probes[:, 1].long())[owner]
            pb = _vfr.VideoBank(V[rows], poff.to(torch.int32), 0, max_clips=int(lens_h.max()), total_moments=pmom, min_clips=int(lens_h.min()))
            sc = _vfr.score_moments(S, pb)                                       # [Ns, sum of span triangles]
            col = pb.mom_off[:-1] + torch.where(lens == 1, torch.zeros_like(lens), 2 * lens - 2)   # the full span of each triangle
            keys = (sc[:, col].t().contiguous().view(torch.int32).long() << 32) | ids[None, :]
            return keys

        def base():
            keys = dense_route()
            rkey = keys[torch.arange(Nm, device=dev), own]
            cnt = (keys < rkey[:, None]).sum(dim=1)
            top = keys.sort(dim=1).values[:, :K]
            return (top >> 32).to(torch.int32).view(torch.float32), top & 0xFFFFFFFF, cnt

        # the rank key of the new route: the own sentence's key (taken from the dense route once, outside the timing)
        row = {"shape": name, "sentences": Ns, "probes": Nm}
        bd = bi = bc = None
        try:
            if not baseline:
                raise RuntimeError("baseline not requested")
            bd, bi, bc = base()
            keys = dense_route()
            rkey = keys[torch.arange(Nm, device=dev), own]
            del keys
            rd = (rkey >> 32).to(torch.int32).view(torch.float32).contiguous()
            torch.cuda.synchronize()
        except (RuntimeError, torch.OutOfMemoryError) as exc:
            row["baseline"] = f"not run: {str(exc).splitlines()[0][:160]}"
            baseline = False
            torch.cuda.empty_cache()
            rd = torch.full((Nm,), 0.25, device=dev)                             # an arbitrary key between scores
        cnt = torch.zeros((1, Nm), dtype=torch.int64, device=dev)

        def new():
            cnt.zero_()
            return _vfr.score_sentences(S, bank, probes, K, 0, 0, rd, own, count_lt=cnt, workspace=ws)

        d, i, c = new()
        torch.cuda.synchronize()
        if baseline:
            row["identical_bits"] = bool(torch.equal(d, bd) and torch.equal(i, bi) and torch.equal(c[0], bc))
            del bd, bi, bc
        tn, tb = timed_pair(new, base if baseline else None, reps)
        row["new"], row["baseline_stats"] = stats(tn), stats(tb)
        pairs = len({(int(v), int(c_)) for v, s, e in probes_h.tolist() for c_ in range(s, e + 1)}) * Ns
        med = row["new"]["median_ms"]
        row["us_per_probe"] = round(1e3 * med / Nm, 4)
        row["algorithmic_tflops_over_call_time"] = round(3.0 * D * pairs / (med * 1e-3) / 1e12, 3)
        if baseline:
            b = row["baseline_stats"]
            row["factor"] = round(b["median_ms"] / med, 2)
            row["distinguishably_faster"] = bool(b["median_ms"] - med > max(b["iqr_ms"], row["new"]["iqr_ms"]))
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        torch.cuda.empty_cache()

    def random_probes(nm, max_len=6):
        v = rs.randint(0, Nv, nm)
        ln = rs.randint(1, max_len + 1, nm)
        s = (rs.rand(nm) * (n - ln + 1)).astype(np.int64)
        return np.stack([v, s, s + ln - 1], axis=1).astype(np.int64)

    if "a" in shapes:
        case("a", 5000, random_probes(5000), reps)
    if "b" in shapes:
        vids = rs.choice(Nv, 64, replace=False)
        case("b", 5000, np.asarray([(v, s, e) for v in vids for s, e in all_moments(n)], np.int64), reps)
    if "c" in shapes:
        for nm in (1, 8, 64):
            case(f"c{nm}", 33000, random_probes(nm), reps)
    if "d" in shapes:
        case("d", 33000, random_probes(33000), reps_d)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
