#!/usr/bin/env python3
"""Diversified moment retrieval (vfr_score_moment_nms_f32) against the video-level pass it builds on (vfr_score_video_topk_f32),
same process, same inputs (GPU box).

    python tools/moment_nms_bench.py [--videos 10000] [--queries 5000] [--clips 21|6|didemo] [--k 100] [--reps 20]

Builds bench.py's corpus (seeded features through the clip / query encoders), then for (per_video, nms_iou) in
(1, 1.0), (3, 0.5), (0, 0.5), (0, 1.0):
  * parity: the "mfma" pass == the "exact" pass (ids and distance bits); identity A: per_video = 1 == the video top-k;
    identity B: no cap, nms_iou = 1 == the exact moment top-k;
  * timing, device events after warm-up, ALTERNATED rep by rep with the video pass (top-k only) for the whole batch and for
    1 / 8 / 64-query requests.
One JSON line at the end."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import vfr_amd  # noqa: E402,F401
from vfr_amd import _vfr, engine, models, synth  # noqa: E402

CONFIGS = ((1, 1.0), (3, 0.5), (0, 0.5), (0, 1.0))


def timed_pair(fa, fb, reps, warm=3):
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            acc.append(s.elapsed_time(e))
    return float(np.median(ta)), float(np.median(tb)), float(np.min(ta)), float(np.min(tb))


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--queries": "5000", "--clips": "21", "--k": "100", "--reps": "20"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, Nq, k, reps = int(opt["--videos"]), int(opt["--queries"]), int(opt["--k"]), int(opt["--reps"])
    clips = opt["--clips"] if opt["--clips"] == "didemo" else int(opt["--clips"])
    F = 4096
    dev = torch.device("cuda", 0)
    counts = synth.clip_counts(Nv, clips, seed=123)
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    mom = np.concatenate([[0], np.cumsum(counts.astype(np.int64) * (counts + 1) // 2)])
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    raw = torch.rand((int(off[-1]), F), generator=gen, device=dev)
    seg = raw / (raw.norm(dim=1, keepdim=True) + 1e-5)
    clip_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    nloc = (clip_off[1:] - clip_off[:-1]).long()
    ctx = torch.segment_reduce(raw, "sum", lengths=nloc, axis=0) / nloc[:, None].float()
    ctx = ctx / (ctx.norm(dim=1, keepdim=True) + 1e-5)
    del raw
    tokens = torch.from_numpy(synth.query_tokens(Nq, seed=123)).to(dev)
    sd = synth.model_weights(F, seed=123)
    model = models.CALModel(2 * F + 2, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]))
    model.load_state_dict({k_: torch.from_numpy(v) for k_, v in sd.items()})
    model = model.to(dev).eval()
    ops = engine.HipOps()
    with torch.no_grad():
        emb = model.encode_clips(seg, ctx, clip_off)
        Q = engine.encode_queries(model, tokens, dev, ops)
    del seg, ctx
    bank = _vfr.VideoBank(emb, clip_off, 0, max_clips=int(counts.max()), total_moments=int(mom[-1]), min_clips=int(counts.min()))
    out = {"videos": Nv, "queries": Nq, "clips": str(clips), "k": k}

    # ---- parity ----
    vd, vi, _ = _vfr.score_video_topk(Q, bank, k, mode="exact")
    td, ti, _ = _vfr.score_topk(Q, bank, k, mode="exact")
    parity = {}
    for pv, thr in CONFIGS:
        d_f, i_f = _vfr.score_moment_nms(Q, bank, k, pv, thr, mode="mfma")
        d_e, i_e = _vfr.score_moment_nms(Q, bank, k, pv, thr, mode="exact")
        row = {"fast_vs_exact": bool(torch.equal(i_f, i_e) and torch.equal(d_f, d_e))}
        if pv == 1:
            row["identity_A_vs_video_topk"] = bool(torch.equal(i_f, vi) and torch.equal(d_f, vd))
        if pv == 0 and thr >= 1:
            row["identity_B_vs_moment_topk"] = bool(torch.equal(i_f, ti) and torch.equal(d_f, td))
        vid = np.searchsorted(mom, i_f.cpu().numpy(), side="right") - 1
        row["max_per_video"] = int(max(np.bincount(r[r >= 0]).max() for r in vid))
        row["videos_per_query_mean"] = float(np.mean([len(np.unique(r[r >= 0])) for r in vid]))
        parity[f"{pv},{thr}"] = row
        print(f"parity per_video={pv} nms_iou={thr}: {row}", flush=True)
        del d_f, i_f, d_e, i_e
    out["parity"] = parity
    del vd, vi, td, ti

    # ---- timing: whole batch, then serving requests ----
    wsv = torch.empty((_vfr.lib().vfr_score_video_topk_workspace_bytes(Nq, Nv, int(off[-1]), k),), dtype=torch.uint8, device=dev)
    rows = {}
    for nq in (Nq, 64, 8, 1):
        Qx = Q[:nq].contiguous()

        def video():
            _vfr.score_video_topk(Qx, bank, k, mode="mfma", workspace=wsv)
        per = {}
        for pv, thr in CONFIGS:
            wsn = torch.empty((_vfr.lib().vfr_score_moment_nms_workspace_bytes(nq, Nv, int(off[-1]), k, pv),), dtype=torch.uint8,
                              device=dev)

            def nms():
                _vfr.score_moment_nms(Qx, bank, k, pv, thr, mode="mfma", workspace=wsn)
            tn, tv, tn_min, tv_min = timed_pair(nms, video, reps)
            per[f"{pv},{thr}"] = {"nms_ms": round(tn, 4), "video_ms": round(tv, 4), "nms_min_ms": round(tn_min, 4),
                                  "video_min_ms": round(tv_min, 4), "added_ms": round(tn - tv, 4)}
            print(f"{nq:5d} queries  per_video={pv} nms_iou={thr}: nms pass {tn:.3f} ms (min {tn_min:.3f})   video pass "
                  f"{tv:.3f} ms (min {tv_min:.3f})   added {tn - tv:+.3f} ms", flush=True)
            del wsn
        rows[str(nq)] = per
    out["timing"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
