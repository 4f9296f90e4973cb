#!/usr/bin/env python3
"""Candidate-restricted retrieval (vfr_score_subset_f32) against the full-corpus passes on the same corpus, same process (GPU box).

    python tools/subset_bench.py [--videos 10000] [--queries 5000] [--reps 20] [--quick 0]

Builds bench.py's corpus (seeded features through the clip / query encoders, 21 clips per video), then:
  * parity: every pool = every video -> the moment level == vfr_score_topk_mfma (top-100 and two rank counts) and the video
    level == vfr_score_video_topk_f32 (top-100 and the own-video rank), ids, distance bits and counts;
  * timing, device events after warm-up, ALTERNATED rep by rep with the full-corpus pass of the same query batch:
      goal shapes  5 000 queries x 100 random candidates (own video included), k = 100, moments, 2 rank keys  (goal <= 1.0 ms)
                   64 queries x 1 000 candidates                                                           (goal <= 0.15 ms)
      requests     1 / 8 / 64 queries x {100, 1 000} candidates, both levels
      density      5 000 queries x {100, 300, 1 000, 3 000} candidates: where the subset path stops beating the full pass
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


def pools_for(rs, own, Nv, n):
    """n random distinct videos per query, the own video among them."""
    out = []
    for v in own:
        c = rs.choice(Nv, n, replace=False)
        if v not in c:
            c[0] = v
        out.append(c)
    return out


def main():
    args = sys.argv[1:]
    opt = {"--videos": "10000", "--queries": "5000", "--reps": "20", "--quick": "0"}
    for i in range(0, len(args), 2):
        opt[args[i]] = args[i + 1]
    Nv, Nq, reps, quick = int(opt["--videos"]), int(opt["--queries"]), int(opt["--reps"]), int(opt["--quick"])
    k, F = 100, 4096
    dev = torch.device("cuda", 0)
    counts = synth.clip_counts(Nv, 21, seed=123)
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
    rs = np.random.RandomState(7)
    own = rs.randint(0, Nv, Nq)
    out = {"videos": Nv, "queries": Nq, "clips": 21, "k": k}

    # rank keys: the 4th and the 40th key of each query's moment ranking (two "ground-truth" keys per query, as bench.py's two
    # IoU thresholds); the own video's best key for the video level
    td, ti, _ = _vfr.score_topk(Q, bank, 40, mode="mfma")
    rd = torch.stack([td[:, 3], td[:, 39]]).contiguous()
    ri = torch.stack([ti[:, 3], ti[:, 39]]).contiguous()
    shard = engine.CorpusShard(bank, 0, Nv, counts.astype(np.int64), mom.astype(np.int64), dev)
    okey = engine.own_best_keys(shard, Q, own, ops)
    od_, oi_ = engine._unpack_key(okey)
    od_, oi_ = od_.contiguous(), oi_.contiguous()

    # ---- parity: full pools == the full-corpus passes ----
    full = engine.candidate_lists([np.arange(Nv)] * Nq, num_videos=Nv, device=dev)
    fo, fv = full.on(dev)
    d, i, c = _vfr.score_subset(Q, bank, fo, fv, k, "moments", 0, rd, ri, max_list=full.max_list)
    wd, wi, wc = _vfr.score_topk(Q, bank, k, rd, ri, mode="mfma")
    par = {"moments_full_pools_eq_topk_mfma": bool(torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c, wc))}
    d, i, c = _vfr.score_subset(Q, bank, fo, fv, k, "videos", 0, od_[None], oi_[None], max_list=full.max_list)
    wd, wi, wc = _vfr.score_video_topk(Q, bank, k, od_, oi_, mode="mfma")
    par["videos_full_pools_eq_video_topk"] = bool(torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c[0], wc))
    print(f"parity: {par}", flush=True)
    out["parity"] = par
    del d, i, c, wd, wi, wc, full, fo, fv
    torch.cuda.empty_cache()

    # ---- timing ----
    wst = torch.empty((_vfr.lib().vfr_score_topk_mfma_workspace_bytes(Nq, Nv, int(off[-1]), k),), dtype=torch.uint8, device=dev)
    wsv = torch.empty((_vfr.lib().vfr_score_video_topk_workspace_bytes(Nq, Nv, int(off[-1]), k),), dtype=torch.uint8, device=dev)
    rows = []

    def case(nq, ncand, level, nrank):
        Qx = Q[:nq].contiguous()
        cl = engine.candidate_lists(pools_for(rs, own[:nq], Nv, ncand), num_videos=Nv, device=dev)
        o, v = cl.on(dev)
        if level == "moments":
            rdx, rix = rd[:nrank, :nq].contiguous(), ri[:nrank, :nq].contiguous()
        else:
            rdx, rix = od_[None, :nq].contiguous(), oi_[None, :nq].contiguous()
        cnt = torch.zeros((max(1, rdx.shape[0]), nq), dtype=torch.int64, device=dev)
        ws = torch.empty((max(1, _vfr.lib().vfr_score_subset_workspace_bytes(nq, cl.vid.size, cl.max_list, k,
                                                                             _vfr.SUBSET_LEVELS[level])),), dtype=torch.uint8, device=dev)
        use_rank = nrank > 0

        def sub():
            _vfr.score_subset(Qx, bank, o, v, k, level, 0, rdx if use_rank else None, rix if use_rank else None,
                              count_lt=cnt[:rdx.shape[0]] if use_rank else None, workspace=ws, max_list=cl.max_list)

        if level == "moments":
            def fullp():
                _vfr.score_topk(Qx, bank, k, rdx if use_rank else None, rix if use_rank else None,
                                count_lt=cnt[:rdx.shape[0]] if use_rank else None, workspace=wst, mode="mfma")
        else:
            def fullp():
                _vfr.score_video_topk(Qx, bank, k, rdx[0] if use_rank else None, rix[0] if use_rank else None,
                                      count=cnt[0] if use_rank else None, workspace=wsv, mode="mfma")
        ts, tf, ts_min, tf_min = timed_pair(sub, fullp, reps)
        row = {"queries": nq, "candidates": ncand, "level": level, "rank_keys": nrank, "subset_ms": round(ts, 4),
               "full_ms": round(tf, 4), "subset_min_ms": round(ts_min, 4), "full_min_ms": round(tf_min, 4)}
        print(f"{nq:5d} q x {ncand:5d} cand  {level:7s} ranks={nrank}: subset {ts:.3f} ms (min {ts_min:.3f})   full pass "
              f"{tf:.3f} ms (min {tf_min:.3f})", flush=True)
        rows.append(row)
        return ts

    goals = {}
    t = case(Nq, 100, "moments", 2)
    goals[f"{Nq}q_x_100_moments_2ranks_le_1.0ms"] = {"ms": round(t, 4), "met": t <= 1.0}
    t = case(64, 1000, "moments", 2)
    goals["64q_x_1000_moments_2ranks_le_0.15ms"] = {"ms": round(t, 4), "met": t <= 0.15}
    if not quick:
        for level in ("moments", "videos"):
            for nq in (1, 8, 64):
                for ncand in (100, 1000):
                    case(nq, ncand, level, 0 if level == "moments" else 1)
        for ncand in (100, 300, 1000, 3000):
            case(Nq, ncand, "moments", 0)
            case(Nq, ncand, "moments", 2)
        case(Nq, 100, "videos", 1)
    out["goals"] = goals
    out["rows"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
