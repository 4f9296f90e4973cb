#!/usr/bin/env python3
"""Video-level retrieval pass (vfr_score_video_topk_f32) against the moment-level fused pass (vfr_score_topk_mfma), same
process, same inputs (GPU box).

    python tools/video_topk_bench.py [--videos 10000] [--queries 5000] [--clips 21|6|didemo] [--k 100] [--reps 20]

Builds bench.py's corpus (seeded features through the clip / query encoders), then:
  * parity: the "mfma" video pass == the "exact" video pass (top-k ids, distances, rank counts), and its top-k == the
    exact moment-level top-448 reduced to distinct videos wherever that list holds k distinct videos;
  * timing, device events after warm-up, the two passes ALTERNATED rep by rep: video pass (top-k + rank counts of the own
    video) vs moment pass (top-k only, k = 100), for the whole batch and for 1 / 8 / 64-query requests;
  * the fast path's per-query work: videos given an exact triangle (candidates + undecided rank counts), and of them the
    undecided ones.
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
    own, _ = synth.annotations(Nq, counts, seed=123)
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
    shard = engine.CorpusShard(bank, 0, Nv, counts, mom, dev)
    okeys = engine.own_best_keys(shard, Q, own, ops)
    od_own, oi_own = engine._unpack_key(okeys)
    od_own, oi_own = od_own.contiguous(), oi_own.contiguous()
    out = {"videos": Nv, "queries": Nq, "clips": str(clips), "k": k}

    # ---- parity ----
    wsv = torch.empty((_vfr.lib().vfr_score_video_topk_workspace_bytes(Nq, Nv, int(off[-1]), k),), dtype=torch.uint8, device=dev)
    d_f, i_f, c_f = _vfr.score_video_topk(Q, bank, k, od_own, oi_own, mode="mfma", workspace=wsv)
    st = _vfr.score_video_topk_stats(wsv, Nq, bank)
    d_e, i_e, c_e = _vfr.score_video_topk(Q, bank, k, od_own, oi_own, mode="exact")
    out["parity_fast_vs_exact"] = bool(torch.equal(i_f, i_e) and torch.equal(d_f, d_e) and torch.equal(c_f, c_e))
    del d_e, i_e, c_e
    md, mi, _ = _vfr.score_topk(Q, bank, 448, mode="exact")
    mi_h, i_h = mi.cpu().numpy(), i_f.cpu().numpy()
    checked = agree = 0
    for q in range(Nq):
        v = np.searchsorted(mom, mi_h[q], side="right") - 1
        _, first = np.unique(v, return_index=True)
        pos = np.sort(first)
        if len(pos) >= k:
            checked += 1
            agree += int(np.array_equal(mi_h[q, pos[:k]], i_h[q]))
    out["parity_vs_exact_moment_topk448"] = {"queries_checked": checked, "identical": agree}
    out["fast_path_per_query"] = {"triangles_mean": float(st[:, 0].mean()), "triangles_median": float(np.median(st[:, 0])),
                                  "triangles_max": int(st[:, 0].max()), "undecided_mean": float(st[:, 1].mean()),
                                  "undecided_max": int(st[:, 1].max())}
    del md, mi

    # ---- timing: whole batch, then serving requests ----
    wsm = _vfr.topk_workspace(Nq, Nv, k, dev, total_clips=int(off[-1]))
    rows = {}
    for nq in (Nq, 64, 8, 1):
        Qx, dx, ix = Q[:nq].contiguous(), od_own[:nq].contiguous(), oi_own[:nq].contiguous()
        cnt = torch.zeros((nq,), dtype=torch.int64, device=dev)

        def video():
            cnt.zero_()
            _vfr.score_video_topk(Qx, bank, k, dx, ix, count=cnt, mode="mfma", workspace=wsv)

        def moment():
            _vfr.score_topk(Qx, bank, k, mode="mfma", workspace=wsm)
        rd, ri = torch.stack([dx, dx]).contiguous(), torch.stack([ix, ix]).contiguous()
        cl = torch.zeros((2, nq), dtype=torch.int64, device=dev)

        def moment_rank():                   # the same pass with rank counts of the own video's best moment (2 keys, as evaluate)
            cl.zero_()
            _vfr.score_topk(Qx, bank, k, rd, ri, count_lt=cl, mode="mfma", workspace=wsm)
        tv, tm, tv_min, tm_min = timed_pair(video, moment, reps)
        tv2, tr, _, tr_min = timed_pair(video, moment_rank, reps)
        rows[str(nq)] = {"video_ms": round(tv, 4), "moment_topk_mfma_ms": round(tm, 4), "video_min_ms": round(tv_min, 4),
                         "moment_min_ms": round(tm_min, 4), "speedup_vs_topk": round(tm / tv, 3),
                         "moment_topk_rank_mfma_ms": round(tr, 4), "speedup_vs_topk_rank": round(tr / tv2, 3)}
        print(f"{nq:5d} queries: video pass {tv:.3f} ms (min {tv_min:.3f})   moment top-{k} mfma {tm:.3f} ms (min {tm_min:.3f})"
              f" x{tm / tv:.2f}   moment top-{k} + rank counts {tr:.3f} ms x{tr / tv2:.2f}", flush=True)
    out["timing"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
