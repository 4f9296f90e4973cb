#!/usr/bin/env python3
"""Training steps of CALModel on a DiDeMo-train-shaped synthetic split (8 400 videos, 86/14 six/five clips, 33 000
annotations, F = 4096, hidden 1000, batch_size 128, dropout 0.3): the same batches along two paths.

  (a) host path    the reference's: make_visual_features + custom_collate on the host, H2D, torch.optim.Adam, utils.grad_norm
  (b) device path  training.TripletLoader (one gather launch) + training.Adam (one launch) + training.grad_norm (fused sums)

Both run the HIP autograd forward / backward.  Prints ms per step (unsynchronised loop) and a per-phase split (a synchronised
pass: sampler, gather / H2D, forward + backward, optimizer, grad norm), then the Adam step alone on the full model's trainable
parameters next to torch.optim.Adam (default foreach) on the same grads.

usage: train_epoch_bench.py [steps] [warmup]
"""
import random
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import vfr_amd  # noqa: E402,F401
from helpers import MemoryDataset  # noqa: E402
from vfr_amd import models, synth, training, utils  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEV = "cuda:0"
F, H, NV, NQ, BS = 4096, 1000, 8400, 33000, 128


def split():
    counts = synth.clip_counts(NV, "didemo", seed=5)
    seg, ctx = synth.video_features(counts, F, seed=5)
    tokens = synth.query_tokens(NQ, seed=5)
    own, times = synth.annotations(NQ, counts, seed=5)
    times = [[[s, e - 1 if s == 0 and e == counts[own[q]] - 1 else e] for s, e in t] for q, t in enumerate(times)]
    return MemoryDataset(seg, ctx, counts, tokens, own, times)


def make_model():
    sd = synth.model_weights(F, vocab=400, hidden=H, seed=6)
    m = models.CALModel(2 * F + 2, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).train()


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def host_batch(ds, b):
    out = training.custom_collate(training.host_triplets(ds, b))
    return {k: v.to(DEV, non_blocking=False) for k, v in out.items()}


def fwd_bwd(trainer, m, opt, batch):
    opt.zero_grad()
    pe, ne, ie = m(batch["posit"]), m(batch["intra"]), m(batch["inter"])
    le = m(batch["lang"], False, DEV)
    loss, n = trainer._loss(pe, ne, ie, le, batch["maskp"], batch["maskn"], batch.get("n_samples"))
    loss.backward()
    return loss


def run(path, ds, batches):
    m = make_model()
    trainer = training.Trainer(device=DEV)
    loader = training.TripletLoader(ds, training.TripletBatchSampler(BS, ds.annotations, ds.num_segments_info), DEV)
    opt = training.Adam(m.parameters(), lr=5e-4, weight_decay=5e-3) if path == "device" else \
        torch.optim.Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)

    def get(b):
        return loader.collate(b) if path == "device" else host_batch(ds, b)

    def gnorm():
        return training.grad_norm(m, opt) if path == "device" else utils.grad_norm(m)
    torch.manual_seed(0)
    for b in batches[:WARMUP]:
        fwd_bwd(trainer, m, opt, get(b))
        opt.step()
        gnorm()
    # (1) the unsynchronised loop: what a training epoch costs per step (sampling included)
    random.seed(7)
    sampler = iter(training.TripletBatchSampler(BS, ds.annotations, ds.num_segments_info))
    t0 = sync()
    for _ in range(STEPS):
        b = next(sampler)
        fwd_bwd(trainer, m, opt, get(b))
        opt.step()
        gnorm()
    total = (sync() - t0) / STEPS * 1e3
    # (2) the phases, synchronised between them
    ph = dict(sampler=0.0, gather=0.0, fwd_bwd=0.0, optimizer=0.0, grad_norm=0.0)
    random.seed(8)
    sampler = iter(training.TripletBatchSampler(BS, ds.annotations, ds.num_segments_info))
    for _ in range(STEPS):
        t = sync()
        b = next(sampler)
        t1 = sync(); ph["sampler"] += t1 - t
        batch = get(b)
        t2 = sync(); ph["gather"] += t2 - t1
        fwd_bwd(trainer, m, opt, batch)
        t3 = sync(); ph["fwd_bwd"] += t3 - t2
        opt.step()
        t4 = sync(); ph["optimizer"] += t4 - t3
        gnorm()
        t5 = sync(); ph["grad_norm"] += t5 - t4
    return total, {k: v / STEPS * 1e3 for k, v in ph.items()}


def adam_alone(reps=50):
    m = make_model()
    params = [p for p in m.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    rs = np.random.RandomState(3)
    for p in params:
        p.grad = torch.from_numpy(rs.randn(*p.shape).astype(np.float32) * 1e-3).to(DEV)
    out = {}
    for name, opt in (("training.Adam (vfr_adam_step_f32)", training.Adam(params, lr=5e-4, weight_decay=5e-3)),
                      ("torch.optim.Adam (foreach)", torch.optim.Adam(params, lr=5e-4, weight_decay=5e-3))):
        for _ in range(5):
            opt.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            opt.step()
        e1.record()
        e1.synchronize()
        out[name] = e0.elapsed_time(e1) / reps * 1e3
    return n, out


def main():
    t = time.perf_counter()
    ds = split()
    print(f"split: {NV} videos ({sum(1 for v in ds.num_segments_info.values() if v == 6)} with 6 clips), {NQ} annotations, "
          f"F = {F}, hidden {H}, batch_size {BS}, dropout 0.3; built in {time.perf_counter() - t:.1f} s")
    random.seed(3)
    it = iter(training.TripletBatchSampler(BS, ds.annotations, ds.num_segments_info))
    batches = [next(it) for _ in range(WARMUP)]
    res = {}
    for path in ("host", "device"):
        res[path] = run(path, ds, batches)
    print(f"{STEPS} steps after {WARMUP} warm-up steps; ms per step (unsynchronised loop) and the phases of a synchronised pass:")
    print(f"{'path':8s} {'ms/step':>8s} | {'sampler':>8s} {'gather/H2D':>10s} {'fwd+bwd':>8s} {'optimizer':>9s} {'grad_norm':>9s}")
    for path, (total, ph) in res.items():
        print(f"{path:8s} {total:8.2f} | {ph['sampler']:8.2f} {ph['gather']:10.2f} {ph['fwd_bwd']:8.2f} {ph['optimizer']:9.2f} "
              f"{ph['grad_norm']:9.2f}")
    n, ad = adam_alone()
    mb = n * 4 * 7 / 1e6
    print(f"Adam step alone on {n} trainable parameters ({mb:.1f} MB moved per step):")
    for name, us in ad.items():
        print(f"  {name:36s} {us:8.1f} us  ({mb / us:.2f} TB/s)")


if __name__ == "__main__":
    main()
