#!/usr/bin/env python3
"""Generate the training-driver fixtures tests/golden/g13_*, g14_* by running the REFERENCE itself (the build machine only).

The unmodified reference (``model/data.py``, ``model/main.py``) is imported with the stubs of tools/gen_golden.py (``h5py``,
and tensorboard's ``SummaryWriter`` replaced by a recorder of the logged scalars); only data is written.

    python tools/gen_golden_train.py            # writes tests/golden/g13_triplet_batches.json, g14_train_epochs.npz

G13  CustomBatchSampler's batches (model/data.py:249-343) under random.seed(s) on a toy split: train mode with same_length
     True and False, test mode, and a split whose full-length moment has no same-length intra-negative (IndexError).
G14  Trainer.train_epoch x 2 with test_epoch and StepLR (model/main.py:43-119, 358-385) on a reduced CALModel (F = 64, LSTM
     hidden 16, vocab 60, visual_fc[3].p = 0) with optim.Adam(lr=5e-4, weight_decay=5e-3), batch_size 16, features pooled
     by the reference's CustomDataset from per-video .npy files.
"""
import json
import random
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REF = Path("/root/reference")
sys.modules.setdefault("h5py", types.ModuleType("h5py"))
sys.path.insert(0, str(REF / "model"))

LOG = []


class Recorder:                                          # stands in for tensorboard's SummaryWriter
    def __init__(self, tag="", *a, **k):
        self.tag = tag

    def add_scalar(self, name, value, global_step=None):
        LOG.append((self.tag, name, float(value), int(global_step)))

    def add_scalars(self, name, scalars, global_step=None):
        for k, v in scalars.items():
            LOG.append((self.tag, f"{name}/{k}", float(v), int(global_step)))

    def add_figure(self, *a, **k):
        pass


_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = Recorder
sys.modules["torch.utils.tensorboard"] = _tb

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import data as ref_data  # noqa: E402  (reference)
import main as ref_main  # noqa: E402
import models as ref_models  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from vfr_amd import synth  # noqa: E402

OUT = ROOT / "tests" / "golden"
torch.set_num_threads(8)

G14 = dict(F=64, hidden=16, vocab=60, nv=40, nq=120, seed=14, batch_size=16, lr=5e-4, weight_decay=5e-3, sched_step=1,
           sched_gamma=0.1, sampler_seed=123)


def toy_split(nv, nq, seed, full_length_ok=False):
    """Video names, clip counts, annotations (4 spans each) of a DiDeMo-like toy split.  Full-length spans are cut by one
    clip unless ``full_length_ok`` (with same_length=True they have no intra-negative and the reference raises)."""
    counts = synth.clip_counts(nv, "didemo", seed=seed)
    own, times = synth.annotations(nq, counts, seed=seed)
    videos = [f"v{v:05d}" for v in range(nv)]
    annots = {}
    for q in range(nq):
        n = int(counts[own[q]])
        spans = [[s, e - 1 if (s == 0 and e == n - 1 and not full_length_ok) else e] for s, e in times[q]]
        annots[q] = dict(video=videos[own[q]], description="", times=spans)
    return videos, counts, annots


def as_rows(batches):
    return [[[s["annotation_id"], s["video_pos"], s["video_neg"], int(s["start_t"]), int(s["end_t"]), int(s["start_tn"]),
              int(s["end_tn"])] for s in b] for b in batches]


def g13_triplet_batches():
    videos, counts, annots = toy_split(40, 120, seed=13)
    nsi = {v: int(c) for v, c in zip(videos, counts)}
    out = dict(num_segments_info=nsi, annotations={str(k): v for k, v in annots.items()}, batch_size=16, cases={})
    for seed in (5, 2024):
        for tag, train, same in (("train_same", True, True), ("train_iou", True, False), ("test_same", False, True),
                                 ("test_iou", False, False)):
            random.seed(seed)
            sampler = ref_data.CustomBatchSampler(16, annots, nsi, train=train, same_length=same)
            out["cases"][f"{tag}_seed{seed}"] = dict(seed=seed, train=train, same_length=same, batches=as_rows(list(iter(sampler))),
                                                    next_random=random.random())
    # a full-length positive moment with same_length=True: no candidate, the reference raises
    v2, c2, a2 = toy_split(6, 30, seed=7, full_length_ok=True)
    nsi2 = {v: int(c) for v, c in zip(v2, c2)}
    errors = {}
    for seed in (5,):
        random.seed(seed)
        try:
            list(iter(ref_data.CustomBatchSampler(4, a2, nsi2, train=True, same_length=True)))
            errors[str(seed)] = None
        except Exception as e:                          # noqa: BLE001 -- recorded, the test expects the same type
            errors[str(seed)] = type(e).__name__
    out["raising"] = dict(num_segments_info=nsi2, annotations={str(k): v for k, v in a2.items()}, batch_size=4, errors=errors)
    json.dump(out, open(OUT / "g13_triplet_batches.json", "w"))
    print("G13", {k: len(v["batches"]) for k, v in out["cases"].items()}, errors)


def sampled(name, a):
    """What G14 keeps of a parameter-sized tensor: every row of the small ones, every 10th row of the two visual_fc weights
    (their whole-tensor float64 sums are kept as well)."""
    return a[::10] if name in ("visual_fc.0.weight", "visual_fc.2.weight") else a


def g14_train_epochs():
    c = G14
    F, H, V = c["F"], c["hidden"], c["vocab"]
    videos, counts, annots = toy_split(c["nv"], c["nq"], seed=c["seed"])
    tokens = synth.query_tokens(c["nq"], vocab=V, seed=c["seed"])
    for q in range(c["nq"]):
        annots[q]["description"] = " ".join(f"w{t}" for t in tokens[q] if t > 0)
    sd = synth.model_weights(F, vocab=V, hidden=H, seed=c["seed"])
    ref_data.FEATURE_DIM["vgg19"] = F                    # the reference reads it at load time
    rs = np.random.RandomState(c["seed"] + 100)
    with tempfile.TemporaryDirectory() as td:
        d = Path(td) / "features_vgg19"
        d.mkdir()
        for v, n in zip(videos, counts):
            T = int(n) * 25 - int(rs.randint(0, 20))
            x = rs.rand(T, F).astype(np.float32)
            x[x < 0.3] = 0.0
            np.save(d / f"vgg19_ft_{v}.npy", x)
        lines = [f"w{i} " + " ".join(repr(float(x)) for x in sd["word_embedding.weight"][i]) for i in range(1, V)]
        (Path(td) / "glove.6B.100d.txt").write_text("\n".join(lines) + "\n", encoding="UTF-8")
        wi = ref_data.WordIndexer(td)
        ds = ref_data.CustomDataset(videos, annots, td, "vgg19", word_indexer=wi)
    ref_data.FEATURE_DIM["vgg19"] = 4096
    assert np.array_equal(wi.get_embeddings().numpy(), sd["word_embedding.weight"])
    lang = np.concatenate([ds.lang_features[q].numpy() for q in range(c["nq"])])
    assert np.array_equal(lang, tokens)

    model = ref_models.CALModel(2 * F + 2, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.visual_fc[3].p = 0.0
    optimizer = torch.optim.Adam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=c["sched_step"], gamma=c["sched_gamma"])
    trainer = ref_main.Trainer(train_writer=Recorder("train"), test_writer=Recorder("test"), val_writer=Recorder("val"),
                               device="cpu")
    random.seed(c["sampler_seed"])
    LOG.clear()
    train_iter = DataLoader(ds, shuffle=False, collate_fn=ref_data.custom_collate,
                            batch_sampler=ref_data.CustomBatchSampler(c["batch_size"], annots, ds.num_segments_info))
    test_iter = DataLoader(ds, shuffle=False, collate_fn=ref_data.custom_collate,
                           batch_sampler=ref_data.CustomBatchSampler(c["batch_size"], annots, ds.num_segments_info, train=False))
    train_losses, test_losses, lrs = [], [], []
    for epoch in range(2):
        lrs.append(optimizer.param_groups[0]["lr"])
        train_losses.append(trainer.train_epoch(model, train_iter, optimizer))
        test_losses.append(trainer.test_epoch(model, test_iter))
        scheduler.step()
    out = dict(config=json.dumps(c), videos=np.array(videos), counts=np.asarray(counts, np.int32), tokens=tokens,
               times=np.array([annots[q]["times"] for q in range(c["nq"])], np.int32),
               own=np.array([videos.index(annots[q]["video"]) for q in range(c["nq"])], np.int32),
               seg=np.concatenate([ds.video_features[v]["segment_features"] for v in videos]).astype(np.float32),
               ctx=np.stack([np.asarray(ds.video_features[v]["context_features"], np.float32) for v in videos]),
               train_losses=np.array(train_losses), test_losses=np.array(test_losses), lrs=np.array(lrs),
               step_loss=np.array([v for t, n, v, s in LOG if t == "train" and n == "loss"]),
               step_grad_norm=np.array([v for t, n, v, s in LOG if t == "train" and n == "grad_norm"]),
               test_log=np.array([v for t, n, v, s in LOG if t == "test"]),
               test_log_names=np.array([n for t, n, v, s in LOG if t == "test"]))
    assert np.array_equal(out["seg"].astype(np.float64), np.concatenate([ds.video_features[v]["segment_features"] for v in videos]))
    for k, v in sd.items():
        out[f"init_sum/{k}"] = np.float64(v.astype(np.float64).sum())
    state = optimizer.state_dict()["state"]
    for i, (name, p) in enumerate(model.named_parameters()):
        out[f"final_sum/{name}"] = np.float64(p.detach().numpy().astype(np.float64).sum())
        out[f"final/{name}"] = sampled(name, p.detach().numpy())
        if p.requires_grad:
            idx = [j for j, q in enumerate(optimizer.param_groups[0]["params"]) if q is p][0]
            st = state[idx]
            out[f"step/{name}"] = np.float32(st["step"].item())
            for key in ("exp_avg", "exp_avg_sq"):
                out[f"{key}/{name}"] = sampled(name, st[key].numpy())
                out[f"{key}_sum/{name}"] = np.float64(st[key].numpy().astype(np.float64).sum())
    np.savez_compressed(OUT / "g14_train_epochs.npz", **out)
    print("G14 train", train_losses, "test", test_losses, "steps", len(out["step_loss"]))


if __name__ == "__main__":
    names = sys.argv[1:] or ["g13_triplet_batches", "g14_train_epochs"]
    for name in names:
        globals()[name]()
