"""training.py on the host: the triplet sampler against the reference's batches (G13), a whole CPU training run against the
reference's trajectory (G14), the optimizer's state layout and the checkpoint dict."""
import copy
import json
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import MemoryDataset
from vfr_amd import models, synth, training


def g13():
    return json.load(open(GOLDEN / "g13_triplet_batches.json"))


def int_keys(annots):
    return {int(k): v for k, v in annots.items()}


def rows(batches):
    return [[[s["annotation_id"], s["video_pos"], s["video_neg"], s["start_t"], s["end_t"], s["start_tn"], s["end_tn"]]
             for s in b] for b in batches]


@pytest.mark.parametrize("case", sorted(g13()["cases"]))
def test_sampler_matches_reference_batches(case):
    g = g13()
    c = g["cases"][case]
    random.seed(c["seed"])
    sampler = training.TripletBatchSampler(g["batch_size"], int_keys(g["annotations"]), g["num_segments_info"],
                                           train=c["train"], same_length=c["same_length"])
    got = rows(iter(sampler))
    assert got == c["batches"]
    assert all(type(x) is int for b in got for s in b for x in s[3:])
    assert random.random() == c["next_random"]                  # the same amount of randomness was drawn


def test_sampler_raises_where_the_reference_raises():
    r = g13()["raising"]
    for seed, err in r["errors"].items():
        random.seed(int(seed))
        sampler = training.TripletBatchSampler(r["batch_size"], int_keys(r["annotations"]), r["num_segments_info"])
        if err is None:
            list(iter(sampler))
        else:
            with pytest.raises({"IndexError": IndexError, "ValueError": ValueError}[err]):
                list(iter(sampler))


def test_sampler_builds_no_list_per_annotation():
    counts = synth.clip_counts(5000, "didemo", seed=3)
    own, times = synth.annotations(20000, counts, seed=3)
    nsi = {f"v{v:05d}": int(n) for v, n in enumerate(counts)}
    videos = list(nsi)
    annots = {q: dict(video=videos[own[q]], times=[[s, e - 1 if s == 0 and e == counts[own[q]] - 1 else e] for s, e in times[q]])
              for q in range(len(own))}
    for same in (True, False):
        sampler = training.TripletBatchSampler(128, annots, nsi, same_length=same)

        def refuse(*a, **k):
            raise AssertionError("the O(V) candidate list was built")
        sampler.get_possible_videos = refuse
        random.seed(1)
        n = sum(len(b) for b in iter(sampler))
        assert n == len(annots)
        # candidate lists: one per distinct key -- (clips, span) or (clips, annotated spans) -- and per negative threshold,
        # never one per annotation: 6 thresholds + at most 5 * 21 same-length keys; the IoU rule keys by the span set
        assert sampler.candidate_builds <= 6 + (21 + 15 if same else len(annots))
        if same:
            assert sampler.candidate_builds < 100


def test_inter_negative_maps_into_the_reference_list():
    nsi = {"a": 5, "b": 6, "c": 5, "d": 6, "e": 3, "f": 6}
    s = training.TripletBatchSampler(4, {}, nsi)
    s.train = False
    for video in ("a", "b", "d"):
        for min_clips in (1, 4, 6):
            if nsi[video] < min_clips:
                continue
            ref = s.get_possible_videos(min_clips)
            ref.remove(video)
            for j in range(len(ref)):
                state = random.getstate()
                random.seed(0)
                s.train = True
                orig = random.choice
                random.choice = lambda seq, j=j: seq[j]
                try:
                    assert s._inter_negative(video, min_clips) == ref[j]
                finally:
                    random.choice = orig
                    random.setstate(state)


def g14():
    z = np.load(GOLDEN / "g14_train_epochs.npz", allow_pickle=False)
    return z, json.loads(str(z["config"]))


def g14_dataset(z):
    times = [t.tolist() for t in z["times"]]
    return MemoryDataset(z["seg"], z["ctx"], z["counts"], z["tokens"], z["own"], times)


def g14_model(c, device="cpu"):
    sd = synth.model_weights(c["F"], vocab=c["vocab"], hidden=c["hidden"], seed=c["seed"])
    m = models.CALModel(2 * c["F"] + 2, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=c["hidden"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.visual_fc[3].p = 0.0
    return m.to(device), sd


class Log:
    def __init__(self):
        self.items = []

    def add_scalar(self, name, value, global_step=None):
        self.items.append((name, float(value), global_step))

    def add_scalars(self, name, scalars, global_step=None):
        for k, v in scalars.items():
            self.items.append((f"{name}/{k}", float(v), global_step))


def run_g14(device, writers=True):
    z, c = g14()
    ds = g14_dataset(z)
    model, sd = g14_model(c, device)
    for k, v in sd.items():
        assert v.astype(np.float64).sum() == z[f"init_sum/{k}"]       # the recorded initial weights
    opt = training.Adam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=c["sched_step"], gamma=c["sched_gamma"])
    tw, sw = (Log(), Log()) if writers else (None, None)
    trainer = training.Trainer(train_writer=tw, test_writer=sw, device=device)
    random.seed(c["sampler_seed"])
    train_iter = training.TripletLoader(ds, training.TripletBatchSampler(c["batch_size"], ds.annotations, ds.num_segments_info),
                                        device)
    test_iter = training.TripletLoader(ds, training.TripletBatchSampler(c["batch_size"], ds.annotations, ds.num_segments_info,
                                                                        train=False), device)
    tr, te, lrs = [], [], []
    for _ in range(2):
        lrs.append(opt.param_groups[0]["lr"])
        tr.append(trainer.train_epoch(model, train_iter, opt))
        te.append(trainer.test_epoch(model, test_iter))
        sched.step()
    return z, model, opt, tr, te, lrs, tw, sw


def test_cpu_training_reproduces_reference_trajectory():
    z, model, opt, tr, te, lrs, tw, sw = run_g14("cpu")
    assert lrs == z["lrs"].tolist() and lrs[1] != lrs[0]
    loss = [v for n, v, s in tw.items if n == "loss"]
    gn = [v for n, v, s in tw.items if n == "grad_norm"]
    assert np.array_equal(loss, z["step_loss"]) and np.array_equal(gn, z["step_grad_norm"])
    assert tr == z["train_losses"].tolist() and te == z["test_losses"].tolist()
    assert [v for n, v, s in sw.items] == z["test_log"].tolist()
    assert [n for n, v, s in sw.items] == z["test_log_names"].tolist()
    for name, p in model.named_parameters():
        a = p.detach().numpy()
        assert a.astype(np.float64).sum() == z[f"final_sum/{name}"], name
        sel = a[::10] if name in ("visual_fc.0.weight", "visual_fc.2.weight") else a
        assert np.array_equal(sel, z[f"final/{name}"]), name
        if p.requires_grad:
            st = opt.state[p]
            assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
            assert st["step"].item() == z[f"step/{name}"]
            for key in ("exp_avg", "exp_avg_sq"):
                s = st[key].numpy()
                assert s.astype(np.float64).sum() == z[f"{key}_sum/{name}"], (name, key)
                assert np.array_equal(s[::10] if name in ("visual_fc.0.weight", "visual_fc.2.weight") else s,
                                      z[f"{key}/{name}"]), (name, key)


def test_cpu_training_without_writers_same_losses():
    z, model, opt, tr, te, *_ = run_g14("cpu", writers=False)
    assert tr == z["train_losses"].tolist() and te == z["test_losses"].tolist()


def small_problem(seed=0):
    torch.manual_seed(seed)
    lin = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    x = torch.randn(11, 7)
    return lin, x


def steps(model, opt, x, n, sched=None):
    for i in range(n):
        opt.zero_grad()
        model(x * (1 + i)).square().sum().backward()
        opt.step()
        if sched is not None:
            sched.step()


@pytest.mark.parametrize("forward", [True, False])
def test_state_dict_round_trip_with_torch_adam(forward):
    a_cls, b_cls = (training.Adam, torch.optim.Adam) if forward else (torch.optim.Adam, training.Adam)
    m1, x = small_problem()
    o1 = a_cls(m1.parameters(), lr=1e-2, weight_decay=1e-3)
    steps(m1, o1, x, 4)
    m2, _ = small_problem()
    m2.load_state_dict(m1.state_dict())
    o2 = b_cls(m2.parameters(), lr=1e-2, weight_decay=1e-3)
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))          # load_state_dict keeps the tensors it is given
    m3, _ = small_problem()
    m3.load_state_dict(m1.state_dict())
    o3 = a_cls(m3.parameters(), lr=1e-2, weight_decay=1e-3)
    o3.load_state_dict(copy.deepcopy(o1.state_dict()))
    steps(m2, o2, x, 3)
    steps(m3, o3, x, 3)
    for p, q in zip(m2.parameters(), m3.parameters()):
        assert torch.equal(p, q)
    for p, q in zip(m2.parameters(), m3.parameters()):
        assert torch.equal(o2.state[p]["exp_avg_sq"], o3.state[q]["exp_avg_sq"])
        assert o2.state[p]["step"].item() == o3.state[q]["step"].item() == 7


def test_adam_matches_torch_on_cpu_and_steplr_changes_lr():
    m1, x = small_problem()
    m2, _ = small_problem()
    o1 = training.Adam(m1.parameters(), lr=1e-2, weight_decay=5e-3)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-2, weight_decay=5e-3)
    s1 = torch.optim.lr_scheduler.StepLR(o1, step_size=2, gamma=0.1)
    s2 = torch.optim.lr_scheduler.StepLR(o2, step_size=2, gamma=0.1)
    steps(m1, o1, x, 5, s1)
    steps(m2, o2, x, 5, s2)
    assert o1.param_groups[0]["lr"] == pytest.approx(1e-4)
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p, q)
    m3, _ = small_problem()
    o3 = training.Adam(m3.parameters(), lr=1e-2, weight_decay=5e-3)
    steps(m3, o3, x, 5)                                          # no schedule: a different trajectory
    assert any(not torch.equal(p, q) for p, q in zip(m1.parameters(), m3.parameters()))


def test_adam_skips_params_without_grad():
    m, x = small_problem()
    m[2].bias.requires_grad_(False)
    o = training.Adam(m.parameters(), lr=1e-2)
    steps(m, o, x, 2)
    assert m[2].bias not in o.state and len(o.state) == 3


def test_checkpoint_state_round_trip(tmp_path):
    import argparse
    m, x = small_problem()
    o = training.Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
    steps(m, o, x, 2)
    tr = training.Trainer(device="cpu")
    tr.global_step = 17
    args = argparse.Namespace(device="cpu", feature_type="vgg19", normalize_loss=False, normalize_lang=False, pooling="avg",
                              batch_size=128, n_epoches=5)
    state = tr.checkpoint_state(3, m, o, 0.25, args)
    assert set(state) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "params", "global_step"}
    assert set(state["params"]) == {"device", "feature_type", "normalize_loss", "normalize_lang", "pooling"}
    torch.save(state, tmp_path / "last.pth")
    back = torch.load(tmp_path / "last.pth", weights_only=False)
    assert back["epoch"] == 3 and back["loss"] == 0.25 and back["global_step"] == 17
    t = torch.optim.Adam(m.parameters(), lr=1.0)
    t.load_state_dict(back["optimizer_state_dict"])
    assert t.param_groups[0]["lr"] == 5e-4 and t.param_groups[0]["weight_decay"] == 5e-3
    for k, v in m.state_dict().items():
        assert torch.equal(back["model_state_dict"][k], v)


def test_custom_collate_and_host_loader_shapes():
    z, c = g14()
    ds = g14_dataset(z)
    random.seed(0)
    loader = training.TripletLoader(ds, training.TripletBatchSampler(16, ds.annotations, ds.num_segments_info), "cpu")
    b = next(iter(loader))
    W = 2 * c["F"] + 2
    assert b["posit"].shape[1] == W and b["posit"].shape == b["inter"].shape and b["intra"].shape[1] == W
    assert b["lang"].shape == (b["n_samples"], 20) and b["maskp"].max().item() + 1 == b["n_samples"]
    assert b["maskp"].dtype == torch.int64 and b["maskn"].shape[0] == b["intra"].shape[0]


def test_no_training_surface_added_to_data():
    from vfr_amd import data
    assert not hasattr(data, "CustomBatchSampler") and not hasattr(data, "custom_collate")
