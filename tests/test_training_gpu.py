"""training.py on one MI355X: the device triplet batches against the host path, the fused Adam step against a restatement of
its op order and against torch.optim.Adam, the fused gradient norm, the HIP training run against the reference's trajectory
(G14) and a full-size training step without per-step host synchronisation."""
import random

import numpy as np
import pytest
import torch

from helpers import MemoryDataset
from test_training_host import g14, run_g14
from vfr_amd import models, synth, training, utils

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def make_dataset(nv, nq, F, seed, clips="didemo"):
    counts = synth.clip_counts(nv, clips, seed=seed)
    seg, ctx = synth.video_features(counts, F, seed=seed)
    tokens = synth.query_tokens(nq, seed=seed)
    own, times = synth.annotations(nq, counts, seed=seed)
    times = [[[s, e - 1 if s == 0 and e == counts[own[q]] - 1 else e] for s, e in t] for q, t in enumerate(times)]
    return MemoryDataset(seg, ctx, counts, tokens, own, times)


def assert_same_batch(dev_b, host_b):
    for k in ("posit", "intra", "inter", "lang", "maskp", "maskn"):
        d, h = dev_b[k].cpu(), host_b[k]
        assert d.dtype == h.dtype and d.shape == h.shape, k
        assert torch.equal(d, h), k
    assert dev_b["n_samples"] == host_b["n_samples"]


@pytest.mark.parametrize("F, clips", [(4096, "didemo"), (33, "didemo"), (64, 6)])
def test_device_batches_equal_host_collate(vfr, F, clips):
    ds = make_dataset(30, 90, F, seed=F, clips=clips)
    sampler = training.TripletBatchSampler(128 if F == 4096 else 24, ds.annotations, ds.num_segments_info)
    dev = training.TripletLoader(ds, sampler, DEV)
    host = training.TripletLoader(ds, sampler, "cpu")
    random.seed(4)
    batches = list(iter(sampler))
    assert len(batches) >= 2
    # plus a hand-made batch with one-clip moments (start == end) and the last clip of a 5-clip video
    v5 = [v for v in ds.videos if ds.num_segments_info[v] == 5] or ds.videos
    v6 = [v for v in ds.videos if ds.num_segments_info[v] == 6] or ds.videos
    batches.append([dict(annotation_id=0, video_pos=v5[0], video_neg=v6[0], start_t=4, end_t=4, start_tn=0, end_tn=0),
                    dict(annotation_id=7, video_pos=v6[-1], video_neg=v5[-1], start_t=0, end_t=3, start_tn=5, end_tn=5)])
    for b in batches:
        assert_same_batch(dev.collate(b), host.collate(b))


def restate(p, g, m, v, coefs, wd):
    """The op order of vfr_adam_step_f32 in numpy fp32, every op rounded (include/vfr.h)."""
    f = np.float32
    wd_, w1, b2, c2, eps, nss, ibc2 = (f(x) for x in coefs)
    if wd != 0:
        g = g + wd_ * p
    d = g - m
    m = m + w1 * d if w1 < f(0.5) else g - d * (f(1) - w1)
    v = v * b2
    v = v + c2 * (g * g)
    den = np.sqrt(v) * ibc2 + eps
    return p + nss * (m / den), m, v


def adam_case(offset):
    """Params with numel not a multiple of 4, one with a misaligned storage offset, one without a gradient."""
    rs = np.random.RandomState(5)
    shapes = [(37, 29), (4099,), (3,), (8, 16), (1,)]
    base = torch.from_numpy(rs.randn(sum(int(np.prod(s)) for s in shapes) + 64).astype(np.float32)).to(DEV)
    params, pos = [], offset
    for s in shapes:
        n = int(np.prod(s))
        params.append(torch.nn.Parameter(base[pos:pos + n].view(s)))
        pos += n + 3
    return params


@pytest.mark.parametrize("wd", [0.0, 5e-3])
def test_adam_step_equals_restatement(vfr, wd):
    params = adam_case(offset=1)                                      # storage offset 1: the scalar path
    params += adam_case(offset=0)[:2]
    assert any(p.data_ptr() % 16 for p in params) and any(p.data_ptr() % 16 == 0 for p in params)
    opt = training.Adam(params, lr=1e-3, weight_decay=wd)
    rs = np.random.RandomState(9)
    host = {i: [p.detach().cpu().numpy().copy(), None, np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)]
            for i, p in enumerate(params)}
    skip = 3                                                          # this param never gets a gradient
    for step in range(1, 5):
        for i, p in enumerate(params):
            p.grad = None if i == skip else torch.from_numpy(rs.randn(*p.shape).astype(np.float32)).to(DEV)
            if i != skip:
                host[i][1] = p.grad.cpu().numpy()
        opt.step()
        for i, p in enumerate(params):
            if i == skip:
                continue
            c = training.Adam.coefficients(opt.param_groups[0], float(step))
            host[i][0], host[i][2], host[i][3] = restate(host[i][0], host[i][1], host[i][2], host[i][3], c, wd)
            assert np.array_equal(p.detach().cpu().numpy(), host[i][0]), (step, i)
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), host[i][2]), (step, i)
            assert np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy(), host[i][3]), (step, i)
        assert params[skip] not in opt.state
    torch.cuda.synchronize()


def test_adam_against_torch_adam(vfr, capsys):
    sd = synth.model_weights(64, vocab=60, hidden=16, seed=3)
    def model():
        m = models.CALModel(130, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=16)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(DEV)
    a, b = model(), model()
    oa = training.Adam(a.parameters(), lr=5e-4, weight_decay=5e-3)
    ob = torch.optim.Adam(b.parameters(), lr=5e-4, weight_decay=5e-3, foreach=False)
    rs = np.random.RandomState(1)
    for _ in range(20):
        for p, q in zip(a.parameters(), b.parameters()):
            if p.requires_grad:
                g = torch.from_numpy(rs.randn(*p.shape).astype(np.float32) * 0.01).to(DEV)
                p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    same, total, worst, worst_abs = 0, 0, 0.0, 0.0
    for p, q in zip(a.parameters(), b.parameters()):
        x, y = p.detach().cpu().numpy(), q.detach().cpu().numpy()
        same += int((x == y).sum())
        total += x.size
        d = float(np.abs(x - y).max())
        worst_abs = max(worst_abs, d)
        worst = max(worst, d / max(float(np.abs(y).max()), 1e-30))    # relative to the tensor's scale
    with capsys.disabled():
        print(f"\n[training.Adam vs torch.optim.Adam(foreach=False), 20 steps] {same}/{total} parameters bit-identical, "
              f"worst difference {worst_abs:.3e} absolute, {worst:.3e} relative to the tensor's largest entry")
    # not all identical: where ATen's kernels fuse a multiply-add (add with alpha, lerp, addcmul, addcdiv) the result
    # differs from the separately rounded ops by rounding
    assert worst <= 1e-6


def test_fused_grad_norm(vfr):
    sd = synth.model_weights(64, vocab=60, hidden=16, seed=4)
    m = models.CALModel(130, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=16).to(DEV)
    rs = np.random.RandomState(2)
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.from_numpy(rs.randn(*p.shape).astype(np.float32)).to(DEV)
    ref = utils.grad_norm(m)
    alone = training.grad_norm(m)
    assert alone == pytest.approx(ref, rel=1e-6)
    assert training.grad_norm(m) == alone                            # deterministic
    opt = training.Adam(m.parameters(), lr=1e-3)
    opt.step()
    fused = training.grad_norm(m, opt)
    assert fused == alone                                             # the step's sums are the raw gradients' sums
    sums = opt.grad_sumsq[0]
    assert torch.equal(sums, vfr.grad_sumsq([p.grad for p in m.parameters() if p.grad is not None]))
    m.lang_fc.bias.grad.mul_(2)                                       # stale sums are not reused
    assert training.grad_norm(m, opt) != fused


def test_hip_training_follows_reference_trajectory(vfr):
    z, model, opt, tr, te, lrs, tw, sw = run_g14(DEV)
    loss = np.array([v for n, v, s in tw.items if n == "loss"])
    gn = np.array([v for n, v, s in tw.items if n == "grad_norm"])
    assert loss.shape == z["step_loss"].shape
    np.testing.assert_allclose(loss, z["step_loss"], rtol=1e-4)
    np.testing.assert_allclose(gn, z["step_grad_norm"], rtol=1e-3)
    np.testing.assert_allclose(tr, z["train_losses"], rtol=1e-4)
    np.testing.assert_allclose(te, z["test_losses"], rtol=1e-4)
    for name, p in model.named_parameters():
        a = p.detach().cpu().numpy()
        sel = a[::10] if name in ("visual_fc.0.weight", "visual_fc.2.weight") else a
        np.testing.assert_allclose(sel, z[f"final/{name}"], rtol=0, atol=1e-4, err_msg=name)


class SyncCounter:
    """Counts host reads of device tensors (.item / .cpu / .tolist / .numpy) while active."""

    def __init__(self):
        self.n = 0
        self.saved = {}

    def __enter__(self):
        for name in ("item", "cpu", "tolist", "numpy"):
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.n += 1
                return _orig(t, *a, **k)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


def test_full_size_training_steps_without_host_sync(vfr):
    F, H = 4096, 1000
    ds = make_dataset(200, 400, F, seed=21)
    sd = synth.model_weights(F, vocab=400, hidden=H, seed=21)
    m = models.CALModel(2 * F + 2, pretrained_emb=torch.from_numpy(sd["word_embedding.weight"]), hidden_size=H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV)
    assert m.visual_fc[3].p == 0.3
    random.seed(0)
    loader = training.TripletLoader(ds, training.TripletBatchSampler(128, ds.annotations, ds.num_segments_info), DEV)
    first = next(iter(loader))
    assert first["posit"].shape[1] == 2 * F + 2
    opt = training.Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
    trainer = training.Trainer(device=DEV)
    torch.manual_seed(0)
    per_step = []
    for _ in range(10):                                              # the same batch ten times: the loss has to come down
        with SyncCounter() as sc:
            trainer.train_epoch(m, [first], opt)
        assert sc.n <= 1                                             # the one read at the end of the epoch
        per_step.append(trainer._last_losses[0])
    assert np.isfinite(per_step).all()
    assert np.mean(per_step[-3:]) < np.mean(per_step[:3])
    with SyncCounter() as sc:                                        # a whole multi-step epoch: still one read
        random.seed(1)
        loss = trainer.train_epoch(m, loader, opt)
    assert sc.n <= 1 and np.isfinite(loss)
    assert trainer.global_step > 10
