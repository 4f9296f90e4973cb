"""The reference's training driver (``model/main.py:27-119, 358-385`` with ``model/data.py:249-356``) on our kernels.

* ``TripletBatchSampler`` -- ``data.CustomBatchSampler`` with the same constructor and, for the same ``random`` state, the
  same batches down to the draws; without the per-annotation O(V) list build (prefix counts per clip count map the drawn
  index into the virtual list of candidate videos, candidate segment lists are cached).
* ``custom_collate`` -- the reference's collate for host tensors (the CPU path and the tests).
* ``TripletLoader`` -- the sampler's batches as ``custom_collate`` dicts built on the device by ONE launch each
  (``vfr_triplet_gather_f32``) from the resident ``FeatureBank`` and token table, plus the host int ``n_samples``.
* ``Adam`` -- ``torch.optim.Adam`` (L2 weight decay, same state layout) whose step on ROCm tensors is one launch
  (``vfr_adam_step_f32``) that also writes every raw gradient's sum of squares; CPU params take torch's functional ``adam``.
* ``grad_norm`` -- ``utils.grad_norm`` with one device-to-host copy, reusing the Adam step's sums when they are current.
* ``Trainer`` -- the reference's class: ``train_epoch`` / ``test_epoch`` / ``validate_epoch`` / ``ranking_loss`` with the same
  returns and logged scalars.  Without a writer it never synchronises per step.
"""
from __future__ import annotations

import bisect
import random
from collections import Counter, defaultdict

import numpy as np
import torch
from torch.optim.adam import adam as _torch_adam
from torch.utils.data.sampler import BatchSampler

from . import losses
from .utils import generate_moments


# ------------------------------------------------------------------------------------------------ sampler
class TripletBatchSampler(BatchSampler):
    """``CustomBatchSampler`` (``model/data.py:249-343``): yields lists of triplet dicts (annotation_id, video_pos,
    video_neg, start_t, end_t, start_tn, end_tn).  Every ``random.shuffle`` / ``random.choice`` of the reference is made in
    the same order over a sequence of the same length, so the same ``random`` state gives the same batches."""

    def __init__(self, batch_size, annotations, num_segments_info, train=True, drop_last=False, same_length=True):
        self.batch_size = batch_size
        self.annotations = annotations
        self.num_segments_info = num_segments_info
        self.train = train
        self.drop_last = drop_last
        self.same_length = same_length
        self.indices = defaultdict(list)
        for video, num_segments in self.num_segments_info.items():
            self.indices[num_segments].append(video)
        self._pos_in_group = {v: i for vids in self.indices.values() for i, v in enumerate(vids)}
        self._neg_tables = {}        # min clips -> (eligible clip counts in key order, prefix counts)
        self._intra_cache = {}       # (n, start_t, end_t) or (n, annotated spans) -> candidate segments
        self._spans = {}             # annot_id -> the reference's get_annotations rows, as tuples
        self.candidate_builds = 0    # cache misses (the tests count these: no list is built per annotation)

    def get_annotations(self, annot_id):
        annot_info = self.annotations[annot_id]
        annotations = np.array(annot_info["times"])
        return annotations[annotations[:, 1] <= self.num_segments_info[annot_info["video"]]]

    def get_possible_videos(self, num_segments):
        """The reference's candidate list (kept for API parity; ``__iter__`` does not build it)."""
        return [v for num in self.indices for v in (self.indices[num] if num_segments <= num else ())]

    def _positive_spans(self, annot_id):
        spans = self._spans.get(annot_id)
        if spans is None:
            spans = [(int(s), int(e)) for s, e in self.get_annotations(annot_id)]
            self._spans[annot_id] = spans
        return spans

    def _intra_candidates(self, annot_info, n, start_t, end_t):
        if self.same_length:
            key = (n, start_t, end_t)
        else:
            key = (n, tuple(sorted({(int(s), int(e)) for s, e in annot_info["times"]})))
        cand = self._intra_cache.get(key)
        if cand is None:
            self.candidate_builds += 1
            moments = generate_moments(n)
            if self.same_length:
                cand = [m for m in moments if m[1] - m[0] == end_t - start_t and m != (start_t, end_t)]
            else:
                # get_iou(times, s, e).max() < 1  <=>  (s, e) is none of the annotated spans (IoU of integer spans is 1 iff equal)
                spans = set(key[1])
                cand = [m for m in moments if m not in spans]
            self._intra_cache[key] = cand
        return cand

    def _neg_table(self, min_clips):
        tab = self._neg_tables.get(min_clips)
        if tab is None:
            self.candidate_builds += 1
            groups = [num for num in self.indices if min_clips <= num]
            prefix = [0]
            for num in groups:
                prefix.append(prefix[-1] + len(self.indices[num]))
            tab = (groups, prefix, {num: prefix[i] for i, num in enumerate(groups)})
            self._neg_tables[min_clips] = tab
        return tab

    def _inter_negative(self, video, min_clips):
        groups, prefix, start = self._neg_table(min_clips)
        own = start[self.num_segments_info[video]] + self._pos_in_group[video]      # position of the removed entry
        length = prefix[-1] - 1
        if self.train:
            j = random.choice(range(length))         # the same draw as random.choice on the list after remove()
        else:
            if length <= 0:
                raise IndexError("list index out of range")
            j = 0
        if j >= own:
            j += 1
        g = bisect.bisect_right(prefix, j) - 1
        return self.indices[groups[g]][j - prefix[g]]

    def __iter__(self):
        annotation_ids = list(self.annotations.keys())
        if self.train:
            random.shuffle(annotation_ids)
        batch = []
        posit_batch_size, intra_batch_size = 0, 0
        for annot_id in annotation_ids:
            annot_info = self.annotations[annot_id]
            video = annot_info["video"]
            num_segments = self.num_segments_info[video]
            spans = self._positive_spans(annot_id)
            if self.train:
                start_t, end_t = random.choice(spans)
            else:
                start_t, end_t = Counter(spans).most_common()[0][0]
            possible_segments = self._intra_candidates(annot_info, num_segments, start_t, end_t)
            if self.train:
                start_tn, end_tn = random.choice(possible_segments)
            else:
                start_tn, end_tn = possible_segments[0]
            video_neg = self._inter_negative(video, end_t + 1)
            batch.append(dict(annotation_id=annot_id, video_pos=video, video_neg=video_neg, start_t=start_t, end_t=end_t,
                              start_tn=start_tn, end_tn=end_tn))
            posit_batch_size += end_t - start_t + 1
            intra_batch_size += end_tn - start_tn + 1
            if max(posit_batch_size, intra_batch_size) >= self.batch_size:
                yield batch
                batch = []
                posit_batch_size, intra_batch_size = 0, 0
        if len(batch) > 0 and not self.drop_last:
            yield batch


class HardNegativeSampler(TripletBatchSampler):
    """``TripletBatchSampler`` whose two negatives come from the retrieval engine: the ranking loss's terms are retrieval scores,
    so the hardest intra segment and inter video of a training span are exact keys (``engine.corpus_mine_negatives``).

    Before the first ``refresh`` it makes exactly the parent's draws (the same ``random`` state gives the parent's batches).
    ``refresh`` encodes the corpus and the sentences with the current model and mines, per (annotation, distinct annotated span
    inside its video), the ``h`` hardest negatives of each kind.  Afterwards ``__iter__`` is the parent's loop except for the two
    negative draws: with probability ``hard_fraction`` the intra segment and the inter video are drawn from the mined lists
    (``random.choice`` when ``train``, else entry 0 = the hardest); an empty mined list falls back to the parent's draw.  Where the
    parent has no candidate either (a span that covers its whole video has no same-length neighbour) the any-length rule supplies
    the intra segment, and an annotation whose video has no other moment at all is left out of the epoch.
    ``last_stats``: items mined, the margin violators (with ``margin``), the draws taken from the mined lists / the parent, and
    ``skipped`` = the annotations left out of the last epoch."""

    def __init__(self, batch_size, annotations, num_segments_info, train=True, drop_last=False, same_length=True, h=16,
                 hard_fraction=1.0):
        super().__init__(batch_size, annotations, num_segments_info, train, drop_last, same_length)
        self.h = int(h)
        self.hard_fraction = float(hard_fraction)
        self.mined = None            # (annot_id, start_t, end_t) -> (inter video names, intra spans), hardest first
        self.last_stats = {}

    def refresh(self, model, dataset, device, ops=None, semi_hard=False, margin=None):
        """Mine with the current ``model`` (eval mode for the encoders, the caller's mode restored): one corpus encode, one sentence
        encode, one ``engine.corpus_mine_negatives``; the results are kept as host tables."""
        from . import engine
        from .evaluate import _eval_mode
        ops = ops or engine.ops_for(device)
        bank = dataset.feature_bank()
        index = {v: i for i, v in enumerate(bank.videos)}
        annot_ids = list(self.annotations.keys())
        with _eval_mode(model), torch.no_grad():
            shard = engine.build_corpus(model, bank, device, ops)
            tokens = torch.cat([torch.as_tensor(dataset.lang_features[a]).reshape(1, -1) for a in annot_ids]) if annot_ids else None
            Q = engine.encode_queries(model, tokens, device, ops) if annot_ids else None
        rows, keys, excl = [], [], []
        for r, a in enumerate(annot_ids):
            info = self.annotations[a]
            n = self.num_segments_info[info["video"]]
            named = sorted({(int(s), int(e)) for s, e in info["times"]})
            if not self.same_length and len(named) > engine.MINE_MAX_EXCL:
                continue                                   # more annotated spans than the kernel excludes: the parent's draws
            for s, e in dict.fromkeys(self._positive_spans(a)):
                if 0 <= s <= e < n:
                    rows.append((r, index[info["video"]], s, e))
                    keys.append((a, s, e))
                    excl.append(named)
        self.mined = {}
        self.last_stats = dict(items=len(rows), mined_draws=0, parent_draws=0, skipped=0)
        if not rows or self.h <= 0:
            return self
        ex = None
        if not self.same_length:
            X = max(len(x) for x in excl)
            ex = np.full((len(rows), X, 2), -1, np.int64)
            for i, x in enumerate(excl):
                ex[i, :len(x)] = x
        res = engine.corpus_mine_negatives(shard, Q, np.asarray(rows, np.int64), self.h, "same_length" if self.same_length else "any",
                                           ex, semi_hard, margin, ops)
        vids, spans = res.inter_vid.cpu().numpy(), res.intra_spans()
        for i, key in enumerate(keys):
            self.mined[key] = ([bank.videos[v] for v in vids[i] if v >= 0], [(int(s), int(e)) for s, e in spans[i] if s >= 0])
        if margin is not None:
            self.last_stats.update(violators_inter=int(res.count_inter.sum()), violators_intra=int(res.count_intra.sum()))
        return self

    def __iter__(self):
        if self.mined is None:
            yield from super().__iter__()
            return
        stats = self.last_stats
        stats["mined_draws"] = stats["parent_draws"] = stats["skipped"] = 0
        pick = random.choice if self.train else (lambda seq: seq[0])
        annotation_ids = list(self.annotations.keys())
        if self.train:
            random.shuffle(annotation_ids)
        batch = []
        posit_batch_size, intra_batch_size = 0, 0
        for annot_id in annotation_ids:
            annot_info = self.annotations[annot_id]
            video = annot_info["video"]
            num_segments = self.num_segments_info[video]
            spans = self._positive_spans(annot_id)
            if self.train:
                start_t, end_t = random.choice(spans)
            else:
                start_t, end_t = Counter(spans).most_common()[0][0]
            hard = self.hard_fraction > 0 and (self.hard_fraction >= 1 or random.random() < self.hard_fraction)
            inter, intra = self.mined.get((annot_id, start_t, end_t), ((), ())) if hard else ((), ())
            if intra:
                start_tn, end_tn = pick(intra)
            else:
                possible_segments = self._intra_candidates(annot_info, num_segments, start_t, end_t)
                if not possible_segments and self.same_length:          # no same-length neighbour: any other moment
                    possible_segments = [m for m in generate_moments(num_segments) if m != (start_t, end_t)]
                if not possible_segments:
                    stats["skipped"] += 1
                    continue
                start_tn, end_tn = pick(possible_segments)
            video_neg = pick(inter) if inter else self._inter_negative(video, end_t + 1)
            stats["mined_draws"] += bool(intra) + bool(inter)
            stats["parent_draws"] += (not intra) + (not inter)
            batch.append(dict(annotation_id=annot_id, video_pos=video, video_neg=video_neg, start_t=start_t, end_t=end_t,
                              start_tn=start_tn, end_tn=end_tn))
            posit_batch_size += end_t - start_t + 1
            intra_batch_size += end_tn - start_tn + 1
            if max(posit_batch_size, intra_batch_size) >= self.batch_size:
                yield batch
                batch = []
                posit_batch_size, intra_batch_size = 0, 0
        if len(batch) > 0 and not self.drop_last:
            yield batch


def custom_collate(batch):
    """``model/data.py:346-356`` for host tensors: samples with posit / intra / inter / lang -> one batch dict."""
    posit, intra, inter, lang, mask_posit, mask_intra = [], [], [], [], [], []
    for i, sample in enumerate(batch):
        posit.append(sample["posit"])
        intra.append(sample["intra"])
        inter.append(sample["inter"])
        lang.append(sample["lang"])
        mask_posit.extend([i] * sample["posit"].size(0))
        mask_intra.extend([i] * sample["intra"].size(0))
    return dict(posit=torch.cat(posit, axis=0), intra=torch.cat(intra, axis=0), inter=torch.cat(inter, axis=0),
                lang=torch.cat(lang, axis=0), maskp=torch.LongTensor(mask_posit), maskn=torch.LongTensor(mask_intra))


def host_triplets(dataset, batch):
    """The reference's ``CustomDataset.__getitem__`` for training samples (``model/data.py:232-246``) on ``dataset``'s
    ``make_visual_features`` -- the host batch the device gather reproduces."""
    out = []
    for s in batch:
        mvf = dataset.make_visual_features
        out.append(dict(lang=dataset.lang_features[s["annotation_id"]],
                        posit=mvf(s["video_pos"], s["start_t"], s["end_t"]),
                        intra=mvf(s["video_pos"], s["start_tn"], s["end_tn"]),
                        inter=mvf(s["video_neg"], s["start_t"], s["end_t"])))
    return out


# ------------------------------------------------------------------------------------------------ device batches
class TripletLoader:
    """Iterates ``sampler`` and yields ``custom_collate`` dicts (posit, intra, inter, lang, maskp, maskn) plus the host int
    ``n_samples``.  On a ROCm device the feature bank and a [A, Tq] token table stay resident and each batch is one
    ``vfr_triplet_gather_f32`` launch (the plan travels in the kernel arguments; no per-step synchronisation, so the host
    samples batch i+1 while step i runs).  On the CPU it is the reference's host path (make_visual_features + collate)."""

    def __init__(self, dataset, sampler, device):
        self.dataset, self.sampler = dataset, sampler
        self.device = torch.device(device)
        self.annot_row = {a: i for i, a in enumerate(sampler.annotations)}
        if self.device.type == "cuda":
            bank = dataset.feature_bank()
            self.bank = bank.to(self.device)
            self.video_index = {v: i for i, v in enumerate(bank.videos)}
            toks = [torch.as_tensor(dataset.lang_features[a]).reshape(1, -1) for a in sampler.annotations]
            self.tokens = torch.cat(toks).to(torch.int64).to(self.device)

    def plan(self, batch) -> np.ndarray:
        vi, ar = self.video_index, self.annot_row
        return np.array([[vi[s["video_pos"]], vi[s["video_neg"]], s["start_t"], s["end_t"], s["start_tn"], s["end_tn"],
                          ar[s["annotation_id"]]] for s in batch], dtype=np.int32).reshape(-1, 7)

    def collate(self, batch) -> dict:
        if self.device.type != "cuda":
            out = custom_collate(host_triplets(self.dataset, batch))
            out["n_samples"] = len(batch)
            return out
        from . import _vfr
        n = self.sampler.num_segments_info
        for s in batch:                               # the make_visual_features slices must lie inside both videos
            if s["end_t"] >= n[s["video_pos"]] or s["end_t"] >= n[s["video_neg"]] or s["end_tn"] >= n[s["video_pos"]]:
                raise IndexError(f"triplet {s} reaches past the end of a video")
        posit, intra, inter, lang, maskp, maskn = _vfr.triplet_gather(self.bank.seg, self.bank.ctx, self.bank.clip_off,
                                                                      self.tokens, self.plan(batch))
        return dict(posit=posit, intra=intra, inter=inter, lang=lang, maskp=maskp, maskn=maskn, n_samples=len(batch))

    def __iter__(self):
        for batch in self.sampler:
            yield self.collate(batch)


# ------------------------------------------------------------------------------------------------ optimizer
class Adam(torch.optim.Adam):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (L2 decay, amsgrad off) with the same ``state`` /
    ``state_dict`` (``step`` a 0-dim float32 CPU tensor, ``exp_avg``, ``exp_avg_sq``), so checkpoints load both ways and
    ``StepLR`` works unchanged.  On ROCm tensors a step is one ``vfr_adam_step_f32`` launch per 32 tensors, which also
    leaves every raw gradient's sum of squares in ``self.grad_sumsq`` (read by ``grad_norm``)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
        self.grad_sumsq = None       # (device sums [n], [(param, grad, grad._version)]) of the last device step

    @staticmethod
    def coefficients(group, step: float):
        """fp32 (wd, 1-beta1, beta2, 1-beta2, eps, -step_size, 1/bc2_sqrt) as ``_single_tensor_adam`` forms them: the scalars
        in double from the step count, rounded to fp32 where ATen's kernels take them (the division by the CPU scalar
        bc2_sqrt is a multiply by its fp32 reciprocal)."""
        beta1, beta2 = (float(b) for b in group["betas"])
        lr = float(group["lr"])
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        f = np.float32
        return [f(group["weight_decay"]), f(1 - beta1), f(beta2), f(1 - beta2), f(group["eps"]), f(-step_size),
                f(1.0) / f(bias_correction2_sqrt)]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fused = []                                    # (param, grad, exp_avg, exp_avg_sq, coefs) of device params
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            if not params:
                continue
            if not params[0].is_cuda:
                _torch_adam(params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps, foreach=False, capturable=False,
                                      differentiable=False, fused=None, grad_scale=None, found_inf=None,
                           has_complex=has_complex, amsgrad=group["amsgrad"], beta1=group["betas"][0],
                                      beta2=group["betas"][1], lr=group["lr"], weight_decay=group["weight_decay"],
                                      eps=group["eps"], maximize=group["maximize"],
                                      decoupled_weight_decay=group.get("decoupled_weight_decay", False))
                continue
            if group["amsgrad"] or group["maximize"] or group.get("decoupled_weight_decay", False) or has_complex:
                raise NotImplementedError("training.Adam on the device: amsgrad, maximize, decoupled decay and complex "
                                          "params are not implemented")
            for p, g, m, v, st in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
                if p.dtype != torch.float32 or g.is_sparse:
                    raise NotImplementedError("training.Adam on the device: fp32 dense params only")
                st += 1
                fused.append((p, g, m, v, self.coefficients(group, st.item())))
        if fused:
            from . import _vfr
            live = [f for f in fused if f[0].numel() > 0]
            grads = [f[1] if f[1].is_contiguous() else f[1].contiguous() for f in live]
            sums = _vfr.adam_step([f[0] for f in live], grads, [f[2] for f in live], [f[3] for f in live],
                                  [f[4] for f in live])
            self.grad_sumsq = (sums, [(f[0], f[1], f[1]._version) for f in live])
        return loss


def _current_sums(model_grads, optimizer):
    """The Adam step's sums of squares if they belong to exactly these (param, grad) pairs, unchanged since."""
    rec = getattr(optimizer, "grad_sumsq", None) if optimizer is not None else None
    if rec is None:
        return None
    sums, owners = rec
    where = {id(p): i for i, (p, g, ver) in enumerate(owners) if p.grad is g and g._version == ver}
    idx = [where.get(id(p)) for p, _ in model_grads]
    if any(i is None for i in idx):
        return None
    return sums[torch.as_tensor(idx, device=sums.device)] if idx != list(range(len(sums))) else sums


def grad_norm(model, optimizer=None) -> float:
    """``utils.grad_norm``: the mean over params with a gradient of ``||grad||_2``.  On the device one launch of sums of
    squares (or the ones ``training.Adam`` just wrote for these grads) and ONE device-to-host copy."""
    pg = [(p, p.grad) for _, p in model.named_parameters() if p.grad is not None]
    if not pg:
        raise ZeroDivisionError("grad_norm: no parameter has a gradient")
    if not pg[0][1].is_cuda:
        norms = [g.data.norm().cpu().item() for _, g in pg]
        return sum(norms) / len(norms)
    sums = _current_sums(pg, optimizer)
    if sums is None:
        from . import _vfr
        sums = _vfr.grad_sumsq([g.data for _, g in pg])
    norms = np.sqrt(sums.cpu().numpy().astype(np.float32))
    return sum(float(x) for x in norms) / len(norms)


# ------------------------------------------------------------------------------------------------ trainer
class Trainer:
    """``model/main.py:27-232``'s Trainer.  Writers are duck-typed (``add_scalar`` / ``add_scalars``) and optional: with
    none, the epoch runs without a per-step host synchronisation (losses stay on the device and are read once per epoch;
    the sample count is the batch's ``n_samples`` when it carries one)."""

    def __init__(self, train_writer=None, test_writer=None, val_writer=None, normalize_loss=False, compute_grads=True,
                 device=None, bert=False, b=0.1, lamb=0.4):
        self.device = device
        self.train_writer = train_writer
        self.test_writer = test_writer
        self.val_writer = val_writer
        self.compute_grads = compute_grads
        self.global_step = 0
        self.b = b
        self.lamb = lamb
        self.bert = bert
        self.normalize_loss = normalize_loss
        self._last_losses = []       # summed losses of the last train_epoch's steps (host floats)

    def _batch(self, batch):
        dev = self.device
        return [batch[k].to(dev) for k in ("posit", "intra", "inter", "lang", "maskp", "maskn")]

    def _loss(self, posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn, n_samples=None):
        if n_samples is None:
            return self.ranking_loss(posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn)
        if self.normalize_loss:
            posit_emb, intra_emb, inter_emb, lang_emb = (losses._normalize(x) for x in (posit_emb, intra_emb, inter_emb, lang_emb))
        if posit_emb.is_cuda:
            loss = losses._RankingLossFn.apply(posit_emb.contiguous(), intra_emb.contiguous(), inter_emb.contiguous(),
                                               lang_emb.contiguous(), maskp.contiguous(), maskn.contiguous(), int(n_samples),
                                               float(self.b), float(self.lamb))
            return loss, int(n_samples)
        return losses.ranking_loss(posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn, self.b, self.lamb)

    def train_epoch(self, model, iterator, optimizer):
        model = model.to(self.device)
        model.train()
        step_losses, count_loss = [], 0
        for batch in iterator:
            posit_ft, intra_ft, inter_ft, lang_ft, maskp, maskn = self._batch(batch)
            optimizer.zero_grad()
            posit_emb = model(posit_ft)
            intra_emb = model(intra_ft)
            inter_emb = model(inter_ft)
            lang_emb = model(lang_ft, False, self.device, self.bert)
            loss, n_samples = self._loss(posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn, batch.get("n_samples"))
            step_losses.append(loss.detach())
            count_loss += n_samples
            loss.backward()
            optimizer.step()
            if self.train_writer is not None:           # the reference's per-step log (and its host syncs)
                log_entry = dict(loss=loss.item() / n_samples)
                if self.compute_grads:
                    log_entry["grad_norm"] = grad_norm(model, optimizer)
                for name, value in log_entry.items():
                    self.train_writer.add_scalar(name, value, global_step=self.global_step)
            self.global_step += 1
        self._last_losses = torch.stack(step_losses).cpu().tolist() if step_losses else []    # the epoch's one read
        epoch_loss = sum(float(x) for x in self._last_losses)
        return epoch_loss / count_loss

    def test_epoch(self, model, iterator):
        model = model.to(self.device)
        model.eval()
        step_losses, count_loss = [], 0
        posit_emb = lang_emb = None
        for batch in iterator:
            posit_ft, intra_ft, inter_ft, lang_ft, maskp, maskn = self._batch(batch)
            with torch.no_grad():
                posit_emb = model(posit_ft)
                intra_emb = model(intra_ft)
                inter_emb = model(inter_ft)
                lang_emb = model(lang_ft, False, self.device, self.bert)
                loss, n_samples = self._loss(posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn, batch.get("n_samples"))
                step_losses.append(loss.detach().reshape(()))
                count_loss += n_samples
        epoch_loss = sum(float(x) for x in torch.stack(step_losses).cpu().tolist()) if step_losses else 0
        log_entry = dict(loss=epoch_loss / count_loss)
        if self.test_writer is not None:
            for name, value in log_entry.items():
                self.test_writer.add_scalar(name, value, global_step=self.global_step)
            scalars = dict(video=posit_emb.norm(dim=1).mean().cpu().item(), language=lang_emb.norm(dim=1).mean().cpu().item())
            self.test_writer.add_scalars("embedding_norm", scalars, global_step=self.global_step)
        return log_entry["loss"]

    def validate_epoch(self, model, video_iterator, lang_iterator, annotations, size=250, iou_thresholds=[0.5, 0.7],
                       atk=[1, 10, 100]):
        from . import evaluate
        out = evaluate.validate_epoch(model, video_iterator, lang_iterator, annotations, self.device, size=size,
                                      iou_thresholds=iou_thresholds, atk=atk, bert=self.bert)
        if self.val_writer is not None:
            for tag in ("CustomRecall", "MedianRank", "MeanReciprocalRank"):
                self.val_writer.add_scalars(tag, out[tag], global_step=self.global_step)
        return out["pr_curve"]

    def ranking_loss(self, posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn):
        return losses.ranking_loss(posit_emb, intra_emb, inter_emb, lang_emb, maskp, maskn, self.b, self.lamb,
                                   self.normalize_loss)

    def checkpoint_state(self, epoch, model, optimizer, loss, params):
        """``main.py:371-379``'s ``state`` dict (``last.pth`` / ``best.pth``); ``params`` is the argparse namespace or a dict,
        filtered to the keys the reference keeps."""
        if not isinstance(params, dict):
            params = vars(params)
        keep = ("device", "feature_type", "normalize_loss", "normalize_lang", "pooling")
        return dict(epoch=epoch, model_state_dict=model.state_dict(), optimizer_state_dict=optimizer.state_dict(), loss=loss,
                    params={k: v for k, v in params.items() if k in keep}, global_step=self.global_step)
