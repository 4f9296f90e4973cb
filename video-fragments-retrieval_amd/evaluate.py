"""Corpus-wide moment retrieval with the reference's ``evaluate`` surface (``model/evaluate.py:19-90``).

``evaluate(model, video_iterator, lang_iterator, annotations, device, ...)`` consumes the same iterators and
returns the same dict (``{"model, IoU=0.5": {"R@1", "R@10", "R@100", "MR"}, ...}``), but batches internally:
all clips are embedded in one clip-encoder launch sequence, all queries in one BiLSTM pass, and every
query is ranked against every moment of every video by the fused scoring kernel -- the Nq x Nv x M Python
iterations and per-moment ``.item()`` syncs of ``evaluate.py:49-65`` do not exist here.  What the metrics
need is the 0-based rank of the best ground-truth-positive moment (``:77``), which the kernel counts
directly; ``R@k`` is ``rank < k`` (``:80``).

Differences kept on purpose: ties are broken by global moment id (the reference's
unstable argsort leaves them unspecified); ``np.random.choice`` is drawn only when 'chance' is requested
(Q7).  A query without any positive moment raises IndexError as in the reference (Q3).
"""
from __future__ import annotations

import contextlib
import itertools

import numpy as np
import torch

from . import engine


def get_metrics(recalls):
    """lists -> ``{"R@k": mean*100, "MR": median}``."""
    return {(name if name == "MR" else f"R@{name}"): (np.median(v) if name == "MR" else np.mean(v) * 100)
            for name, v in recalls.items()}


def _drain_videos(video_iterator):
    names, feats = [], []
    for batch in video_iterator:
        names.append(batch["video"])
        feats.append(batch["feature"])
    return names, feats


def _drain_queries(lang_iterator):
    tokens, videos, annot_ids = [], [], []
    for batch in lang_iterator:
        tokens.append(batch["feature"])
        videos.append(batch["video"])
        annot_ids.append(batch["annot_id"])
    return tokens, videos, annot_ids


def embed_corpus(model, video_iterator, device, ops, rank=0, world=1, drained=None):
    """-> (CorpusShard, video names).  Uses the dataset's packed FeatureBank (factored clip encoder, one
    launch sequence for the whole shard) when the iterator exposes one; otherwise embeds the per-video
    ``[n, 2F+2]`` tensors the iterator yields, concatenated into one batch."""
    names, feats = drained if drained is not None else _drain_videos(video_iterator)
    dataset = getattr(video_iterator, "dataset", None)
    if hasattr(dataset, "feature_bank"):
        return engine.build_corpus(model, dataset.feature_bank(names), device, ops, rank, world), names
    counts = [int(f.shape[0]) for f in feats]
    with torch.no_grad():
        emb = model(torch.cat(feats).to(device)) if feats else torch.zeros((0, 1))
    return engine.corpus_from_embeddings(emb, counts, device, ops, rank, world), names


def _encode_both(model, video_iterator, drained, tokens, device, ops, rank, world, query_fn=None):
    """Clip shard and query batch; from 4 shards on the two independent encoders run side by side (engine.overlapped)."""
    def queries():
        with torch.no_grad():
            return query_fn() if query_fn else engine.encode_queries(model, torch.cat(tokens), device, ops, rank, world)
    (shard, names), Q = engine.overlapped(device, lambda: embed_corpus(model, video_iterator, device, ops, rank, world, drained),
                                          queries, enable=world >= 4 and len(tokens) > 0)
    return shard, names, Q


@contextlib.contextmanager
def _eval_mode(model):
    """``model.eval()`` for the block; the caller's mode comes back on EVERY way out, an exception included."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def _prepare(model, video_iterator, lang_iterator, device, rank, world, query_fn=None, empty_ok=True):
    """What every entry point starts with: the provider, both iterators drained, the clip shard and the query batch encoded
    (``query_fn(tokens)`` instead of the model's query encoder when given), each query's global video index.
    Returns (ops, tokens, annot_ids, shard, names, Q, own); without queries (``empty_ok``) the corpus is still embedded and
    shard / names / Q / own are None."""
    ops = engine.ops_for(device)
    drained = _drain_videos(video_iterator)
    tokens, q_videos, annot_ids = _drain_queries(lang_iterator)
    if not tokens and empty_ok:
        embed_corpus(model, video_iterator, device, ops, rank, world, drained)
        return ops, tokens, annot_ids, None, None, None, None
    shard, names, Q = _encode_both(model, video_iterator, drained, tokens, device, ops, rank, world,
                                   (lambda: query_fn(tokens)) if query_fn else None)
    video_index = {name: i for i, name in enumerate(names)}
    own = np.asarray([video_index[v] for v in q_videos], np.int64)
    return ops, tokens, annot_ids, shard, names, Q, own


def _rank_metrics(ranks, atk):
    """0-based ranks [N] -> the recall lists ``get_metrics`` folds: hit at k per entry of ``atk``, and "MR"."""
    rec = {k: (ranks < k).astype(int) for k in atk}
    rec["MR"] = ranks
    return rec


def _empty_metrics(atk, with_mr=True):
    """The recall lists of an empty query batch."""
    return {k: [] for k in list(atk) + (["MR"] if with_mr else [])}


def evaluate(model, video_iterator, lang_iterator, annotations, device, preliminary=100, model_types=['model'],
             iou_thresholds=[0.5, 0.7], rank=0, world=1, return_topk=0):
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            return {f"{mt}, IoU={thr}": get_metrics(_empty_metrics((1, 10, 100)))
                    for mt, thr in itertools.product(model_types, iou_thresholds)}
        times = [annotations[a]["times"] for a in annot_ids]
        labels = engine.gt_labels(times, shard.counts_all[own], list(iou_thresholds), True, shard.device, ops)   # a11, on the device
        ranks, top_dist, top_idx = engine.corpus_ranks(shard, Q, own, labels, ops, k=return_topk, world=world)
        ranks = ranks.cpu().numpy()

    recalls = {}
    total = int(shard.mom_off_all[-1])
    first = None
    if "chance" in model_types:
        # evaluate.py:68-72: ONE permutation per query (drawn in query order), shared by every IoU threshold; the chance
        # rank is the first position of the permutation that holds a positive moment
        lab_h = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels
        first = np.empty((len(iou_thresholds), len(own)), np.int64)
        for q in range(len(own)):
            perm = np.random.choice(np.arange(total), size=total, replace=False)
            base = int(shard.mom_off_all[own[q]])
            for r in range(len(iou_thresholds)):
                pos = np.nonzero(lab_h[r, q])[0] + base
                hit = np.nonzero(np.isin(perm, pos))[0]
                if not len(hit):
                    engine.raise_no_positive()
                first[r, q] = hit[0]
    for r, thr in enumerate(iou_thresholds):
        if "model" in model_types:
            recalls[("model", thr)] = _rank_metrics(ranks[r], (1, 10, 100))
        if "chance" in model_types:
            recalls[("chance", thr)] = _rank_metrics(first[r], (1, 10, 100))
    if preliminary and len(own) > preliminary and rank == 0:
        for upto in range(preliminary + 1, len(own) + 1, preliminary):   # the reference prints at li = 100, 200, ... (li + 1 queries)
            print()
            for (mt, thr), rec in recalls.items():
                part = get_metrics({k: v[:upto] for k, v in rec.items()})
                print(f"{mt}, IoU={thr}:\t", "".join(f"{n}: {v:.4f}\t" for n, v in part.items()))
    out = {f"{mt}, IoU={thr}": get_metrics(recalls[(mt, thr)])
           for mt, thr in itertools.product(model_types, iou_thresholds) if (mt, thr) in recalls}
    if return_topk:
        return out, (top_dist, top_idx)
    return out


def validate_epoch(model, video_iterator, lang_iterator, annotations, device, size=250, iou_thresholds=[0.5, 0.7],
                   atk=[1, 10, 100], bert=False, rank=0, world=1):
    """The retrieval metrics of ``Trainer.validate_epoch`` (``model/main.py:121-212``) through the same fused pass.

    Same arguments as the method (minus ``self``; ``device``/``bert`` are the Trainer attributes it reads) and the
    same numbers, returned instead of written to TensorBoard::

        {"CustomRecall": {"1_IoU05": ..}, "MedianRank": {"IoU05": ..}, "MeanReciprocalRank": {"IoU05": ..},
         "pr_curve": {"precision": {k: [..11..]}, "recall": {k: [..11..]}}}      # pr_curve == {} unless size == -1

    Semantics that differ from ``evaluate`` and are kept: IoU ``>=`` threshold (``:161``), 1-based rank
    (``:169``), only the first ``size`` queries are scored (``:186``; ``-1`` = all, and then the 11-point threshold
    sweep with precision/recall@k, ``:137,178-179,200-206``).  A query without a positive moment raises IndexError.
    """
    thr_range = [i / 10 for i in range(11)] if size == -1 else list(iou_thresholds)
    bert_fn = (lambda tokens: model(torch.cat(tokens).to(device), False, device, True).contiguous()) if bert else None
    with _eval_mode(model):
        ops, tokens, annot_ids, shard, names, Q, own = _prepare(
            model, video_iterator, lang_iterator if size <= 0 else itertools.islice(lang_iterator, size),   # :186 never fires for size <= 0
            device, rank, world, bert_fn, empty_ok=False)
        nq = len(tokens)
        times = [annotations[a]["times"] for a in annot_ids]
        labels = engine.gt_labels(times, shard.counts_all[own], thr_range, False, shard.device, ops)   # main.py:161: >=
        kmax = max(atk) if size == -1 else 0
        ranks0, _, top_idx = engine.corpus_ranks(shard, Q, own, labels, ops, k=kmax, world=world)
        ranks = ranks0.cpu().numpy() + 1                                              # :169  "+ 1"

    keep = [r for r, thr in enumerate(thr_range) if thr in iou_thresholds]
    tag = lambda thr: f"IoU0{round(thr * 10)}"
    out = {"CustomRecall": {f"{k}_{tag(thr_range[r])}": float(np.mean(ranks[r] <= k)) for r in keep for k in atk},
           "MedianRank": {tag(thr_range[r]): float(np.median(ranks[r])) for r in keep},
           "MeanReciprocalRank": {tag(thr_range[r]): float(np.mean(1.0 / ranks[r])) for r in keep},
           "pr_curve": {}}
    if size == -1:
        # positives among the top-k: only moments of the query's own video can be positive (:162-166)
        labels = labels.cpu().numpy()
        top = top_idx.cpu().numpy()                                               # [Nq, kmax] global moment ids, -1 padded
        base = shard.mom_off_all[own][:, None]
        local = top - base
        Mown = (shard.counts_all[own] * (shard.counts_all[own] + 1) // 2)[:, None]
        inside = (top >= 0) & (local >= 0) & (local < Mown)
        qsel = np.arange(nq)[:, None]
        hits = labels[:, qsel, np.where(inside, local, 0)] & inside[None]         # [R, Nq, kmax]
        relevant = labels.sum(axis=(1, 2))
        pr = {"precision": {}, "recall": {}}
        for k in atk:
            tp = hits[:, :, :k].sum(axis=(1, 2))
            pr["precision"][k] = [float(t) / (k * nq) for t in tp]
            pr["recall"][k] = [float(t) / float(rel) for t, rel in zip(tp, relevant)]
        out["pr_curve"] = pr
    return out


def evaluate_videos(model, video_iterator, lang_iterator, annotations, device, atk=(1, 10, 100), rank=0, world=1,
                    return_topk=0):
    """Video retrieval (VR) metrics of the same iterators ``evaluate`` consumes: which VIDEOS match a query.

    A video's best key is its smallest (score, global moment id) over all its moments; the 0-based video rank of a query
    is the number of videos whose best key sorts before its own video's best key.  Returns ``{"video": {"R@1", "R@10",
    "R@100", "MR"}}`` (``get_metrics``: R@k = mean(rank < k) x 100, MR = median 0-based rank, as ``evaluate``); with
    ``return_topk`` = k also ``(dist, moment idx, video idx)`` [Nq, k] of the k best distinct videos per query (the
    moment is each video's best one).  Labels, IoU and annotation times play no part (``annotations`` is accepted for the
    shared signature)."""
    with _eval_mode(model):
        ops, _, _, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = {"video": get_metrics(_empty_metrics(atk))}
            return (out, (None, None, None)) if return_topk else out
        dist, idx, vid, ranks = engine.corpus_video_topk(shard, Q, int(return_topk), own, ops, world)
        ranks = ranks.cpu().numpy()
    out = {"video": get_metrics(_rank_metrics(ranks, atk))}
    if return_topk:
        return out, (dist, idx, vid)
    return out


def evaluate_moments_nms(model, video_iterator, lang_iterator, annotations, device, per_video=0, nms_iou=0.5,
                         atk=(1, 10, 100), iou_thresholds=(0.5, 0.7), rank=0, world=1, return_topk=False):
    """Moment retrieval metrics over a DIVERSIFIED list (``engine.corpus_moment_nms``): per video, moments are accepted in
    (score, global id) order unless their IoU with an accepted moment of the same video is > ``nms_iou``, at most
    ``per_video`` of them (0 = no cap); the list is the max(atk) best accepted moments.

    A query is a hit at k for threshold thr when one of its first k results is a positive moment: in the query's own video
    and with ``(get_iou(times, s, e) > thr).sum() >= 2`` -- the strict label table ``evaluate`` builds (reference
    ``evaluate.py:62``).  Returns ``{"model, IoU=<thr>": {"R@1", "R@10", "R@100"}}`` (``get_metrics``; no MR: a rank inside
    the diversified list is not defined here); with ``return_topk`` also ``(dist, moment idx, video idx)`` [Nq, max(atk)].
    With ``per_video`` = 0 and ``nms_iou`` >= 1 the list is the plain moment ranking and R@k equals ``evaluate``'s."""
    K = max(atk)
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = {f"model, IoU={thr}": get_metrics(_empty_metrics(atk, with_mr=False)) for thr in iou_thresholds}
            return (out, (None, None, None)) if return_topk else out
        times = [annotations[a]["times"] for a in annot_ids]
        labels = engine.gt_labels(times, shard.counts_all[own], list(iou_thresholds), True, shard.device, ops)
        dist, idx, vid = engine.corpus_moment_nms(shard, Q, K, per_video, nms_iou, ops, world)
    lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    ids, vids = idx.cpu().numpy(), vid.cpu().numpy()
    local = ids - np.asarray(shard.mom_off_all, np.int64)[own][:, None]
    mine = (vids == own[:, None]) & (ids >= 0)
    local = np.where(mine, local, 0)
    rows = np.arange(len(own))[:, None]
    out = {}
    for r, thr in enumerate(iou_thresholds):
        pos = mine & lab[r][rows, local].astype(bool)
        first = np.where(pos.any(axis=1), pos.argmax(axis=1), K)          # position of the first positive result
        out[f"model, IoU={thr}"] = get_metrics({k: (first < k).astype(int) for k in atk})
    if return_topk:
        return out, (dist, idx, vid)
    return out


def evaluate_candidates(model, video_iterator, lang_iterator, annotations, device, pools, level="moments", atk=(1, 10, 100),
                        iou_thresholds=(0.5, 0.7), rank=0, world=1, return_topk=0):
    """Retrieval metrics among per-query CANDIDATE POOLS (``engine.corpus_subset_topk``): each query is ranked only against the
    videos of its pool -- a per-user library, a first-stage shortlist, or the usual protocol of the query's own video plus N
    distractors.  ``pools``: one iterable of video names or global video indices per query, in ``lang_iterator`` order.  The
    query's own video is ALWAYS added to its pool (a pool without it would leave the rank undefined).

    ``level`` "moments": per IoU threshold, the 0-based rank of the best ground-truth-positive moment (the strict labels and the
    best-positive keys of ``evaluate``) among all moments of the pool -> ``{"model, IoU=<thr>": {"R@1", "R@10", "R@100", "MR"}}``;
    a query without a positive moment raises IndexError as in ``evaluate``.  ``level`` "videos": the 0-based rank of the own video's
    best key among the pool's videos -> ``{"video": {...}}`` as ``evaluate_videos``.  With every pool = all videos the dicts equal
    ``evaluate``'s "model" entries and ``evaluate_videos``.  ``return_topk`` = k also returns ``(dist, moment idx, video idx)``
    [Nq, k] of the pool's k best moments (videos)."""
    if level not in ("moments", "videos"):
        raise ValueError(f"evaluate_candidates: unknown level {level!r} (moments, videos)")
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            empty = ({"video": get_metrics(_empty_metrics(atk))} if level == "videos" else
                     {f"model, IoU={thr}": get_metrics(_empty_metrics(atk)) for thr in iou_thresholds})
            return (empty, (None, None, None)) if return_topk else empty
        pools = list(pools)
        if len(pools) != len(own):
            raise ValueError(f"evaluate_candidates: {len(pools)} pools for {len(own)} queries")
        lists = engine.candidate_lists([list(p) + [int(own[q])] for q, p in enumerate(pools)], names=names)
        K = int(return_topk)
        if level == "videos":
            dist, idx, vid, ranks = engine.corpus_subset_topk(shard, Q, K, lists, "videos", own_global=own, ops=ops, world=world)
            out = {"video": get_metrics(_rank_metrics(ranks.cpu().numpy(), atk))}
        else:
            times = [annotations[a]["times"] for a in annot_ids]
            labels = engine.gt_labels(times, shard.counts_all[own], list(iou_thresholds), True, shard.device, ops)
            keys = engine.best_positive_keys(shard, Q, engine.prepare_gt(shard, own, labels), ops, world)
            if bool((keys == engine.KEY_INF).any()):
                engine.raise_no_positive()
            dist, idx, vid, ranks = engine.corpus_subset_topk(shard, Q, K, lists, "moments", ops=ops, world=world, rank_keys=keys)
            ranks = ranks.cpu().numpy()
            out = {f"model, IoU={thr}": get_metrics(_rank_metrics(ranks[r], atk)) for r, thr in enumerate(iou_thresholds)}
    if return_topk:
        return out, (dist, idx, vid)
    return out


def sentence_probes(annotations, annot_ids, own, counts_all):
    """The probe moment of each annotation: the evaluation-mode positive of the reference's ``CustomBatchSampler``
    (``model/data.py:289-291``) -- the most common annotated span (``Counter(...).most_common()[0][0]``: the first seen wins a
    tie) -- among the spans that lie inside the video (``0 <= s <= e <= n - 1``).  ``own`` [Nq] = global video index per
    annotation.  Returns (probes [P, 3] int64 = (video, start_t, end_t), rows [P] = positions in ``annot_ids`` that got a probe)."""
    from collections import Counter
    probes, rows = [], []
    for q, a in enumerate(annot_ids):
        n = int(counts_all[own[q]])
        spans = [(int(t[0]), int(t[1])) for t in annotations[a]["times"]]
        spans = [(s, e) for s, e in spans if 0 <= s <= e <= n - 1]
        if not spans:
            continue
        s, e = Counter(spans).most_common()[0][0]
        probes.append((int(own[q]), s, e))
        rows.append(q)
    return np.asarray(probes, np.int64).reshape(-1, 3), np.asarray(rows, np.int64)


def evaluate_sentences(model, video_iterator, lang_iterator, annotations, device, atk=(1, 10, 100), rank=0, world=1,
                       return_topk=0):
    """Sentence retrieval (moment -> sentence) metrics of the same iterators ``evaluate`` consumes: given an annotation's moment,
    where does its own sentence rank among ALL sentences of ``lang_iterator``.

    The probe of an annotation is ``sentence_probes``' span (the reference sampler's evaluation-mode positive); the sentence bank
    is every query of ``lang_iterator`` -- other sentences of the same video, and other annotations of the same moment, compete
    like any other sentence.  The 0-based rank is the number of sentences whose (score, sentence index) key sorts before the own
    sentence's key (``engine.corpus_sentence_topk``).  Returns ``{"sentence": {"R@1", "R@10", "R@100", "MR"}}`` (``get_metrics``,
    as ``evaluate_videos``); annotations without a span inside their video get no probe and are counted in
    ``out["sentence"]["skipped"]`` (present only when non-zero).  With ``return_topk`` = k also ``(dist, sentence idx, annotation
    rows)``: [P, k] lists of the probes and the positions in the iteration order they belong to."""
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, S, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = {"sentence": get_metrics(_empty_metrics(atk))}
            return (out, (None, None, None)) if return_topk else out
        probes, rows = sentence_probes(annotations, annot_ids, own, shard.counts_all)
        dist, idx, ranks = engine.corpus_sentence_topk(shard, S, probes, int(return_topk), rows, ops, world)
        ranks = ranks.cpu().numpy()
    out = {"sentence": get_metrics(_rank_metrics(ranks, atk))}
    if len(rows) < len(annot_ids):
        out["sentence"]["skipped"] = len(annot_ids) - len(rows)
    if return_topk:
        return out, (dist, idx, rows)
    return out


def evaluate_paragraphs(model, video_iterator, lang_iterator, annotations, device, atk=(1, 5, 10, 50), rank=0, world=1,
                        return_topk=0):
    """Paragraph-to-video retrieval metrics of the same iterators ``evaluate`` consumes: all sentences of a video together form
    the query, and the question is which video they describe (the usual video-retrieval protocol on datasets with several
    descriptions per video).

    The queries of ``lang_iterator`` are grouped by their video with a stable sort (iteration order is kept inside a paragraph):
    one paragraph per video that has queries, in video order.  The score of (paragraph, video) is the fp32 mean, in sentence order,
    of the video's best moment distance for each sentence; the 0-based rank of a paragraph is the number of videos whose (score,
    video index) key sorts before its own video's (``engine.corpus_paragraph_topk``).  Returns ``{"paragraph": {"R@1", "R@5",
    "R@10", "R@50", "MR"}}`` (``get_metrics``, as ``evaluate_videos``); with ``return_topk`` = k also ``(score, video idx, own
    video)``: [Ng, k] lists of the k best videos per paragraph and the global video index [Ng] each paragraph belongs to.  A video
    with more than 64 queries raises ValueError.  Labels, IoU and annotation times play no part."""
    with _eval_mode(model):
        ops, _, _, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = {"paragraph": get_metrics(_empty_metrics(atk))}
            return (out, (None, None, None)) if return_topk else out
        order = np.argsort(own, kind="stable")
        videos, lengths = np.unique(own, return_counts=True)
        groups = engine.paragraph_groups(lengths=lengths, device=shard.device)
        Qs = Q[torch.from_numpy(order).to(Q.device)].contiguous()
        score, vid, ranks, _ = engine.corpus_paragraph_topk(shard, Qs, groups, int(return_topk), videos, ops=ops, world=world)
        ranks = ranks.cpu().numpy()
    out = {"paragraph": get_metrics(_rank_metrics(ranks, atk))}
    if return_topk:
        return out, (score, vid, videos)
    return out


def evaluate_video_sentences(model, video_iterator, lang_iterator, annotations, device, atk=(1, 5, 10, 50), rank=0, world=1,
                             return_topk=0):
    """Video-to-sentence retrieval metrics of the same iterators ``evaluate`` consumes (the video -> text half of a two-way
    retrieval table): given a whole video, where do its own sentences rank among ALL sentences of ``lang_iterator``.

    One probe per video that has queries, in video order; the sentence bank is every query of ``lang_iterator`` in iteration
    order.  The score of (video, sentence) is the video's best moment distance for the sentence (``evaluate_videos``' quantity);
    the 0-based rank of a video is that of its best-ranked own sentence = the number of sentences whose (score, sentence index)
    key sorts before its smallest own key (``engine.corpus_video_sentence_topk``).  Returns ``{"video_sentence": {"R@1", "R@5",
    "R@10", "R@50", "MR"}}`` (``get_metrics``, as ``evaluate_videos``); with ``return_topk`` = k also ``(dist, sentence idx, probe
    videos)``: [Np, k] lists of the k best sentences per probe and the global video index [Np] of each probe.  Labels, IoU and
    annotation times play no part."""
    with _eval_mode(model):
        ops, _, _, shard, names, S, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = {"video_sentence": get_metrics(_empty_metrics(atk))}
            return (out, (None, None, None)) if return_topk else out
        rows = np.argsort(own, kind="stable")                 # the bank rows grouped by their video: a CSR over the probes
        videos, lengths = np.unique(own, return_counts=True)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        dist, idx, ranks, _ = engine.corpus_video_sentence_topk(shard, S, videos, int(return_topk), off, rows, ops=ops, world=world)
        ranks = ranks.cpu().numpy()
    out = {"video_sentence": get_metrics(_rank_metrics(ranks, atk))}
    if return_topk:
        return out, (dist, idx, videos)
    return out


def _fusion_streams(models, video_iterators, lang_iterators, device, rank, world, who):
    """The streams of a late fusion, encoded: one ``_prepare`` per (model, video iterator, language iterator); every stream must
    iterate the queries of stream 0 in its order (ValueError).  Returns (ops, annot_ids, own, shards, names per stream, Qs);
    ``shards[0] is None`` for an empty corpus."""
    shards, names_all, Qs, first = [], [], [], None
    for s, (model, vi, li) in enumerate(zip(models, video_iterators, lang_iterators)):
        with _eval_mode(model):
            ops, _, annot_ids, shard, names, Q, own = _prepare(model, vi, li, device, rank, world)
        if first is None:
            first = (annot_ids, own)
        elif list(annot_ids) != list(first[0]) or (own is None) != (first[1] is None) or (own is not None and not np.array_equal(own, first[1])):
            raise ValueError(f"{who}: stream {s} iterates other queries (or another query order) than stream 0")
        shards.append(shard)
        names_all.append(names)
        Qs.append(Q)
    annot_ids, own = first
    return ops, annot_ids, own, shards, names_all, Qs


def _fusion_empty(level, atk, thresholds):
    """The metric dict of a fusion over an empty corpus."""
    return ({"video": get_metrics(_empty_metrics(atk))} if level == "videos" else
            {f"model, IoU={thr}": get_metrics(_empty_metrics(atk)) for thr in thresholds})


def evaluate_fusion(models, video_iterators, lang_iterators, annotations, device, weights, level="moments", atk=(1, 10, 100),
                    thresholds=(0.5, 0.7), rank=0, world=1, return_topk=0):
    """Late-fusion retrieval metrics: one ``(model, video iterator, language iterator)`` per stream -- a VGG and a ResNet model, RGB
    and flow, several seeds; the language iterators differ because the vocabularies may -- and one weight per stream (finite,
    >= 0, at most 4 streams).  Every moment is ranked by the weighted sum of the streams' clip distances carried through the moment
    chain (``engine.corpus_fusion_topk``; DESIGN section 4 states the arithmetic).

    ``level`` "moments": per IoU threshold the 0-based rank of the best ground-truth-positive moment in the fused order ->
    ``{"model, IoU=<thr>": {"R@1", "R@10", "R@100", "MR"}}`` as ``evaluate`` (strict labels; a query without a positive moment
    raises IndexError); "videos": the 0-based rank of the own video's best fused key among the videos' -> ``{"video": {...}}`` as
    ``evaluate_videos``.  One stream with weight 1, or weights (1, 0, ..), give exactly ``evaluate`` / ``evaluate_videos`` of
    stream 0.  The streams must iterate the same videos with the same clip counts and the same queries in the same order:
    ValueError otherwise, as for a bad weight.  ``return_topk`` = k also returns ``(dist, moment idx, video idx)`` [Nq, k]."""
    models, video_iterators, lang_iterators = list(models), list(video_iterators), list(lang_iterators)
    if level not in ("moments", "videos"):
        raise ValueError(f"evaluate_fusion: unknown level {level!r} (moments, videos)")
    if not (len(models) == len(video_iterators) == len(lang_iterators)):
        raise ValueError(f"evaluate_fusion: {len(models)} models, {len(video_iterators)} video and {len(lang_iterators)} language iterators")
    w = engine.fusion_weights(weights, len(models))
    ops, annot_ids, own, shards, names_all, Qs = _fusion_streams(models, video_iterators, lang_iterators, device, rank, world,
                                                                 "evaluate_fusion")
    if shards[0] is None:
        empty = _fusion_empty(level, atk, thresholds)
        return (empty, (None, None, None)) if return_topk else empty
    fused = engine.fuse_corpora(shards, w, names=names_all)
    shard = fused.first
    K = int(return_topk)
    if level == "videos":
        dist, idx, vid, ranks = engine.corpus_fusion_topk(fused, Qs, K, "videos", own_global=own, ops=ops, world=world)
        out = {"video": get_metrics(_rank_metrics(ranks.cpu().numpy(), atk))}
    else:
        times = [annotations[a]["times"] for a in annot_ids]
        labels = engine.gt_labels(times, shard.counts_all[own], list(thresholds), True, shard.device, ops)
        dist, idx, vid, ranks = engine.corpus_fusion_topk(fused, Qs, K, "moments", own_global=own, labels=labels, ops=ops, world=world)
        ranks = ranks.cpu().numpy()
        out = {f"model, IoU={thr}": get_metrics(_rank_metrics(ranks[r], atk)) for r, thr in enumerate(thresholds)}
    if return_topk:
        return out, (dist, idx, vid)
    return out


def sweep_fusion(models, video_iterators, lang_iterators, annotations, device, grid, level="moments", atk=(1, 10, 100),
                 thresholds=(0.5, 0.7), rank=0, world=1, select=None):
    """``evaluate_fusion`` for every row of a weight grid [W, S] (``engine.simplex_grid``) with ONE encoding of the streams and one
    pass over the corpus per 16 rows (``engine.corpus_fusion_sweep``): tuning the fusion weights on a validation split.

    Returns ``(metrics, best)``: ``metrics[i]`` is exactly the dict ``evaluate_fusion`` returns with ``weights = grid[i]``;
    ``best`` is the index of the row chosen by ``select = (dict key, metric name)``, e.g. ``("model, IoU=0.5", "R@1")`` or
    ``("video", "MR")`` -- "MR" is minimised, every other metric maximised, a tie goes to the lowest index -- and None without
    ``select``.  Streams, levels and errors are those of ``evaluate_fusion``; a bad row of the grid raises ValueError."""
    models, video_iterators, lang_iterators = list(models), list(video_iterators), list(lang_iterators)
    if level not in ("moments", "videos"):
        raise ValueError(f"sweep_fusion: unknown level {level!r} (moments, videos)")
    if not (len(models) == len(video_iterators) == len(lang_iterators)):
        raise ValueError(f"sweep_fusion: {len(models)} models, {len(video_iterators)} video and {len(lang_iterators)} language iterators")
    grid = engine.fusion_weight_grid(grid, len(models))
    ops, annot_ids, own, shards, names_all, Qs = _fusion_streams(models, video_iterators, lang_iterators, device, rank, world,
                                                                 "sweep_fusion")
    if shards[0] is None:
        metrics = [_fusion_empty(level, atk, thresholds) for _ in grid]
    else:
        fused = engine.fuse_corpora(shards, grid[0], names=names_all)
        shard = fused.first
        if level == "videos":
            ranks = engine.corpus_fusion_sweep(fused, Qs, grid, "videos", own_global=own, ops=ops, world=world).cpu().numpy()
            metrics = [{"video": get_metrics(_rank_metrics(ranks[w], atk))} for w in range(len(grid))]
        else:
            times = [annotations[a]["times"] for a in annot_ids]
            labels = engine.gt_labels(times, shard.counts_all[own], list(thresholds), True, shard.device, ops)
            ranks = engine.corpus_fusion_sweep(fused, Qs, grid, "moments", own_global=own, labels=labels, ops=ops, world=world)
            ranks = ranks.cpu().numpy()
            metrics = [{f"model, IoU={thr}": get_metrics(_rank_metrics(ranks[w, r], atk)) for r, thr in enumerate(thresholds)}
                       for w in range(len(grid))]
    best = None
    if select is not None:
        key, name = select
        vals = [m[key][name] for m in metrics]
        best = int(np.argmin(vals) if name == "MR" else np.argmax(vals))          # argmin / argmax: the first of equal values
    return metrics, best


def evaluate_prior(model, video_iterator, lang_iterator, annotations, device, table, level="moments", atk=(1, 10, 100),
                   iou_thresholds=(0.5, 0.7), rank=0, world=1, k=0):
    """Retrieval metrics under a moment table (``engine.moment_table`` / ``engine.prior_table``): every moment is ranked by its
    score plus the table's bias and the moments the table excludes are no candidates (``engine.corpus_prior_topk``) -- "prior +
    model" of the papers, sliding-window proposal protocols, length limits.

    ``level`` "moments": per IoU threshold the 0-based rank of the best ground-truth-positive CANDIDATE in the biased order ->
    ``{"model, IoU=<thr>": {"R@1", "R@10", "R@100", "MR"}}`` in ``evaluate``'s key format (strict labels; a query without a
    positive moment raises IndexError); "videos": the rank of the own video's best candidate key -> ``{"video": {...}}`` as
    ``evaluate_videos``.  A query whose every positive moment is excluded is never found: its rank is the number of candidates.  The
    share of such queries is reported next to the metrics, ``out["unreachable"] = {"IoU=<thr>": percent}`` (``{"video": percent}``)
    -- 100 minus it is the recall ceiling of the proposal set.  With a table of zeros the other entries equal ``evaluate``'s
    (``evaluate_videos``'s) and every share is 0.  ``k`` > 0 also returns ``(dist, moment idx, video idx)`` [Nq, k]."""
    if level not in ("moments", "videos"):
        raise ValueError(f"evaluate_prior: unknown level {level!r} (moments, videos)")
    K = int(k)
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = _fusion_empty(level, atk, iou_thresholds)
            out["unreachable"] = {"video": 0.0} if level == "videos" else {f"IoU={thr}": 0.0 for thr in iou_thresholds}
            return (out, (None, None, None)) if K else out
        if level == "videos":
            dist, idx, vid, ranks, unreach = engine.corpus_prior_topk(shard, Q, table, K, "videos", own_global=own, ops=ops, world=world)
            out = {"video": get_metrics(_rank_metrics(ranks.cpu().numpy(), atk)),
                   "unreachable": {"video": float(unreach.float().mean()) * 100}}
        else:
            times = [annotations[a]["times"] for a in annot_ids]
            labels = engine.gt_labels(times, shard.counts_all[own], list(iou_thresholds), True, shard.device, ops)
            dist, idx, vid, ranks, unreach = engine.corpus_prior_topk(shard, Q, table, K, "moments", own_global=own, labels=labels,
                                                                      ops=ops, world=world)
            ranks, unreach = ranks.cpu().numpy(), unreach.cpu().numpy()
            out = {f"model, IoU={thr}": get_metrics(_rank_metrics(ranks[r], atk)) for r, thr in enumerate(iou_thresholds)}
            out["unreachable"] = {f"IoU={thr}": float(unreach[r].mean()) * 100 for r, thr in enumerate(iou_thresholds)}
    if K:
        return out, (dist, idx, vid)
    return out


def evaluate_windowed(model, video_iterator, lang_iterator, annotations, device, max_len, atk=(1, 10, 100), thresholds=(0.5, 0.7),
                      agree=2, rank=0, world=1):
    """Retrieval metrics over the WINDOW proposal set (``engine.corpus_window_topk``): the candidates are the moments of at most
    ``max_len`` clips (1 .. 64), in videos of any length up to 1 024 clips -- how Charades-STA, ActivityNet Captions and TACoS are
    searched; ``evaluate`` and the other entry points refuse a corpus with a video of more than 64 clips.

    Per IoU threshold the 0-based rank of the best ground-truth-positive window among the candidates ->
    ``{"model, IoU=<thr>": {"R@1", "R@10", "R@100", "MR"}}`` in ``evaluate``'s key format.  A window is positive when at least
    ``agree`` annotators overlap it with IoU > the threshold (``engine.window_positives``, the strict rule of ``evaluate``).  A query
    without a positive window is never found: its rank is the number of candidates; the share of such queries is
    ``out["unreachable"] = {"IoU=<thr>": percent}`` -- 100 minus it is the recall ceiling of the proposal set.  With ``max_len`` >=
    the longest video the "model" rows are ``evaluate``'s and every share is 0 (when every query has a positive moment).  The chance
    and prior baselines of ``evaluate`` are not offered here."""
    thresholds = list(thresholds)
    with _eval_mode(model):
        ops, _, annot_ids, shard, names, Q, own = _prepare(model, video_iterator, lang_iterator, device, rank, world)
        if shard is None:
            out = _fusion_empty("moments", atk, thresholds)
            out["unreachable"] = {f"IoU={thr}": 0.0 for thr in thresholds}
            return out
        times = [annotations[a]["times"] for a in annot_ids]
        positives = engine.window_positives(times, shard.counts_all[own], thresholds, max_len, strict=True, agree=agree)
        _, _, _, ranks, unreach = engine.corpus_window_topk(shard, Q, max_len, 0, own_global=own, positives=positives, ops=ops,
                                                            world=world)
        ranks, unreach = ranks.cpu().numpy(), unreach.cpu().numpy()
    out = {f"model, IoU={thr}": get_metrics(_rank_metrics(ranks[r], atk)) for r, thr in enumerate(thresholds)}
    out["unreachable"] = {f"IoU={thr}": float(unreach[r].mean()) * 100 for r, thr in enumerate(thresholds)}
    return out
