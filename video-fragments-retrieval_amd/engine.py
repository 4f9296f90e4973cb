"""Batched retrieval engine under ``evaluate`` / ``evaluate_single`` / ``bench.py``.

The reference scores one (query, video) pair per Python iteration (``model/evaluate.py:42-80``).  Here a
corpus (or one rank's shard of it) is a ``CorpusShard``: its clip embeddings stay resident in HBM and a
query batch is answered by three launches -- own-video scores (for ground truth), fused scoring + top-k +
rank counting, merge -- with one exchange step when the corpus is sharded over ranks:

    rank r holds videos [lo_r, hi_r)  (contiguous in iteration order, so global moment ids are unchanged)
    best-GT key   : all_reduce(MIN) of the packed (distance, id) key  (only the owner rank has a finite one)
    rank counts   : all_reduce(SUM) of count_lt
    top-k         : all_gather of the per-shard [Nq, k] lists, then vfr_topk_merge

``ops`` is the provider of the device arithmetic; the product default is ``HipOps`` (libvfr.so).  Tests of
the multi-rank plumbing on CPU-only machines inject their own provider.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ._vfr import KEY_EMPTY as KEY_INF, csr_offsets, fusion_weight_grid, fusion_weights, table_offsets   # (does not load libvfr.so)  KEY_INF = key of (+inf, max id): "no positive moment here"
from .utils import generate_moments, get_iou


class HipOps:
    """Device arithmetic through the C ABI (``_vfr``).  Raises if libvfr.so or the GPU is missing."""

    def __init__(self, score_mode=None):
        from . import _vfr
        _vfr.lib()
        self.v = _vfr
        self.score_mode = score_mode          # None: _vfr.DEFAULT_SCORE_MODE ("mfma": MFMA pre-filter, exact results)

    def _video_mode(self):
        """Mode of the video-level kernels, which have no approximate form: "bf16" gets their default."""
        return None if self.score_mode == "bf16" else self.score_mode

    def make_bank(self, emb, clip_off, id_base):
        return self.v.VideoBank(emb, clip_off, id_base)

    def encode_clips(self, model, seg, ctx, clip_off):
        return model.encode_clips(seg, ctx, clip_off)

    def encode_queries(self, model, tokens):
        return model.encode_queries(tokens)

    def score_own(self, Q, bank, own_local):
        return self.v.score_own(Q, bank, own_local)

    def score_topk(self, Q, bank, k, rank_dist, rank_idx, workspace=None, count_lt=None, thr_seed=None):
        return self.v.score_topk(Q, bank, k, rank_dist, rank_idx, count_lt=count_lt, workspace=workspace,
                                 thr_seed=thr_seed, mode=self.score_mode)

    def score_video_topk(self, Q, bank, k, own_dist=None, own_idx=None, count=None, workspace=None):
        return self.v.score_video_topk(Q, bank, k, own_dist, own_idx, count=count, workspace=workspace, mode=self._video_mode())

    def score_moment_nms(self, Q, bank, k, per_video=0, nms_iou=1.0, workspace=None):
        return self.v.score_moment_nms(Q, bank, k, per_video, nms_iou, workspace=workspace, mode=self._video_mode())

    def score_subset(self, Q, bank, cand_off, cand_vid, k, level="moments", vid_base=0, rank_dist=None, rank_idx=None, count_lt=None,
                     workspace=None, bad=None, max_list=None):
        return self.v.score_subset(Q, bank, cand_off, cand_vid, k, level, vid_base, rank_dist, rank_idx, count_lt=count_lt,
                                   workspace=workspace, bad=bad, max_list=max_list)

    def score_sentences(self, S, bank, probes, k, vid_base=0, sent_base=0, rank_dist=None, rank_idx=None, count_lt=None, bad=None,
                        workspace=None):
        return self.v.score_sentences(S, bank, probes, k, vid_base, sent_base, rank_dist, rank_idx, count_lt=count_lt, bad=bad,
                                      workspace=workspace)

    def score_video_sentences(self, S, bank, videos, k, vid_base=0, sent_base=0, rank_dist=None, rank_idx=None, count_lt=None,
                              bad=None, workspace=None):
        return self.v.score_video_sentences(S, bank, videos, k, vid_base, sent_base, rank_dist, rank_idx, count_lt=count_lt, bad=bad,
                                            workspace=workspace)

    def score_paragraphs(self, Q, bank, grp_off, max_len, k, vid_base=0, own_dist=None, own_idx=None, count=None, workspace=None,
                         bad=None):
        return self.v.score_paragraphs(Q, bank, grp_off, max_len, k, vid_base, own_dist, own_idx, count=count, workspace=workspace,
                                       bad=bad, mode=self._video_mode())

    def score_paragraph_pairs(self, Q, bank, grp_off, max_len, pairs, vid_base=0, out_score=None, out_moments=None, moments=True,
                              bad=None):
        return self.v.score_paragraph_pairs(Q, bank, grp_off, max_len, pairs, vid_base, out_score, out_moments, moments, bad=bad)

    def score_spans(self, Q, bank, items, vid_base=0, out=None, bad=None):
        return self.v.score_spans(Q, bank, items, vid_base, out, bad=bad)

    def mine_negatives(self, Q, bank, items, h, vid_base=0, intra="same_length", excl=None, floor=None, thr=None, want_inter=True,
                       want_intra=True, intra_out=None, count_inter=None, count_intra=None, bad=None, workspace=None):
        return self.v.mine_negatives(Q, bank, items, h, vid_base, intra, excl, floor, thr, want_inter, want_intra, intra_out,
                                     count_inter, count_intra, bad=bad, workspace=workspace)

    def score_fusion(self, Qs, banks, weights, k, level="moments", rank_dist=None, rank_idx=None, count_lt=None, workspace=None):
        return self.v.score_fusion(Qs, banks, weights, k, level, rank_dist, rank_idx, count_lt=count_lt, workspace=workspace)

    def score_fusion_own(self, Qs, banks, weights, own_local):
        return self.v.score_fusion_own(Qs, banks, weights, own_local)

    def score_fusion_sweep_own(self, Qs, banks, grid, own_local):
        return self.v.score_fusion_sweep_own(Qs, banks, grid, own_local)

    def score_fusion_sweep(self, Qs, banks, grid, level, rank_dist, rank_idx, count_lt=None):
        return self.v.score_fusion_sweep(Qs, banks, grid, level, rank_dist, rank_idx, count_lt=count_lt)

    def score_prior(self, Q, bank, table, k, level="moments", rank_dist=None, rank_idx=None, count_lt=None, workspace=None, bad=None):
        return self.v.score_prior(Q, bank, table, k, level, rank_dist, rank_idx, count_lt=count_lt, workspace=workspace, bad=bad)

    def score_prior_own(self, Q, bank, table, own_local, bad=None):
        return self.v.score_prior_own(Q, bank, table, own_local, bad=bad)

    def score_window(self, Q, bank, max_len, k, rank_dist=None, rank_idx=None, count_lt=None, workspace=None):
        return self.v.score_window(Q, bank, max_len, k, rank_dist, rank_idx, count_lt=count_lt, workspace=workspace)

    def window_span_keys(self, Q, bank, items, vid_base=0, out=None, bad=None):
        return self.v.window_span_keys(Q, bank, items, vid_base, out, bad=bad)

    def slice_bank(self, bank, counts, v0, v1):
        return self.v.slice_bank(bank, counts, v0, v1)

    def poll_faults(self):
        """Device-side recoveries since the last poll (``_vfr.poll_faults``: a RuntimeWarning each; results were repaired)."""
        return self.v.poll_faults()

    def topk_merge(self, part_dist, part_idx):
        return self.v.topk_merge(part_dist, part_idx)

    def pack_keys(self, dist_t, idx_t, out=None):
        return self.v.topk_pack_keys(dist_t, idx_t, out)

    def merge_keys(self, part_keys, want_lists=True, want_keys=False):
        return self.v.topk_merge_keys(part_keys, want_lists, want_keys)

    def gt_best_keys(self, own_scores, labels, id_base, sel, Nq):
        return self.v.gt_best_keys(own_scores, labels, id_base, sel, Nq)

    def gt_rank_keys(self, own_scores, labels, id_base, sel, Nq):
        return self.v.gt_rank_keys(own_scores, labels, id_base, sel, Nq)

    def gt_labels(self, packed_times, n_own, thresholds, strict, device, Mmax=None):
        """``packed_times`` / ``n_own``: host arrays (uploaded here) or tensors already resident on the device (then pass
        ``Mmax`` = moments of the longest own video, so no device value has to be read back)."""
        t, na = packed_times
        as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(device)
        if Mmax is None:
            nmax = int(n_own.max()) if len(n_own) else 0
            Mmax = nmax * (nmax + 1) // 2
        return self.v.gt_labels(as_dev(t), as_dev(na), as_dev(n_own), thresholds, strict, Mmax)


def shard_range(num_videos: int, rank: int, world: int):
    """Contiguous, balanced split of the video iteration order."""
    return (num_videos * rank) // world, (num_videos * (rank + 1)) // world


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


# Rehearsal switch: with ONE rank the exchange steps are skipped (nothing to exchange).  Setting this makes a world-size-1
# process group run the full sharded protocol -- sample pass, the packed all-gathers, MIN / SUM folds, merges -- so that the
# RCCL code path can be executed, and checked against the plain single-GPU pass, on a one-GPU box
# (tests/test_gpu_parity.py::test_rccl_world1_runs_the_sharded_protocol, bench.py VFR_BENCH_FORCE_DIST=1).
FORCE_COLLECTIVES = False


def _group(world):
    """The process group the exchange steps of a ``world``-rank pass go through, or None when there is nothing to exchange."""
    return _dist() if (world > 1 or FORCE_COLLECTIVES) else None


def _all_gather_rows(dist, out, mine):
    """out[g] <- rank g's ``mine`` for a contiguous ``out [world, *mine.shape]``: ONE collective straight into the buffer
    (``all_gather_into_tensor``; the list form makes the RCCL backend gather into a scratch tensor and copy the parts out).
    Which form is used is decided from what the ``dist`` object offers -- the same on every rank, never from an exception
    at call time (a rank that fell back alone would issue a different collective than its peers and hang them): the list
    form is only for the thread-rank / provider stand-ins of the tests, which have no ``all_gather_into_tensor``."""
    if _gather_form(dist) == "tensor":
        # concatenated form (rank g's rows at [g * rows, (g + 1) * rows)): the same memory as out[g], and the shape both
        # the RCCL and the gloo process groups accept
        dist.all_gather_into_tensor(out.view((out.shape[0] * mine.shape[0],) + tuple(mine.shape[1:])) if mine.dim() >= 1 else out, mine)
    else:
        dist.all_gather([out[g] for g in range(out.shape[0])], mine)


_GATHER_FORM = {}


def _gather_form(dist) -> str:
    """"tensor" or "list", chosen ONCE per provider from rank-uniform facts: the stand-ins of the tests have no
    ``all_gather_into_tensor``; for ``torch.distributed`` the backend decides -- RCCL ("nccl") always has the tensor form, gloo
    only in builds whose ProcessGroupGloo implements ``_allgather_base`` (probed once with a 1-element collective whose
    outcome is MIN-reduced over the ranks, so a build in which some rank refuses makes EVERY rank take the list form)."""
    backend = str(dist.get_backend()).lower() if hasattr(dist, "get_backend") else None
    key = (id(dist), backend)
    form = _GATHER_FORM.get(key)
    if form is None:
        if getattr(dist, "all_gather_into_tensor", None) is None:
            form = "list"
        elif backend != "gloo":
            form = "tensor"
        else:
            world = dist.get_world_size()
            ok = torch.ones(1, dtype=torch.int32)
            try:
                dist.all_gather_into_tensor(torch.zeros(world, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
            except (RuntimeError, NotImplementedError):
                ok.zero_()                                   # refused before anything was sent: the ranks still agree below
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            form = "tensor" if int(ok[0]) else "list"
        _GATHER_FORM[key] = form
    return form


@dataclass
class CorpusShard:
    bank: object                 # ops.make_bank(...) result: clip embeddings + CSR offsets on the device
    lo: int                      # first global video index of this shard
    hi: int
    counts_all: np.ndarray       # clips per video for the WHOLE corpus (host)
    mom_off_all: np.ndarray      # [Nv_all + 1] int64 global moment offsets (host)
    device: torch.device

    @property
    def num_videos_all(self):
        return len(self.counts_all)


def build_corpus(model, feature_bank, device, ops=None, rank=0, world=1) -> CorpusShard:
    """Encode this rank's contiguous slice of ``feature_bank`` (``data.FeatureBank`` on the host or device)."""
    ops = ops or HipOps()
    off_all = feature_bank.clip_off.cpu().numpy().astype(np.int64)
    counts = np.diff(off_all)
    mom_off_all = csr_offsets(counts)[1]
    lo, hi = shard_range(len(counts), rank, world)
    c0, c1 = int(off_all[lo]), int(off_all[hi])
    clip_off = torch.from_numpy((off_all[lo:hi + 1] - c0).astype(np.int32)).to(device)
    if feature_bank.seg.device.type == "cpu" and torch.device(device).type == "cuda" and c1 - c0 > STREAM_CHUNK_CLIPS:
        emb = encode_clips_streamed(ops, model, feature_bank.seg[c0:c1], feature_bank.ctx[lo:hi],
                                    off_all[lo:hi + 1] - c0, device)
    else:
        emb = ops.encode_clips(model, feature_bank.seg[c0:c1].to(device), feature_bank.ctx[lo:hi].to(device), clip_off)
    bank = ops.make_bank(emb, clip_off, int(mom_off_all[lo]))
    return CorpusShard(bank, lo, hi, counts, mom_off_all, torch.device(device))


STREAM_CHUNK_CLIPS = 1 << 15        # 512 MB of fp32 VGG rows per staging buffer; >= 1024 GEMM tiles per chunk


def encode_clips_streamed(ops, model, seg, ctx, off, device, chunk_clips=None):
    """Clip embeddings of host-resident pooled rows, H2D copy overlapped with the clip encoder.

    ``seg [C, F]`` / ``ctx [Nv, F]`` are host tensors (page-locked ones -- ``store.FeatureStore.pin()`` -- copy
    asynchronously at PCIe rate; pageable ones still work, through the runtime's staging), ``off`` the CSR offsets
    (host, int64, ``off[0] == 0``).  Videos are grouped into chunks of at most ``chunk_clips`` clips; chunk i+1 is
    copied on a side stream into the other of two device staging buffers while chunk i is encoded, so the step
    costs max(copy, encode) instead of their sum and the features never have to be resident in HBM as a whole.
    Each output row depends on its own clip and its video's context row only, so the result is bit-identical to
    the one-launch path."""
    chunk_clips = chunk_clips or STREAM_CHUNK_CLIPS
    off = np.asarray(off, np.int64)
    Nv, C, F = len(off) - 1, int(off[-1]), int(seg.shape[1])
    bounds, v0 = [], 0
    while v0 < Nv:                                              # greedy video-aligned chunks
        v1 = int(np.searchsorted(off, off[v0] + chunk_clips, side="right")) - 1
        v1 = min(max(v1, v0 + 1), Nv)
        bounds.append((v0, v1))
        v0 = v1
    max_c = max(int(off[b] - off[a]) for a, b in bounds)
    max_v = max(b - a for a, b in bounds)
    dev = torch.device(device)
    main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    seg_buf = [torch.empty((max_c, F), dtype=torch.float32, device=dev) for _ in range(2)]
    ctx_buf = [torch.empty((max_v, F), dtype=torch.float32, device=dev) for _ in range(2)]
    off_dev = torch.from_numpy(off.astype(np.int32)).to(dev)
    ready = [torch.cuda.Event() for _ in range(2)]
    free = [torch.cuda.Event() for _ in range(2)]
    side.wait_stream(main)
    out = None
    for i, (a, b) in enumerate(bounds):
        s = i & 1
        c0, c1 = int(off[a]), int(off[b])
        with torch.cuda.stream(side):
            if i >= 2:
                side.wait_event(free[s])                        # the encoder is done with this staging buffer
            seg_buf[s][:c1 - c0].copy_(seg[c0:c1], non_blocking=True)
            ctx_buf[s][:b - a].copy_(ctx[a:b], non_blocking=True)
            ready[s].record(side)
        main.wait_event(ready[s])
        part = ops.encode_clips(model, seg_buf[s][:c1 - c0], ctx_buf[s][:b - a], off_dev[a:b + 1] - c0)
        free[s].record(main)
        if out is None:
            out = torch.empty((C, part.shape[1]), dtype=torch.float32, device=dev)
        out[c0:c1] = part
    return out


_SIDE_STREAMS = {}
_TLS = __import__("threading").local()          # per-thread pinned flag words (one per device and dtype)


def _pinned_flag(device, dtype=torch.int32):
    """This thread's page-locked [1] word the "no positive moment" flag of a pass on ``device`` is copied to."""
    flags = _TLS.__dict__.setdefault("flags", {})
    flag = flags.get((device, dtype))
    if flag is None:
        flag = flags[(device, dtype)] = torch.zeros((1,), dtype=dtype).pin_memory()
    return flag


def raise_no_positive():
    """What ``np.where(...)[0][0]`` raises in the reference (``evaluate.py:77``, Q3) for a query without a positive moment."""
    raise IndexError("index 0 is out of bounds for axis 0 with size 0 (no ground-truth-positive moment)")


def overlapped(device, main_fn, side_fn, enable=True):
    """Run two independent encoder passes concurrently: ``side_fn`` on a side HIP stream, ``main_fn`` on the current one.

    The clip encoder and the query encoder do not depend on each other; run back to back, each leaves CUs idle in its
    partial tile rounds (a rank's LSTM step at 8 GPUs is 576 tiles on 512 slots), run side by side the dispatcher fills
    those with the other kernel's workgroups.  Returns (main result, side result) with the current stream ordered after
    both.  Off (``enable`` false, or a CPU device) it is ``main_fn(), side_fn()``."""
    dev = torch.device(device)
    if not enable or dev.type != "cuda":
        return main_fn(), side_fn()
    cur = torch.cuda.current_stream(dev)
    side = _SIDE_STREAMS.get((dev, cur.cuda_stream))
    if side is None:
        side = _SIDE_STREAMS[(dev, cur.cuda_stream)] = torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        b = side_fn()
    a = main_fn()
    cur.wait_stream(side)
    for t in (b if isinstance(b, (tuple, list)) else (b,)):
        if isinstance(t, torch.Tensor):
            t.record_stream(cur)                      # allocated on the side stream, consumed on the current one
    return a, b


def corpus_from_embeddings(emb, counts, device, ops=None, rank=0, world=1) -> CorpusShard:
    """Same, from precomputed clip embeddings [sum n, D] of the whole corpus (per-item iterator API)."""
    ops = ops or HipOps()
    counts = np.asarray(counts, np.int64)
    off_all, mom_off_all = csr_offsets(counts)
    lo, hi = shard_range(len(counts), rank, world)
    c0, c1 = int(off_all[lo]), int(off_all[hi])
    clip_off = torch.from_numpy((off_all[lo:hi + 1] - c0).astype(np.int32)).to(device)
    bank = ops.make_bank(emb[c0:c1].to(device).contiguous(), clip_off, int(mom_off_all[lo]))
    return CorpusShard(bank, lo, hi, counts, mom_off_all, torch.device(device))


def encode_queries(model, tokens, device, ops=None, rank=0, world=1):
    """Query embeddings for the whole batch; with world > 1 each rank encodes a slice and they are gathered."""
    ops = ops or HipOps()
    dist = _group(world)
    if dist is None:
        return ops.encode_queries(model, tokens.to(device))
    Nq = tokens.shape[0]
    per = -(-Nq // world)
    lo = min(rank * per, Nq)
    hi = min(lo + per, Nq)
    mine = tokens[lo:hi]
    if mine.shape[0] < per:                                   # pad so every rank gathers equal chunks
        mine = torch.cat([mine, tokens.new_zeros((per - mine.shape[0], tokens.shape[1]))])
    q = ops.encode_queries(model, mine.to(device))
    parts = torch.empty((world,) + tuple(q.shape), dtype=q.dtype, device=q.device)
    _all_gather_rows(dist, parts, q)
    return parts.reshape(world * per, -1)[:Nq].contiguous()


def pack_times(times):
    """Annotator spans of a query batch -> (int32 [Nq, A, 2] zero padded, int32 [Nq] annotator counts).  Host; the only
    per-query Python work of a11 (flattening the nested lists), ~1.5 ms for 5000 queries."""
    import itertools
    nq = len(times)
    na = np.fromiter((len(t) for t in times), dtype=np.int32, count=nq)
    amax = int(na.max()) if nq else 0
    flat = np.fromiter(itertools.chain.from_iterable(itertools.chain.from_iterable(times)), dtype=np.int32,
                       count=2 * int(na.sum()))
    if nq and int(na.min()) == amax:
        return flat.reshape(nq, amax, 2), na
    out = np.zeros((nq, amax, 2), np.int32)
    mask = np.arange(amax)[None, :] < na[:, None]
    out[mask] = flat.reshape(-1, 2)
    return out, na


def gt_label_table(times, counts_own, thresholds, strict=True):
    """labels[r, q, m] = 1 iff >= 2 annotators have IoU (>, or >= when not strict) thresholds[r] with local
    moment m of the query's own video (``model/evaluate.py:59-62``; ``main.py:161`` uses >=).  Host numpy, vectorised
    over the queries (one pass per distinct clip count): float64 ``intersection / union`` like ``utils.get_iou``."""
    counts_own = np.asarray(counts_own, np.int64)
    nmax = int(counts_own.max()) if len(counts_own) else 0
    Mmax = nmax * (nmax + 1) // 2
    t, na = times if isinstance(times, tuple) else pack_times(times)
    labels = np.zeros((len(thresholds), len(na), Mmax), dtype=bool)
    if not len(na):
        return labels
    valid = np.arange(t.shape[1])[None, :, None] < na[:, None, None]              # [Nq, A, 1]
    for n in np.unique(counts_own):
        q = np.nonzero(counts_own == n)[0]
        mom = np.asarray(generate_moments(int(n)), np.int64).reshape(-1, 2)
        tq = t[q].astype(np.int64)
        # the IoU of an annotator span with a moment depends only on the two spans: tabulate it for every span (ts, te) in
        # [0, T)^2 once per clip count, then every query just gathers its annotators' rows
        T = max(int(n), int(tq.max()) + 1 if tq.size else 0)
        lo = int(tq.min()) if tq.size else 0
        if T - lo > 64:
            # spans far outside the clip range (a foreign annotation file): the (T - lo)^2 table would be quadratic in the
            # largest index; the per-query broadcast form is O(nq A M) like the reference's loop
            s, e = mom[None, None, :, 0], mom[None, None, :, 1]
            ts, te = tq[:, :, 0:1], tq[:, :, 1:2]
            inter = np.maximum(np.minimum(te, e) + 1 - np.maximum(ts, s), 0)
            union = np.maximum(te, e) + 1 - np.minimum(ts, s)
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = inter / union                                                   # [nq_n, A, M] float64
            for r, thr in enumerate(thresholds):
                hit = ((iou > thr) if strict else (iou >= thr)) & valid[q]
                labels[r, q, :len(mom)] = hit.sum(axis=1) >= 2
            continue
        ts, te = np.meshgrid(np.arange(lo, T), np.arange(lo, T), indexing="ij")
        ts, te = ts[:, :, None], te[:, :, None]
        s, e = mom[None, None, :, 0], mom[None, None, :, 1]
        inter = np.maximum(np.minimum(te, e) + 1 - np.maximum(ts, s), 0)
        union = np.maximum(te, e) + 1 - np.minimum(ts, s)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = (inter / union).reshape(-1, len(mom))                           # [(T-lo)^2, M] float64, like get_iou
        ids = (tq[:, :, 0] - lo) * (T - lo) + (tq[:, :, 1] - lo)                  # [nq_n, A]
        for r, thr in enumerate(thresholds):
            hit = ((iou > thr) if strict else (iou >= thr))[ids] & valid[q]       # [nq_n, A, M]
            labels[r, q, :len(mom)] = hit.sum(axis=1) >= 2
    return labels


def gt_labels(times, counts_own, thresholds, strict, device, ops):
    """a11 for a query batch on ``device``: the label table [R, Nq, Mmax] (bool), built by the provider -- one kernel
    launch on a ROCm device (``vfr_gt_labels_u8``), the vectorised numpy table on the CPU device."""
    packed = times if isinstance(times, tuple) else pack_times(times)
    return ops.gt_labels(packed, np.asarray(counts_own, np.int32), list(thresholds), strict, device)


def _pack_key(dist_t: torch.Tensor, idx_t: torch.Tensor) -> torch.Tensor:
    """(fp32 distance >= 0, id < 2^32) -> int64 key whose signed order is the (distance, id) order."""
    bits = dist_t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (bits << 32) | (idx_t.to(torch.int64) & 0xFFFFFFFF)


def _unpack_key(key: torch.Tensor):
    bits = (key >> 32).to(torch.int32)
    return bits.view(torch.float32), key & 0xFFFFFFFF


@dataclass
class QueryGT:
    """Ground truth of a query batch on the device: the index part (which queries' own videos live in this shard, where
    their moments start -- bookkeeping of the batch, ``gt_index``) and the a11 label table of those queries."""
    num_thresholds: int
    num_queries: int
    sel: object = None           # int64 [n_sel] positions of the queries whose own video lives in this shard
    own_local: object = None     # int32 [n_sel] shard-local video index
    labels: object = None        # bool  [R, n_sel, Mloc]
    base: object = None          # int64 [n_sel] global id of the own video's first moment
    all_local: bool = False      # sel == every query, in order (single shard): the label table is used as it is
    Mloc: int = 0


def gt_index(shard: CorpusShard, own_global) -> QueryGT:
    """The label-free part of ``prepare_gt``: depends only on which video each query belongs to."""
    own = np.asarray(own_global, np.int64)
    gt = QueryGT(0, len(own))
    local = (own >= shard.lo) & (own < shard.hi)
    if local.any():
        sel = np.nonzero(local)[0]
        nloc = shard.counts_all[shard.lo:shard.hi]
        nmax = int(nloc.max()) if len(nloc) else 0
        dev = shard.device
        gt.Mloc = nmax * (nmax + 1) // 2
        gt.all_local = len(sel) == len(own)
        gt.sel = torch.from_numpy(sel).to(dev)
        gt.own_local = torch.from_numpy((own[sel] - shard.lo).astype(np.int32)).to(dev)
        gt.base = torch.from_numpy(shard.mom_off_all[own[sel]]).to(dev)
    return gt


def prepare_gt(shard: CorpusShard, own_global, labels, index: QueryGT | None = None) -> QueryGT:
    """``labels`` [R, Nq, Mmax]: the host table (``gt_label_table``) or the device one (``gt_labels``)."""
    idx = index if index is not None else gt_index(shard, own_global)
    R, Nq, Mmax = labels.shape
    gt = QueryGT(R, Nq, idx.sel, idx.own_local, None, idx.base, idx.all_local, idx.Mloc)
    if idx.sel is not None and Mmax > 0:
        Mloc = min(Mmax, idx.Mloc)
        if isinstance(labels, torch.Tensor):
            lab = labels if labels.device == shard.device else labels.to(shard.device)
            gt.labels = lab if (idx.all_local and Mloc == Mmax) else lab[:, idx.sel, :Mloc].contiguous()
        else:
            sel = idx.sel.cpu().numpy()
            gt.labels = torch.from_numpy(np.ascontiguousarray(labels[:, sel, :Mloc])).to(shard.device)
    else:
        gt.sel = None
    return gt


def best_positive_keys(shard: CorpusShard, Q, gt: QueryGT, ops, world=1, reduce=True):
    """Per (threshold, query): key of the best ground-truth-positive moment = min over positives of
    (score, global id).  Only the rank that owns the query's video can see it; others contribute KEY_INF.
    ``reduce=False`` returns this rank's keys only (the caller folds the MIN into another exchange)."""
    if gt.sel is not None:
        sc = ops.score_own(Q if gt.all_local else Q[gt.sel].contiguous(), shard.bank, gt.own_local)      # [n_sel, Mown], +inf padded
        keys = ops.gt_best_keys(sc, gt.labels, gt.base, gt.sel, gt.num_queries)
    else:
        keys = torch.full((gt.num_thresholds, gt.num_queries), KEY_INF, dtype=torch.int64, device=shard.device)
    dist = _group(world)
    if dist is not None and reduce:
        dist.all_reduce(keys, op=dist.ReduceOp.MIN)
    return keys


def _single_shard_pass(ops, bank, Q, gt: QueryGT, k, workspace, flag, landed=None):
    """One shard, one IoU pair, a ROCm device: own-video scores, then keys + their rank-key form + the zeroed count buffer + the
    "no positive moment" flag from the same two launches (vfr_gt_rank_keys_f32), the flag on its way to the page-locked
    ``flag`` (``landed``, outside a graph capture only: the event the host waits on instead of the scoring), then the fused pass.
    Device work on the current stream only -- this is also the body a HIP graph captures.  Returns (counts, dist, idx)."""
    sc = ops.score_own(Q, bank, gt.own_local)
    _keys, rank_dist, rank_idx, counts0, missing = ops.gt_rank_keys(sc, gt.labels, gt.base, gt.sel, gt.num_queries)
    flag.copy_(missing, non_blocking=True)
    if landed is not None:
        landed.record()
    od, oi, counts = ops.score_topk(Q, bank, k, rank_dist, rank_idx, workspace=workspace, count_lt=counts0)
    return counts, od, oi


def corpus_ranks(shard: CorpusShard, Q, own_global, labels, ops=None, k=0, world=1, workspace=None, gt=None):
    """The fused pass.  Returns (ranks [R, Nq] int64 = 0-based position of the best GT-positive moment in the
    global (score, id) order -- ``evaluate.py:77``'s MR --, top-k (dist, idx) or (None, None)).

    Raises IndexError (``raise_no_positive``) when some query has no positive moment, like ``np.where(...)[0][0]`` does
    in the reference (Q3)."""
    ops = ops or HipOps()
    gt = gt if gt is not None else prepare_gt(shard, own_global, labels)
    fused = k > 0 and gt.num_thresholds == 2 and _group(world) is not None
    state = {}
    if (_group(world) is None and gt.num_thresholds == 2 and gt.sel is not None and gt.all_local and hasattr(ops, "gt_rank_keys")
            and Q.is_cuda):
        # a serving request, the single-GPU bench step: two launches instead of the keys and seven small torch kernels behind
        # them -- ~40 us of a 0.26 ms single-query request
        flag, landed = _pinned_flag(Q.device), torch.cuda.Event()
        out = _single_shard_pass(ops, shard.bank, Q, gt, k, workspace, flag, landed)
        landed.synchronize()
        getattr(ops, "poll_faults", int)()
        if int(flag[0]):
            raise_no_positive()
        return out
    keys = best_positive_keys(shard, Q, gt, ops, world, reduce=not fused)

    def watch(keys_global):
        # "no positive moment" is known as soon as the (global) keys are: its flag travels to pinned host memory right behind
        # them and is read AFTER the passes below are queued, waiting only for that copy -- the host is never held until the
        # scoring ends, so it can already queue the next batch's encoders
        state["missing"] = (keys_global == KEY_INF).any()
        state["async"] = keys_global.is_cuda
        if state["async"]:
            state["flag"] = _pinned_flag(keys_global.device, torch.bool)
            state["flag"].copy_(state["missing"], non_blocking=True)
            state["landed"] = torch.cuda.Event()
            state["landed"].record()

    def check():
        if state["async"]:
            state["landed"].synchronize()
            getattr(ops, "poll_faults", int)()       # the query encoder finished before the keys: a give-up of its sequence kernel is known by now
        if bool(state["flag"] if state["async"] else state["missing"]):
            raise_no_positive()
    if fused:
        # three collectives per pass instead of five: the best-GT keys ride on the sample exchange, the rank counts on the
        # final one (sharded_search_fused)
        od, oi, counts = sharded_search_fused(shard, Q, k, keys, ops, world, workspace, watch)
        check()
        return counts, od, oi
    watch(keys)
    rank_dist, rank_idx = _unpack_key(keys)
    R = keys.shape[0]
    if R == 2:
        od, oi, counts = sharded_search(shard, Q, k, rank_dist.contiguous(), rank_idx.contiguous(), ops, world, workspace)
        check()
        return counts, od, oi
    # any other number of thresholds (validate_epoch's 11-point PR sweep, a single threshold): pairs of rank keys,
    # the shape the fused kernel is instantiated for; an odd tail repeats its last key.  Top-k rides on the first pair.
    od = oi = None
    parts = []
    for r0 in range(0, R, 2):
        rows = [r0, min(r0 + 1, R - 1)]
        d, i, c = sharded_search(shard, Q, k if r0 == 0 else 0, rank_dist[rows].contiguous(), rank_idx[rows].contiguous(),
                                 ops, world, workspace)
        if r0 == 0:
            od, oi = d, i
        parts.append(c[:R - r0])
    check()
    return torch.cat(parts), od, oi


class GraphedRequest:
    """One evaluation pass of a FIXED batch shape against a resident shard -- query encoder, a11 labels, best ground-truth
    keys, fused top-k + rank counts: what ``corpus_ranks`` runs for one IoU pair -- captured ONCE into a HIP graph
    (``torch.cuda.CUDAGraph``) and replayed per request.

    A serving request is ~15-30 short launches (0.26 ms at one query, of which the BiLSTM sequence kernel is 0.15): issued
    one by one from Python each costs 5-10 us of stream time; replayed as a graph the host does nothing but ``load`` the
    request into the static input buffers and ``replay``.  Everything inside the capture is device work on the capture
    stream through the same C-ABI calls as the eager path (same kernels, same bits: GPU test); the library's
    bank-side products are guarded on the device (VFR_MFMA_BANK_READY is re-verified by hash inside every replay), so a bank
    rewritten between replays costs a recomputation, never a wrong result.  The "no positive moment" flag
    (``evaluate.py:77``'s IndexError) travels to page-locked memory inside the graph and is read by ``check`` after the
    caller's synchronisation.  Single shard (world == 1); the query count, token length, annotator capacity and k are fixed
    at construction -- build one instance per served batch shape."""

    def __init__(self, model, shard: CorpusShard, num_queries: int, k: int, ops=None, thresholds=(0.5, 0.7), strict=True,
                 max_annotators: int = 8, token_len: int = 20, warmup: int = 2):
        self.ops = ops or HipOps()
        self.model, self.shard, self.k = model, shard, int(k)
        self.thresholds, self.strict = [float(t) for t in thresholds], bool(strict)
        dev = shard.device
        if dev.type != "cuda" or shard.lo != 0 or shard.hi != shard.num_videos_all:
            raise RuntimeError("GraphedRequest: a ROCm device holding the whole corpus (one shard)")
        Nq, A = int(num_queries), int(max_annotators)
        nloc = shard.counts_all[shard.lo:shard.hi]
        nmax = int(nloc.max()) if len(nloc) else 0
        self.Mmax = nmax * (nmax + 1) // 2
        self.num_queries, self.max_annotators = Nq, A
        # static inputs (device) and their page-locked staging twins (host)
        self.tokens = torch.zeros((Nq, token_len), dtype=torch.int64, device=dev)
        self.times = torch.zeros((Nq, A, 2), dtype=torch.int32, device=dev)
        self.nannot = torch.zeros((Nq,), dtype=torch.int32, device=dev)
        self.n_own = torch.ones((Nq,), dtype=torch.int32, device=dev)
        self.own_local = torch.zeros((Nq,), dtype=torch.int32, device=dev)
        self.base = torch.zeros((Nq,), dtype=torch.int64, device=dev)
        self.sel = torch.arange(Nq, dtype=torch.int64, device=dev)
        self._host = {n: torch.empty(t.shape, dtype=t.dtype).pin_memory() for n, t in
                      (("tokens", self.tokens), ("times", self.times), ("nannot", self.nannot), ("n_own", self.n_own),
                       ("own_local", self.own_local), ("base", self.base))}
        self.flag = torch.zeros((1,), dtype=torch.int32).pin_memory()
        self.workspace = self.ops.v.topk_workspace(Nq, shard.hi - shard.lo, self.k, dev, total_clips=shard.bank.total_clips)
        self.graph, self.out, self._warmup = None, None, int(warmup)

    def _body(self):
        ops, shard = self.ops, self.shard
        Q = ops.encode_queries(self.model, self.tokens)
        labels = ops.gt_labels((self.times, self.nannot), self.n_own, self.thresholds, self.strict, shard.device, Mmax=self.Mmax)
        gt = QueryGT(len(self.thresholds), self.num_queries, self.sel, self.own_local, labels, self.base, True, self.Mmax)
        return _single_shard_pass(ops, shard.bank, Q, gt, self.k, self.workspace, self.flag)

    def load(self, tokens, times, own_global):
        """The request into the static buffers (asynchronous copies on the current stream, from page-locked staging):
        ``tokens`` int64 [Nq, T], ``times`` = per query the annotators' (s, e) spans (or the ``pack_times`` pair), ``own_global``
        = the video each query belongs to."""
        t, na = times if isinstance(times, tuple) else pack_times(times)
        own = np.asarray(own_global, np.int64)
        Nq, A = self.num_queries, self.max_annotators
        if len(own) != Nq or tuple(np.shape(tokens)) != tuple(self.tokens.shape) or t.shape[0] != Nq or t.shape[1] > A:
            raise RuntimeError("GraphedRequest.load: the request does not have the shape this graph was built for")
        h = self._host
        h["tokens"].copy_(torch.as_tensor(tokens, dtype=torch.int64))
        h["times"].zero_(); h["times"][:, :t.shape[1]] = torch.from_numpy(np.ascontiguousarray(t, np.int32))
        h["nannot"].copy_(torch.from_numpy(np.ascontiguousarray(na, np.int32)))
        h["n_own"].copy_(torch.from_numpy(self.shard.counts_all[own].astype(np.int32)))
        h["own_local"].copy_(torch.from_numpy((own - self.shard.lo).astype(np.int32)))
        h["base"].copy_(torch.from_numpy(np.ascontiguousarray(self.shard.mom_off_all[own], np.int64)))
        for n in h:
            getattr(self, n).copy_(h[n], non_blocking=True)

    def replay(self):
        """Run the pass on what ``load`` put in place.  First call: warm-up + capture.  Returns (rank counts [R, Nq], top-k
        distances [Nq, k], top-k ids [Nq, k]) -- STATIC tensors, overwritten by the next replay."""
        dev = self.shard.device
        if self.graph is None:
            with torch.no_grad():
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(max(self._warmup, 1)):     # allocator, one-time self-checks and kernel attributes settle here
                        self._body()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self.out = self._body()
                self.graph = graph
        self.graph.replay()
        return self.out

    def check(self):
        """After the caller has synchronised: raise what ``corpus_ranks`` raises when some query has no positive moment, and
        report device-side recoveries (``_vfr.poll_faults``)."""
        getattr(self.ops, "poll_faults", int)()
        if int(self.flag[0]):
            raise_no_positive()


def corpus_topk(shard: CorpusShard, Q, k, ops=None, world=1, workspace=None):
    ops = ops or HipOps()
    od, oi, _ = sharded_search(shard, Q, k, None, None, ops, world, workspace)
    return od, oi


def own_best_keys(shard: CorpusShard, Q, own_global, ops, world=1):
    """[Nq] int64 key of each query's own video's best moment (min over ALL its moments of (score, global id)); KEY_INF on
    the ranks that do not hold the video, MIN-reduced over the ranks when world > 1."""
    own = np.asarray(own_global, np.int64)
    Nq = len(own)
    gt = gt_index(shard, own)
    if gt.sel is not None and gt.Mloc > 0:
        labels = torch.ones((1, int(gt.sel.numel()), gt.Mloc), dtype=torch.bool, device=shard.device)
        keys = best_positive_keys(shard, Q, QueryGT(1, Nq, gt.sel, gt.own_local, labels, gt.base, gt.all_local, gt.Mloc), ops,
                                  world, reduce=False)[0]
    else:
        keys = torch.full((Nq,), KEY_INF, dtype=torch.int64, device=shard.device)
    dist = _group(world)
    if dist is not None:
        dist.all_reduce(keys, op=dist.ReduceOp.MIN)
    return keys


def corpus_video_topk(shard: CorpusShard, Q, k, own_global=None, ops=None, world=1, workspace=None):
    """Video-level retrieval over the corpus: the k best DISTINCT videos per query, each with its best moment, and (with
    ``own_global``, the query's own global video index) the 0-based video rank of the query's own video = the number of
    videos whose best key sorts strictly before that video's best key.  A video never spans shards, so the per-shard
    lists merge with the moment-key merge and the counts add.
    Returns (dist [Nq,k], best-moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding), ranks [Nq] int64 | None)."""
    ops = ops or HipOps()
    Nq = Q.shape[0]
    own_d = own_i = None
    if own_global is not None:
        own_d, own_i = _unpack_key(own_best_keys(shard, Q, own_global, ops, world))
        own_d, own_i = own_d.contiguous(), own_i.contiguous()
    od, oi, cnt = _exchange(*ops.score_video_topk(Q, shard.bank, k, own_d, own_i, workspace=workspace), k, ops, world)
    vid = _video_of(shard, oi) if k > 0 else None
    return od, oi, vid, cnt


def _exchange(od, oi, cnt, k, ops, world):
    """The sharded tail of a retrieval variant: the per-shard lists merged (one packed all_gather, k > 0), then the counts
    summed (one all_reduce, when there are counts) -- in this order on every rank.  One shard: nothing to do."""
    dist = _group(world)
    if dist is not None:
        if k > 0:
            od, oi = gather_merge_topk(od, oi, ops, world)
        if cnt is not None:
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
    return od, oi, cnt


def _video_of(shard: CorpusShard, oi):
    """[Nq, k] global video index of global moment ids (-1 stays -1)."""
    mom = torch.from_numpy(shard.mom_off_all).to(oi.device)
    return torch.where(oi >= 0, torch.searchsorted(mom, oi.clamp(min=0), right=True) - 1, torch.full_like(oi, -1))


def corpus_moment_nms(shard: CorpusShard, Q, k, per_video=0, nms_iou=1.0, ops=None, world=1, workspace=None):
    """Diversified moment retrieval over the corpus: the k best moments per query where each video's moments are accepted
    greedily in (distance, global id) order, a moment whose IoU with an accepted moment of its video is > ``nms_iou`` is
    suppressed (``utils.get_iou``, float64) and at most ``per_video`` moments are accepted (0 = no cap).  NMS never crosses
    a video and a video never spans shards, so the per-shard lists merge with the moment-key merge.
    Returns (dist [Nq,k], moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding)); the ids feed ``video_results``."""
    ops = ops or HipOps()
    od, oi, _ = _exchange(*ops.score_moment_nms(Q, shard.bank, k, per_video, nms_iou, workspace=workspace), None, k, ops, world)
    return od, oi, _video_of(shard, oi)


@dataclass
class CandidateLists:
    """Per-query candidate videos as CSR (``candidate_lists``): ``off`` [Nq+1] int64 and ``vid`` [nnz] int32 corpus-global video
    indices, sorted and de-duplicated per query, on the host; ``max_list`` = the longest list.  ``on(device)`` uploads them once."""
    off: np.ndarray
    vid: np.ndarray
    max_list: int
    _dev: dict = None

    @property
    def num_queries(self):
        return len(self.off) - 1

    def on(self, device):
        device = torch.device(device)
        if self._dev is None:
            self._dev = {}
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.off).to(device), torch.from_numpy(self.vid).to(device))
        return self._dev[key]


def candidate_lists(pools, names=None, num_videos=None, device=None) -> CandidateLists:
    """CSR candidate lists from per-query iterables of video names (looked up in ``names``, the corpus order) or global video
    indices (0 <= i < ``num_videos``, default len(names)); each list is sorted and de-duplicated.  Unknown names and indices out
    of range raise ValueError.  ``device``: upload the CSR there as well (``CandidateLists.on``)."""
    index = {n: i for i, n in enumerate(names)} if names is not None else None
    if num_videos is None and names is not None:
        num_videos = len(names)
    rows = []
    for q, pool in enumerate(pools):
        ids = []
        for x in pool:
            if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
                i = int(x)
                if i < 0 or (num_videos is not None and i >= num_videos):
                    raise ValueError(f"candidate_lists: query {q}: video index {i} out of range [0, {num_videos})")
            else:
                if index is None:
                    raise ValueError(f"candidate_lists: query {q}: video name {x!r} given without `names`")
                i = index.get(x)
                if i is None:
                    raise ValueError(f"candidate_lists: query {q}: unknown video {x!r}")
            ids.append(i)
        rows.append(np.unique(np.asarray(ids, np.int64)))
    lens = np.asarray([len(r) for r in rows], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vid = (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int32)
    out = CandidateLists(off, vid, int(lens.max()) if len(lens) else 0)
    if device is not None:
        out.on(device)
    return out


def corpus_subset_topk(shard: CorpusShard, Q, k, lists: CandidateLists, level="moments", own_global=None, ops=None, world=1,
                       workspace=None, rank_keys=None):
    """Candidate-restricted retrieval: each query searches only the videos of its list (``candidate_lists``).  ``level``
    "moments": the k best moments of the listed videos; "videos": the k best listed videos, each as its best moment.  Every rank
    passes the same lists with its first video as ``vid_base``; a video never spans shards, so the lists merge with the
    moment-key merge and the counts add.
    Counts: ``rank_keys`` [R, Nq] packed keys -> [R, Nq] = the listed moments (videos) that sort before each key; else
    ``own_global`` -> [Nq] = the 0-based rank of the query's own video's best key among the listed moments (videos).
    Returns (dist [Nq,k], moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding), counts | None); the ids feed
    ``video_results``."""
    ops = ops or HipOps()
    if level not in ("moments", "videos"):
        raise ValueError(f"corpus_subset_topk: unknown level {level!r} (moments, videos)")
    if lists.num_queries != Q.shape[0]:
        raise ValueError(f"corpus_subset_topk: {lists.num_queries} lists for {Q.shape[0]} queries")
    squeeze = False
    rd = ri = None
    if rank_keys is None and own_global is not None:
        rank_keys = own_best_keys(shard, Q, own_global, ops, world)[None]
        squeeze = True
    if rank_keys is not None:
        rd, ri = _unpack_key(rank_keys)
        rd, ri = rd.contiguous(), ri.contiguous()
    off_t, vid_t = lists.on(shard.device)
    od, oi, cnt = _exchange(*ops.score_subset(Q, shard.bank, off_t, vid_t, k, level, shard.lo, rd, ri, workspace=workspace,
                                              max_list=lists.max_list), k, ops, world)
    vid = _video_of(shard, oi) if k > 0 else None
    if cnt is not None and squeeze:
        cnt = cnt[0]
    return od, oi, vid, cnt


@dataclass
class FusedCorpus:
    """S streams of the SAME videos for late fusion (``fuse_corpora``): one ``CorpusShard`` per stream -- each stream's own clip
    embeddings, of its own width -- and the fp32 stream weights."""
    shards: list
    weights: np.ndarray          # fp32 [S], finite, >= 0
    names: object = None         # the corpus' video names (when given)

    @property
    def first(self) -> CorpusShard:
        return self.shards[0]

    @property
    def banks(self):
        return [s.bank for s in self.shards]


def fuse_corpora(shards, weights, names=None) -> FusedCorpus:
    """S ``CorpusShard``s (1 <= S <= 4) of the same videos + one weight per stream -> ``FusedCorpus``.  ValueError when the streams do
    not describe the same corpus: different clip counts, a different shard range, a weight that is negative, NaN or infinite, or
    (``names``: one list of video names per stream) a different video order."""
    shards = list(shards)
    w = fusion_weights(weights, len(shards))
    a = shards[0]
    for s, b in enumerate(shards[1:], 1):
        if not np.array_equal(np.asarray(a.counts_all), np.asarray(b.counts_all)):
            raise ValueError(f"fuse_corpora: stream {s} has other clip counts than stream 0")
        if (a.lo, a.hi) != (b.lo, b.hi):
            raise ValueError(f"fuse_corpora: stream {s} holds videos [{b.lo}, {b.hi}), stream 0 [{a.lo}, {a.hi})")
        if torch.device(a.device) != torch.device(b.device):
            raise ValueError(f"fuse_corpora: stream {s} lives on {b.device}, stream 0 on {a.device}")
    if names is not None:
        names = [list(n) for n in names]
        if len(names) != len(shards):
            raise ValueError(f"fuse_corpora: {len(names)} name lists for {len(shards)} streams")
        for s, n in enumerate(names[1:], 1):
            if n != names[0]:
                raise ValueError(f"fuse_corpora: stream {s} iterates the videos in another order than stream 0")
        names = names[0]
    return FusedCorpus(shards, w, names)


def corpus_fusion_topk(fused: FusedCorpus, Qs, k, level="moments", own_global=None, labels=None, ops=None, world=1, workspace=None):
    """Late-fusion retrieval over the corpus: moments ranked by the weighted sum over the streams of ``fused`` (``fuse_corpora``),
    ``Qs`` = one query matrix per stream.  ``level`` "moments": the k best moments; "videos": the k best videos, each as its best
    moment.  Every rank scores its shard of every stream; a video never spans shards, so the lists merge with the moment-key merge
    and the counts add.
    Ground truth: "moments" with ``own_global`` and ``labels`` [R, Nq, Mmax] (``gt_labels``) -> ranks [R, Nq] = 0-based position of
    the best positive moment in the fused order (IndexError for a query without a positive moment, as ``corpus_ranks``); "videos"
    with ``own_global`` -> ranks [Nq] = videos whose best fused key sorts before the own video's.  Own fused scores go through the
    GT key functions ``corpus_ranks`` uses.
    Returns (dist [Nq,k], moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding), ranks | None); lists are None for k = 0."""
    ops = ops or HipOps()
    if level not in ("moments", "videos"):
        raise ValueError(f"corpus_fusion_topk: unknown level {level!r} (moments, videos)")
    Qs = list(Qs)
    if len(Qs) != len(fused.shards):
        raise ValueError(f"corpus_fusion_topk: {len(Qs)} query matrices for {len(fused.shards)} streams")
    shard, banks = fused.first, fused.banks
    Nq = Qs[0].shape[0]
    gt = None
    if own_global is not None and level == "videos":
        idx = gt_index(shard, own_global)
        if idx.sel is not None and idx.Mloc > 0:
            ones = torch.ones((1, int(idx.sel.numel()), idx.Mloc), dtype=torch.bool, device=shard.device)
            gt = QueryGT(1, Nq, idx.sel, idx.own_local, ones, idx.base, idx.all_local, idx.Mloc)
        else:
            gt = QueryGT(1, Nq)
    elif own_global is not None and labels is not None:
        gt = prepare_gt(shard, own_global, labels)
    rd = ri = None
    if gt is not None:
        if gt.sel is not None:
            mine = Qs if gt.all_local else [Q[gt.sel].contiguous() for Q in Qs]
            sc = ops.score_fusion_own(mine, banks, fused.weights, gt.own_local)                  # [n_sel, Mown], +inf padded
            keys = ops.gt_best_keys(sc, gt.labels, gt.base, gt.sel, Nq)
        else:
            keys = torch.full((gt.num_thresholds, Nq), KEY_INF, dtype=torch.int64, device=shard.device)
        dist = _group(world)
        if dist is not None:
            dist.all_reduce(keys, op=dist.ReduceOp.MIN)
        if level == "moments" and bool((keys == KEY_INF).any()):
            raise_no_positive()
        rd, ri = _unpack_key(keys)
        rd, ri = rd.contiguous(), ri.contiguous()
    od, oi, cnt = _exchange(*ops.score_fusion(Qs, banks, fused.weights, k, level, rd, ri, workspace=workspace), k, ops, world)
    vid = _video_of(shard, oi) if k > 0 else None
    if cnt is not None and level == "videos":
        cnt = cnt[0]
    return od, oi, vid, cnt


def simplex_grid(S, steps):
    """Every weight vector of ``S`` components ``i / steps`` (integers i >= 0) that sum to 1, in lexicographic order: float32
    [C(steps + S - 1, S - 1), S] -- the usual grid for tuning fusion weights; ``simplex_grid(2, 10)`` is (0, 1), (0.1, 0.9), ..,
    (1, 0)."""
    S, steps = int(S), int(steps)
    if S < 1 or steps < 1:
        raise ValueError(f"simplex_grid: S = {S} components in {steps} steps (both >= 1)")

    def rows(left, total):
        if left == 1:
            return [(total,)]
        return [(i,) + r for i in range(total + 1) for r in rows(left - 1, total - i)]
    return (np.asarray(rows(S, steps), np.float64) / steps).astype(np.float32)


def corpus_fusion_sweep(fused: FusedCorpus, Qs, grid, level="moments", own_global=None, labels=None, ops=None, world=1):
    """The ranks of ``corpus_fusion_topk`` for every row of a weight grid [W, S] (``simplex_grid``) in one pass over the corpus --
    what tuning the weights needs; ``fused.weights`` is not used.  The stream clip distances are computed once per 16 rows of the
    grid, the fuse and the moment chain per row.  Ground truth as ``corpus_fusion_topk`` takes it: "moments" with ``own_global``
    and ``labels`` [R, Nq, Mmax] -> ranks [W, R, Nq] int64 (IndexError when, for some row of the grid, a query has no positive
    moment); "videos" with ``own_global`` -> ranks [W, Nq].  Slice w equals the ranks ``corpus_fusion_topk`` returns with the weights
    ``grid[w]``.  Sharded: the keys [W, R, Nq] go through ONE all-reduce (MIN), the counts through one (SUM)."""
    ops = ops or HipOps()
    if level not in ("moments", "videos"):
        raise ValueError(f"corpus_fusion_sweep: unknown level {level!r} (moments, videos)")
    Qs = list(Qs)
    if len(Qs) != len(fused.shards):
        raise ValueError(f"corpus_fusion_sweep: {len(Qs)} query matrices for {len(fused.shards)} streams")
    grid = fusion_weight_grid(grid, len(fused.shards))
    shard, banks = fused.first, fused.banks
    Nq, W = Qs[0].shape[0], len(grid)
    if own_global is None or (level == "moments" and labels is None):
        raise ValueError("corpus_fusion_sweep: ranks need own_global (and labels at the moment level)")
    if level == "videos":
        idx = gt_index(shard, own_global)
        if idx.sel is not None and idx.Mloc > 0:
            ones = torch.ones((1, int(idx.sel.numel()), idx.Mloc), dtype=torch.bool, device=shard.device)
            gt = QueryGT(1, Nq, idx.sel, idx.own_local, ones, idx.base, idx.all_local, idx.Mloc)
        else:
            gt = QueryGT(1, Nq)
    else:
        gt = prepare_gt(shard, own_global, labels)
    if gt.sel is not None:
        mine = Qs if gt.all_local else [Q[gt.sel].contiguous() for Q in Qs]
        sc = ops.score_fusion_sweep_own(mine, banks, grid, gt.own_local)                         # [W, n_sel, Mown], +inf padded
        keys = torch.stack([ops.gt_best_keys(sc[w], gt.labels, gt.base, gt.sel, Nq) for w in range(W)])
    else:
        keys = torch.full((W, gt.num_thresholds, Nq), KEY_INF, dtype=torch.int64, device=shard.device)
    dist = _group(world)
    if dist is not None:
        dist.all_reduce(keys, op=dist.ReduceOp.MIN)
    if level == "moments" and bool((keys == KEY_INF).any()):
        raise_no_positive()
    rd, ri = _unpack_key(keys)
    cnt = ops.score_fusion_sweep(Qs, banks, grid, level, rd.contiguous(), ri.contiguous())
    if dist is not None:
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
    return cnt[:, 0] if level == "videos" else cnt


PRIOR_MAX_CLIPS = 64                          # include/vfr.h: max_clips <= 64


@dataclass
class MomentTable:
    """A moment table of prior-aware retrieval (include/vfr.h): for every clip count n in 0 .. ``max_clips`` and every local moment
    in ``generate_moments(n)`` order one fp32 entry -- a finite bias >= 0 added to the moment's score, or +inf = excluded.
    ``values``: the host array; ``table_off`` int32 [max_clips + 2] / ``table`` fp32: the arrays the kernels read, on one device
    (``on(device)`` gives the table there).  Built by ``moment_table`` / ``prior_table``."""
    max_clips: int
    values: np.ndarray
    table_off: torch.Tensor
    table: torch.Tensor

    def row(self, n):
        """The entries of n-clip videos, fp32 [n (n + 1) / 2] (a view of ``values``)."""
        off = table_offsets(self.max_clips)
        if not 0 <= n <= self.max_clips:
            raise ValueError(f"MomentTable: no row for {n} clips (0 .. {self.max_clips})")
        return self.values[int(off[n]):int(off[n + 1])]

    def enabled(self, n):
        """bool [n (n + 1) / 2]: which moments of an n-clip video are candidates (entry < +inf)."""
        return self.row(n) < np.inf

    def on(self, device):
        device = torch.device(device)
        if self.table.device == device:
            return self
        return MomentTable(self.max_clips, self.values, self.table_off.to(device), self.table.to(device))


def _moment_table(max_clips, values, device, who):
    """Checked fp32 entries -> MomentTable on ``device`` (None: the host)."""
    v64 = np.asarray(values, np.float64)
    with np.errstate(over="ignore"):
        v32 = v64.astype(np.float32) + np.float32(0.0)                            # (-0 -> +0)
    if np.isnan(v32).any() or (v32 < 0).any():
        raise ValueError(f"{who}: an entry is NaN, negative or -inf (a bias is finite and >= 0; +inf excludes the moment)")
    if (np.isinf(v32) & np.isfinite(v64)).any():
        raise ValueError(f"{who}: a finite bias overflows fp32")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    return MomentTable(int(max_clips), v32, torch.from_numpy(table_offsets(max_clips)).to(dev), torch.from_numpy(v32).to(dev))


def moment_table(max_clips, bias=None, min_len=1, max_len=None, lengths=None, stride=1, device=None) -> MomentTable:
    """A moment table for videos of up to ``max_clips`` clips (<= 64): zeros by default.  ``bias``: a callable
    ``(n, start, end) -> float`` or a dict ``n -> array`` of n (n + 1) / 2 values in ``generate_moments(n)`` order (clip counts the
    dict does not name get zeros).  A moment (start, end) is EXCLUDED (+inf) when its length end - start + 1 is outside
    [``min_len``, ``max_len``], or not in ``lengths`` (when given), or ``start % stride != 0`` -- sliding-window proposal sets and
    length limits.  ValueError for an entry that is NaN, negative or -inf."""
    max_clips = int(max_clips)
    if not 0 <= max_clips <= PRIOR_MAX_CLIPS:
        raise ValueError(f"moment_table: max_clips = {max_clips} (0 .. {PRIOR_MAX_CLIPS})")
    if int(stride) < 1 or int(min_len) < 0:
        raise ValueError(f"moment_table: stride = {stride} (>= 1), min_len = {min_len} (>= 0)")
    allowed = None if lengths is None else {int(x) for x in lengths}
    rows = []
    for n in range(max_clips + 1):
        spans = generate_moments(n)
        if bias is None:
            row = np.zeros(len(spans), np.float64)
        elif callable(bias):
            row = np.asarray([float(bias(n, s, e)) for s, e in spans], np.float64).reshape(len(spans))
        else:
            row = np.asarray(bias[n], np.float64).reshape(-1).copy() if n in bias else np.zeros(len(spans), np.float64)
            if len(row) != len(spans):
                raise ValueError(f"moment_table: bias[{n}] has {len(row)} entries, an {n}-clip video has {len(spans)} moments")
        for j, (s, e) in enumerate(spans):
            length = e - s + 1
            if (length < min_len or (max_len is not None and length > max_len) or (allowed is not None and length not in allowed)
                    or s % int(stride) != 0):
                if np.isnan(row[j]) or row[j] < 0:                            # a bad bias stays an error under the mask
                    raise ValueError("moment_table: an entry is NaN, negative or -inf")
                row[j] = np.inf
        rows.append(row)
    return _moment_table(max_clips, np.concatenate(rows) if rows else np.zeros(0), device, "moment_table")


def prior_table(times, counts, lam=1.0, alpha=1.0, max_clips=None, device=None) -> MomentTable:
    """The temporal prior of the training annotations as a penalty table: ``times[i]`` = the annotator spans (start, end) of
    training annotation i, ``counts[i]`` = the clip count of its video.  Per clip count n seen in training, with c[j] = how often
    moment j of ``generate_moments(n)`` was annotated, total = sum c and M = n (n + 1) / 2:

        entry(n, j) = fp32(lam * -log((c[j] + alpha) / (total + alpha * M)))

    -- ``lam`` x the negative log of the add-``alpha`` smoothed frequency, >= 0.  Clip counts never seen in training get zeros.
    ``alpha`` = 0 gives +inf for a moment nobody annotated: it is never proposed.  EVERY span of every annotation is counted; the
    reference's ``moment_frequency`` loop (``model/evaluate.py``) skips the first annotation it meets of each clip count.  Spans
    that do not lie inside their video (end >= n, start > end) are ignored."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    if len(times) != len(counts):
        raise ValueError(f"prior_table: {len(times)} annotations with {len(counts)} clip counts")
    if not (np.isfinite(lam) and lam >= 0 and np.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"prior_table: lam = {lam}, alpha = {alpha} (finite, >= 0)")
    if max_clips is None:
        max_clips = int(counts.max()) if len(counts) else 0
    max_clips = int(max_clips)
    if not 0 <= max_clips <= PRIOR_MAX_CLIPS:
        raise ValueError(f"prior_table: max_clips = {max_clips} (0 .. {PRIOR_MAX_CLIPS})")
    off = table_offsets(max_clips).astype(np.int64)
    freq = np.zeros(int(off[-1]), np.float64)
    for spans, n in zip(times, counts.tolist()):
        if not 0 < n <= max_clips:
            continue
        for s, e in spans:
            s, e = int(s), int(e)
            if 0 <= s <= e < n:
                freq[off[n] + (s if s == e else n + (s * (2 * n - s - 1)) // 2 + (e - s - 1))] += 1
    values = np.zeros_like(freq)
    for n in range(1, max_clips + 1):
        c = freq[off[n]:off[n + 1]]
        total = c.sum()
        if total == 0:
            continue
        with np.errstate(divide="ignore"):
            pen = -np.log((c + alpha) / (total + alpha * len(c)))
        values[off[n]:off[n + 1]] = np.where(np.isinf(pen), np.inf, float(lam) * np.where(np.isinf(pen), 0.0, pen))
    return _moment_table(max_clips, values, device, "prior_table")


def _enabled_rows(table: MomentTable, n_own, Mmax):
    """bool [Nq, Mmax]: the candidate moments of each query's own video (``n_own`` clips), False past its moments."""
    n_own = np.asarray(n_own, np.int64)
    out = np.zeros((len(n_own), Mmax), bool)
    for n in np.unique(n_own):
        en = table.enabled(int(n))[:Mmax]
        out[np.nonzero(n_own == n)[0], :len(en)] = en
    return out


def corpus_prior_topk(shard: CorpusShard, Q, table: MomentTable, k, level="moments", own_global=None, labels=None, ops=None, world=1,
                      workspace=None):
    """Prior-aware retrieval over the corpus: every moment is ranked by fl(score + table entry) and the moments ``table`` excludes
    (+inf) are no candidates (``moment_table`` / ``prior_table``; include/vfr.h states the arithmetic).  ``level`` "moments": the k
    best candidate moments; "videos": the k best videos that have a candidate, each as its best one.  A video never spans shards,
    so the lists merge with the moment-key merge and the counts add.
    Ground truth: "moments" with ``own_global`` and ``labels`` [R, Nq, Mmax] (``gt_labels``) -> ranks [R, Nq] = 0-based position of
    the best positive CANDIDATE in the biased order; "videos" with ``own_global`` -> ranks [Nq] = videos whose best candidate key
    sorts before the own video's.  The labels are ANDed with ``table.enabled`` of the own video first.  A query whose every positive
    is excluded does not raise: its rank is the number of candidates (videos with one) in the corpus -- no k finds it -- and it is
    marked in ``unreachable`` (bool, the shape of ranks): the proposal-recall ceiling of a sliding-window protocol.  A query
    without a positive moment before the mask raises IndexError as ``corpus_ranks``.
    Returns (dist [Nq,k], moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding), ranks | None, unreachable | None);
    lists are None for k = 0."""
    ops = ops or HipOps()
    if level not in ("moments", "videos"):
        raise ValueError(f"corpus_prior_topk: unknown level {level!r} (moments, videos)")
    if table.max_clips < (int(shard.counts_all.max()) if len(shard.counts_all) else 0):
        raise ValueError(f"corpus_prior_topk: the moment table covers videos of up to {table.max_clips} clips, the corpus has "
                         f"{int(shard.counts_all.max())}")
    table = table.on(shard.device)
    Nq = Q.shape[0]
    gt = None
    if own_global is not None and (level == "videos" or labels is not None):
        own = np.asarray(own_global, np.int64)
        n_own = np.asarray(shard.counts_all, np.int64)[own]
        if level == "videos":
            nmax = int(n_own.max()) if Nq else 0
            labels = _enabled_rows(table, n_own, nmax * (nmax + 1) // 2)[None]
        else:
            if bool((~labels.any(-1)).any()):
                raise_no_positive()
            en = _enabled_rows(table, n_own, labels.shape[2])[None]
            labels = labels & (torch.from_numpy(en).to(labels.device) if isinstance(labels, torch.Tensor) else en)
        gt = prepare_gt(shard, own, labels)
    rd = ri = unreachable = None
    if gt is not None:
        if gt.sel is not None:
            sc = ops.score_prior_own(Q if gt.all_local else Q[gt.sel].contiguous(), shard.bank, table, gt.own_local)
            keys = ops.gt_best_keys(sc, gt.labels, gt.base, gt.sel, Nq)
        else:
            keys = torch.full((gt.num_thresholds, Nq), KEY_INF, dtype=torch.int64, device=shard.device)
        dist = _group(world)
        if dist is not None:
            dist.all_reduce(keys, op=dist.ReduceOp.MIN)
        unreachable = keys == KEY_INF
        rd, ri = _unpack_key(keys)
        rd, ri = rd.contiguous(), ri.contiguous()
    od, oi, cnt = _exchange(*ops.score_prior(Q, shard.bank, table, k, level, rd, ri, workspace=workspace), k, ops, world)
    vid = _video_of(shard, oi) if k > 0 else None
    if cnt is not None and level == "videos":
        cnt, unreachable = cnt[0], unreachable[0]
    return od, oi, vid, cnt, unreachable


WINDOW_MAX_LEN = 64                           # include/vfr.h: 1 <= max_len <= 64
WINDOW_MAX_CLIPS = 1024                       # include/vfr.h: the longest video the CPU oracle can check


def _check_window(max_len, who):
    if not 1 <= int(max_len) <= WINDOW_MAX_LEN:
        raise ValueError(f"{who}: max_len = {max_len} (1 .. {WINDOW_MAX_LEN})")
    return int(max_len)


def window_positives(times, counts_own, thresholds, max_len, strict=True, agree=2):
    """The ground-truth-positive WINDOWS of a query batch, per threshold: ``out[r]`` = int32 [P_r, 3] rows (query row, start, end)
    of every window of at most ``max_len`` clips of the query's own video (``counts_own[q]`` clips, any number of them) that at
    least ``agree`` annotators of ``times[q]`` overlap with IoU > ``thresholds[r]`` (>= when not ``strict``) -- the label rule of
    ``gt_label_table`` (float64 ``intersection / union`` like ``utils.get_iou``), stated on windows instead of on a row of all
    n (n + 1) / 2 moments.  Rows are ordered by query, then start, then end.  Host numpy, vectorised over the queries of one clip
    count; for a video of at most 64 clips and ``max_len >= n`` the rows are exactly the moments ``gt_label_table`` labels 1."""
    L = _check_window(max_len, "window_positives")
    counts_own = np.asarray(counts_own, np.int64).reshape(-1)
    t, na = times if isinstance(times, tuple) else pack_times(times)
    if len(na) != len(counts_own):
        raise ValueError(f"window_positives: {len(na)} annotations with {len(counts_own)} clip counts")
    found = [[] for _ in thresholds]
    A = t.shape[1] if len(na) else 0
    valid = np.arange(A)[None, :, None] < na[:, None, None] if len(na) else None          # [Nq, A, 1]
    for n in np.unique(counts_own):
        n = int(n)
        if n <= 0:
            continue
        s = np.repeat(np.arange(n, dtype=np.int64), L)
        e = s + np.tile(np.arange(L, dtype=np.int64), n)
        keep = e < n
        s, e = s[keep], e[keep]                                                       # (start, end) ascending
        qs = np.nonzero(counts_own == n)[0]
        step = max(1, (1 << 22) // max(1, A * len(s)))                                # queries per block: ~32 MB of float64 IoUs
        for b in range(0, len(qs), step):
            q = qs[b:b + step]
            ts, te = t[q, :, 0:1].astype(np.int64), t[q, :, 1:2].astype(np.int64)     # [nq, A, 1]
            inter = np.maximum(np.minimum(te, e) + 1 - np.maximum(ts, s), 0)
            union = np.maximum(te, e) + 1 - np.minimum(ts, s)
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = inter / union                                                   # [nq, A, M] float64
            for r, thr in enumerate(thresholds):
                hit = ((iou > thr) if strict else (iou >= thr)) & valid[q]
                qi, mi = np.nonzero(hit.sum(axis=1) >= agree)
                found[r].append(np.stack([q[qi], s[mi], e[mi]], axis=1))
    out = []
    for rows in found:
        rows = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
        out.append(np.ascontiguousarray(rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], dtype=np.int32))
    return out


def decode_moments(shard: CorpusShard, ids):
    """Global moment ids (any shape, int64; < 0 = padding) -> (video, start, end) int64 tensors of that shape, -1 at the padding:
    the video by ``searchsorted`` on the corpus's moment offsets, the span by the closed-form inverse of the position in
    ``generate_moments(n)`` order (singles first, then per start the ends after it) -- no table of a video's moments is built."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    dev = ids.device
    mom = torch.from_numpy(np.asarray(shard.mom_off_all, np.int64)).to(dev)
    cnt = torch.from_numpy(np.asarray(shard.counts_all, np.int64)).to(dev)
    ok = (ids >= 0) & (ids < int(shard.mom_off_all[-1]))
    if not len(shard.counts_all):
        none = torch.full_like(ids, -1)
        return none, none.clone(), none.clone()
    safe = torch.where(ok, ids, torch.zeros_like(ids))
    vid = (torch.searchsorted(mom, safe, right=True) - 1).clamp(0, len(shard.counts_all) - 1)
    n = cnt[vid]
    j = safe - mom[vid]
    # j >= n: x = j - n lies in the row of start s, which begins at R(s) = s (2 n - s - 1) / 2: s = the largest start with R(s) <= x
    x = (j - n).clamp(min=0)
    b = 2 * n - 1
    s = ((b.double() - torch.sqrt((b * b - 8 * x).clamp(min=0).double())) / 2).floor().long().clamp(min=0)
    row = lambda u: (u * (2 * n - u - 1)) // 2
    s = torch.where(row(s) > x, s - 1, s)                                             # (the square root rounded the wrong way)
    s = torch.where(row(s + 1) <= x, s + 1, s)
    e = s + 1 + (x - row(s))
    single = j < n
    s, e = torch.where(single, j, s), torch.where(single, j, e)
    none = torch.full_like(ids, -1)
    return torch.where(ok, vid, none), torch.where(ok, s, none), torch.where(ok, e, none)


def corpus_window_topk(shard: CorpusShard, Q, max_len, k, own_global=None, positives=None, ops=None, world=1, workspace=None):
    """Windowed retrieval over the corpus: the candidates are the moments of at most ``max_len`` clips (1 .. 64) in videos of any
    length up to 1 024 clips -- the sliding-window proposal set of the long-video corpora; scores and ids are the canonical ones
    (``decode_moments`` gives the spans).  A moment never spans shards, so the lists merge with the moment-key merge and the counts
    add.  This path is chosen by the caller: nothing switches between it and ``corpus_topk`` / ``corpus_prior_topk`` by itself.
    Ground truth: ``own_global`` [Nq] and ``positives`` = per threshold (at most 4) the rows (query row, start, end) of the positive
    windows of the query's own video (``window_positives``; rows longer than ``max_len`` are no candidates and are dropped) ->
    ranks [R, Nq] = 0-based position of the best positive window in the (score, id) order of the candidates.  A query without a
    positive window does not raise: its rank is the number of candidates in the corpus -- no k finds it -- and it is marked in
    ``unreachable`` (bool [R, Nq]).  A row that does not lie inside its video raises ValueError.
    Returns (dist [Nq,k], moment id [Nq,k] int64, video index [Nq,k] int64 (-1 = padding), ranks | None, unreachable | None);
    lists are None for k = 0."""
    ops = ops or HipOps()
    L = _check_window(max_len, "corpus_window_topk")
    nmax = int(shard.counts_all.max()) if len(shard.counts_all) else 0
    if nmax > WINDOW_MAX_CLIPS:
        raise ValueError(f"corpus_window_topk: videos of up to {WINDOW_MAX_CLIPS} clips, the corpus has one of {nmax}")
    Nq = Q.shape[0]
    rd = ri = unreachable = None
    if own_global is not None and positives is not None:
        own = np.asarray(own_global, np.int64).reshape(-1)
        if len(own) != Nq:
            raise ValueError(f"corpus_window_topk: {len(own)} own videos for {Nq} queries")
        n_own = np.asarray(shard.counts_all, np.int64)[own]
        R = len(positives)
        if not 1 <= R <= 4:
            raise ValueError(f"corpus_window_topk: {R} thresholds (1 .. 4 rank keys per query)")
        keys = torch.full((R, Nq), KEY_INF, dtype=torch.int64, device=shard.device)
        for r, rows in enumerate(positives):
            rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, np.int64).reshape(-1, 3)
            qi, s0, e0 = rows[:, 0], rows[:, 1], rows[:, 2]
            if len(rows) and (qi.min() < 0 or qi.max() >= Nq or s0.min() < 0 or (e0 < s0).any() or (e0 >= n_own[qi]).any()):
                raise ValueError("corpus_window_topk: a positive window does not lie inside its query's own video")
            gv = own[qi] if len(rows) else qi
            mine = (e0 - s0 < L) & (gv >= shard.lo) & (gv < shard.hi)
            if not mine.any():
                continue
            items = torch.from_numpy(np.ascontiguousarray(np.stack([qi, gv, s0, e0], axis=1)[mine], dtype=np.int32)).to(shard.device)
            kp = ops.window_span_keys(Q, shard.bank, items, vid_base=shard.lo)
            keys[r].scatter_reduce_(0, items[:, 0].long(), kp, "amin")                 # the best positive window of each query
        dist = _group(world)
        if dist is not None:
            dist.all_reduce(keys, op=dist.ReduceOp.MIN)
        unreachable = keys == KEY_INF
        rd, ri = _unpack_key(keys)
        rd, ri = rd.contiguous(), ri.contiguous()
    od, oi, cnt = _exchange(*ops.score_window(Q, shard.bank, L, k, rd, ri, workspace=workspace), k, ops, world)
    vid = _video_of(shard, oi) if k > 0 else None
    return od, oi, vid, cnt, unreachable


def corpus_sentence_topk(shard: CorpusShard, S, probes, k, own_sentence=None, ops=None, world=1, workspace=None):
    """Sentence retrieval for moments over the corpus: per probe ``(global video, start_t, end_t)`` (inclusive clip span,
    ``utils.generate_moments`` units; host array-like [Nm, 3]) the k sentences of the bank ``S`` [Ns, D] with the smallest mean clip
    distance, in (distance, sentence index) order.  With ``own_sentence`` [Nm] (row of ``S`` that belongs to each probe) also the
    0-based rank of that sentence = the number of sentences whose key sorts strictly before its own key for that probe (the key
    comes from one own-video scoring launch on the rank that holds the video).  ``world`` > 1: the clip bank is sharded by video,
    ``S`` is replicated and every rank passes the same probes; the ranks that do not hold a probe's video emit padding and zero,
    so the lists merge with the key merge and the counts add.  A probe with a span outside its video gives padding and rank 0.
    Returns (dist [Nm,k], sentence index [Nm,k] int64 (-1 = padding), ranks [Nm] int64 | None); dist / index are None for k = 0."""
    ops = ops or HipOps()
    pr = np.asarray(probes.cpu() if isinstance(probes, torch.Tensor) else probes, np.int64).reshape(-1, 3)
    Nm, Ns = len(pr), int(S.shape[0])
    rd = ri = None
    if own_sentence is not None:
        own = np.asarray(own_sentence.cpu() if isinstance(own_sentence, torch.Tensor) else own_sentence, np.int64).reshape(-1)
        if len(own) != Nm:
            raise ValueError(f"corpus_sentence_topk: {len(own)} own sentences for {Nm} probes")
        if Nm and (own.min() < 0 or own.max() >= Ns):
            raise ValueError(f"corpus_sentence_topk: own_sentence out of range [0, {Ns})")
        gv, s0, e0 = pr[:, 0], pr[:, 1], pr[:, 2]
        mine = (gv >= shard.lo) & (gv < shard.hi) & (s0 >= 0) & (e0 >= s0)
        n = np.where(mine, shard.counts_all[np.clip(gv, 0, max(shard.num_videos_all - 1, 0))], 0) if shard.num_videos_all else np.zeros(Nm, np.int64)
        mine &= e0 < n
        rd = torch.full((Nm,), float("inf"), dtype=torch.float32, device=shard.device)
        ri = torch.from_numpy(own).to(shard.device)
        sel = np.nonzero(mine)[0]
        if len(sel):
            sel_t = torch.from_numpy(sel).to(shard.device)
            sc = ops.score_own(S[ri[sel_t]].contiguous(), shard.bank, torch.from_numpy((gv[sel] - shard.lo).astype(np.int32)).to(shard.device))
            ns, ss, es = n[sel], s0[sel], e0[sel]
            col = np.where(ss == es, ss, ns + (ss * (2 * ns - ss - 1)) // 2 + (es - ss - 1))     # utils.generate_moments position
            rd[sel_t] = sc[torch.arange(len(sel), device=sc.device), torch.from_numpy(col).to(sc.device)]
    probes_t = torch.from_numpy(pr.astype(np.int32)).to(shard.device)
    od, oi, cnt = _exchange(*ops.score_sentences(S, shard.bank, probes_t, k, shard.lo, 0, rd, ri, workspace=workspace), k, ops, world)
    return od, oi, (cnt[0] if cnt is not None else None)


MINE_MAX_EXCL = 8                         # include/vfr.h: excluded spans per item (VFR_MINE_ANY)


@dataclass
class MinedNegatives:
    """What ``corpus_mine_negatives`` returns, per item (training span) in the caller's order: ``pos`` [Nm] the positive's score
    (+inf for an item without one: malformed, or a video of no shard); ``inter_dist`` / ``inter_vid`` [Nm, h] the hardest other
    videos as (score, global video index); ``intra_dist`` / ``intra_idx`` [Nm, h] the hardest other moments of the own video as
    (score, global moment id); both padded with (+inf, -1), None for h = 0.  ``count_inter`` / ``count_intra`` [Nm] int64 = the
    eligible negatives whose score is below positive + margin (None without a margin).  ``bad`` (device int32 [1]) is 1 when some
    item was malformed (query row or video out of range, start_t < 0, end_t < start_t, end_t past its video): such an item has
    pos = +inf and padded lists, like one without eligible negatives; ``malformed()`` reads the flag (one synchronisation).
    ``intra_spans()`` decodes the moment ids on the host."""
    pos: torch.Tensor
    inter_dist: torch.Tensor
    inter_vid: torch.Tensor
    intra_dist: torch.Tensor
    intra_idx: torch.Tensor
    count_inter: torch.Tensor
    count_intra: torch.Tensor
    bad: torch.Tensor = None
    own: np.ndarray = None                 # [Nm] the items' own global video (host)
    counts_all: np.ndarray = None
    mom_off_all: np.ndarray = None

    def malformed(self) -> bool:
        return bool(int(self.bad.item()))

    def intra_spans(self) -> np.ndarray:
        """[Nm, h, 2] int64 (start_t, end_t) of the intra negatives, (-1, -1) for padding (one device-to-host copy)."""
        ids = self.intra_idx.cpu().numpy()
        out = np.full(ids.shape + (2,), -1, np.int64)
        tables = {}
        for m in range(ids.shape[0]):
            real = ids[m] >= 0
            if not real.any():
                continue
            v = int(self.own[m])
            n = int(self.counts_all[v])
            if n not in tables:
                tables[n] = np.asarray(generate_moments(n), np.int64).reshape(-1, 2)
            out[m, real] = tables[n][ids[m, real] - int(self.mom_off_all[v])]
        return out


def corpus_mine_negatives(shard: CorpusShard, Q, items, h, intra="same_length", excl=None, semi_hard=False, margin=None, ops=None,
                          world=1, workspace=None) -> MinedNegatives:
    """Hard-negative mining over the corpus for the ranking loss: ``items`` (host array-like [Nm, 4]) = (row of ``Q``, own global
    video, start_t, end_t) training spans.  The loss's terms are retrieval scores, so the hardest negatives are exact keys: per item
    the ``h`` other videos (of at least end_t + 1 clips) with the smallest score at the item's span, and the ``h`` other moments of
    the own video -- of the same length (``intra`` "same_length") or all but the item's span and the spans of ``excl`` [Nm, X <= 8, 2]
    ("any") -- with the smallest score.  ``semi_hard``: only negatives scoring above the positive.  ``margin``: also the numbers of
    inter / intra negatives below fp32(positive + margin), the margin violators.  Order: the positives' scores (one launch on the
    rank that holds the video, MIN-reduced), floor and threshold from them, one mining call, then the sharded tail: inter lists
    merged by key, intra lists MIN / MAX-merged (only the own video's rank writes them), counts summed."""
    ops = ops or HipOps()
    if intra not in ("same_length", "any"):
        raise ValueError(f"corpus_mine_negatives: unknown intra mode {intra!r} (same_length, any)")
    it = np.asarray(items.cpu() if isinstance(items, torch.Tensor) else items, np.int64).reshape(-1, 4)
    Nm, dev = len(it), shard.device
    items_t = torch.from_numpy(it.astype(np.int32)).to(dev)
    excl_t = None
    if excl is not None and intra == "any":
        ex = np.asarray(excl.cpu() if isinstance(excl, torch.Tensor) else excl, np.int64)
        if ex.ndim != 3 or ex.shape[0] != Nm or ex.shape[2] != 2 or ex.shape[1] > MINE_MAX_EXCL:
            raise ValueError(f"corpus_mine_negatives: excl must be [Nm, X <= {MINE_MAX_EXCL}, 2], got {ex.shape}")
        excl_t = torch.from_numpy(ex.astype(np.int32)).to(dev)
    dist = _group(world)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    pos = ops.score_spans(Q, shard.bank, items_t, shard.lo, bad=bad)
    if dist is not None:
        dist.all_reduce(pos, op=dist.ReduceOp.MIN)
    floor = pos if semi_hard else None
    thr = None if margin is None else pos + torch.full_like(pos, float(margin))          # fp32(pos + fp32(margin))
    ind, inv, itd, iti, ci, ca = ops.mine_negatives(Q, shard.bank, items_t, h, shard.lo, intra, excl_t, floor, thr, bad=bad,
                                                    workspace=workspace)
    if dist is not None:
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)             # end_t past the video is seen by the owning rank only
        ind, inv, ci = _exchange(ind, inv, ci, h, ops, world)
        if h > 0:
            dist.all_reduce(itd, op=dist.ReduceOp.MIN)
            dist.all_reduce(iti, op=dist.ReduceOp.MAX)
        if ca is not None:
            dist.all_reduce(ca, op=dist.ReduceOp.SUM)
    return MinedNegatives(pos, ind, inv, itd, iti, ci, ca, bad, it[:, 1].copy(), shard.counts_all, shard.mom_off_all)


PARAGRAPH_MAX_LEN = 64                    # include/vfr.h: sentences per paragraph


@dataclass
class ParagraphGroups:
    """Paragraphs as runs of consecutive sentence rows (``paragraph_groups``): ``off`` [Ng+1] int64 on the host, non-decreasing from
    0 to the number of sentences; ``max_len`` = the longest run.  ``on(device)`` uploads ``off`` once."""
    off: np.ndarray
    max_len: int
    _dev: dict = None

    @property
    def num_groups(self):
        return len(self.off) - 1

    @property
    def num_sentences(self):
        return int(self.off[-1])

    def on(self, device):
        device = torch.device(device)
        if self._dev is None:
            self._dev = {}
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.off).to(device)
        return self._dev[key]


def paragraph_groups(lengths=None, labels=None, device=None) -> ParagraphGroups:
    """Paragraph runs from ``lengths`` (sentences per paragraph, 0 allowed: an empty paragraph) or from ``labels`` (one per
    sentence row: every maximal run of equal consecutive labels is a paragraph -- sort the rows by label first, stably, to get one
    paragraph per label).  A paragraph longer than 64 sentences raises ValueError.  ``device``: upload the offsets there as well."""
    if (lengths is None) == (labels is None):
        raise ValueError("paragraph_groups: give lengths or labels")
    if lengths is None:
        lab = list(labels)
        starts = [i for i in range(len(lab)) if i == 0 or lab[i] != lab[i - 1]]
        lengths = np.diff(np.asarray(starts + [len(lab)], np.int64))
    lens = np.asarray(lengths, np.int64).reshape(-1)
    if len(lens) and lens.min() < 0:
        raise ValueError("paragraph_groups: negative length")
    longest = int(lens.max()) if len(lens) else 0
    if longest > PARAGRAPH_MAX_LEN:
        raise ValueError(f"paragraph_groups: a paragraph of {longest} sentences (at most {PARAGRAPH_MAX_LEN})")
    out = ParagraphGroups(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), longest)
    if device is not None:
        out.on(device)
    return out


def corpus_paragraph_topk(shard: CorpusShard, Q, groups: ParagraphGroups, k, own_global=None, ground=False, ops=None, world=1,
                          workspace=None):
    """Paragraph-to-video retrieval over the corpus: per paragraph (``paragraph_groups`` over the rows of ``Q``) the k videos with
    the smallest score = fp32 mean, in sentence order, of the video's best moment distance for each sentence, in (score, global
    video index) order.  With ``own_global`` [Ng] (each paragraph's own global video index) also its 0-based rank = the number of
    videos whose key sorts strictly before the own video's key; the own key comes from one pairs launch on the rank that holds the
    video, MIN-reduced.  ``ground``: also where each sentence lands in each returned video (global id of that video's best moment
    for the sentence; -1 past the paragraph's length and for padding) from one pairs launch on the merged result, MAX-reduced.  A
    video never spans shards, so the lists merge with the key merge and the counts add.
    Returns (score [Ng,k], video index [Ng,k] int64 (-1 = padding), ranks [Ng] int64 | None, moments [Ng,k,max_len] int64 | None);
    score / video are None for k = 0."""
    ops = ops or HipOps()
    if groups.num_sentences != Q.shape[0]:
        raise ValueError(f"corpus_paragraph_topk: the groups cover {groups.num_sentences} sentences, Q has {Q.shape[0]}")
    Ng, dev = groups.num_groups, shard.device
    off_t = groups.on(dev)
    dist = _group(world)
    own_d = own_i = None
    if own_global is not None:
        own = np.asarray(own_global.cpu() if isinstance(own_global, torch.Tensor) else own_global, np.int64).reshape(-1)
        if len(own) != Ng:
            raise ValueError(f"corpus_paragraph_topk: {len(own)} own videos for {Ng} paragraphs")
        pairs = torch.from_numpy(np.stack([np.arange(Ng, dtype=np.int64), own], axis=1).astype(np.int32)).to(dev)
        own_d, _ = ops.score_paragraph_pairs(Q, shard.bank, off_t, groups.max_len, pairs, shard.lo, moments=False)
        if dist is not None:
            dist.all_reduce(own_d, op=dist.ReduceOp.MIN)
        own_i = torch.from_numpy(own).to(dev)
    od, oi, cnt = _exchange(*ops.score_paragraphs(Q, shard.bank, off_t, groups.max_len, k, shard.lo, own_d, own_i, workspace=workspace),
                            k, ops, world)
    moments = None
    if ground and k > 0:
        pairs = torch.stack([torch.arange(Ng, device=oi.device)[:, None].expand(Ng, k), oi], dim=2).reshape(Ng * k, 2).to(torch.int32)
        _, moments = ops.score_paragraph_pairs(Q, shard.bank, off_t, groups.max_len, pairs.contiguous(), shard.lo)
        if dist is not None:
            dist.all_reduce(moments, op=dist.ReduceOp.MAX)
        moments = moments.reshape(Ng, k, groups.max_len)
    return od, oi, cnt, moments


def corpus_video_sentence_topk(shard: CorpusShard, S, videos, k, own_off=None, own_rows=None, ground=False, ops=None, world=1,
                               workspace=None):
    """Video-to-sentence retrieval over the corpus: per probe video (``videos`` [Np]: global video indices, host array-like, any
    order, repeats allowed) the k sentences of the bank ``S`` [Ns, D] with the smallest score = the video's best moment distance for
    the sentence (``corpus_video_topk``'s quantity), in (score, sentence index) order.  With ``own_off`` [Np+1] / ``own_rows`` (a CSR
    of the rows of ``S`` that belong to each probe) also the 0-based rank of the probe's best-ranked own sentence = the number of
    sentences whose key sorts strictly before the smallest own key; the own distances come from one pairs launch (groups of
    length 1) on the rank that holds the video, MIN-reduced.  A probe without own rows gets rank -1; a probe whose video has no
    clips (or is out of range) scores nothing, so its rank is 0.  ``ground``: also the global id of the moment of the probe video
    that each returned sentence lands on (-1 for padding), from one pairs launch on the merged result, MAX-reduced.  ``world`` > 1:
    the clip bank is sharded by video, ``S`` is replicated and every rank passes the same probes; the lists merge with the key
    merge and the counts add.
    Returns (dist [Np,k], sentence index [Np,k] int64 (-1 = padding), ranks [Np] int64 | None, moments [Np,k] int64 | None);
    dist / index are None for k = 0."""
    ops = ops or HipOps()
    vids = np.asarray(videos.cpu() if isinstance(videos, torch.Tensor) else videos, np.int64).reshape(-1)
    Np, Ns, dev = len(vids), int(S.shape[0]), shard.device
    if Np and (vids.min() < -(1 << 31) or vids.max() >= (1 << 31)):
        raise ValueError("corpus_video_sentence_topk: video index outside int32")
    dist = _group(world)
    vids_t = torch.from_numpy(vids.astype(np.int32)).to(dev)
    rd = ri = has = None
    if (own_off is None) != (own_rows is None):
        raise ValueError("corpus_video_sentence_topk: give own_off and own_rows together")
    if own_off is not None:
        off = np.asarray(own_off.cpu() if isinstance(own_off, torch.Tensor) else own_off, np.int64).reshape(-1)
        rows = np.asarray(own_rows.cpu() if isinstance(own_rows, torch.Tensor) else own_rows, np.int64).reshape(-1)
        if len(off) != Np + 1 or off[0] != 0 or off[-1] != len(rows) or (np.diff(off) < 0).any():
            raise ValueError(f"corpus_video_sentence_topk: own_off must be a non-decreasing run [Np + 1] from 0 to {len(rows)}")
        if len(rows) and (rows.min() < 0 or rows.max() >= Ns):
            raise ValueError(f"corpus_video_sentence_topk: own_rows out of range [0, {Ns})")
        lens = np.diff(off)
        has = torch.from_numpy(lens > 0).to(dev)
        key = torch.full((Np,), KEY_INF & ~0xFFFFFFFF, dtype=torch.int64, device=dev)      # (+inf, 0): no own row
        if len(rows):
            nnz = len(rows)
            probe = np.repeat(np.arange(Np), lens)
            rows_t = torch.from_numpy(rows).to(dev)
            pairs = torch.from_numpy(np.stack([np.arange(nnz), vids[probe]], axis=1).astype(np.int32)).to(dev)
            one = torch.arange(nnz + 1, dtype=torch.int64, device=dev)
            own_d, _ = ops.score_paragraph_pairs(S[rows_t].contiguous(), shard.bank, one, 1, pairs, shard.lo, moments=False)
            if dist is not None:
                dist.all_reduce(own_d, op=dist.ReduceOp.MIN)
            best = torch.full((Np,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
            best.scatter_reduce_(0, torch.from_numpy(probe).to(dev), _pack_key(own_d, rows_t), reduce="amin")
            key = torch.where(has, best, key)
        if Np:                                                # (no probes: no keys, and the ranks are an empty tensor)
            rd, ri = _unpack_key(key)
            rd, ri = rd.contiguous(), ri.contiguous()
    od, oi, cnt = _exchange(*ops.score_video_sentences(S, shard.bank, vids_t, k, shard.lo, 0, rd, ri, workspace=workspace), k, ops, world)
    ranks = None
    if cnt is not None:
        ranks = torch.where(has, cnt[0], torch.full_like(cnt[0], -1))
    elif has is not None:
        ranks = torch.zeros((0,), dtype=torch.int64, device=dev)
    moments = None
    if ground and k > 0:
        moments = torch.full((Np * k,), -1, dtype=torch.int64, device=dev)
        if Np:
            flat = oi.reshape(-1)
            gv = torch.where(flat >= 0, vids_t.to(torch.int64).repeat_interleave(k), torch.full_like(flat, -1))
            pairs = torch.stack([torch.arange(Np * k, device=dev), gv], dim=1).to(torch.int32).contiguous()
            one = torch.arange(Np * k + 1, dtype=torch.int64, device=dev)
            _, mom = ops.score_paragraph_pairs(S[flat.clamp(min=0)].contiguous(), shard.bank, one, 1, pairs, shard.lo)
            moments = mom.reshape(-1)
            if dist is not None:
                dist.all_reduce(moments, op=dist.ReduceOp.MAX)
        moments = moments.reshape(Np, k)
    return od, oi, ranks, moments


def video_results(ids, dist, names, counts_all, mom_off_all):
    """Search results as rows: per query a list of (video name, start_t, end_t, distance) for the global moment ids ``ids``
    [Nq, k] (``corpus_video_topk`` / ``corpus_topk``); start_t / end_t are the inclusive clip span of the moment
    (``utils.generate_moments``), the unit of the annotations' times.  Padding (-1) is skipped."""
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, np.int64)
    dist = np.asarray(dist.cpu() if isinstance(dist, torch.Tensor) else dist, np.float32)
    mom = np.asarray(mom_off_all, np.int64)
    rows = []
    for q in range(ids.shape[0]):
        out = []
        for j in range(ids.shape[1]):
            m = int(ids[q, j])
            if m < 0:
                continue
            v = int(np.searchsorted(mom, m, side="right") - 1)
            s, e = generate_moments(int(counts_all[v]))[m - int(mom[v])]
            out.append((names[v], int(s), int(e), float(dist[q, j])))
        rows.append(out)
    return rows


SAMPLE_VIDEOS = 256      # corpus-wide size of the threshold sample (the single-GPU kernel samples the same number itself)


def sharded_search(shard: CorpusShard, Q, k, rank_dist, rank_idx, ops, world=1, workspace=None):
    """Fused scoring of one shard plus the exchange steps of SURVEY.md 8e.  Returns (dist, idx, counts).

    world == 1: one call (the kernel runs its own sample pre-pass).  world > 1 with k > 0: the threshold sample is
    split over the ranks so its cost scales too -- every rank scores its first 256/world videos exactly, the
    per-rank sample lists are all-gathered and merged into the GLOBAL sample top-k, whose k-th key seeds every
    rank's main pass over the rest of its shard (``thr_seed``); the final lists (main parts + the sample list) are
    all-gathered and merged once more.  Rank counts are summed with one all_reduce."""
    dist = _group(world)
    if dist is None or k == 0:
        od, oi, counts = ops.score_topk(Q, shard.bank, k, rank_dist, rank_idx, workspace=workspace)
        if dist is not None and counts is not None:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        return od, oi, counts
    nloc = shard.hi - shard.lo
    counts_loc = shard.counts_all[shard.lo:shard.hi]
    s_r = min(nloc, max(1, -(-SAMPLE_VIDEOS // world)))
    bank_a = ops.slice_bank(shard.bank, counts_loc, 0, s_r)
    d_a, i_a, cnt = ops.score_topk(Q, bank_a, k, rank_dist, rank_idx, workspace=workspace)
    # exchange buffer: slot g < world = rank g's list, slot world = the global sample list (second exchange only)
    buf = torch.empty((world + 1,) + tuple(d_a.shape), dtype=torch.int64, device=d_a.device)
    _all_gather_rows(dist, buf[:world], ops.pack_keys(d_a, i_a))
    _, _, s_k = ops.merge_keys(buf[:world], want_lists=False, want_keys=True)   # global sample top-k, every rank
    buf[world].copy_(s_k)
    seed = s_k[:, k - 1].contiguous()                                           # its k-th key (KEY_INF if fewer than k)
    if s_r < nloc:
        bank_b = ops.slice_bank(shard.bank, counts_loc, s_r, nloc)
        d_b, i_b, cnt = ops.score_topk(Q, bank_b, k, rank_dist, rank_idx, workspace=workspace, count_lt=cnt, thr_seed=seed)
        mine = ops.pack_keys(d_b, i_b)
    else:
        mine = torch.full_like(s_k, KEY_INF)
    if cnt is not None:
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
    _all_gather_rows(dist, buf[:world], mine)
    od, oi, _ = ops.merge_keys(buf)
    return od, oi, cnt


def sharded_search_fused(shard: CorpusShard, Q, k, keys_local, ops, world, workspace=None, on_keys=None):
    """``sharded_search`` with the small reductions folded into its two list exchanges (k > 0, two rank keys):

        exchange 1  all_gather of [Nq x k sample keys | 2 x Nq best-GT keys] per rank -> the global sample top-k (its k-th key
                    seeds every rank's main pass) and, by a MIN over the ranks, the global best-GT keys;
        exchange 2  all_gather of [Nq x k final keys | 2 x Nq rank counts] per rank -> the merged top-k and, by a SUM over the
                    ranks, the global rank counts.

    The sample pass (the rank's first 256/world videos, no rank keys yet) only produces the seed; the main pass then covers
    the WHOLE shard, sample videos included (2-3 % more scorings than skipping them, but no separate rank-only pass over the
    sample, no sub-bank and one list fewer in the final merge).  The seed handed on is the sample's k-th key + 1: the kernel
    collects keys strictly below its seed, and the k-th sample moment itself must stay collectable.  Everything stays int64
    (keys and counts), so both folds are exact.  Returns (dist, idx, counts)."""
    dist = _dist()
    Nq = Q.shape[0]
    nloc = shard.hi - shard.lo
    counts_loc = shard.counts_all[shard.lo:shard.hi]
    s_r = min(nloc, max(1, -(-SAMPLE_VIDEOS // world)))
    bank_a = ops.slice_bank(shard.bank, counts_loc, 0, s_r)
    d_a, i_a, _ = ops.score_topk(Q, bank_a, k, None, None, workspace=workspace)
    row = Nq * k + 2 * Nq
    mine = torch.empty((row,), dtype=torch.int64, device=d_a.device)
    ops.pack_keys(d_a, i_a, out=mine[:Nq * k].view(Nq, k))
    mine[Nq * k:].copy_(keys_local.reshape(-1))
    buf = torch.empty((world, row), dtype=torch.int64, device=d_a.device)
    _all_gather_rows(dist, buf, mine)
    keys = buf[:, Nq * k:].min(dim=0).values.view(2, Nq)                             # global best-GT keys (KEY_INF: none)
    if on_keys is not None:
        on_keys(keys)
    lists = buf[:, :Nq * k].view(world, Nq, k)                                       # strided view: merge_keys takes slot strides
    _, _, s_k = ops.merge_keys(lists, want_lists=False, want_keys=True)
    seed = (s_k[:, k - 1] + 1).clamp_(max=KEY_INF)
    rank_dist, rank_idx = _unpack_key(keys)
    d_b, i_b, cnt = ops.score_topk(Q, shard.bank, k, rank_dist.contiguous(), rank_idx.contiguous(), workspace=workspace,
                                   thr_seed=seed)
    ops.pack_keys(d_b, i_b, out=mine[:Nq * k].view(Nq, k))
    mine[Nq * k:].copy_(cnt.reshape(-1))
    _all_gather_rows(dist, buf, mine)
    counts = buf[:, Nq * k:].sum(dim=0).view(2, Nq)
    od, oi, _ = ops.merge_keys(lists)
    return od, oi, counts


def gather_merge_topk(od, oi, ops, world, extra=None):
    """Exchange step on its own: all_gather the per-shard [Nq, k] lists as packed int64 keys (a single collective),
    then merge with the (distance, id) tie-break.  ``extra`` = an additional (dist, idx) list every rank holds."""
    dist = _dist()
    buf = torch.empty((world + (extra is not None),) + tuple(od.shape), dtype=torch.int64, device=od.device)
    _all_gather_rows(dist, buf[:world], ops.pack_keys(od, oi))
    if extra is not None:
        ops.pack_keys(extra[0], extra[1], out=buf[world])
    d, i, _ = ops.merge_keys(buf)
    return d, i


class TorchCpuOps:
    """The same provider interface on CPU tensors with plain torch ops.

    This is the CPU *device* of the API (``evaluate(..., device='cpu')``, BASELINE.md C1, and the
    multi-rank plumbing tests under gloo) -- it is selected only by an explicit CPU device, never as a
    substitute when a ROCm device was asked for."""

    @dataclass
    class Bank:
        emb: torch.Tensor
        clip_off: torch.Tensor
        id_base: int

        @property
        def counts(self):
            return (self.clip_off[1:] - self.clip_off[:-1]).tolist()

    def make_bank(self, emb, clip_off, id_base):
        return TorchCpuOps.Bank(emb.float().cpu(), clip_off.cpu(), int(id_base))

    def encode_clips(self, model, seg, ctx, clip_off):
        n = (clip_off[1:] - clip_off[:-1]).long()
        vid = torch.repeat_interleave(torch.arange(len(n)), n)
        t = torch.arange(int(clip_off[-1])) - clip_off[:-1].long()[vid]
        nn_ = n[vid].float()
        x = torch.cat([seg, ctx[vid], (t.float() / nn_)[:, None], ((t + 1).float() / nn_)[:, None]], dim=1)
        with torch.no_grad():
            return model(x)

    def encode_queries(self, model, tokens):
        with torch.no_grad():
            return model(tokens, False, "cpu")

    @staticmethod
    def _video_scores(dist_v):                      # dist_v [Nq, n] -> [Nq, M] in generate_moments order
        n = dist_v.shape[1]
        cols = []
        for s, e in generate_moments(n):
            acc = dist_v[:, s]
            for c in range(s + 1, e + 1):
                acc = acc + dist_v[:, c]
            cols.append(acc / float(e - s + 1))
        return torch.stack(cols, dim=1) if cols else dist_v.new_zeros((dist_v.shape[0], 0))

    @staticmethod
    def _fma32(t, acc):
        """fp32 fma(t, t, acc) for acc >= 0, correctly rounded.  t * t is exact in float64 and s = acc + t * t is rounded once there;
        rounding s again to fp32 can only differ from rounding the exact sum when s is inexact AND sits on an fp32 midpoint (or the
        result is subnormal).  Those few elements are redone with s rounded to odd (the two-sum's error term gives the sticky bit;
        53 >= 2 * 24 + 2 bits make the final rounding exact)."""
        a = acc.astype(np.float64)
        p = t.astype(np.float64)
        p *= p
        s = a + p
        out = s.astype(np.float32)
        i = np.flatnonzero(((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | (s < 2.0 ** -125))
        if len(i):
            a, p, s = a.ravel()[i], p.ravel()[i], s.ravel()[i]
            bb = s - a
            err = (a - (s - bb)) + (p - bb)
            bits = s.view(np.int64)
            odd = np.where(err > 0, bits | 1, (bits - 1) | 1)             # exact sum above / below s (s > 0 whenever err != 0)
            out.ravel()[i] = np.where(err == 0, bits, odd).view(np.float64).astype(np.float32)
        return out

    @classmethod
    def _clip_dist(cls, Q, V, eps=1e-6):
        """[Nq, C] clip distances ||(v - q) + eps||_2 with the kernels' own chain -- k-ascending fp32 fma of ((v - q) + eps)^2 and
        an IEEE sqrt -- so every score of this provider carries the HIP path's bits (a vectorised sum orders the additions
        differently).  The ONE distance of the provider: lists, own keys and rank counts all compare keys built on it."""
        q, v = Q.float().numpy(), V.float().numpy()
        e32 = np.float32(eps)
        out = np.empty((q.shape[0], v.shape[0]), np.float32)
        step = max(1, 32768 // max(1, q.shape[0]))                        # clips per block: the temporaries stay in cache
        for c0 in range(0, v.shape[0], step):
            vb = v[c0:c0 + step]
            acc = np.zeros((q.shape[0], vb.shape[0]), np.float32)
            for kk in range(q.shape[1]):
                acc = cls._fma32((vb[None, :, kk] - q[:, None, kk]) + e32, acc)
            out[:, c0:c0 + step] = np.sqrt(acc)
        return torch.from_numpy(out)

    def _dense(self, Q, bank, eps=1e-6):
        d = self._clip_dist(Q, bank.emb, eps)
        off = bank.clip_off.tolist()
        out = [self._video_scores(d[:, off[v]:off[v + 1]]) for v in range(len(off) - 1)]
        return torch.cat(out, dim=1) if out else Q.new_zeros((Q.shape[0], 0))

    def score_own(self, Q, bank, own_local, eps=1e-6):
        counts = bank.counts
        nmax = max(counts) if counts else 0
        out = torch.full((Q.shape[0], nmax * (nmax + 1) // 2), float("inf"))
        off = bank.clip_off.tolist()
        for q, v in enumerate(own_local.tolist()):
            V = bank.emb[off[v]:off[v + 1]]
            d = self._clip_dist(Q[q:q + 1], V, eps)
            sc = self._video_scores(d)[0]
            out[q, :sc.numel()] = sc
        return out

    def _dense_keys(self, Q, bank):
        """[Nq, M] packed (score, global id) keys of every moment of the bank."""
        sc = self._dense(Q, bank)
        return _pack_key(sc, (bank.id_base + torch.arange(sc.shape[1]))[None, :].expand_as(sc))

    @staticmethod
    def _pad_k(srt, k):
        """Keys padded with KEY_INF to k along the last axis."""
        pad = k - srt.shape[-1]
        return srt if pad <= 0 else torch.cat([srt, torch.full(tuple(srt.shape[:-1]) + (pad,), KEY_INF, dtype=torch.int64)], dim=-1)

    @staticmethod
    def _lists_of(keys):
        """Keys -> (dist, idx) lists, KEY_INF as the padding (+inf, -1)."""
        od, oi = _unpack_key(keys)
        return torch.where(keys == KEY_INF, torch.full_like(od, float("inf")), od), torch.where(keys == KEY_INF, torch.full_like(oi, -1), oi)

    @classmethod
    def _topk_lists(cls, keys, k):
        """The k smallest keys per row of ``keys`` [N, M] as padded lists; (None, None) for k == 0."""
        return cls._lists_of(cls._pad_k(keys.sort(dim=1).values[:, :k], k)) if k > 0 else (None, None)

    @staticmethod
    def _counts_below(keys, kstar, count_lt):
        """[R, N] = per packed rank key ``kstar`` [R, N] the keys of its row of ``keys`` [N, M] that sort strictly before it, plus
        ``count_lt``; None without rank keys."""
        if kstar is None:
            return None
        counts = (keys[None, :, :] < kstar[:, :, None]).sum(-1)
        return counts if count_lt is None else counts + count_lt

    def slice_bank(self, bank, counts, v0, v1):
        off, mom = csr_offsets(counts)
        clip_off = torch.from_numpy((off[v0:v1 + 1] - off[v0]).astype(np.int32))
        return TorchCpuOps.Bank(bank.emb[int(off[v0]):int(off[v1])], clip_off, bank.id_base + int(mom[v0]))

    def score_topk(self, Q, bank, k, rank_dist, rank_idx, workspace=None, count_lt=None, thr_seed=None):
        keys = self._dense_keys(Q, bank)     # thr_seed is only an accelerator: the exact result does not depend on it
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Q.shape[0]), rank_idx.reshape(-1, Q.shape[0]))
        return self._topk_lists(keys, k) + (self._counts_below(keys, kstar, count_lt),)

    def score_video_topk(self, Q, bank, k, own_dist=None, own_idx=None, count=None, workspace=None):
        """Video-level retrieval from the dense scores: per video the smallest (score, id) key, then the k smallest of those
        and the number of videos below the own key (same semantics as ``_vfr.score_video_topk``)."""
        keys = self._dense_keys(Q, bank)
        Nq = Q.shape[0]
        mo = csr_offsets(bank.counts)[1]
        best = [keys[:, int(a):int(b)].min(dim=1).values for a, b in zip(mo[:-1], mo[1:]) if b > a]
        best = torch.stack(best, dim=1) if best else torch.zeros((Nq, 0), dtype=torch.int64)
        if own_dist is not None:             # one key per query, [Nq] counts
            count = self._counts_below(best, _pack_key(own_dist.reshape(1, Nq), own_idx.reshape(1, Nq)), count)[0]
        return self._topk_lists(best, k) + (count,)

    def score_moment_nms(self, Q, bank, k, per_video=0, nms_iou=1.0, workspace=None):
        """Diversified moment retrieval from the dense scores (same rule as ``_vfr.score_moment_nms``): per video, moments in
        key order, greedy acceptance under the float64 IoU test and the cap, then the k smallest accepted keys."""
        keys = self._dense_keys(Q, bank)
        Nq = Q.shape[0]
        acc = torch.full_like(keys, KEY_INF)
        cap = per_video if per_video > 0 else keys.shape[1] + 1
        m0 = 0
        for n in bank.counts:
            spans = np.asarray(generate_moments(int(n)), np.int64).reshape(-1, 2)
            M = len(spans)
            if M == 0:
                continue
            s, e = spans[:, 0], spans[:, 1]
            inter = np.maximum(np.minimum(e[:, None], e[None, :]) + 1 - np.maximum(s[:, None], s[None, :]), 0)
            union = np.maximum(e[:, None], e[None, :]) + 1 - np.minimum(s[:, None], s[None, :])
            supp = torch.from_numpy(inter / union > nms_iou) | torch.eye(M, dtype=torch.bool)
            kv = keys[:, m0:m0 + M]
            order = kv.argsort(dim=1)
            alive = torch.ones((Nq, M), dtype=torch.bool)
            taken = torch.zeros((Nq,), dtype=torch.int64)
            rows = torch.arange(Nq)
            for r in range(M):
                j = order[:, r]
                take = alive[rows, j] & (taken < cap)
                alive &= ~(supp[j] & take[:, None])
                taken += take.long()
                acc[rows[take], m0 + j[take]] = kv[rows[take], j[take]]
            m0 += M
        return self._lists_of(self._pad_k(acc.sort(dim=1).values[:, :k], k))

    def score_subset(self, Q, bank, cand_off, cand_vid, k, level="moments", vid_base=0, rank_dist=None, rank_idx=None, count_lt=None,
                     workspace=None, bad=None, max_list=None):
        """Candidate-restricted retrieval from the dense scores (same semantics as ``_vfr.score_subset``): per query the keys of
        the listed videos of this bank (moments, or each video's smallest key), the k smallest, and the keys below each rank key."""
        if level not in ("moments", "videos"):
            raise RuntimeError(f"score_subset: unknown level {level!r} (moments, videos)")
        keys = self._dense_keys(Q, bank)
        Nq = Q.shape[0]
        n = np.asarray(bank.counts, np.int64)
        Nv = len(n)
        mo = csr_offsets(n)[1]
        off = [int(x) for x in torch.as_tensor(cand_off).tolist()]
        vid = [int(x) for x in torch.as_tensor(cand_vid).tolist()]
        rows = []
        for q in range(Nq):
            sel = [v - vid_base for v in vid[off[q]:off[q + 1]] if 0 <= v - vid_base < Nv and n[v - vid_base] > 0]
            if level == "moments":
                cols = np.concatenate([np.arange(mo[v], mo[v + 1]) for v in sel]) if sel else np.zeros(0, np.int64)
                kk = keys[q, torch.from_numpy(cols)]
            else:
                kk = torch.stack([keys[q, int(mo[v]):int(mo[v + 1])].min() for v in sel]) if sel else torch.zeros(0, dtype=torch.int64)
            rows.append(kk)
        longest = max([r.numel() for r in rows], default=0)             # each query's keys as one KEY_INF-padded row
        sub = torch.stack([self._pad_k(r, longest) for r in rows]) if rows else torch.zeros((0, 0), dtype=torch.int64)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Nq), rank_idx.reshape(-1, Nq))
        return self._topk_lists(sub, k) + (self._counts_below(sub, kstar, count_lt),)

    def _fusion_check(self, Qs, banks, weights, who):
        """Late fusion on this provider: the streams' banks must describe the same videos -> (Qs, banks, fp32 weights)."""
        Qs, banks = list(Qs), list(banks)
        if len(Qs) != len(banks):
            raise ValueError(f"{who}: {len(Qs)} query matrices for {len(banks)} banks")
        w = fusion_weights(weights, len(banks))
        for s, b in enumerate(banks[1:], 1):
            if b.id_base != banks[0].id_base or not torch.equal(b.clip_off, banks[0].clip_off):
                raise ValueError(f"{who}: bank {s} does not describe the videos of bank 0 (clip_off, id_base)")
        return Qs, banks, w

    def _fused_clip_dist(self, Qs, embs, w, eps=1e-6):
        """[Nq, C] fused clip distances: f = w_0 d_0, f = f + w_s d_s -- SEPARATE float32 multiplies and adds on the provider's one
        ``_clip_dist``, so the CPU device carries the fusion kernels' bits."""
        f = None
        for s, (Q, V) in enumerate(zip(Qs, embs)):
            t = np.multiply(w[s], self._clip_dist(Q, V, eps).numpy(), dtype=np.float32)
            f = t if f is None else np.add(f, t, dtype=np.float32)
        return torch.from_numpy(f)

    def score_fusion_own(self, Qs, banks, weights, own_local, eps=1e-6):
        """Fused scores of each query against its own video: the layout of ``score_own`` (same semantics as
        ``_vfr.score_fusion_own``)."""
        Qs, banks, w = self._fusion_check(Qs, banks, weights, "score_fusion_own")
        counts = banks[0].counts
        nmax = max(counts) if counts else 0
        Nq = Qs[0].shape[0]
        out = torch.full((Nq, nmax * (nmax + 1) // 2), float("inf"))
        off = banks[0].clip_off.tolist()
        for q, v in enumerate(own_local.tolist()):
            if not 0 <= v < len(counts):
                continue
            f = self._fused_clip_dist([Q[q:q + 1] for Q in Qs], [b.emb[off[v]:off[v + 1]] for b in banks], w, eps)
            sc = self._video_scores(f)[0]
            out[q, :sc.numel()] = sc
        return out

    def score_fusion(self, Qs, banks, weights, k, level="moments", rank_dist=None, rank_idx=None, count_lt=None, workspace=None,
                     eps=1e-6):
        """Late-fusion retrieval from dense scores (same semantics as ``_vfr.score_fusion``): the fused clip distances, the moment
        chain on them (``_video_scores``), keys (score, global id); moments, or each video's smallest key."""
        if level not in ("moments", "videos"):
            raise ValueError(f"score_fusion: unknown level {level!r} (moments, videos)")
        Qs, banks, w = self._fusion_check(Qs, banks, weights, "score_fusion")
        b0 = banks[0]
        Nq = Qs[0].shape[0]
        f = self._fused_clip_dist(Qs, [b.emb for b in banks], w, eps)
        off = b0.clip_off.tolist()
        cols = [self._video_scores(f[:, off[v]:off[v + 1]]) for v in range(len(off) - 1)]
        sc = torch.cat(cols, dim=1) if cols else torch.zeros((Nq, 0))
        keys = _pack_key(sc, (b0.id_base + torch.arange(sc.shape[1]))[None, :].expand_as(sc))
        if level == "videos":
            mo = csr_offsets(b0.counts)[1]
            best = [keys[:, int(a):int(b)].min(dim=1).values for a, b in zip(mo[:-1], mo[1:]) if b > a]
            keys = torch.stack(best, dim=1) if best else torch.zeros((Nq, 0), dtype=torch.int64)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Nq), rank_idx.reshape(-1, Nq))
        return self._topk_lists(keys, k) + (self._counts_below(keys, kstar, count_lt),)

    def score_fusion_sweep_own(self, Qs, banks, grid, own_local, eps=1e-6):
        """``score_fusion_own`` per row of the weight grid, [W, Nq, Mmax] (same semantics as ``_vfr.score_fusion_sweep_own``): the
        provider's one ``_clip_dist`` and its fp32 multiply / add fuse, row by row."""
        grid = fusion_weight_grid(grid, len(list(banks)))
        return torch.stack([self.score_fusion_own(Qs, banks, w, own_local, eps) for w in grid])

    def score_fusion_sweep(self, Qs, banks, grid, level, rank_dist, rank_idx, count_lt=None, eps=1e-6):
        """The rank counts of ``score_fusion`` (k = 0) per row of the weight grid, [W, R, Nq] (same semantics as
        ``_vfr.score_fusion_sweep``); ``count_lt`` [W, R, Nq] is added."""
        grid = fusion_weight_grid(grid, len(list(banks)))
        W, Nq = len(grid), Qs[0].shape[0]
        if rank_dist is None or rank_idx is None:
            raise ValueError("score_fusion_sweep: rank_dist and rank_idx [W, R, Nq] are required (the sweep only counts)")
        if rank_dist.dim() == 2 and rank_idx.dim() == 2:
            rank_dist, rank_idx = rank_dist[:, None], rank_idx[:, None]
        if rank_dist.dim() != 3 or rank_dist.shape[0] != W or rank_dist.shape[2] != Nq or rank_idx.shape != rank_dist.shape:
            raise ValueError(f"score_fusion_sweep: rank_dist / rank_idx must be [{W}, R, {Nq}], got {tuple(rank_dist.shape)} / "
                             f"{tuple(rank_idx.shape)}")
        return torch.stack([self.score_fusion(Qs, banks, grid[w], 0, level, rank_dist[w], rank_idx[w],
                                              None if count_lt is None else count_lt[w], eps=eps)[2] for w in range(W)])

    @staticmethod
    def _biased(sc, bias, bad):
        """g = fl(score + entry) as float32 numpy, +inf where the entry is NaN or < 0 (reported in ``bad``): ONE float32 addition on
        the provider's dense scores, so the CPU device carries the prior kernels' bits."""
        wrong = ~(bias >= 0)
        if wrong.any() and bad is not None:
            bad.fill_(1)
        with np.errstate(invalid="ignore"):
            g = np.add(sc, np.where(wrong, np.float32(np.inf), bias)[None, :], dtype=np.float32)
        return g

    def score_prior_own(self, Q, bank, table, own_local, bad=None, eps=1e-6):
        """Biased scores of each query against its own video: the layout of ``score_own``, +inf at excluded moments (same semantics
        as ``_vfr.score_prior_own``)."""
        counts = bank.counts
        nmax = max(counts) if counts else 0
        if table.max_clips < nmax:
            raise ValueError(f"score_prior_own: the moment table covers videos of up to {table.max_clips} clips, the bank has {nmax}")
        out = torch.full((Q.shape[0], nmax * (nmax + 1) // 2), float("inf"))
        off = bank.clip_off.tolist()
        for q, v in enumerate(own_local.tolist()):
            if not 0 <= v < len(counts):
                continue
            sc = self._video_scores(self._clip_dist(Q[q:q + 1], bank.emb[off[v]:off[v + 1]], eps)).numpy()
            out[q, :sc.shape[1]] = torch.from_numpy(self._biased(sc, table.row(counts[v]), bad)[0])
        return out

    def score_prior(self, Q, bank, table, k, level="moments", rank_dist=None, rank_idx=None, count_lt=None, workspace=None, bad=None,
                    eps=1e-6):
        """Prior-aware retrieval from dense scores (same semantics as ``_vfr.score_prior``): the dense scores, one float32 addition of
        the table entries, keys (biased score, global id) of the candidates (g < +inf; the others become KEY_INF, which sorts last,
        is never below a rank key and turns into padding); moments, or each video's smallest candidate key."""
        if level not in ("moments", "videos"):
            raise ValueError(f"score_prior: unknown level {level!r} (moments, videos)")
        counts = bank.counts
        if table.max_clips < (max(counts) if counts else 0):
            raise ValueError(f"score_prior: the moment table covers videos of up to {table.max_clips} clips, the bank has {max(counts)}")
        Nq = Q.shape[0]
        sc = self._dense(Q, bank, eps).numpy()
        bias = np.concatenate([table.row(n) for n in counts]) if counts else np.zeros(0, np.float32)
        g = torch.from_numpy(self._biased(sc, bias, bad))
        keys = _pack_key(g, (bank.id_base + torch.arange(g.shape[1]))[None, :].expand_as(g))
        keys = torch.where(g < float("inf"), keys, torch.full_like(keys, KEY_INF))
        if level == "videos":
            mo = csr_offsets(counts)[1]
            best = [keys[:, int(a):int(b)].min(dim=1).values for a, b in zip(mo[:-1], mo[1:]) if b > a]
            keys = torch.stack(best, dim=1) if best else torch.zeros((Nq, 0), dtype=torch.int64)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Nq), rank_idx.reshape(-1, Nq))
        return self._topk_lists(keys, k) + (self._counts_below(keys, kstar, count_lt),)

    def score_window(self, Q, bank, max_len, k, rank_dist=None, rank_idx=None, count_lt=None, workspace=None, eps=1e-6):
        """Windowed retrieval (same semantics and bits as ``_vfr.score_window``): lane = flat start clip, a sequential float32 sum
        over the next ``max_len`` end clips of the same video on the provider's one clip distance, one division, the canonical id.
        Nothing is sized by n (n + 1) / 2 of a video."""
        L = _check_window(max_len, "score_window")
        counts = np.asarray(bank.counts, np.int64)
        if len(counts) and int(counts.max()) > WINDOW_MAX_CLIPS:
            raise ValueError(f"score_window: videos of up to {WINDOW_MAX_CLIPS} clips, the bank has one of {int(counts.max())}")
        Nq = Q.shape[0]
        off, mom = csr_offsets(counts)
        vid = np.repeat(np.arange(len(counts)), counts)
        s, n = np.arange(int(off[-1])) - off[vid], counts[vid]
        d = self._clip_dist(Q, bank.emb, eps).numpy()
        acc = d.copy()
        parts = []
        for i in range(L):
            live = np.nonzero(s + i < n)[0]                                   # (nested: a start clip that ran out stays out)
            if not len(live):
                break
            if i:
                acc[:, live] = acc[:, live] + d[:, live + i]
            sl, nl = s[live], n[live]
            j = sl if i == 0 else nl + (sl * (2 * nl - sl - 1)) // 2 + (i - 1)
            ids = torch.from_numpy(bank.id_base + mom[vid[live]] + j)
            parts.append(_pack_key(torch.from_numpy(acc[:, live] / np.float32(i + 1)), ids[None, :].expand(Nq, len(live))))
        keys = torch.cat(parts, dim=1) if parts else torch.zeros((Nq, 0), dtype=torch.int64)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Nq), rank_idx.reshape(-1, Nq))
        return self._topk_lists(keys, k) + (self._counts_below(keys, kstar, count_lt),)

    def window_span_keys(self, Q, bank, items, vid_base=0, out=None, bad=None, eps=1e-6):
        """Keys of named (query row, global video, start, end) spans (same semantics and bits as ``_vfr.window_span_keys``): items of
        other shards and malformed ones (query row out of range, start < 0, end < start, end past the video, more than 64 clips)
        are left untouched (KEY_INF pre-filled), the malformed ones set ``bad``."""
        rows = [[int(x) for x in r] for r in torch.as_tensor(items).reshape(-1, 4).tolist()]
        off = bank.clip_off.tolist()
        mom = csr_offsets(bank.counts)[1]
        Nv, Nq = len(off) - 1, Q.shape[0]
        if out is None:
            out = torch.full((len(rows),), KEY_INF, dtype=torch.int64)
        for p, (q, gv, s0, e0) in enumerate(rows):
            wrong = q < 0 or q >= Nq or s0 < 0 or e0 < s0 or e0 - s0 + 1 > WINDOW_MAX_LEN
            lv = gv - vid_base
            owned = 0 <= lv < Nv
            if owned and e0 >= off[lv + 1] - off[lv]:
                wrong = True
            if wrong and bad is not None:
                bad.fill_(1)
            if wrong or not owned:
                continue
            n = off[lv + 1] - off[lv]
            d = self._clip_dist(Q[q:q + 1], bank.emb[off[lv] + s0:off[lv] + e0 + 1], eps)[0]
            acc = d[0]
            for c in range(1, d.shape[0]):
                acc = acc + d[c]
            j = s0 if s0 == e0 else n + (s0 * (2 * n - s0 - 1)) // 2 + (e0 - s0 - 1)
            out[p] = _pack_key((acc / float(e0 - s0 + 1)).reshape(1), torch.tensor([bank.id_base + int(mom[lv]) + j]))[0]
        return out

    def score_sentences(self, S, bank, probes, k, vid_base=0, sent_base=0, rank_dist=None, rank_idx=None, count_lt=None, bad=None,
                        workspace=None, eps=1e-6):
        """Sentence retrieval for moments from dense torch arithmetic (same semantics as ``_vfr.score_sentences``): per probe
        (global video, start_t, end_t) the mean clip distance of every sentence of ``S``, keys (score, sent_base + row), the k
        smallest, and the keys below each rank key.  Probes of other shards or with a bad span give padding and add nothing."""
        S = S.float()
        Ns = S.shape[0]
        rows = [[int(x) for x in r] for r in torch.as_tensor(probes).tolist()]
        Nm = len(rows)
        off = bank.clip_off.tolist()
        Nv = len(off) - 1
        ids = sent_base + torch.arange(Ns)
        out = torch.full((Nm, Ns), KEY_INF, dtype=torch.int64)          # a probe without keys here: padding, nothing below
        for m, (gv, s0, e0) in enumerate(rows):
            wrong = gv < 0 or s0 < 0 or e0 < s0
            lv = gv - vid_base
            owned = gv >= 0 and 0 <= lv < Nv
            if owned and e0 >= off[lv + 1] - off[lv]:
                wrong = True
            if wrong and bad is not None:
                bad.fill_(1)
            if wrong or not owned:
                continue
            V = bank.emb[off[lv] + s0:off[lv] + e0 + 1]
            d = self._clip_dist(S, V, eps)
            acc = d[:, 0]
            for c in range(1, d.shape[1]):
                acc = acc + d[:, c]
            out[m] = _pack_key(acc / float(e0 - s0 + 1), ids)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Nm), rank_idx.reshape(-1, Nm))
        return self._topk_lists(out, k) + (self._counts_below(out, kstar, count_lt),)

    def score_video_sentences(self, S, bank, videos, k, vid_base=0, sent_base=0, rank_dist=None, rank_idx=None, count_lt=None,
                              bad=None, workspace=None, eps=1e-6):
        """Video-to-sentence retrieval from dense torch arithmetic (same semantics and bits as ``_vfr.score_video_sentences``): per
        probe video the smallest moment score of every sentence of ``S`` over the video's whole triangle, keys (score, sent_base +
        row), the k smallest, and the keys below each rank key.  Probes of other shards or on a video without clips give padding
        and add nothing; a video < 0 sets ``bad``."""
        S = S.float()
        Ns = S.shape[0]
        vids = [int(x) for x in torch.as_tensor(videos).reshape(-1).tolist()]
        Np = len(vids)
        off = bank.clip_off.tolist()
        Nv = len(off) - 1
        ids = sent_base + torch.arange(Ns)
        out = torch.full((Np, Ns), KEY_INF, dtype=torch.int64)          # a probe without keys here: padding, nothing below
        best = {}                                                        # local video -> [Ns] best distances, once per video
        for p, gv in enumerate(vids):
            if gv < 0:
                if bad is not None:
                    bad.fill_(1)
                continue
            lv = gv - vid_base
            if lv < 0 or lv >= Nv or off[lv + 1] <= off[lv] or Ns == 0:
                continue
            if lv not in best:
                best[lv] = self._video_scores(self._clip_dist(S, bank.emb[off[lv]:off[lv + 1]], eps)).min(dim=1).values
            out[p] = _pack_key(best[lv], ids)
        kstar = None if rank_dist is None else _pack_key(rank_dist.reshape(-1, Np), rank_idx.reshape(-1, Np))
        return self._topk_lists(out, k) + (self._counts_below(out, kstar, count_lt),)

    def _span_scores(self, Q, bank, items, vid_base, bad, eps=1e-6):
        """What the mining entry points share: the items as host rows with their malformed flag and own local video, and the clip
        distances of every distinct query row against the bank ([U, C], the provider's one distance)."""
        rows = [[int(x) for x in r] for r in torch.as_tensor(items).tolist()]
        off = bank.clip_off.tolist()
        Nv, Nq = len(off) - 1, Q.shape[0]
        out = []
        for q, gv, s0, e0 in rows:
            wrong = q < 0 or q >= Nq or gv < 0 or s0 < 0 or e0 < s0
            lv = gv - vid_base
            owned = gv >= 0 and 0 <= lv < Nv
            if owned and e0 >= off[lv + 1] - off[lv]:
                wrong = True
            if wrong and bad is not None:
                bad.fill_(1)
            out.append((q, gv, s0, e0, wrong, lv if owned else -1))
        used = sorted({r[0] for r in out if not r[4]})
        slot = {q: i for i, q in enumerate(used)}
        d = self._clip_dist(Q.float()[used], bank.emb, eps) if used else torch.zeros((0, bank.emb.shape[0]))
        return out, off, slot, d

    def score_spans(self, Q, bank, items, vid_base=0, out=None, bad=None):
        """Named (query, global video, span) scores (same semantics as ``_vfr.score_spans``): the fp32 chain s -> e of the clip
        distances and one division; items of other shards and malformed ones are left untouched (+inf pre-filled)."""
        rows, off, slot, d = self._span_scores(Q, bank, items, vid_base, bad)
        if out is None:
            out = torch.full((len(rows),), float("inf"))
        for p, (q, gv, s0, e0, wrong, lv) in enumerate(rows):
            if wrong or lv < 0:
                continue
            acc = d[slot[q], off[lv] + s0]
            for c in range(s0 + 1, e0 + 1):
                acc = acc + d[slot[q], off[lv] + c]
            out[p] = acc / float(e0 - s0 + 1)
        return out

    def mine_negatives(self, Q, bank, items, h, vid_base=0, intra="same_length", excl=None, floor=None, thr=None, want_inter=True,
                       want_intra=True, intra_out=None, count_inter=None, count_intra=None, bad=None, workspace=None):
        """Hard-negative mining from dense torch arithmetic (same semantics and bits as ``_vfr.mine_negatives``): per item the keys
        (score at the item's span, vid_base + video) of the other videos with at least end_t + 1 clips, the keys (score, global
        moment id) of the own video's eligible moments, the ``h`` smallest above the floor, and the eligible keys below ``thr``."""
        if intra not in ("same_length", "any"):
            raise RuntimeError(f"mine_negatives: unknown intra mode {intra!r} (same_length, any)")
        rows, off, slot, d = self._span_scores(Q, bank, items, vid_base, bad)
        Nm = len(rows)
        offs = np.asarray(off, np.int64)
        n_all = np.diff(offs)
        mo = csr_offsets(n_all)[1]
        vids = vid_base + torch.arange(len(n_all))
        ex = None if excl is None or intra != "any" else torch.as_tensor(excl).tolist()
        lists = h > 0
        ind = inv = itd = iti = None
        if want_inter and lists:
            ind, inv = torch.full((Nm, h), float("inf")), torch.full((Nm, h), -1, dtype=torch.int64)
        if want_intra and lists:
            itd, iti = (torch.full((Nm, h), float("inf")), torch.full((Nm, h), -1, dtype=torch.int64)) if intra_out is None else intra_out
        if thr is None or not (want_inter or want_intra):
            thr = count_inter = count_intra = None
        else:
            count_inter = (torch.zeros(Nm, dtype=torch.int64) if count_inter is None else count_inter) if want_inter else None
            count_intra = (torch.zeros(Nm, dtype=torch.int64) if count_intra is None else count_intra) if want_intra else None

        def select(m, sc, ids):
            """(listed keys sorted and padded as lists, number below the threshold) of the eligible (score, id) pairs"""
            below = int((sc < thr[m]).sum()) if thr is not None else 0
            if floor is not None:
                keep = ~(sc <= floor[m])
                sc, ids = sc[keep], ids[keep]
            return self._topk_lists(_pack_key(sc, ids)[None], h) if lists else (None, None), below

        for m, (q, gv, s0, e0, wrong, lv) in enumerate(rows):
            if wrong:
                continue
            dq = d[slot[q]]
            if want_inter:
                el = np.flatnonzero((n_all > e0) & (np.arange(len(n_all)) != gv - vid_base))
                base = torch.from_numpy(offs[el])
                acc = dq[base + s0]
                for c in range(s0 + 1, e0 + 1):
                    acc = acc + dq[base + c]
                (ld, li), below = select(m, acc / float(e0 - s0 + 1), vids[torch.from_numpy(el)])
                if lists:
                    ind[m], inv[m] = ld[0], li[0]
                if count_inter is not None:
                    count_inter[m] += below
            if want_intra and lv >= 0:
                n = int(n_all[lv])
                spans = generate_moments(n)
                sc = self._video_scores(dq[None, off[lv]:off[lv + 1]])[0]
                if intra == "same_length":
                    ok = [e1 - s1 == e0 - s0 and (s1, e1) != (s0, e0) for s1, e1 in spans]
                else:
                    gone = {(s0, e0)} | ({(int(a), int(b)) for a, b in ex[m]} if ex is not None else set())
                    ok = [(s1, e1) not in gone for s1, e1 in spans]
                ok = torch.tensor(ok, dtype=torch.bool)
                ids = bank.id_base + int(mo[lv]) + torch.arange(len(spans))
                (ld, li), below = select(m, sc[ok], ids[ok])
                if lists:
                    itd[m], iti[m] = ld[0], li[0]
                if count_intra is not None:
                    count_intra[m] += below
        return ind, inv, itd, iti, count_inter, count_intra

    def _video_best_keys(self, Q, bank):
        """[Nq, Nv] packed (distance, global moment id) best key of every video for every row of ``Q`` (KEY_INF: no clips)."""
        keys = self._dense_keys(Q, bank)
        mo = csr_offsets(bank.counts)[1]
        cols = [keys[:, int(a):int(b)].min(dim=1).values if b > a else torch.full((Q.shape[0],), KEY_INF, dtype=torch.int64)
                for a, b in zip(mo[:-1], mo[1:])]
        return torch.stack(cols, dim=1) if cols else torch.zeros((Q.shape[0], 0), dtype=torch.int64)

    @staticmethod
    def _group_runs(grp_off, Nq, max_len, bad):
        """The runs of ``grp_off`` as (j0, L) clamped like the kernels clamp them; ``bad`` is set for a malformed ``grp_off``."""
        off = [int(x) for x in torch.as_tensor(grp_off).tolist()]
        runs, wrong = [], off[0] != 0 or off[-1] != Nq
        for a, b in zip(off[:-1], off[1:]):
            wrong = wrong or b < a or b - a > max_len
            a = min(max(a, 0), Nq)
            b = min(max(b, a), Nq, a + max_len)
            runs.append((a, b - a))
        if wrong and bad is not None:
            bad.fill_(1)
        return runs

    @staticmethod
    def _paragraph_score(dist_rows):
        """[L, n] best distances -> [n] paragraph scores: the fp32 chain in sentence order, then one division."""
        acc = dist_rows[0]
        for t in range(1, dist_rows.shape[0]):
            acc = acc + dist_rows[t]
        return acc / float(dist_rows.shape[0])

    def score_paragraphs(self, Q, bank, grp_off, max_len, k, vid_base=0, own_dist=None, own_idx=None, count=None, workspace=None,
                         bad=None):
        """Paragraph-to-video retrieval from the dense scores (same semantics and bits as ``_vfr.score_paragraphs``): per
        (sentence, video) the smallest (score, id) key, per paragraph the fp32 chain of their distances in sentence order and one
        division, keys (score, vid_base + video); the k smallest and the number of videos below the own key."""
        Q = Q.float()
        best = _unpack_key(self._video_best_keys(Q, bank))[0]
        live = torch.tensor([n > 0 for n in bank.counts], dtype=torch.bool)
        vids = vid_base + torch.arange(len(bank.counts))
        runs = self._group_runs(grp_off, Q.shape[0], max_len, bad)
        keys = torch.full((len(runs), len(bank.counts)), KEY_INF, dtype=torch.int64)
        for g, (j0, L) in enumerate(runs):
            if L > 0 and len(vids):
                kk = _pack_key(self._paragraph_score(best[j0:j0 + L]), vids)
                keys[g] = torch.where(live, kk, torch.full_like(kk, KEY_INF))
        if own_dist is not None:
            Ng = len(runs)
            real = torch.where(keys == KEY_INF, torch.full_like(keys, torch.iinfo(torch.int64).max), keys)    # never counted
            count = self._counts_below(real, _pack_key(own_dist.reshape(1, Ng), own_idx.reshape(1, Ng)), count)[0]
        return self._topk_lists(keys, k) + (count,)

    def score_paragraph_pairs(self, Q, bank, grp_off, max_len, pairs, vid_base=0, out_score=None, out_moments=None, moments=True,
                              bad=None):
        """Named (paragraph, global video) pairs (same semantics as ``_vfr.score_paragraph_pairs``): the paragraph score and, per
        sentence, the global id of the video's best moment; pairs of other shards are left untouched (+inf / -1 pre-filled)."""
        Q = Q.float()
        rows = [[int(x) for x in r] for r in torch.as_tensor(pairs).tolist()]
        Np, Nv = len(rows), len(bank.counts)
        if out_score is None:
            out_score = torch.full((Np,), float("inf"))
        if moments and out_moments is None:
            out_moments = torch.full((Np, int(max_len)), -1, dtype=torch.int64)
        runs = self._group_runs(grp_off, Q.shape[0], max_len, bad)
        bk = self._video_best_keys(Q, bank)
        bd, bi = _unpack_key(bk)
        for p, (g, gv) in enumerate(rows):
            lv = gv - vid_base
            if g < 0 or g >= len(runs):
                if bad is not None:
                    bad.fill_(1)
                continue
            if lv < 0 or lv >= Nv:
                continue
            j0, L = runs[g]
            ranked = L > 0 and bank.counts[lv] > 0
            out_score[p] = self._paragraph_score(bd[j0:j0 + L, lv:lv + 1])[0] if ranked else float("inf")
            if out_moments is not None:
                out_moments[p] = -1
                if ranked:
                    out_moments[p, :L] = bi[j0:j0 + L, lv]
        return out_score, out_moments

    def topk_merge(self, part_dist, part_idx):
        return self.merge_keys(self.pack_keys(part_dist, part_idx))[:2]

    def pack_keys(self, dist_t, idx_t, out=None):
        keys = torch.where(idx_t >= 0, _pack_key(dist_t, idx_t.clamp(min=0)), torch.full_like(idx_t, KEY_INF))
        if out is not None:
            out.copy_(keys)
            return out
        return keys

    def merge_keys(self, part_keys, want_lists=True, want_keys=False):
        G, Nq, k = part_keys.shape
        srt = part_keys.clamp(max=KEY_INF).permute(1, 0, 2).reshape(Nq, G * k).sort(dim=1).values[:, :k].contiguous()
        return (self._lists_of(srt) if want_lists else (None, None)) + ((srt if want_keys else None),)

    def gt_labels(self, packed_times, n_own, thresholds, strict, device, Mmax=None):
        return torch.from_numpy(gt_label_table(packed_times, np.asarray(n_own), thresholds, strict))

    def gt_best_keys(self, own_scores, labels, id_base, sel, Nq):
        R = labels.shape[0]
        M = min(own_scores.shape[1], labels.shape[2])
        ids = id_base[:, None] + torch.arange(M)[None, :]
        k = _pack_key(own_scores[:, :M].contiguous(), ids)
        k = torch.where(labels[:, :, :M].bool(), k[None], torch.full_like(k, KEY_INF)[None])
        keys = torch.full((R, Nq), KEY_INF, dtype=torch.int64)
        keys[:, sel] = k.min(dim=2).values.clamp(max=KEY_INF)
        return keys


def ops_for(device):
    """Provider by DEVICE: a ROCm device gets the HIP kernels (and raises if they are unavailable)."""
    return HipOps() if torch.device(device).type == "cuda" else TorchCpuOps()
