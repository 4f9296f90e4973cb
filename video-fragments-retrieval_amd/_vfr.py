"""ctypes binding of ``lib/libvfr.so`` (C ABI: ``include/vfr.h``) for torch tensors on a ROCm device.

PyTorch is plumbing here: it owns device memory and the stream; every kernel is ours.  Wrappers take
``torch`` CUDA(=HIP) tensors, pass ``data_ptr()`` / sizes / ``torch.cuda.current_stream().cuda_stream``
and raise ``RuntimeError`` with ``vfr_last_error()`` on a non-zero return.  There is NO fallback: if the
shared library is missing or a tensor is not on the GPU these functions raise.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import torch

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["VFR_LIB"]).resolve() if os.environ.get("VFR_LIB") else _PKG / "lib" / "libvfr.so"   # VFR_LIB: A/B another build
_lib = None

_vp, _i32, _i64, _f32, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t

# name -> (restype, argtypes); must list every symbol include/vfr.h declares (checked by tests)
SIGNATURES = {
    "vfr_version": (_i32, []),
    "vfr_last_error": (ctypes.c_char_p, []),
    "vfr_set_option": (_i32, [ctypes.c_char_p, _i32]),
    "vfr_get_option": (_i32, [ctypes.c_char_p]),
    "vfr_set_fault_word": (_i32, [_vp]),
    "vfr_poll_faults": (_i32, []),
    "vfr_profile_sites": (_i32, []),
    "vfr_profile_site_name": (ctypes.c_char_p, [_i32]),
    "vfr_profile_read": (_i32, [_i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), _i32]),
    "vfr_math_f32": (_i32, [_i32, _vp, _vp, _vp, _i64, _vp]),
    "vfr_segment_pool_norm_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vfr_segment_pool_norm_batch_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vfr_visual_mlp_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "vfr_visual_mlp_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vfr_linear_f32": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "vfr_bilstm_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "vfr_bilstm_debug_offset": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "vfr_lstm_plan": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vfr_bilstm_final_f32": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp] + [_vp] * 8 + [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "vfr_score_moments_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _f32, _vp, _vp]),
    "vfr_score_own_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp]),
    "vfr_score_topk_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vfr_score_topk_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _vp, _vp, _i32,
                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_topk_mfma_prefilter": (_i32, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "vfr_score_topk_mfma_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "vfr_score_topk_mfma": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _vp, _vp, _i32,
                                   _vp, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "vfr_score_topk_mfma_stats": (_i32, [_vp, _i64, _i32, _i32, _i32, ctypes.POINTER(ctypes.c_int64), _vp]),
    "vfr_score_video_topk_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "vfr_score_video_topk_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _vp, _vp,
                                        _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "vfr_score_video_topk_stats": (_i32, [_vp, _i64, _i32, _i32, ctypes.POINTER(ctypes.c_int64), _vp]),
    "vfr_score_moment_nms_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "vfr_score_moment_nms_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _i32,
                                        ctypes.c_double, _vp, _vp, _i32, _vp, _sz, _vp]),
    "vfr_nms_inter_table": (_i32, [ctypes.c_double, _i32, ctypes.POINTER(ctypes.c_int32)]),
    "vfr_score_subset_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i32]),
    "vfr_score_subset_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i64, _vp, _vp, _i64, _i64,
                                    _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_sentences_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "vfr_score_sentences_f32": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i32,
                                       _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_video_sentences_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "vfr_score_video_sentences_f32": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _i64, _i64, _i32, _vp, _vp,
                                             _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_paragraphs_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "vfr_score_paragraphs_f32": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _vp, _vp,
                                        _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "vfr_score_paragraph_pairs_f32": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i64,
                                             _vp, _i64, _vp, _vp, _vp, _vp]),
    "vfr_score_paragraphs_stats": (_i32, [_vp, _i64, _i64, _i32, _i32, ctypes.POINTER(ctypes.c_int64), _vp]),
    "vfr_score_spans_f32": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i64, _vp, _i64, _vp, _vp, _vp]),
    "vfr_mine_negatives_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vfr_mine_negatives_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i64, _i64, _vp, _i64, _i32, _i32, _vp, _i32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_fusion_own_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp]),
    "vfr_score_fusion_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vfr_score_fusion_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _i32, _vp, _vp,
                                    _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_fusion_sweep_own_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp]),
    "vfr_score_fusion_sweep_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _f32, _i64, _i32, _i32,
                                          _vp, _vp, _vp, _vp]),
    "vfr_score_prior_own_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "vfr_score_prior_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vfr_score_prior_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _i32, _vp, _vp, _i32,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_score_window_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vfr_score_window_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp,
                                    _vp, _vp, _sz, _vp]),
    "vfr_score_window_span_keys_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "vfr_mfma_selfcheck": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "vfr_mfma_selfcheck_i8": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "vfr_score_i8_debug": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _f32, _vp, ctypes.c_size_t] + [_vp] * 11),
    "vfr_topk_merge_f32": (_i32, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp]),
    "vfr_topk_pack_keys": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "vfr_topk_merge_keys": (_i32, [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "vfr_topk_merge_keys_strided": (_i32, [_vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "vfr_gt_best_keys_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "vfr_gt_rank_keys_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vfr_gt_labels_u8": (_i32, [_vp, _vp, _vp, _i64, _i32, ctypes.POINTER(ctypes.c_double), _i32, _i32, _i32, _vp, _vp]),
    "vfr_ranking_loss_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "vfr_ranking_loss_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _sz, _vp]),
    "vfr_ranking_loss_grad_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp]),
    "vfr_transpose_f32": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "vfr_colsum_f32": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "vfr_relu_backward_f32": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "vfr_lstm_cell_forward_f32": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "vfr_lstm_cell_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "vfr_bilstm_train_forward_f32": (_i32, [_vp, _i64, _i32, _i32, _i32] + [_vp] * 8 + [_vp, _vp, _vp, _vp]),
    "vfr_bilstm_train_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "vfr_bilstm_train_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vfr_triplet_gather_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp]),
    "vfr_adam_workspace_bytes": (_sz, [_vp, _i32]),
    "vfr_adam_step_f32": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_grad_sumsq_f32": (_i32, [_i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vfr_frames_normalize_f32": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "vfr_conv3x3_relu_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "vfr_maxpool2_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vfr_adaptive_avgpool7_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vfr_vgg_fc7_workspace_bytes": (_sz, [_i32, _i32, _i32, _vp, _i32, _i32]),
    "vfr_resnet_pool_workspace_bytes": (_sz, [_i32, _i32, _i32, _vp, _i32]),
    "vfr_resnet_pool_f32": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    "vfr_resnet_folded_bytes": (_sz, [_vp, _i32]),
    "vfr_resnet_fold_f32": (_i32, [_vp, _i32, _vp, _vp, _f32, _vp, _sz, _vp]),
    "vfr_resnet_pool_folded_f32": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "vfr_vgg_fc7_f32": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
}


def build(force: bool = False) -> Path:
    """Compile the HIP sources for gfx950 (``make`` drives hipcc; cross-compiles without a GPU)."""
    cmd = ["make", "-C", str(_PKG / "csrc"), "-j8"] + (["-B"] if force else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libvfr.so build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no fallback path for the HIP kernels)")
        l = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().vfr_last_error().decode()}")


def _dev(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the ROCm device (no CPU fallback in the HIP path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _workspace(workspace, nbytes: int, device) -> torch.Tensor:
    """The caller's workspace when it is large enough (the SAME object: the ``_vfr_bank`` claim lives on it), else a new one."""
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)
    return workspace


def _out_lists(n: int, k: int, device):
    """(dist fp32 [n, k], idx int64 [n, k]) to be filled by a kernel; (None, None) for k == 0."""
    if k == 0:
        return None, None
    return torch.empty((n, k), dtype=torch.float32, device=device), torch.empty((n, k), dtype=torch.int64, device=device)


def _rank_keys(rank_dist, rank_idx, count_lt, n: int, device, what=("rank_dist", "rank_idx", "count_lt")):
    """Rank keys [R, n] (or [n]) of a scoring wrapper -> (rank_dist [R, n], rank_idx [R, n], count_lt, R): ``count_lt`` is
    allocated zeroed [R, n] when None, else checked and ADDED to by the kernel.  No keys: R == 0, nothing is touched."""
    if rank_dist is None:
        return rank_dist, rank_idx, count_lt, 0
    rank_dist = _dev(rank_dist, torch.float32, what[0]).reshape(-1, n)
    rank_idx = _dev(rank_idx, torch.int64, what[1]).reshape(-1, n)
    R = rank_dist.shape[0]
    if count_lt is None:
        count_lt = torch.zeros((R, n), dtype=torch.int64, device=device)
    return rank_dist, rank_idx, _dev(count_lt, torch.int64, what[2]), R


def csr_offsets(counts):
    """Host clip counts per video -> (clip offsets, moment offsets), int64 [Nv + 1] each (a video of n clips has n (n + 1) / 2
    moments)."""
    counts = np.asarray(counts, np.int64)
    return np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])


def set_option(name: str, value: int) -> None:
    _check(lib().vfr_set_option(name.encode(), int(value)), "vfr_set_option")


def get_option(name: str) -> int:
    return int(lib().vfr_get_option(name.encode()))


FAULT_SEQ_RESCUED = 1                      # include/vfr.h VFR_FAULT_SEQ_RESCUED
_FAULT_WORD = None                         # page-locked int32 word the kernels raise fault bits in (registered once per process)
FAULT_LOG = []                             # (bits, message) of every fault poll_faults() has reported


def _register_fault_word() -> None:
    """Give the library its fault word (include/vfr.h vfr_set_fault_word): device-side recoveries -- a single-launch sequence
    encoder that gave up and was re-encoded by the rescue kernel -- are reported through it, lazily, by ``poll_faults``."""
    global _FAULT_WORD
    if _FAULT_WORD is None:
        word = torch.zeros(1, dtype=torch.int32).pin_memory()
        _check(lib().vfr_set_fault_word(word.data_ptr()), "vfr_set_fault_word")
        _FAULT_WORD = word


def poll_faults() -> int:
    """Fault bits raised on the device since the last poll (0: none).  Host-only, never synchronises: call it after a point
    where the work of interest has completed (``.cpu()`` / ``.item()`` / ``torch.cuda.synchronize()``); the wrappers of the
    entry points that can raise a fault also poll on entry, so a fault is reported at the latest by the next such call.
    Every reported fault is a ``RuntimeWarning`` carrying ``vfr_last_error()`` and an entry of ``FAULT_LOG`` -- the results
    of the affected call were REPAIRED on the device (include/vfr.h), nothing needs re-running."""
    if _FAULT_WORD is None:
        return 0
    bits = int(lib().vfr_poll_faults())
    if bits:
        import warnings
        msg = lib().vfr_last_error().decode()
        FAULT_LOG.append((bits, msg))
        warnings.warn(f"vfr: device-side recovery (fault bits {bits:#x}): {msg}", RuntimeWarning, stacklevel=2)
    return bits


def profile_read(reset: bool = True) -> dict:
    """{site name: (total device ms, launches)} since the last reset.  Synchronise the device first."""
    l = lib()
    out = {}
    n = l.vfr_profile_sites()
    for site in range(1, n):
        ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
        _check(l.vfr_profile_read(site, ctypes.byref(ms), ctypes.byref(cnt), 0), "vfr_profile_read")
        if cnt.value:
            out[l.vfr_profile_site_name(site).decode()] = (ms.value, cnt.value)
    if reset:
        _check(l.vfr_profile_read(1, None, None, 1), "vfr_profile_read")
    return out


# ------------------------------------------------------------------------------------------------
def math_f32(op: int, x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    y = _dev(y, torch.float32, "y") if y is not None else None
    out = torch.empty_like(x)
    _check(lib().vfr_math_f32(op, x.data_ptr(), _ptr(y), out.data_ptr(), x.numel(), _stream()), "vfr_math_f32")
    return out


def segment_pool_norm(frames: torch.Tensor, seg_len: int = 25, mode: str = "avg"):
    """[T,F] fc7 frames -> (seg [ceil(T/seg_len),F], ctx [F])  (model/data.py:163-181)."""
    frames = _dev(frames, torch.float32, "frames")
    T, F = frames.shape
    nseg = (T + seg_len - 1) // seg_len
    seg = torch.empty((nseg, F), dtype=torch.float32, device=frames.device)
    ctx = torch.empty((F,), dtype=torch.float32, device=frames.device)
    _check(lib().vfr_segment_pool_norm_f32(frames.data_ptr(), T, F, seg_len, 0 if mode == "avg" else 1,
                                           seg.data_ptr(), ctx.data_ptr(), _stream()), "vfr_segment_pool_norm_f32")
    return seg, ctx


def segment_pool_norm_batch(frames: torch.Tensor, frame_counts, seg_len: int = 25, mode: str = "avg"):
    """frames [sum T, F] for many videos, frame_counts = list of T_v -> (seg [sum n,F], ctx [Nv,F], clip_counts)."""
    frames = _dev(frames, torch.float32, "frames")
    F = frames.shape[1]
    counts = torch.as_tensor(list(frame_counts), dtype=torch.int64)
    nseg = (counts + seg_len - 1) // seg_len
    foff = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32).to(frames.device)
    soff = torch.cat([torch.zeros(1, dtype=torch.int64), nseg.cumsum(0)]).to(torch.int32).to(frames.device)
    total = int(nseg.sum())
    Nv = len(counts)
    seg = torch.empty((total, F), dtype=torch.float32, device=frames.device)
    ctx = torch.empty((Nv, F), dtype=torch.float32, device=frames.device)
    _check(lib().vfr_segment_pool_norm_batch_f32(frames.data_ptr(), foff.data_ptr(), soff.data_ptr(), Nv, total, F,
                                                 seg_len, 0 if mode == "avg" else 1, seg.data_ptr(), ctx.data_ptr(),
                                                 _stream()), "vfr_segment_pool_norm_batch_f32")
    return seg, ctx, nseg.to(torch.int32)


def visual_mlp(seg, ctx, clip_off, W1, b1, W2, b2) -> torch.Tensor:
    seg, ctx = _dev(seg, torch.float32, "seg"), _dev(ctx, torch.float32, "ctx")
    W1, b1, W2, b2 = (_dev(t, torch.float32, n) for t, n in ((W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2")))
    clip_off = _dev(clip_off, torch.int32, "clip_off")
    C, F = seg.shape
    Nv, hid, D = ctx.shape[0], W1.shape[0], W2.shape[0]
    if W1.shape[1] != 2 * F + 2 or clip_off.numel() != Nv + 1 or W2.shape[1] != hid:
        raise RuntimeError("visual_mlp: inconsistent shapes")
    out = torch.empty((C, D), dtype=torch.float32, device=seg.device)
    ws_bytes = lib().vfr_visual_mlp_workspace_bytes(C, Nv, F, hid)
    ws = _workspace(None, ws_bytes, seg.device)
    _check(lib().vfr_visual_mlp_f32(seg.data_ptr(), ctx.data_ptr(), clip_off.data_ptr(), Nv, C, F, W1.data_ptr(),
                                    b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), hid, D, out.data_ptr(), ws.data_ptr(),
                                    ws_bytes, _stream()), "vfr_visual_mlp_f32")
    return out


def linear(A, W, b=None, relu: bool = False) -> torch.Tensor:
    A, W = _dev(A, torch.float32, "A"), _dev(W, torch.float32, "W")
    b = _dev(b, torch.float32, "b") if b is not None else None
    out = torch.empty((A.shape[0], W.shape[0]), dtype=torch.float32, device=A.device)
    _check(lib().vfr_linear_f32(A.data_ptr(), A.shape[0], A.shape[1], W.data_ptr(), _ptr(b), W.shape[0], int(relu),
                                out.data_ptr(), _stream()), "vfr_linear_f32")
    return out


_LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def bilstm_final(tokens, emb, lstm: dict, Wfc, bfc, len_tab=None, workspace=None) -> torch.Tensor:
    """tokens int64 [B,T] -> query embeddings [B,D]  (model/models.py:61-66).  ``workspace``: a uint8 device tensor to run
    in when it is large enough (tests read the debug counters out of it: ``lstm_issued_blocks``)."""
    tokens = _dev(tokens, torch.int64, "tokens")
    emb = _dev(emb, torch.float32, "emb")
    ws_ = [_dev(lstm[n], torch.float32, n) for n in _LSTM_NAMES] + \
          [_dev(lstm[n + "_reverse"], torch.float32, n + "_reverse") for n in _LSTM_NAMES]
    Wfc, bfc = _dev(Wfc, torch.float32, "Wfc"), _dev(bfc, torch.float32, "bfc")
    lt = _dev(len_tab, torch.float32, "len_tab") if len_tab is not None else None
    B, T = tokens.shape
    E, H, D = emb.shape[1], ws_[1].shape[1], Wfc.shape[0]
    _register_fault_word()
    poll_faults()                              # (a give-up of an EARLIER call's sequence kernel: repaired there, reported here)
    out = torch.empty((B, D), dtype=torch.float32, device=tokens.device)
    nbytes = lib().vfr_bilstm_workspace_bytes(B, T, E, H, emb.shape[0])
    ws = _workspace(workspace, nbytes, tokens.device)
    _check(lib().vfr_bilstm_final_f32(tokens.data_ptr(), B, T, emb.data_ptr(), emb.shape[0], _ptr(lt),
                                      *[w.data_ptr() for w in ws_], E, H, Wfc.data_ptr(), bfc.data_ptr(), D,
                                      out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "vfr_bilstm_final_f32")
    return out


def bilstm_workspace(B: int, T: int, E: int, H: int, vocab: int, device) -> torch.Tensor:
    """A workspace for ``bilstm_final(..., workspace=)`` at this shape."""
    return torch.empty((max(lib().vfr_bilstm_workspace_bytes(B, T, E, H, vocab), 1),), dtype=torch.uint8, device=device)


def lstm_plan(rows: int, H: int, T: int, cus: int):
    """(one_launch, tile, slots) of the fused BiLSTM steps under the current options (include/vfr.h vfr_lstm_plan; host only)."""
    one, tile, slots = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    _check(lib().vfr_lstm_plan(rows, H, T, cus, ctypes.addressof(one), ctypes.addressof(tile), ctypes.addressof(slots)), "vfr_lstm_plan")
    return bool(one.value), tile.value, slots.value


def lstm_issued_blocks(workspace: torch.Tensor, B: int, T: int, E: int, H: int, vocab: int):
    """(forward, reverse) counts of (16-row x 16-unit) MFMA blocks the fused LSTM steps of the last ``bilstm_final`` in
    ``workspace`` issued (option ``lstm_live_blocks`` bit 1; include/vfr.h vfr_bilstm_debug_offset).  Synchronises."""
    off = lib().vfr_bilstm_debug_offset(B, T, E, H, vocab)
    f, r = workspace[off:off + 8].view(torch.int32).cpu().tolist()
    return f, r


def moment_offsets(clip_off: torch.Tensor) -> torch.Tensor:
    n = (clip_off[1:] - clip_off[:-1]).to(torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=clip_off.device), (n * (n + 1) // 2).cumsum(0)])


class VideoBank:
    """Clip embeddings of a (shard of a) corpus resident in HBM, with the CSR offsets the kernels take.

    ``emb`` [sum n, D] fp32, ``clip_off`` [Nv+1] int32, ``mom_off`` [Nv+1] int64 (all on the device);
    ``max_clips`` / ``total_moments`` are host ints computed once at construction (one D2H of two scalars).
    """

    def __init__(self, emb: torch.Tensor, clip_off: torch.Tensor, id_base: int = 0, max_clips: int | None = None,
                 total_moments: int | None = None, min_clips: int | None = None, mom_off: torch.Tensor | None = None):
        self.emb = _dev(emb, torch.float32, "emb")
        self.clip_off = _dev(clip_off, torch.int32, "clip_off")
        self.mom_off = moment_offsets(self.clip_off) if mom_off is None else _dev(mom_off, torch.int64, "mom_off")
        self.num_videos = int(self.clip_off.numel() - 1)
        if max_clips is None or total_moments is None or min_clips is None:   # scalar D2H reads, skipped when the host knows
            n = self.clip_off[1:] - self.clip_off[:-1]
            max_clips = int(n.max()) if self.num_videos else 0
            min_clips = int(n.min()) if self.num_videos else 0
            total_moments = int(self.mom_off[-1])
        self.max_clips, self.min_clips, self.total_moments = int(max_clips), int(min_clips), int(total_moments)
        self.total_clips = int(self.emb.shape[0])
        self.id_base = int(id_base)
        self.dim = int(self.emb.shape[1])
        self.serial = next(VideoBank._counter)   # identity of this bank object for the workspace-side cache (score_topk); atomic under the GIL

    _counter = itertools.count(1)

    def invalidate(self) -> None:
        """Forget every workspace-side product computed for this bank (call after writing ``emb`` / ``clip_off`` through
        anything torch does not version: ``.data``, DLPack / numpy views, a raw-pointer kernel).  Not needed for
        correctness -- the library hashes the bank on the device before it reuses anything (include/vfr.h,
        VFR_MFMA_BANK_READY) -- but it saves that call the hash + compare."""
        self.serial = next(VideoBank._counter)

    def prep_token(self, dtype: int, eps: float = 1e-6):
        """When the host may CLAIM the bank-side products of the MFMA pre-filter as reusable: this object, no torch-versioned
        in-place edit of its tensors since, the base dtype, the same eps.  The claim is verified on the device."""
        return (self.serial, self.emb.data_ptr(), self.emb._version, self.clip_off.data_ptr(), self.clip_off._version,
                self.num_videos, self.total_clips, int(dtype), float(eps))


def slice_bank(bank: VideoBank, counts, v0: int, v1: int) -> VideoBank:
    """Videos [v0, v1) of ``bank`` as a bank of their own (``counts`` = host clip counts of ``bank``'s videos)."""
    off, mom = csr_offsets(counts)
    sub = np.asarray(counts, np.int64)[v0:v1]
    clip_off = bank.clip_off[v0:v1 + 1] if v0 == 0 else bank.clip_off[v0:v1 + 1] - bank.clip_off[v0]   # on the device
    mom_off = bank.mom_off[v0:v1 + 1] if v0 == 0 else bank.mom_off[v0:v1 + 1] - bank.mom_off[v0]
    return VideoBank(bank.emb[int(off[v0]):int(off[v1])], clip_off.contiguous(), bank.id_base + int(mom[v0]),
                     max_clips=int(sub.max()) if len(sub) else 0, total_moments=int(mom[v1] - mom[v0]),
                     min_clips=int(sub.min()) if len(sub) else 0, mom_off=mom_off.contiguous())


def score_moments(Q: torch.Tensor, bank: VideoBank, eps: float = 1e-6) -> torch.Tensor:
    Q = _dev(Q, torch.float32, "Q")
    out = torch.empty((Q.shape[0], bank.total_moments), dtype=torch.float32, device=Q.device)
    _check(lib().vfr_score_moments_f32(Q.data_ptr(), Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                       bank.mom_off.data_ptr(), bank.num_videos, bank.max_clips, bank.total_moments,
                                       bank.dim, eps, out.data_ptr(), _stream()), "vfr_score_moments_f32")
    return out


def score_own(Q: torch.Tensor, bank: VideoBank, own: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    Q = _dev(Q, torch.float32, "Q")
    own = _dev(own, torch.int32, "own")
    Mmax = bank.max_clips * (bank.max_clips + 1) // 2
    out = torch.empty((Q.shape[0], Mmax), dtype=torch.float32, device=Q.device)
    _check(lib().vfr_score_own_f32(Q.data_ptr(), Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                   own.data_ptr(), bank.max_clips, bank.dim, eps, Mmax, out.data_ptr(), _stream()),
           "vfr_score_own_f32")
    return out


# scoring mode of score_topk: "mfma" = fp32 MFMA pre-filter + exact re-scoring (bit-identical to "exact", the default),
# "exact" = the exact VALU kernels only, "bf16" = bf16 MFMA operands, approximate
SCORE_MODES = {"exact": None, "mfma": 0, "bf16": 1}
MFMA_BANK_READY = 0x100                    # include/vfr.h VFR_MFMA_BANK_READY
DEFAULT_SCORE_MODE = os.environ.get("VFR_SCORE_MODE", "mfma")


_MFMA_CHECKED = {}                         # device index -> bool, one self-check per process and device


def mfma_selfcheck(device=None, reversed_reference: bool = False) -> int:
    """Number of elements (of 256) on which the matrix pipe's 16x16xK product differs from an explicit k-ascending fmaf chain
    (include/vfr.h vfr_mfma_selfcheck) on adversarial rows: exponents spread over 2^-40 .. 2^40, every second product the
    near-negation of its neighbour (cancellation), denormal operands.  0 on a conforming device.  SYNCHRONISES."""
    device = torch.device(device if device is not None else "cuda")
    rs = np.random.RandomState(2024)
    K = 100

    def rows():
        m = rs.uniform(1.0, 2.0, (16, K)) * np.exp2(rs.randint(-40, 41, (16, K))) * rs.choice([-1.0, 1.0], (16, K))
        m[:, 7::13] = 1e-41 * rs.randint(1, 9, m[:, 7::13].shape)          # denormal operands
        return m.astype(np.float32)
    A, B = rows(), rows()
    A[:, 1::2] = -A[:, 0::2] * (1.0 + np.float32(2.0 ** -20))               # a_{2j+1} b_{2j+1} ~ -(a_2j b_2j): cancellation
    B[:, 1::2] = B[:, 0::2]
    a, b = torch.from_numpy(A).to(device), torch.from_numpy(B).to(device)
    mis = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(lib().vfr_mfma_selfcheck(a.data_ptr(), b.data_ptr(), K, 1 if reversed_reference else 0, mis.data_ptr(), _stream()),
               "vfr_mfma_selfcheck")
    return int(mis.item())


def mfma_selfcheck_i8(device=None, permuted_reference: bool = False) -> int:
    """The int8 arm (include/vfr.h vfr_mfma_selfcheck_i8): elements (of 256) on which the matrix pipe's 16x16x128 int8 product
    differs from integer dot products on the vector ALU, on asymmetric data that reaches -128 and 127.  0 on a conforming
    device; ``permuted_reference`` compares with the transposed product (what a failing check looks like).  SYNCHRONISES."""
    device = torch.device(device if device is not None else "cuda")
    rs = np.random.RandomState(2025)
    A = rs.randint(-128, 128, (16, 128)).astype(np.int8)
    B = rs.randint(-128, 128, (16, 128)).astype(np.int8)
    A[:, 0], A[:, 1], B[:, 0], B[:, 1] = -128, 127, 127, -128
    B[:, 64:] //= 2                                                         # the two k-steps, and the two operands, are not alike
    a, b = torch.from_numpy(A).to(device), torch.from_numpy(B).to(device)
    mis = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(lib().vfr_mfma_selfcheck_i8(a.data_ptr(), b.data_ptr(), 1 if permuted_reference else 0, mis.data_ptr(), _stream()),
               "vfr_mfma_selfcheck_i8")
    return int(mis.item())


def _mfma_mode_ok(device) -> bool:
    """The first "mfma" / "bf16" scoring call on a device runs the self-check; a device that fails it gets the exact kernels
    (and a warning) for the rest of the process: the pre-filter's margins assume the checked arithmetic.  A device that fails
    only the int8 arm keeps the pre-filter on its fp32 operands ("score_i8" 0: process-global, like every option)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ok = _MFMA_CHECKED.get(idx)
    if ok is None:
        ok = _MFMA_CHECKED[idx] = mfma_selfcheck(device) == 0
        if not ok:
            import warnings
            warnings.warn("vfr: the MFMA self-check failed on this device (v_mfma_f32_16x16x4_f32 is not a k-ascending fp32 fma "
                          "chain here); scoring falls back to the exact kernels")
        elif mfma_selfcheck_i8(device) != 0:
            import warnings
            set_option("score_i8", 0)
            warnings.warn("vfr: the int8 arm of the MFMA self-check failed on this device (v_mfma_i32_16x16x64_i8 does not have the "
                          "assumed lane map); the pre-filter runs on its fp32 operands")
    return ok


def score_i8_debug(Q: torch.Tensor, bank: "VideoBank", eps: float = 1e-6) -> dict:
    """TEST HOOK (include/vfr.h vfr_score_i8_debug): the products of the int8 operand mode's pre-passes and the ring values
    d~^2 - b_q of every (query, clip), as numpy arrays.  SYNCHRONISES."""
    Q = _dev(Q, torch.float32, "Q")
    Nq, C, dev = Q.shape[0], bank.total_clips, Q.device
    groups = (Nq + 63) // 64
    nbytes = lib().vfr_score_topk_mfma_workspace_bytes(Nq, bank.num_videos, C, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {"vlimbs": torch.zeros(C, 3, 128, dtype=torch.int8, device=dev), "qlimbs": torch.zeros(Nq, 3, 128, dtype=torch.int8, device=dev),
           "bank_const": torch.zeros(4, dtype=torch.float64, device=dev), "query_const": torch.zeros(Nq, 2, dtype=torch.float64, device=dev),
           "query_scale": torch.zeros(groups, dtype=torch.float64, device=dev), "query_factor": torch.zeros(groups, dtype=torch.float32, device=dev),
           "qmeta": torch.zeros(Nq, 4, dtype=torch.float32, device=dev), "va": torch.zeros(C, dtype=torch.float32, device=dev),
           "mu": torch.zeros(128, dtype=torch.float32, device=dev), "ring": torch.zeros(Nq, C, dtype=torch.float32, device=dev)}
    _check(lib().vfr_score_i8_debug(Q.data_ptr(), Nq, bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.num_videos, C, bank.dim, eps,
                                    ws.data_ptr(), nbytes, *[t.data_ptr() for t in out.values()], _stream()), "vfr_score_i8_debug")
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in out.items()}


def _bank_args(Q: torch.Tensor, bank: VideoBank, eps: float):
    """The leading arguments the bank-scoring entry points share (include/vfr.h): queries, the bank's CSR, eps, id base."""
    return (Q.data_ptr(), Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.mom_off.data_ptr(), bank.num_videos,
            bank.total_clips, bank.min_clips, bank.max_clips, bank.dim, eps, bank.id_base)


def score_topk(Q: torch.Tensor, bank: VideoBank, k: int, rank_dist=None, rank_idx=None, count_lt=None,
               eps: float = 1e-6, workspace: torch.Tensor | None = None, thr_seed: torch.Tensor | None = None,
               mode: str | None = None):
    """Fused scoring + top-k (+ rank counting for up to 4 keys per query).

    rank_dist / rank_idx: [R, Nq] (or [Nq]) -> count_lt [R, Nq] int64 is ADDED to (allocated zeroed when None).
    ``mode``: see SCORE_MODES (None = DEFAULT_SCORE_MODE).
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count_lt | None)."""
    mode = mode or DEFAULT_SCORE_MODE
    if mode not in SCORE_MODES:
        raise RuntimeError(f"score_topk: unknown mode {mode!r}")
    Q = _dev(Q, torch.float32, "Q")
    if mode != "exact" and not _mfma_mode_ok(Q.device):
        mode = "exact"
    Nq = Q.shape[0]
    od, oi = _out_lists(Nq, k, Q.device)
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nq, Q.device)
    if thr_seed is not None:
        thr_seed = _dev(thr_seed, torch.int64, "thr_seed")
    dtype = SCORE_MODES[mode]
    if dtype is None:
        nbytes = lib().vfr_score_topk_workspace_bytes(Nq, bank.num_videos, k)
    else:
        nbytes = lib().vfr_score_topk_mfma_workspace_bytes(Nq, bank.num_videos, bank.total_clips, k)
    workspace = _workspace(workspace, nbytes, Q.device)
    common = _bank_args(Q, bank, eps) + (k, _ptr(od), _ptr(oi), R, _ptr(rank_dist), _ptr(rank_idx), _ptr(count_lt), _ptr(thr_seed))
    if dtype is None:
        workspace._vfr_bank = None               # the exact kernels carve the workspace their own way
        _check(lib().vfr_score_topk_f32(*common, workspace.data_ptr(), nbytes, _stream()), "vfr_score_topk_f32")
    else:
        # the bank-side products of the pre-filter stay in the workspace: a later call on the SAME bank object (and untouched
        # tensors) with this workspace reuses them (VFR_MFMA_BANK_READY); anything else recomputes
        token = bank.prep_token(dtype, eps)
        ready = getattr(workspace, "_vfr_bank", None) == token
        pre = lib().vfr_score_topk_mfma_prefilter(Nq, bank.num_videos, bank.total_clips, bank.max_clips, bank.dim, R, k, dtype)
        workspace._vfr_bank = None
        _check(lib().vfr_score_topk_mfma(*common, dtype | (MFMA_BANK_READY if ready and pre else 0), workspace.data_ptr(), nbytes,
                                         _stream()), "vfr_score_topk_mfma")
        if pre:
            workspace._vfr_bank = token
    return od, oi, count_lt


VIDEO_EXACT = 2                            # include/vfr.h VFR_SCORE_EXACT


def _video_mode(mode, Q, who: str):
    """``mode`` of the video-level wrappers ("mfma" | "exact", None = DEFAULT_SCORE_MODE; a device that fails the MFMA
    self-check gets "exact") -> (the library's dtype word, the checked ``Q``)."""
    mode = mode or DEFAULT_SCORE_MODE
    if mode not in ("exact", "mfma"):
        raise RuntimeError(f"{who}: unsupported mode {mode!r} (exact, mfma)")
    Q = _dev(Q, torch.float32, "Q")
    if mode == "mfma" and not _mfma_mode_ok(Q.device):
        mode = "exact"
    return (VIDEO_EXACT if mode == "exact" else SCORE_MODES["mfma"]), Q


def _video_bank_ready(workspace: torch.Tensor, bank: VideoBank, dtype: int, eps: float):
    """Before a video-level call: (token, may the call CLAIM the bank-side products a previous call left in ``workspace``);
    the workspace's claim is dropped until ``_video_bank_claim`` renews it."""
    token = ("video",) + bank.prep_token(0, eps)
    ready = dtype == 0 and getattr(workspace, "_vfr_bank", None) == token
    workspace._vfr_bank = None
    return token, ready


def _video_bank_claim(workspace: torch.Tensor, token, bank: VideoBank, dtype: int, ran: bool = True) -> None:
    """After the call: when the MFMA fast path ran (``ran``: the call had work at all), its bank-side products are in the workspace."""
    if ran and dtype == 0 and bank.dim == 100 and bank.max_clips <= 21 and bank.num_videos >= max(1, get_option("score_mfma_min")):
        workspace._vfr_bank = token


def score_video_topk(Q: torch.Tensor, bank: VideoBank, k: int, own_dist=None, own_idx=None, count=None,
                     mode: str | None = None, workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Video-level retrieval (include/vfr.h vfr_score_video_topk_f32): the k best DISTINCT videos per query, each as
    (distance, global moment id) of its best moment, in (distance, id) order, padded with (+inf, -1); and, with
    ``own_dist`` / ``own_idx`` [Nq] (the best key of each query's own video), ``count`` [Nq] int64 += the number of this
    bank's videos whose best key sorts before it (allocated zeroed when None).  ``mode``: "mfma" (MFMA bounds + exact
    triangles where they cannot decide) or "exact"; None = DEFAULT_SCORE_MODE.  Both give the same bits.
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count | None)."""
    dtype, Q = _video_mode(mode, Q, "score_video_topk")
    Nq = Q.shape[0]
    od, oi = _out_lists(Nq, k, Q.device)
    own_dist, own_idx, cnt, R = _rank_keys(own_dist, own_idx, count, Nq, Q.device, ("own_dist", "own_idx", "count"))
    if R:                                    # ONE key per query, and the public count is [Nq]
        own_dist, own_idx = own_dist.reshape(Nq), own_idx.reshape(Nq)
        if count is None:
            cnt = cnt.reshape(Nq)
    nbytes = lib().vfr_score_video_topk_workspace_bytes(Nq, bank.num_videos, bank.total_clips, k)
    workspace = _workspace(workspace, nbytes, Q.device)
    token, ready = _video_bank_ready(workspace, bank, dtype, eps)
    _check(lib().vfr_score_video_topk_f32(*_bank_args(Q, bank, eps), k, _ptr(od), _ptr(oi), _ptr(own_dist), _ptr(own_idx), _ptr(cnt),
                                          dtype | (MFMA_BANK_READY if ready else 0), workspace.data_ptr(), nbytes, _stream()),
           "vfr_score_video_topk_f32")
    _video_bank_claim(workspace, token, bank, dtype)
    return od, oi, cnt


def score_moment_nms(Q: torch.Tensor, bank: VideoBank, k: int, per_video: int = 0, nms_iou: float = 1.0,
                     mode: str | None = None, workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Diversified moment retrieval (include/vfr.h vfr_score_moment_nms_f32): the k best moments per query in (distance,
    global id) order, where each video's moments are accepted greedily in that order, a moment whose IoU with an accepted
    moment of its video is > ``nms_iou`` is suppressed, and at most ``per_video`` are accepted (0 = no cap).  Padded with
    (+inf, -1).  ``per_video`` = 1 is ``score_video_topk``; no cap and ``nms_iou`` >= 1 is ``score_topk``.  ``mode``:
    "mfma" or "exact" (same bits); None = DEFAULT_SCORE_MODE.  Returns (dist [Nq,k], idx [Nq,k] int64)."""
    dtype, Q = _video_mode(mode, Q, "score_moment_nms")
    Nq = Q.shape[0]
    od, oi = _out_lists(Nq, k, Q.device)
    if k == 0:                               # this wrapper returns lists only, and never None
        od, oi = Q.new_empty((Nq, 0)), Q.new_empty((Nq, 0), dtype=torch.int64)
    nbytes = lib().vfr_score_moment_nms_workspace_bytes(Nq, bank.num_videos, bank.total_clips, k, int(per_video))
    workspace = _workspace(workspace, nbytes, Q.device)
    token, ready = _video_bank_ready(workspace, bank, dtype, eps)       # the workspace front is score_video_topk's
    _check(lib().vfr_score_moment_nms_f32(*_bank_args(Q, bank, eps), k, int(per_video), float(nms_iou), _ptr(od), _ptr(oi),
                                          dtype | (MFMA_BANK_READY if ready else 0), workspace.data_ptr(), nbytes, _stream()),
           "vfr_score_moment_nms_f32")
    _video_bank_claim(workspace, token, bank, dtype, ran=k > 0 and Nq > 0)
    return od, oi


SUBSET_LEVELS = {"moments": 0, "videos": 1}   # include/vfr.h VFR_SUBSET_MOMENTS / VFR_SUBSET_VIDEOS


def score_subset(Q: torch.Tensor, bank: VideoBank, cand_off: torch.Tensor, cand_vid: torch.Tensor, k: int, level: str = "moments",
                 vid_base: int = 0, rank_dist=None, rank_idx=None, count_lt=None, workspace: torch.Tensor | None = None,
                 bad: torch.Tensor | None = None, max_list: int | None = None, eps: float = 1e-6):
    """Candidate-restricted retrieval (include/vfr.h vfr_score_subset_f32): each query searches only the videos its list names.
    ``cand_off`` [Nq+1] int64 / ``cand_vid`` [nnz] int32 = CSR lists of corpus-global video indices, strictly ascending per query;
    ``vid_base`` = global index of the bank's first video (entries of other shards are skipped).  ``level`` "moments": the k best
    moments of the listed videos; "videos": the k best listed videos as (best distance, best moment id).  Padded with (+inf, -1).
    rank_dist / rank_idx [R, Nq] (or [Nq]), R <= 4: ``count_lt`` [R, Nq] int64 += the moments (videos) of the lists that sort
    before each rank key (allocated zeroed when None).  ``bad`` (device int32 [1], nullable) is set to 1 for a malformed list.
    ``max_list`` = the longest list (read from ``cand_off`` -- one synchronisation -- when None).
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count_lt | None)."""
    if level not in SUBSET_LEVELS:
        raise RuntimeError(f"score_subset: unknown level {level!r} (moments, videos)")
    Q = _dev(Q, torch.float32, "Q")
    Nq = Q.shape[0]
    cand_off = _dev(cand_off, torch.int64, "cand_off")
    cand_vid = _dev(cand_vid, torch.int32, "cand_vid")
    if cand_off.numel() != Nq + 1:
        raise RuntimeError(f"score_subset: cand_off has {cand_off.numel()} entries, expected Nq + 1 = {Nq + 1}")
    nnz = int(cand_vid.numel())
    if max_list is None:
        max_list = int((cand_off[1:] - cand_off[:-1]).max()) if Nq > 0 else 0
    od, oi = _out_lists(Nq, k, Q.device)
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nq, Q.device)
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    lv = SUBSET_LEVELS[level]
    nbytes = lib().vfr_score_subset_workspace_bytes(Nq, nnz, int(max_list), k, lv)
    workspace = _workspace(workspace, nbytes, Q.device)
    _check(lib().vfr_score_subset_f32(*_bank_args(Q, bank, eps), int(vid_base), cand_off.data_ptr(), _ptr(cand_vid) if nnz else 0, nnz,
                                      int(max_list), lv, k,
                                      _ptr(od), _ptr(oi), R, _ptr(rank_dist), _ptr(rank_idx), _ptr(count_lt), _ptr(bad),
                                      workspace.data_ptr(), nbytes, _stream()), "vfr_score_subset_f32")
    return od, oi, count_lt


FUSION_LEVELS = {"moments": 0, "videos": 1}   # include/vfr.h VFR_FUSION_MOMENTS / VFR_FUSION_VIDEOS
FUSION_MAX_STREAMS = 4                        # include/vfr.h VFR_FUSION_MAX_STREAMS


def fusion_weights(weights, S: int) -> np.ndarray:
    """The stream weights of a late fusion as fp32 [S]: one per stream, finite, >= 0 (ValueError otherwise).  Host only."""
    w = np.asarray(list(weights), dtype=np.float64).reshape(-1)
    if not 1 <= S <= FUSION_MAX_STREAMS:
        raise ValueError(f"late fusion takes 1 .. {FUSION_MAX_STREAMS} streams, got {S}")
    if len(w) != S:
        raise ValueError(f"late fusion: {len(w)} weights for {S} streams")
    w32 = w.astype(np.float32)
    if not (np.all(np.isfinite(w32)) and np.all(w32 >= 0)):
        raise ValueError(f"late fusion: weights must be finite and >= 0, got {w.tolist()}")
    return w32


def _same_clip_off(b: VideoBank, b0: VideoBank) -> bool:
    """Do two banks hold the same clip offsets?  Banks that own a tensor each are compared on the device ONCE (a host
    synchronisation); the answer is kept on ``b`` for as long as neither tensor is replaced or edited in place."""
    if b.clip_off.data_ptr() == b0.clip_off.data_ptr():
        return True
    token = (b0.clip_off.data_ptr(), b0.clip_off._version, b.clip_off.data_ptr(), b.clip_off._version)
    if getattr(b, "_fusion_same", None) != token:
        if not torch.equal(b.clip_off, b0.clip_off):
            return False
        b._fusion_same = token
    return True


def _fusion_streams(Qs, banks, weights, who: str):
    """The stream description both fusion entry points take: the checked tensors and the four host arrays (device pointers of the
    query matrices and clip banks, widths, weights).  The banks must describe the same videos on one device."""
    Qs, banks = list(Qs), list(banks)
    if len(Qs) != len(banks):
        raise ValueError(f"{who}: {len(Qs)} query matrices for {len(banks)} banks")
    w = fusion_weights(weights, len(banks))
    Qs = [_dev(Q, torch.float32, f"Qs[{s}]") for s, Q in enumerate(Qs)]
    b0 = banks[0]
    for s, (Q, b) in enumerate(zip(Qs, banks)):
        if Q.dim() != 2 or Q.shape[1] != b.dim or Q.shape[0] != Qs[0].shape[0]:
            raise ValueError(f"{who}: Qs[{s}] must be [{Qs[0].shape[0]}, {b.dim}], got {tuple(Q.shape)}")
        if Q.device != b.emb.device or b.emb.device != b0.emb.device:
            raise ValueError(f"{who}: stream {s} lives on another device")
        if b is not b0 and (b.id_base != b0.id_base or b.num_videos != b0.num_videos or b.total_clips != b0.total_clips or
                            not _same_clip_off(b, b0)):
            raise ValueError(f"{who}: bank {s} does not describe the videos of bank 0 (clip_off, id_base)")
    S = len(banks)
    hosts = ((ctypes.c_void_p * S)(*[Q.data_ptr() for Q in Qs]), (ctypes.c_void_p * S)(*[b.emb.data_ptr() for b in banks]),
             (ctypes.c_int * S)(*[b.dim for b in banks]), (ctypes.c_float * S)(*w.tolist()), S)
    return Qs, banks, hosts


def score_fusion_own(Qs, banks, weights, own: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """Late-fusion scores of each query against ONE video ``own[q]`` (include/vfr.h vfr_score_fusion_own_f32): [Nq, Mmax] fused
    moment scores in ``utils.generate_moments`` order, tail +inf -- the layout of ``score_own``, so ``gt_best_keys`` /
    ``gt_rank_keys`` take it.  ``Qs`` / ``banks`` / ``weights``: one query matrix [Nq, D_s], one ``VideoBank`` of the same videos
    and one weight (finite, >= 0) per stream."""
    Qs, banks, hosts = _fusion_streams(Qs, banks, weights, "score_fusion_own")
    b0 = banks[0]
    own = _dev(own, torch.int32, "own")
    Nq = Qs[0].shape[0]
    if own.numel() != Nq:
        raise ValueError(f"score_fusion_own: {own.numel()} own videos for {Nq} queries")
    Mmax = b0.max_clips * (b0.max_clips + 1) // 2
    out = torch.empty((Nq, Mmax), dtype=torch.float32, device=Qs[0].device)
    _check(lib().vfr_score_fusion_own_f32(*hosts, Nq, b0.clip_off.data_ptr(), _ptr(own) if Nq else 0, b0.num_videos, b0.max_clips, eps,
                                          Mmax, out.data_ptr() if out.numel() else 0, _stream()), "vfr_score_fusion_own_f32")
    return out


def score_fusion(Qs, banks, weights, k: int, level: str = "moments", rank_dist=None, rank_idx=None, count_lt=None,
                 workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Late-fusion retrieval (include/vfr.h vfr_score_fusion_f32): moments ranked by the weighted sum over S <= 4 streams.  ``Qs``:
    one query matrix [Nq, D_s] per stream; ``banks``: one ``VideoBank`` per stream over the SAME videos (equal device, ``clip_off``
    and ``id_base``, else ValueError); ``weights``: one finite weight >= 0 per stream.  The fused clip distance is
    fl(.. fl(fl(w_0 d_0) + fl(w_1 d_1)) ..) and the moment chain runs on it.  ``level`` "moments": the k best moments; "videos":
    the k best videos as (best fused score, best moment id).  Padded with (+inf, -1).  rank_dist / rank_idx [R, Nq] (or [Nq]),
    R <= 4: ``count_lt`` [R, Nq] int64 += the moments (videos) that sort before each rank key (allocated zeroed when None).
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count_lt | None)."""
    if level not in FUSION_LEVELS:
        raise ValueError(f"score_fusion: unknown level {level!r} (moments, videos)")
    Qs, banks, hosts = _fusion_streams(Qs, banks, weights, "score_fusion")
    b0 = banks[0]
    Nq, dev = Qs[0].shape[0], Qs[0].device
    od, oi = _out_lists(Nq, k, dev)
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nq, dev)
    nbytes = lib().vfr_score_fusion_workspace_bytes(Nq, b0.num_videos, k)
    workspace = _workspace(workspace, nbytes, dev)
    workspace._vfr_bank = None                   # whatever a pre-filter left in this workspace is overwritten
    _check(lib().vfr_score_fusion_f32(*hosts, Nq, b0.clip_off.data_ptr(), b0.mom_off.data_ptr(), b0.num_videos, b0.total_clips,
                                      b0.min_clips, b0.max_clips, eps, b0.id_base, FUSION_LEVELS[level], k, _ptr(od), _ptr(oi), R,
                                      _ptr(rank_dist), _ptr(rank_idx), _ptr(count_lt), workspace.data_ptr(), nbytes, _stream()),
           "vfr_score_fusion_f32")
    return od, oi, count_lt


def table_offsets(max_clips: int) -> np.ndarray:
    """int32 [max_clips + 2]: where the row of n-clip videos starts in a moment table (prefix sums of n (n + 1) / 2; the last entry is
    the number of entries).  Host only."""
    n = np.arange(max_clips + 1, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(n * (n + 1) // 2)]).astype(np.int32)


def _prior_table(table, bank: VideoBank, device, who: str):
    """The device arrays of a moment table (``engine.MomentTable``: ``max_clips``, ``table_off`` int32, ``table`` fp32), checked
    against the bank.  A table built for longer videos serves a bank of shorter ones: its rows are a prefix."""
    if table.max_clips < bank.max_clips:
        raise ValueError(f"{who}: the moment table covers videos of up to {table.max_clips} clips, the bank has {bank.max_clips}")
    off, val = _dev(table.table_off, torch.int32, "table_off"), _dev(table.table, torch.float32, "table")
    if off.device != device or val.device != device:
        raise ValueError(f"{who}: the moment table lives on {val.device}, the queries on {device}")
    n = table.max_clips
    if off.numel() != n + 2 or val.numel() != n * (n + 1) * (n + 2) // 6:
        raise ValueError(f"{who}: a moment table of {n} clips has {n + 2} offsets and {n * (n + 1) * (n + 2) // 6} entries, got "
                         f"{off.numel()} and {val.numel()}")
    return off, val


def score_prior_own(Q: torch.Tensor, bank: VideoBank, table, own: torch.Tensor, bad: torch.Tensor | None = None,
                    eps: float = 1e-6) -> torch.Tensor:
    """Biased scores of each query against ONE video ``own[q]`` (include/vfr.h vfr_score_prior_own_f32): [Nq, Mmax] =
    fl(score + table entry) in ``utils.generate_moments`` order, +inf at excluded moments and in the tail -- the layout of
    ``score_own``, so ``gt_best_keys`` / ``gt_rank_keys`` take it.  ``table``: an ``engine.MomentTable`` on the device; ``bad``
    (int32 [1], optional) is set to 1 by an entry that is NaN or < 0."""
    Q = _dev(Q, torch.float32, "Q")
    own = _dev(own, torch.int32, "own")
    Nq = Q.shape[0]
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise ValueError(f"score_prior_own: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    if own.numel() != Nq:
        raise ValueError(f"score_prior_own: {own.numel()} own videos for {Nq} queries")
    off, val = _prior_table(table, bank, Q.device, "score_prior_own")
    Mmax = bank.max_clips * (bank.max_clips + 1) // 2
    out = torch.empty((Nq, Mmax), dtype=torch.float32, device=Q.device)
    _check(lib().vfr_score_prior_own_f32(Q.data_ptr(), Nq, bank.emb.data_ptr(), bank.clip_off.data_ptr(), _ptr(own) if Nq else 0,
                                         bank.num_videos, bank.max_clips, bank.dim, eps, Mmax, off.data_ptr(), val.data_ptr(),
                                         out.data_ptr() if out.numel() else 0, _ptr(bad), _stream()), "vfr_score_prior_own_f32")
    return out


def score_prior(Q: torch.Tensor, bank: VideoBank, table, k: int, level: str = "moments", rank_dist=None, rank_idx=None, count_lt=None,
                workspace: torch.Tensor | None = None, bad: torch.Tensor | None = None, eps: float = 1e-6):
    """Prior-aware retrieval (include/vfr.h vfr_score_prior_f32): moments ranked by fl(score + table entry), moments whose entry is
    +inf excluded.  ``table``: an ``engine.MomentTable`` on the device (``engine.moment_table`` / ``engine.prior_table``).
    ``level`` "moments": the k best candidate moments; "videos": the k best videos that have a candidate, each as (best biased
    score, id of that moment).  Padded with (+inf, -1).  rank_dist / rank_idx [R, Nq] (or [Nq]), R <= 4: ``count_lt`` [R, Nq] int64
    += the candidates (videos) that sort before each rank key (allocated zeroed when None); the key (+inf, -1) counts them all.
    ``bad`` (int32 [1], optional) is set to 1 by an entry that is NaN or < 0.
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count_lt | None)."""
    if level not in FUSION_LEVELS:
        raise ValueError(f"score_prior: unknown level {level!r} (moments, videos)")
    Q = _dev(Q, torch.float32, "Q")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise ValueError(f"score_prior: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    Nq, dev = Q.shape[0], Q.device
    off, val = _prior_table(table, bank, dev, "score_prior")
    od, oi = _out_lists(Nq, k, dev)
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nq, dev)
    nbytes = lib().vfr_score_prior_workspace_bytes(Nq, bank.num_videos, k)
    workspace = _workspace(workspace, nbytes, dev)
    workspace._vfr_bank = None                   # whatever a pre-filter left in this workspace is overwritten
    _check(lib().vfr_score_prior_f32(*_bank_args(Q, bank, eps), FUSION_LEVELS[level], k, _ptr(od), _ptr(oi), R, _ptr(rank_dist),
                                     _ptr(rank_idx), _ptr(count_lt), off.data_ptr(), val.data_ptr(), _ptr(bad), workspace.data_ptr(),
                                     nbytes, _stream()), "vfr_score_prior_f32")
    return od, oi, count_lt


WINDOW_MAX_LEN = 64                           # include/vfr.h: 1 <= max_len <= 64


def score_window(Q: torch.Tensor, bank: VideoBank, max_len: int, k: int, rank_dist=None, rank_idx=None, count_lt=None,
                 workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Windowed retrieval (include/vfr.h vfr_score_window_f32): the candidates are the moments of at most ``max_len`` clips
    (1 .. 64), in videos of any length up to 1 024 clips; scores and ids are the canonical ones, so ``max_len >= bank.max_clips``
    gives ``score_topk(mode="exact")``.  The k best candidates, padded with (+inf, -1).  rank_dist / rank_idx [R, Nq] (or [Nq]),
    R <= 4: ``count_lt`` [R, Nq] int64 += the candidates that sort before each rank key (allocated zeroed when None).
    Returns (dist [Nq,k] | None, idx [Nq,k] int64 | None, count_lt | None)."""
    Q = _dev(Q, torch.float32, "Q")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise ValueError(f"score_window: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    if bank.emb.device != Q.device:
        raise ValueError(f"score_window: the bank lives on {bank.emb.device}, the queries on {Q.device}")
    Nq, dev = Q.shape[0], Q.device
    od, oi = _out_lists(Nq, k, dev)
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nq, dev)
    nbytes = lib().vfr_score_window_workspace_bytes(Nq, bank.total_clips, k)
    workspace = _workspace(workspace, nbytes, dev)
    workspace._vfr_bank = None                   # whatever a pre-filter left in this workspace is overwritten
    _check(lib().vfr_score_window_f32(Q.data_ptr(), Nq, bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.mom_off.data_ptr(),
                                      bank.num_videos, bank.total_clips, bank.max_clips, bank.dim, eps, bank.id_base, int(max_len), k,
                                      _ptr(od), _ptr(oi), R, _ptr(rank_dist), _ptr(rank_idx), _ptr(count_lt), workspace.data_ptr(),
                                      nbytes, _stream()), "vfr_score_window_f32")
    return od, oi, count_lt


def window_span_keys(Q: torch.Tensor, bank: VideoBank, items: torch.Tensor, vid_base: int = 0, out: torch.Tensor | None = None,
                     bad: torch.Tensor | None = None, eps: float = 1e-6) -> torch.Tensor:
    """Keys of named spans (include/vfr.h vfr_score_window_span_keys_f32): ``items`` int32 [Np, 4] = (query row, corpus-global
    video, start, end), spans of at most 64 clips -> int64 [Np] packed (score, canonical moment id) keys.  Items whose video is
    outside [vid_base, vid_base + Nv) and malformed items are left untouched (``out`` is KEY_EMPTY pre-filled when None); ``bad``
    (int32 [1], optional) is set to 1 by a malformed item."""
    Q = _dev(Q, torch.float32, "Q")
    items = _dev(items, torch.int32, "items")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise ValueError(f"window_span_keys: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    if items.dim() != 2 or items.shape[1] != 4:
        raise ValueError(f"window_span_keys: items must be int32 [Np, 4], got {tuple(items.shape)}")
    if bank.emb.device != Q.device or items.device != Q.device:
        raise ValueError(f"window_span_keys: the bank lives on {bank.emb.device}, the items on {items.device}, the queries on {Q.device}")
    Np = items.shape[0]
    if out is None:
        out = torch.full((Np,), KEY_EMPTY, dtype=torch.int64, device=Q.device)
    elif out.numel() != Np or not out.is_contiguous():
        raise ValueError(f"window_span_keys: out must be contiguous int64 [{Np}]")
    out = _dev(out, torch.int64, "out")
    _check(lib().vfr_score_window_span_keys_f32(Q.data_ptr(), Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                                bank.mom_off.data_ptr(), bank.num_videos, bank.total_clips, bank.dim, eps,
                                                bank.id_base, int(vid_base), items.data_ptr() if Np else 0,
                                                Np, out.data_ptr() if Np else 0, _ptr(bad), _stream()),
           "vfr_score_window_span_keys_f32")
    return out


FUSION_MAX_SWEEP = 16                         # include/vfr.h VFR_FUSION_MAX_SWEEP


def fusion_weight_grid(grid, S: int) -> np.ndarray:
    """A grid of stream weights as fp32 [W, S], W >= 1: every row as ``fusion_weights`` takes it (ValueError otherwise).  Host only."""
    if not 1 <= S <= FUSION_MAX_STREAMS:
        raise ValueError(f"late fusion takes 1 .. {FUSION_MAX_STREAMS} streams, got {S}")
    g = np.asarray(grid.cpu() if isinstance(grid, torch.Tensor) else grid, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] != S:
        raise ValueError(f"late fusion: a weight grid is [W >= 1, {S}], got shape {g.shape}")
    g32 = np.ascontiguousarray(g, dtype=np.float32)
    bad = np.nonzero(~(np.isfinite(g32) & (g32 >= 0)).all(axis=1))[0]
    if len(bad):
        raise ValueError(f"late fusion: weights must be finite and >= 0, got {g[bad[0]].tolist()} in grid row {int(bad[0])}")
    return g32


def _sweep_hosts(hosts, g: np.ndarray):
    """The host arrays of ``_fusion_streams`` with the weights replaced by the rows ``g`` [W <= 16, S] of a grid."""
    Qh, Vh, Dh, _, S = hosts
    return Qh, Vh, Dh, (ctypes.c_float * g.size)(*g.reshape(-1).tolist()), g.shape[0], S


def score_fusion_sweep_own(Qs, banks, grid, own: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """``score_fusion_own`` for every row of a weight grid [W, S] in one pass (include/vfr.h vfr_score_fusion_sweep_own_f32):
    [W, Nq, Mmax], slice w bit for bit ``score_fusion_own(Qs, banks, grid[w], own)``.  The stream clip distances are computed once
    per 16 rows of the grid (a longer grid is split into slices of 16)."""
    g = fusion_weight_grid(grid, len(list(banks)))
    Qs, banks, hosts = _fusion_streams(Qs, banks, g[0], "score_fusion_sweep_own")
    b0 = banks[0]
    own = _dev(own, torch.int32, "own")
    Nq = Qs[0].shape[0]
    if own.numel() != Nq:
        raise ValueError(f"score_fusion_sweep_own: {own.numel()} own videos for {Nq} queries")
    Mmax = b0.max_clips * (b0.max_clips + 1) // 2
    out = torch.empty((len(g), Nq, Mmax), dtype=torch.float32, device=Qs[0].device)
    for a in range(0, len(g), FUSION_MAX_SWEEP):
        part = out[a:a + FUSION_MAX_SWEEP]
        _check(lib().vfr_score_fusion_sweep_own_f32(*_sweep_hosts(hosts, g[a:a + FUSION_MAX_SWEEP]), Nq, b0.clip_off.data_ptr(),
                                                    _ptr(own) if Nq else 0, b0.num_videos, b0.max_clips, eps, Mmax,
                                                    part.data_ptr() if part.numel() else 0, _stream()),
               "vfr_score_fusion_sweep_own_f32")
    return out


def score_fusion_sweep(Qs, banks, grid, level: str, rank_dist, rank_idx, count_lt=None, eps: float = 1e-6) -> torch.Tensor:
    """Rank counts of late fusion for every row of a weight grid [W, S] in one pass (include/vfr.h vfr_score_fusion_sweep_f32).
    rank_dist / rank_idx [W, R, Nq] (or [W, Nq]), R <= 4: the rank keys of each weight vector; ``count_lt`` [W, R, Nq] int64 += the
    moments (``level`` "moments") or videos ("videos") that sort strictly before each key (allocated zeroed when None) -- slice w
    bit for bit what ``score_fusion(Qs, banks, grid[w], 0, level, rank_dist[w], rank_idx[w])`` counts.  No lists and no workspace;
    a grid of more than 16 rows is split into slices of 16.  Returns count_lt."""
    if level not in FUSION_LEVELS:
        raise ValueError(f"score_fusion_sweep: unknown level {level!r} (moments, videos)")
    g = fusion_weight_grid(grid, len(list(banks)))
    Qs, banks, hosts = _fusion_streams(Qs, banks, g[0], "score_fusion_sweep")
    b0 = banks[0]
    Nq, dev, W = Qs[0].shape[0], Qs[0].device, len(g)
    if rank_dist is None or rank_idx is None:
        raise ValueError("score_fusion_sweep: rank_dist and rank_idx [W, R, Nq] are required (the sweep only counts)")
    rank_dist, rank_idx = _dev(rank_dist, torch.float32, "rank_dist"), _dev(rank_idx, torch.int64, "rank_idx")
    if rank_dist.dim() == 2 and rank_idx.dim() == 2:
        rank_dist, rank_idx = rank_dist[:, None], rank_idx[:, None]
    if rank_dist.dim() != 3 or rank_dist.shape[0] != W or rank_dist.shape[2] != Nq or rank_idx.shape != rank_dist.shape:
        raise ValueError(f"score_fusion_sweep: rank_dist / rank_idx must be [{W}, R, {Nq}], got {tuple(rank_dist.shape)} / "
                         f"{tuple(rank_idx.shape)}")
    R = rank_dist.shape[1]
    if count_lt is None:
        count_lt = torch.zeros((W, R, Nq), dtype=torch.int64, device=dev)
    count_lt = _dev(count_lt, torch.int64, "count_lt")
    if count_lt.shape != rank_dist.shape:
        raise ValueError(f"score_fusion_sweep: count_lt {tuple(count_lt.shape)} for rank keys {tuple(rank_dist.shape)}")
    for a in range(0, W, FUSION_MAX_SWEEP):
        z = a + FUSION_MAX_SWEEP
        _check(lib().vfr_score_fusion_sweep_f32(*_sweep_hosts(hosts, g[a:z]), Nq, b0.clip_off.data_ptr(), b0.mom_off.data_ptr(),
                                                b0.num_videos, b0.total_clips, b0.max_clips, eps, b0.id_base, FUSION_LEVELS[level],
                                                R if Nq else 0,             # (no queries: the empty tensors have no address)
                                                _ptr(rank_dist[a:z]), _ptr(rank_idx[a:z]), _ptr(count_lt[a:z]), _stream()),
               "vfr_score_fusion_sweep_f32")
    return count_lt


def score_sentences(S: torch.Tensor, bank: VideoBank, probes: torch.Tensor, k: int, vid_base: int = 0, sent_base: int = 0,
                    rank_dist=None, rank_idx=None, count_lt=None, bad: torch.Tensor | None = None,
                    workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Sentence retrieval for moments (include/vfr.h vfr_score_sentences_f32): per probe moment the k best sentences of the bank
    ``S`` [Ns, D].  ``probes`` [Nm, 3] int32 = (corpus-global video, start_t, end_t), any order; ``vid_base`` = global index of the
    bank's first video (probes of other shards give padding and add nothing); ids are ``sent_base`` + row of ``S``.
    rank_dist / rank_idx [R, Nm] (or [Nm]), R <= 4: ``count_lt`` [R, Nm] int64 += the sentences that sort before each rank key
    (allocated zeroed when None).  ``bad`` (device int32 [1], nullable) is set to 1 for a malformed probe.
    The probes are handed to the library sorted by video (stable device sort, no synchronisation), so probes of one video share
    their clip distances; results come back in the caller's order.
    Returns (dist [Nm,k] | None, idx [Nm,k] int64 | None, count_lt | None)."""
    S = _dev(S, torch.float32, "S")
    probes = _dev(probes, torch.int32, "probes")
    if probes.dim() != 2 or probes.shape[1] != 3:
        raise RuntimeError(f"score_sentences: probes must be [Nm, 3] (video, start_t, end_t), got {tuple(probes.shape)}")
    if S.dim() != 2 or S.shape[1] != bank.dim:
        raise RuntimeError(f"score_sentences: S must be [Ns, {bank.dim}], got {tuple(S.shape)}")
    Ns, Nm = int(S.shape[0]), int(probes.shape[0])
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Nm, S.device)
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    order = torch.sort(probes[:, 0], stable=True).indices if Nm > 1 else None
    sp = probes if order is None else probes[order].contiguous()
    od, oi = _out_lists(Nm, k, S.device)
    rd = ri = cl = None
    if R:
        rd = rank_dist if order is None else rank_dist[:, order].contiguous()
        ri = rank_idx if order is None else rank_idx[:, order].contiguous()
        cl = count_lt if order is None else torch.zeros_like(count_lt)
    nbytes = lib().vfr_score_sentences_workspace_bytes(Nm, Ns, k)
    workspace = _workspace(workspace, nbytes, S.device)
    _check(lib().vfr_score_sentences_f32(_ptr(S) if Ns else 0, Ns, bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.num_videos,
                                         bank.total_clips, bank.max_clips, bank.dim, eps, _ptr(sp) if Nm else 0, Nm, int(vid_base),
                                         int(sent_base), k, _ptr(od), _ptr(oi), R, _ptr(rd), _ptr(ri), _ptr(cl), _ptr(bad),
                                         workspace.data_ptr(), nbytes, _stream()), "vfr_score_sentences_f32")
    if order is not None:                         # back to the caller's order
        if k > 0:
            od, oi = torch.empty_like(od).index_copy_(0, order, od), torch.empty_like(oi).index_copy_(0, order, oi)
        if R:
            count_lt.index_add_(1, order, cl)
    return od, oi, count_lt


def score_video_sentences(S: torch.Tensor, bank: VideoBank, videos: torch.Tensor, k: int, vid_base: int = 0, sent_base: int = 0,
                          rank_dist=None, rank_idx=None, count_lt=None, bad: torch.Tensor | None = None,
                          workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Video-to-sentence retrieval (include/vfr.h vfr_score_video_sentences_f32): per probe video the k best sentences of the bank
    ``S`` [Ns, D], the score of (video, sentence) being the video's best moment distance for the sentence (``score_video_topk``'s
    quantity).  ``videos`` [Np] int32 = corpus-global video indices, any order, repeats allowed; ``vid_base`` = global index of the
    bank's first video (probes of other shards give padding and add nothing); ids are ``sent_base`` + row of ``S``.
    rank_dist / rank_idx [R, Np] (or [Np]), R <= 4: ``count_lt`` [R, Np] int64 += the sentences that sort before each rank key
    (allocated zeroed when None).  ``bad`` (device int32 [1], nullable) is set to 1 for a probe with video < 0.
    Returns (dist [Np,k] | None, idx [Np,k] int64 | None, count_lt | None)."""
    S = _dev(S, torch.float32, "S")
    videos = _dev(videos, torch.int32, "videos")
    if videos.dim() != 1:
        raise RuntimeError(f"score_video_sentences: videos must be [Np], got {tuple(videos.shape)}")
    if S.dim() != 2 or S.shape[1] != bank.dim:
        raise RuntimeError(f"score_video_sentences: S must be [Ns, {bank.dim}], got {tuple(S.shape)}")
    Ns, Np = int(S.shape[0]), int(videos.shape[0])
    rank_dist, rank_idx, count_lt, R = _rank_keys(rank_dist, rank_idx, count_lt, Np, S.device)
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    od, oi = _out_lists(Np, k, S.device)
    nbytes = lib().vfr_score_video_sentences_workspace_bytes(Np, Ns, k)
    workspace = _workspace(workspace, nbytes, S.device)
    _check(lib().vfr_score_video_sentences_f32(_ptr(S) if Ns else 0, Ns, bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.num_videos,
                                               bank.total_clips, bank.max_clips, bank.dim, eps, _ptr(videos) if Np else 0, Np,
                                               int(vid_base), int(sent_base), k, _ptr(od), _ptr(oi), R if Np else 0, _ptr(rank_dist),
                                               _ptr(rank_idx), _ptr(count_lt), _ptr(bad), workspace.data_ptr(), nbytes, _stream()),
           "vfr_score_video_sentences_f32")
    return od, oi, count_lt


def _items(items, who: str) -> torch.Tensor:
    items = _dev(items, torch.int32, "items")
    if items.dim() != 2 or items.shape[1] != 4:
        raise RuntimeError(f"{who}: items must be [N, 4] (query row, video, start_t, end_t), got {tuple(items.shape)}")
    return items


def score_spans(Q: torch.Tensor, bank: VideoBank, items: torch.Tensor, vid_base: int = 0, out: torch.Tensor | None = None,
                bad: torch.Tensor | None = None, eps: float = 1e-6) -> torch.Tensor:
    """Scores of named (query, video, span) items (include/vfr.h vfr_score_spans_f32): ``items`` [Np, 4] int32 = (row of ``Q``,
    corpus-global video, start_t, end_t); the value ``score_moments`` holds at [row, moment id].  Items of videos outside this bank
    (``vid_base`` .. + its videos) and malformed ones are left untouched: ``out`` [Np] is allocated pre-filled with +inf (or pass
    another shard's result to chain).  ``bad`` (device int32 [1], nullable) is set to 1 for a malformed item."""
    Q = _dev(Q, torch.float32, "Q")
    items = _items(items, "score_spans")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise RuntimeError(f"score_spans: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    Np = int(items.shape[0])
    if out is None:
        out = torch.full((Np,), float("inf"), dtype=torch.float32, device=Q.device)
    out = _dev(out, torch.float32, "out")
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    _check(lib().vfr_score_spans_f32(_ptr(Q) if Q.shape[0] else 0, Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                     bank.num_videos, bank.total_clips, bank.max_clips, bank.dim, eps, int(vid_base),
                                     _ptr(items) if Np else 0, Np, _ptr(out) if Np else 0, _ptr(bad), _stream()), "vfr_score_spans_f32")
    return out


MINE_MODES = {"same_length": 0, "any": 1}         # include/vfr.h VFR_MINE_SAME_LENGTH / VFR_MINE_ANY
MINE_MAX_EXCL = 8


def mine_negatives(Q: torch.Tensor, bank: VideoBank, items: torch.Tensor, h: int, vid_base: int = 0, intra: str = "same_length",
                   excl: torch.Tensor | None = None, floor: torch.Tensor | None = None, thr: torch.Tensor | None = None,
                   want_inter: bool = True, want_intra: bool = True, intra_out=None, count_inter=None, count_intra=None,
                   bad: torch.Tensor | None = None, workspace: torch.Tensor | None = None, eps: float = 1e-6):
    """Hard-negative mining (include/vfr.h vfr_mine_negatives_f32): ``items`` [Nm, 4] int32 = (row of ``Q``, own corpus-global video,
    start_t, end_t) training spans.  Per item the ``h`` hardest inter negatives -- the other videos of this bank with at least
    end_t + 1 clips, scored at the item's span, as (score, ``vid_base`` + video) -- and the ``h`` hardest intra negatives -- the own
    video's other moments of the same length (``intra`` "same_length") or all but the item's span and the spans of ``excl``
    [Nm, X, 2] int32, X <= 8, rows padded with (-1, -1) ("any") -- as (score, global moment id); both padded with (+inf, -1).  The
    intra lists are written only by the bank that holds the own video: they are allocated pre-filled with padding (or pass another
    shard's ``intra_out`` = (dist, idx) to chain).  ``floor`` [Nm]: negatives with score <= floor are not listed.  ``thr`` [Nm]:
    ``count_inter`` / ``count_intra`` [Nm] int64 += the eligible negatives with score < thr (allocated zeroed when None).
    ``bad`` (device int32 [1], nullable) is set to 1 for a malformed item.  The items are handed to the library sorted by span (stable
    device sort, no synchronisation), so neighbouring waves read the same clip rows; results come back in the caller's order.
    Returns (inter_dist, inter_vid, intra_dist, intra_idx, count_inter, count_intra), None for what was not asked for."""
    if intra not in MINE_MODES:
        raise RuntimeError(f"mine_negatives: unknown intra mode {intra!r} (same_length, any)")
    Q = _dev(Q, torch.float32, "Q")
    items = _items(items, "mine_negatives")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise RuntimeError(f"mine_negatives: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    Nm, dev = int(items.shape[0]), Q.device
    X = 0
    if excl is not None and intra == "any":
        excl = _dev(excl, torch.int32, "excl")
        if excl.dim() != 3 or excl.shape[0] != Nm or excl.shape[2] != 2 or excl.shape[1] > MINE_MAX_EXCL:
            raise RuntimeError(f"mine_negatives: excl must be [Nm, X <= {MINE_MAX_EXCL}, 2], got {tuple(excl.shape)}")
        X = int(excl.shape[1])
    if X == 0:
        excl = None
    floor = None if floor is None else _dev(floor, torch.float32, "floor").reshape(Nm)
    thr = None if thr is None else _dev(thr, torch.float32, "thr").reshape(Nm)
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    lists = h > 0
    ind = inv = None
    if want_inter and lists:
        ind, inv = _out_lists(Nm, h, dev)
    itd = iti = None
    if want_intra and lists:
        if intra_out is None:
            itd = torch.full((Nm, h), float("inf"), dtype=torch.float32, device=dev)
            iti = torch.full((Nm, h), -1, dtype=torch.int64, device=dev)
        else:
            itd, iti = _dev(intra_out[0], torch.float32, "intra_out[0]"), _dev(intra_out[1], torch.int64, "intra_out[1]")
    if thr is not None:
        if want_inter:
            count_inter = torch.zeros((Nm,), dtype=torch.int64, device=dev) if count_inter is None else _dev(count_inter, torch.int64, "count_inter")
        if want_intra:
            count_intra = torch.zeros((Nm,), dtype=torch.int64, device=dev) if count_intra is None else _dev(count_intra, torch.int64, "count_intra")
        if not (want_inter or want_intra):
            thr = None
    else:
        count_inter = count_intra = None
    order = None
    if Nm > 1:                                     # by (start_t, end_t): neighbouring waves then read the same clip rows
        order = torch.sort(items[:, 2].to(torch.int64) * (1 << 32) + items[:, 3].to(torch.int64), stable=True).indices
    pick = (lambda t: t) if order is None else (lambda t: None if t is None else t[order].contiguous())
    zero = (lambda t: t) if order is None else (lambda t: None if t is None else torch.zeros_like(t))
    s_items, s_excl, s_floor, s_thr = pick(items), pick(excl), pick(floor), pick(thr)
    s_itd, s_iti = pick(itd), pick(iti)
    s_ci, s_ca = zero(count_inter), zero(count_intra)
    nbytes = lib().vfr_mine_negatives_workspace_bytes(Nm, bank.num_videos, h)
    workspace = _workspace(workspace, nbytes, dev)
    _check(lib().vfr_mine_negatives_f32(_ptr(Q) if Q.shape[0] else 0, Q.shape[0], bank.emb.data_ptr(), bank.clip_off.data_ptr(),
                                        bank.mom_off.data_ptr(), bank.num_videos, bank.total_clips, bank.max_clips, bank.dim, eps,
                                        bank.id_base, int(vid_base), _ptr(s_items) if Nm else 0, Nm, h, MINE_MODES[intra], _ptr(s_excl), X,
                                        _ptr(s_floor), _ptr(s_thr), _ptr(ind), _ptr(inv), _ptr(s_itd), _ptr(s_iti), _ptr(s_ci),
                                        _ptr(s_ca), _ptr(bad), workspace.data_ptr(), nbytes, _stream()), "vfr_mine_negatives_f32")
    if order is not None:                          # back to the caller's order
        if ind is not None:
            ind, inv = torch.empty_like(ind).index_copy_(0, order, ind), torch.empty_like(inv).index_copy_(0, order, inv)
        if itd is not None:
            itd.index_copy_(0, order, s_itd)
            iti.index_copy_(0, order, s_iti)
        if count_inter is not None:
            count_inter.index_add_(0, order, s_ci)
        if count_intra is not None:
            count_intra.index_add_(0, order, s_ca)
    return ind, inv, itd, iti, count_inter, count_intra


def _group_args(Q: torch.Tensor, bank: VideoBank, grp_off: torch.Tensor, max_len: int, eps: float, who: str):
    """The leading arguments the paragraph entry points share: sentences, groups, the bank's CSR, eps -> (arguments, Ng)."""
    grp_off = _dev(grp_off, torch.int64, "grp_off")
    if grp_off.dim() != 1 or grp_off.numel() < 1:
        raise RuntimeError(f"{who}: grp_off must be int64 [Ng + 1]")
    if Q.dim() != 2 or Q.shape[1] != bank.dim:
        raise RuntimeError(f"{who}: Q must be [Nq, {bank.dim}], got {tuple(Q.shape)}")
    Ng = int(grp_off.numel()) - 1
    return (Q.data_ptr(), Q.shape[0], grp_off.data_ptr(), Ng, int(max_len), bank.emb.data_ptr(), bank.clip_off.data_ptr(),
            bank.mom_off.data_ptr(), bank.num_videos, bank.total_clips, bank.min_clips, bank.max_clips, bank.dim, eps), Ng, grp_off


def score_paragraphs(Q: torch.Tensor, bank: VideoBank, grp_off: torch.Tensor, max_len: int, k: int, vid_base: int = 0, own_dist=None,
                     own_idx=None, count=None, mode: str | None = None, workspace: torch.Tensor | None = None,
                     bad: torch.Tensor | None = None, eps: float = 1e-6):
    """Paragraph-to-video retrieval (include/vfr.h vfr_score_paragraphs_f32): ``Q`` [Nq, D] sentences, a paragraph = the run of rows
    ``grp_off[g] .. grp_off[g+1]`` (device int64 [Ng+1]; ``max_len`` = the longest run, <= 64).  The score of (paragraph, video) is
    the fp32 mean, in sentence order, of the video's best distance for each sentence; keys are (score, ``vid_base`` + video).
    Returns the k best videos per paragraph (score [Ng,k] | None, global video index [Ng,k] int64 | None; padded with (+inf, -1)) and,
    with ``own_dist`` / ``own_idx`` [Ng] (``score_paragraph_pairs`` of the own video), ``count`` [Ng] int64 += the number of this
    bank's videos whose key sorts before it (allocated zeroed when None).  ``mode``: "mfma" or "exact" (same bits); None =
    DEFAULT_SCORE_MODE.  ``bad`` (device int32 [1], nullable) is set to 1 for a malformed ``grp_off``."""
    dtype, Q = _video_mode(mode, Q, "score_paragraphs")
    args, Ng, grp_off = _group_args(Q, bank, grp_off, max_len, eps, "score_paragraphs")
    od, oi = _out_lists(Ng, k, Q.device)
    own_dist, own_idx, cnt, R = _rank_keys(own_dist, own_idx, count, Ng, Q.device, ("own_dist", "own_idx", "count"))
    if R:                                    # ONE key per paragraph, and the public count is [Ng]
        own_dist, own_idx = own_dist.reshape(Ng), own_idx.reshape(Ng)
        if count is None:
            cnt = cnt.reshape(Ng)
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    nbytes = lib().vfr_score_paragraphs_workspace_bytes(Q.shape[0], Ng, bank.num_videos, bank.total_clips, k)
    workspace = _workspace(workspace, nbytes, Q.device)
    token, ready = _video_bank_ready(workspace, bank, dtype, eps)       # the workspace front is score_video_topk's
    _check(lib().vfr_score_paragraphs_f32(*args, int(vid_base), k, _ptr(od), _ptr(oi), _ptr(own_dist), _ptr(own_idx), _ptr(cnt),
                                          dtype | (MFMA_BANK_READY if ready else 0), _ptr(bad), workspace.data_ptr(), nbytes, _stream()),
           "vfr_score_paragraphs_f32")
    _video_bank_claim(workspace, token, bank, dtype, ran=Ng > 0 and Q.shape[0] > 0 and max_len > 0 and (k > 0 or R > 0))
    return od, oi, cnt


def score_paragraph_pairs(Q: torch.Tensor, bank: VideoBank, grp_off: torch.Tensor, max_len: int, pairs: torch.Tensor, vid_base: int = 0,
                          out_score: torch.Tensor | None = None, out_moments: torch.Tensor | None = None, moments: bool = True,
                          bad: torch.Tensor | None = None, eps: float = 1e-6):
    """Named (paragraph, video) pairs (include/vfr.h vfr_score_paragraph_pairs_f32): ``pairs`` int32 [Np, 2] = (group, GLOBAL video
    index).  Returns (score [Np], moments int64 [Np, max_len] | None): the paragraph score of each pair and, per sentence of the
    group, the global id of the video's best moment (-1 past the group's length).  Pairs of videos outside this bank (``vid_base``
    .. + its videos) are left untouched: the outputs are allocated pre-filled with +inf / -1 (or pass ``out_score`` /
    ``out_moments`` of another shard's call to chain).  ``moments=False`` skips the grounding."""
    Q = _dev(Q, torch.float32, "Q")
    pairs = _dev(pairs, torch.int32, "pairs")
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise RuntimeError(f"score_paragraph_pairs: pairs must be [Np, 2] (group, video), got {tuple(pairs.shape)}")
    args, Ng, grp_off = _group_args(Q, bank, grp_off, max_len, eps, "score_paragraph_pairs")
    Np = int(pairs.shape[0])
    if out_score is None:
        out_score = torch.full((Np,), float("inf"), dtype=torch.float32, device=Q.device)
    out_score = _dev(out_score, torch.float32, "out_score")
    if moments and out_moments is None:
        out_moments = torch.full((Np, int(max_len)), -1, dtype=torch.int64, device=Q.device)
    if out_moments is not None:
        out_moments = _dev(out_moments, torch.int64, "out_moments")
    if bad is not None:
        bad = _dev(bad, torch.int32, "bad")
    _check(lib().vfr_score_paragraph_pairs_f32(*args, bank.id_base, int(vid_base), _ptr(pairs) if Np else 0, Np, _ptr(out_score) if Np else 0,
                                               _ptr(out_moments) if Np and max_len else 0, _ptr(bad), _stream()),
           "vfr_score_paragraph_pairs_f32")
    return out_score, out_moments


def score_paragraphs_stats(workspace: torch.Tensor, Nq: int, Ng: int, bank: VideoBank) -> np.ndarray:
    """[Ng, 2] int64 of the last ``mode="mfma"`` fast-path ``score_paragraphs`` call on ``workspace``: videos given the exact chain
    per paragraph, and how many of them were undecided rank counts (synchronises)."""
    out = np.zeros((Ng, 2), np.int64)
    _check(lib().vfr_score_paragraphs_stats(workspace.data_ptr(), Nq, Ng, bank.num_videos, bank.total_clips,
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _stream()), "vfr_score_paragraphs_stats")
    return out


def nms_inter_table(nms_iou: float, max_len: int = 64) -> np.ndarray:
    """[max_len + 1] int32: per union length u the smallest integer intersection with inter / u > nms_iou in float64 (u + 1
    when none) -- the exact form of the IoU test of ``score_moment_nms`` (no GPU needed)."""
    out = np.zeros(max_len + 1, np.int32)
    _check(lib().vfr_nms_inter_table(float(nms_iou), int(max_len), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
           "vfr_nms_inter_table")
    return out


def score_video_topk_stats(workspace: torch.Tensor, Nq: int, bank: VideoBank) -> np.ndarray:
    """[Nq, 2] int64 of the last ``mode="mfma"`` fast-path call on ``workspace``: videos given an exact triangle per query, and
    how many of them were undecided rank counts (synchronises)."""
    out = np.zeros((Nq, 2), np.int64)
    _check(lib().vfr_score_video_topk_stats(workspace.data_ptr(), Nq, bank.num_videos, bank.total_clips,
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _stream()),
           "vfr_score_video_topk_stats")
    return out


def score_mfma_stats(workspace: torch.Tensor, Nq: int, bank: VideoBank, k: int) -> dict:
    """What the last ``mode="mfma"`` call on ``workspace`` left to the exact kernels (synchronises)."""
    out = (ctypes.c_int64 * 4)()
    _check(lib().vfr_score_topk_mfma_stats(workspace.data_ptr(), Nq, bank.num_videos, bank.total_clips, k, out, _stream()),
           "vfr_score_topk_mfma_stats")
    return {"groups": out[0], "fallback_groups": out[1], "exact_pairs": out[2], "markable_pairs": out[3],
            "exact_pair_fraction": out[2] / float(max(1, Nq * bank.num_videos))}


def topk_workspace(Nq: int, num_videos: int, k: int, device, total_clips: int | None = None) -> torch.Tensor:
    """Workspace large enough for every scoring mode of a bank of ``num_videos`` videos / ``total_clips`` clips
    (64 clips per video assumed when not given)."""
    total_clips = int(total_clips) if total_clips is not None else 64 * num_videos
    return _workspace(None, max(lib().vfr_score_topk_workspace_bytes(Nq, num_videos, k),
                                lib().vfr_score_topk_mfma_workspace_bytes(Nq, num_videos, total_clips, k)), device)


def topk_merge(part_dist: torch.Tensor, part_idx: torch.Tensor):
    """[G,Nq,k] shard lists -> merged [Nq,k] in (distance, id) order."""
    pd, pi = _dev(part_dist, torch.float32, "part_dist"), _dev(part_idx, torch.int64, "part_idx")
    G, Nq, k = pd.shape
    od = torch.empty((Nq, k), dtype=torch.float32, device=pd.device)
    oi = torch.empty((Nq, k), dtype=torch.int64, device=pd.device)
    _check(lib().vfr_topk_merge_f32(pd.data_ptr(), pi.data_ptr(), G, Nq, k, od.data_ptr(), oi.data_ptr(), _stream()),
           "vfr_topk_merge_f32")
    return od, oi


KEY_EMPTY = 0x7F800000FFFFFFFF     # VFR_KEY_EMPTY: (+inf, max id)


def topk_pack_keys(dist: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """(dist, idx) lists -> int64 exchange keys of the same shape (idx < 0 -> KEY_EMPTY)."""
    d, i = _dev(dist, torch.float32, "dist"), _dev(idx, torch.int64, "idx")
    keys = out if out is not None else torch.empty(d.shape, dtype=torch.int64, device=d.device)
    if out is not None:
        _dev(out, torch.int64, "out")
    _check(lib().vfr_topk_pack_keys(d.data_ptr(), i.data_ptr(), d.numel(), keys.data_ptr(), _stream()), "vfr_topk_pack_keys")
    return keys


def topk_merge_keys(part_keys: torch.Tensor, want_lists: bool = True, want_keys: bool = False):
    """[G,Nq,k] int64 key lists -> (dist [Nq,k] | None, idx [Nq,k] | None, keys [Nq,k] | None).  The slots may be views into
    wider rows (each [Nq,k] dense, any slot stride >= Nq*k): the lists inside a packed exchange buffer are merged in place."""
    pk = part_keys
    G, Nq, k = pk.shape
    if not (pk.is_cuda and pk.dtype == torch.int64 and pk.stride(2) == 1 and pk.stride(1) == k and pk.stride(0) >= Nq * k):
        pk = _dev(part_keys, torch.int64, "part_keys")
    od = torch.empty((Nq, k), dtype=torch.float32, device=pk.device) if want_lists else None
    oi = torch.empty((Nq, k), dtype=torch.int64, device=pk.device) if want_lists else None
    ok = torch.empty((Nq, k), dtype=torch.int64, device=pk.device) if want_keys else None
    _check(lib().vfr_topk_merge_keys_strided(pk.data_ptr(), pk.stride(0) if G > 1 else Nq * k, G, Nq, k, _ptr(od), _ptr(oi), _ptr(ok),
                                             _stream()), "vfr_topk_merge_keys")
    return od, oi, ok


def _gt_key_args(own_scores, labels, id_base, sel, Nq: int, who: str):
    """The checked inputs ``gt_best_keys`` / ``gt_rank_keys`` share -> (their leading arguments, R, device, the tensors the
    pointers belong to: held by the caller until its call is queued)."""
    sc = _dev(own_scores, torch.float32, "own_scores")
    lab = labels.view(torch.uint8) if labels.dtype == torch.bool else labels
    lab = _dev(lab, torch.uint8, "labels")
    base, sel = _dev(id_base, torch.int64, "id_base"), _dev(sel, torch.int64, "sel")
    R, n_sel, Ml = lab.shape
    if sc.shape[0] != n_sel or base.numel() != n_sel or sel.numel() != n_sel:
        raise RuntimeError(f"{who}: inconsistent shapes")
    args = (sc.data_ptr(), n_sel, min(sc.shape[1], Ml), sc.shape[1], lab.data_ptr(), R, Ml, base.data_ptr(), sel.data_ptr(), Nq)
    return args, R, sc.device, (sc, lab, base, sel)


def gt_best_keys(own_scores: torch.Tensor, labels: torch.Tensor, id_base: torch.Tensor, sel: torch.Tensor, Nq: int):
    """own_scores [n_sel, Ms] (``score_own``), labels bool/uint8 [R, n_sel, Ml], id_base / sel int64 [n_sel] ->
    keys int64 [R, Nq]: best positive (score, id) per threshold and query, KEY_EMPTY elsewhere."""
    args, R, device, _held = _gt_key_args(own_scores, labels, id_base, sel, Nq, "gt_best_keys")
    keys = torch.empty((R, Nq), dtype=torch.int64, device=device)
    _check(lib().vfr_gt_best_keys_f32(*args, keys.data_ptr(), _stream()), "vfr_gt_best_keys_f32")
    return keys


def gt_rank_keys(own_scores: torch.Tensor, labels: torch.Tensor, id_base: torch.Tensor, sel: torch.Tensor, Nq: int):
    """``gt_best_keys`` plus, from the same two launches: the keys unpacked as (rank_dist f32 [R, Nq], rank_idx int64 [R, Nq]), a
    zeroed count buffer int64 [R, Nq] and the device flag (int32 [1]) "some selected query has no positive moment"."""
    args, R, device, _held = _gt_key_args(own_scores, labels, id_base, sel, Nq, "gt_rank_keys")
    keys = torch.empty((R, Nq), dtype=torch.int64, device=device)
    rd = torch.empty((R, Nq), dtype=torch.float32, device=device)
    ri = torch.empty((R, Nq), dtype=torch.int64, device=device)
    cnt = torch.empty((R, Nq), dtype=torch.int64, device=device)
    missing = torch.empty((1,), dtype=torch.int32, device=device)
    _check(lib().vfr_gt_rank_keys_f32(*args, keys.data_ptr(), rd.data_ptr(), ri.data_ptr(), cnt.data_ptr(), missing.data_ptr(),
                                      _stream()), "vfr_gt_rank_keys_f32")
    return keys, rd, ri, cnt, missing


def gt_labels(times: torch.Tensor, nannot: torch.Tensor, n_own: torch.Tensor, thresholds, strict: bool, Mmax: int):
    """a11 on the device: times int32 [Nq, A, 2], nannot / n_own int32 [Nq] -> labels bool [R, Nq, Mmax]."""
    t, na, no = _dev(times, torch.int32, "times"), _dev(nannot, torch.int32, "nannot"), _dev(n_own, torch.int32, "n_own")
    Nq, A = t.shape[0], t.shape[1]
    R = len(thresholds)
    thr = (ctypes.c_double * R)(*[float(x) for x in thresholds])
    lab = torch.empty((R, Nq, Mmax), dtype=torch.uint8, device=t.device)
    _check(lib().vfr_gt_labels_u8(t.data_ptr(), na.data_ptr(), no.data_ptr(), Nq, A, thr, R, int(bool(strict)), Mmax,
                                  lab.data_ptr(), _stream()), "vfr_gt_labels_u8")
    return lab.view(torch.bool)


def frames_normalize(frames_thwc: torch.Tensor) -> torch.Tensor:
    fr = _dev(frames_thwc, torch.uint8, "frames")
    T, H, W, _ = fr.shape
    out = torch.empty((T, 3, H, W), dtype=torch.float32, device=fr.device)
    _check(lib().vfr_frames_normalize_f32(fr.data_ptr(), T, H, W, out.data_ptr(), _stream()), "vfr_frames_normalize_f32")
    return out


def conv3x3_relu(x, w, b) -> torch.Tensor:
    x, w, b = _dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"), _dev(b, torch.float32, "b")
    B, Cin, H, W = x.shape
    y = torch.empty((B, w.shape[0], H, W), dtype=torch.float32, device=x.device)
    _check(lib().vfr_conv3x3_relu_f32(x.data_ptr(), B, Cin, H, W, w.data_ptr(), b.data_ptr(), w.shape[0], y.data_ptr(),
                                      _stream()), "vfr_conv3x3_relu_f32")
    return y


def maxpool2(x) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _check(lib().vfr_maxpool2_f32(x.data_ptr(), B, C, H, W, y.data_ptr(), _stream()), "vfr_maxpool2_f32")
    return y


def adaptive_avgpool7(x) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    y = torch.empty((B, C, 7, 7), dtype=torch.float32, device=x.device)
    _check(lib().vfr_adaptive_avgpool7_f32(x.data_ptr(), B, C, H, W, y.data_ptr(), _stream()), "vfr_adaptive_avgpool7_f32")
    return y


def vgg_fc7(frames_thwc, cfg, conv_w, conv_b, fc6, fc7) -> torch.Tensor:
    """uint8 [T,H,W,3] -> fc7 features [T, fc_dim]  (get_rgb_features.py:64-69,122-126,145-147)."""
    fr = _dev(frames_thwc, torch.uint8, "frames")
    T, H, W, _ = fr.shape
    cfg_i = (ctypes.c_int * len(cfg))(*[0 if c == "M" else int(c) for c in cfg])
    cw = [_dev(w, torch.float32, "conv_w") for w in conv_w]
    cb = [_dev(b, torch.float32, "conv_b") for b in conv_b]
    wp = (ctypes.c_void_p * len(cw))(*[w.data_ptr() for w in cw])
    bp = (ctypes.c_void_p * len(cb))(*[b.data_ptr() for b in cb])
    f6w, f6b = _dev(fc6[0], torch.float32, "fc6_w"), _dev(fc6[1], torch.float32, "fc6_b")
    f7w, f7b = _dev(fc7[0], torch.float32, "fc7_w"), _dev(fc7[1], torch.float32, "fc7_b")
    fc_dim = f6w.shape[0]
    out = torch.empty((T, fc_dim), dtype=torch.float32, device=fr.device)
    nbytes = lib().vfr_vgg_fc7_workspace_bytes(T, H, W, ctypes.cast(cfg_i, ctypes.c_void_p), len(cfg), fc_dim)
    ws = _workspace(None, nbytes, fr.device)
    _check(lib().vfr_vgg_fc7_f32(fr.data_ptr(), T, H, W, ctypes.cast(cfg_i, ctypes.c_void_p), len(cfg),
                                 ctypes.cast(wp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p), f6w.data_ptr(),
                                 f6b.data_ptr(), f7w.data_ptr(), f7b.data_ptr(), fc_dim, out.data_ptr(), ws.data_ptr(),
                                 nbytes, _stream()), "vfr_vgg_fc7_f32")
    return out


RESNET152_BLOCKS = (3, 8, 36, 3)


def resnet_conv_plan(blocks=RESNET152_BLOCKS, width: int = 64):
    """The convolutions of a torchvision Bottleneck ResNet in execution order: (conv prefix, bn prefix) of the state dict --
    the stem, then per block conv1, conv2, conv3 and, for the first block of a layer, downsample.0 / downsample.1."""
    plan = [("conv1", "bn1")]
    for li, nb in enumerate(blocks):
        for b in range(nb):
            pre = f"layer{li + 1}.{b}"
            plan += [(f"{pre}.conv1", f"{pre}.bn1"), (f"{pre}.conv2", f"{pre}.bn2"), (f"{pre}.conv3", f"{pre}.bn3")]
            if b == 0:
                plan.append((f"{pre}.downsample.0", f"{pre}.downsample.1"))
    return plan


def resnet_pack(state_dict, blocks=RESNET152_BLOCKS, width: int = 64, device="cuda:0"):
    """torchvision-style resnet state dict (tensors or numpy) -> (conv weights, packed BatchNorm tensors [4, C]) on the device,
    in the order ``vfr_resnet_pool_f32`` takes them.  Done once per model; the result is passed to ``resnet_pool``."""
    def t(x):
        return torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()
    convs, bns = [], []
    for conv, bn in resnet_conv_plan(blocks, width):
        convs.append(t(state_dict[conv + ".weight"]))
        bns.append(torch.stack([t(state_dict[bn + ".weight"]), t(state_dict[bn + ".bias"]), t(state_dict[bn + ".running_mean"]),
                                t(state_dict[bn + ".running_var"])]).contiguous())
    return ResnetPacked((convs, bns))


class ResnetPacked(tuple):
    """``(conv weights, packed BatchNorm tensors)`` as ``resnet_pack`` returns them, plus the folded form ``resnet_pool`` computes
    once per (blocks, width, eps) and keeps here (``vfr_resnet_fold_f32``): a plain tuple everywhere else."""
    def __new__(cls, pair):
        self = super().__new__(cls, pair)
        self.folded = {}
        return self


def resnet_pool(frames_thwc, packed, blocks=RESNET152_BLOCKS, width: int = 64, eps: float = 1e-5) -> torch.Tensor:
    """uint8 [T,H,W,3] -> pooled ResNet features [T, 32 * width]  (get_rgb_features.py:64-69,127-131, 147)."""
    fr = _dev(frames_thwc, torch.uint8, "frames")
    T, H, W, _ = fr.shape
    convs, bns = packed
    convs = [_dev(w, torch.float32, "conv_w") for w in convs]
    bns = [_dev(b, torch.float32, "bn") for b in bns]
    nconv = 1 + sum(3 * n + 1 for n in blocks)
    if len(convs) != nconv or len(bns) != nconv:
        raise RuntimeError(f"resnet_pool: expected {nconv} convolutions for blocks {tuple(blocks)}, got {len(convs)}")
    bl = (ctypes.c_int * 4)(*[int(b) for b in blocks])
    wp = (ctypes.c_void_p * nconv)(*[w.data_ptr() for w in convs])
    bp = (ctypes.c_void_p * nconv)(*[b.data_ptr() for b in bns])
    out = torch.empty((T, 32 * width), dtype=torch.float32, device=fr.device)
    nbytes = lib().vfr_resnet_pool_workspace_bytes(T, H, W, ctypes.cast(bl, ctypes.c_void_p), width)
    ws = _workspace(None, nbytes, fr.device)
    if isinstance(packed, ResnetPacked):
        # the model's weights folded once (BatchNorm into the convolutions, tap-major), reused by every later call
        key = (tuple(int(b) for b in blocks), int(width), float(eps), fr.device)
        folded = packed.folded.get(key)
        if folded is None:
            fb = lib().vfr_resnet_folded_bytes(ctypes.cast(bl, ctypes.c_void_p), width)
            folded = _workspace(None, fb, fr.device)
            _check(lib().vfr_resnet_fold_f32(ctypes.cast(bl, ctypes.c_void_p), width, ctypes.cast(wp, ctypes.c_void_p),
                                             ctypes.cast(bp, ctypes.c_void_p), eps, folded.data_ptr(), folded.numel(), _stream()),
                   "vfr_resnet_fold_f32")
            packed.folded[key] = folded
        _check(lib().vfr_resnet_pool_folded_f32(fr.data_ptr(), T, H, W, ctypes.cast(bl, ctypes.c_void_p), width, folded.data_ptr(),
                                                folded.numel(), out.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "vfr_resnet_pool_folded_f32")
        return out
    _check(lib().vfr_resnet_pool_f32(fr.data_ptr(), T, H, W, ctypes.cast(bl, ctypes.c_void_p), width, ctypes.cast(wp, ctypes.c_void_p),
                                     ctypes.cast(bp, ctypes.c_void_p), eps, out.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "vfr_resnet_pool_f32")
    return out


def transpose(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    r, c = x.shape
    out = torch.empty((c, r), dtype=torch.float32, device=x.device)
    _check(lib().vfr_transpose_f32(x.data_ptr(), r, c, out.data_ptr(), _stream()), "vfr_transpose_f32")
    return out


def colsum(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    _check(lib().vfr_colsum_f32(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream()), "vfr_colsum_f32")
    return out


def relu_backward(grad: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
    grad, act = _dev(grad, torch.float32, "grad"), _dev(act, torch.float32, "act")
    out = torch.empty_like(grad)
    _check(lib().vfr_relu_backward_f32(grad.data_ptr(), act.data_ptr(), grad.numel(), out.data_ptr(), _stream()), "vfr_relu_backward_f32")
    return out


def lstm_cell_forward(pre, xproj_t, x_stride, c_prev, gates_out, c_out, h_out):
    """pre [B,4H]; xproj_t = view whose row b starts b * x_stride floats after its first element."""
    B, H = c_prev.shape
    _check(lib().vfr_lstm_cell_forward_f32(pre.data_ptr(), xproj_t.data_ptr(), x_stride, c_prev.data_ptr(), B, H, gates_out.data_ptr(),
                                           c_out.data_ptr(), h_out.data_ptr(), _stream()), "vfr_lstm_cell_forward_f32")


def lstm_cell_backward(dh, dc, gates, c_prev, c_cur, dpre_out):
    B, H = c_prev.shape
    _check(lib().vfr_lstm_cell_backward_f32(dh.data_ptr(), dc.data_ptr(), gates.data_ptr(), c_prev.data_ptr(), c_cur.data_ptr(), B, H,
                                            dpre_out.data_ptr(), _stream()), "vfr_lstm_cell_backward_f32")


def bilstm_train_forward(x, ws):
    """x [B, T, E] f32, ws = the eight nn.LSTM tensors (forward four, reverse four) -> (gates [2,T,B,4H], cs, hs [2,T+1,B,H])."""
    x = _dev(x, torch.float32, "x")
    ws = [_dev(w, torch.float32, "lstm weight") for w in ws]
    B, T, E = x.shape
    H = ws[1].shape[1]
    gates = torch.empty((2, T, B, 4 * H), dtype=torch.float32, device=x.device)
    cs = torch.empty((2, T + 1, B, H), dtype=torch.float32, device=x.device)
    hs = torch.empty((2, T + 1, B, H), dtype=torch.float32, device=x.device)
    _check(lib().vfr_bilstm_train_forward_f32(x.data_ptr(), B, T, E, H, *[w.data_ptr() for w in ws], gates.data_ptr(), cs.data_ptr(),
                                              hs.data_ptr(), _stream()), "vfr_bilstm_train_forward_f32")
    return gates, cs, hs


def bilstm_train_backward(gout, gates, cs, whhT_f, whhT_b):
    """gout [B, 2H] -> dpre [2, T, B, 4H] (gradient of every step's gate pre-activations, step-major per direction)."""
    gout = _dev(gout, torch.float32, "gout")
    _, T, B, G = gates.shape
    H = G // 4
    nbytes = lib().vfr_bilstm_train_backward_workspace_bytes(B, H)
    wsb = _workspace(None, nbytes, gout.device)
    dpre = torch.empty_like(gates)
    _check(lib().vfr_bilstm_train_backward_f32(gout.data_ptr(), gates.data_ptr(), cs.data_ptr(), whhT_f.data_ptr(), whhT_b.data_ptr(),
                                               B, T, H, dpre.data_ptr(), wsb.data_ptr(), nbytes, _stream()),
           "vfr_bilstm_train_backward_f32")
    return dpre


def ranking_loss_forward(posit, intra, inter, lang, maskp, maskn, n_samples: int, b: float, lamb: float, eps: float = 1e-6):
    """-> (loss [1] f32, workspace) ; the workspace (row distances, per-sample terms) feeds ranking_loss_backward."""
    posit, intra, inter, lang = (_dev(x, torch.float32, n) for x, n in ((posit, "posit"), (intra, "intra"), (inter, "inter"),
                                                                         (lang, "lang")))
    maskp, maskn = _dev(maskp, torch.int64, "maskp"), _dev(maskn, torch.int64, "maskn")
    P, Nn, D = posit.shape[0], intra.shape[0], posit.shape[1]
    nbytes = lib().vfr_ranking_loss_workspace_bytes(P, Nn, n_samples)
    ws = _workspace(None, nbytes, posit.device)
    loss = torch.empty((1,), dtype=torch.float32, device=posit.device)
    _check(lib().vfr_ranking_loss_f32(posit.data_ptr(), intra.data_ptr(), inter.data_ptr(), lang.data_ptr(), maskp.data_ptr(),
                                      maskn.data_ptr(), P, Nn, n_samples, D, b, lamb, eps, loss.data_ptr(), ws.data_ptr(),
                                      nbytes, _stream()), "vfr_ranking_loss_f32")
    return loss, ws


def ranking_loss_backward(posit, intra, inter, lang, maskp, maskn, n_samples: int, lamb: float, grad_loss, ws,
                          eps: float = 1e-6):
    posit, intra, inter, lang = (_dev(x, torch.float32, n) for x, n in ((posit, "posit"), (intra, "intra"), (inter, "inter"),
                                                                         (lang, "lang")))
    maskp, maskn = _dev(maskp, torch.int64, "maskp"), _dev(maskn, torch.int64, "maskn")
    g = _dev(grad_loss.reshape(1), torch.float32, "grad_loss")
    outs = [torch.empty_like(x) for x in (posit, intra, inter, lang)]
    _check(lib().vfr_ranking_loss_grad_f32(posit.data_ptr(), intra.data_ptr(), inter.data_ptr(), lang.data_ptr(),
                                           maskp.data_ptr(), maskn.data_ptr(), posit.shape[0], intra.shape[0], n_samples,
                                           posit.shape[1], lamb, eps, g.data_ptr(), ws.data_ptr(), *[o.data_ptr() for o in outs],
                                           _stream()), "vfr_ranking_loss_grad_f32")
    return outs


# ------------------------------------------------------------------------------------------------
# the training driver (csrc/optim.hip): triplet batches from the resident bank, the fused Adam step and gradient sums of squares
ADAM_MAX_TENSORS = 32                      # include/vfr.h VFR_ADAM_MAX_TENSORS


def triplet_gather(seg, ctx, clip_off, tokens, plan: np.ndarray):
    """One batch of sampler triplets -> (posit, intra, inter, lang, maskp, maskn) on the device (``custom_collate``'s dict,
    ``model/data.py:346-356``).  ``plan`` [S, 7] int32 host array: video_pos, video_neg, start_t, end_t, start_tn, end_tn,
    token row.  Row counts are prefix sums of the spans, taken here on the host."""
    seg = _dev(seg, torch.float32, "seg")
    ctx = _dev(ctx, torch.float32, "ctx")
    clip_off = _dev(clip_off, torch.int32, "clip_off")
    tokens = _dev(tokens, torch.int64, "tokens")
    if seg.dim() != 2 or ctx.dim() != 2 or seg.shape[1] != ctx.shape[1] or clip_off.numel() != ctx.shape[0] + 1 or tokens.dim() != 2:
        raise RuntimeError("triplet_gather: expected seg [sum n, F], ctx [Nv, F], clip_off [Nv+1], tokens [A, Tq]")
    plan = np.ascontiguousarray(plan, dtype=np.int32)
    if plan.ndim != 2 or plan.shape[1] != 7:
        raise RuntimeError("triplet_gather: plan must be [S, 7] int32")
    S, F, Tq = plan.shape[0], seg.shape[1], tokens.shape[1]
    P = int((plan[:, 3] - plan[:, 2] + 1).sum())
    Nn = int((plan[:, 5] - plan[:, 4] + 1).sum())
    dev = seg.device
    posit = torch.empty((P, 2 * F + 2), dtype=torch.float32, device=dev)
    inter = torch.empty((P, 2 * F + 2), dtype=torch.float32, device=dev)
    intra = torch.empty((Nn, 2 * F + 2), dtype=torch.float32, device=dev)
    maskp = torch.empty(P, dtype=torch.int64, device=dev)
    maskn = torch.empty(Nn, dtype=torch.int64, device=dev)
    lang = torch.empty((S, Tq), dtype=torch.int64, device=dev)
    _check(lib().vfr_triplet_gather_f32(seg.data_ptr(), ctx.data_ptr(), clip_off.data_ptr(), ctx.shape[0], F, tokens.data_ptr(),
                                        tokens.shape[0], Tq, plan.ctypes.data, S, P, Nn, posit.data_ptr(), intra.data_ptr(),
                                        inter.data_ptr(), maskp.data_ptr(), maskn.data_ptr(), lang.data_ptr(), _stream()),
           "vfr_triplet_gather_f32")
    return posit, intra, inter, lang, maskp, maskn


def _ptr_array(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


def _flat_f32(ts, name):
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: expected tensors on the ROCm device (no CPU fallback in the HIP path)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: expected torch.float32, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name}: tensors must be contiguous (they are updated in place)")


_ADAM_WS = {}                              # device -> zero-initialised workspace (every call leaves it zero again)


def _adam_workspace(numel, device) -> torch.Tensor:
    arr = (ctypes.c_int64 * len(numel))(*numel)
    need = int(lib().vfr_adam_workspace_bytes(arr, len(numel)))
    ws = _ADAM_WS.get(device)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(max(need, 1 << 16), dtype=torch.uint8, device=device)
        _ADAM_WS[device] = ws
    return ws


def adam_step(params, grads, exp_avgs, exp_avg_sqs, coefs, sumsq: torch.Tensor | None = None) -> torch.Tensor:
    """In-place fused Adam step over the given tensors (include/vfr.h vfr_adam_step_f32), one launch per
    ``ADAM_MAX_TENSORS``; ``coefs`` [n][7] = (wd, 1-beta1, beta2, 1-beta2, eps, -step_size, 1/bc2_sqrt) as fp32.
    -> sums of squares of the raw gradients [n] f32 on the device."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(coefs) == n):
        raise RuntimeError("adam_step: params, grads, exp_avgs, exp_avg_sqs and coefs must have the same length")
    for name, ts in (("params", params), ("grads", grads), ("exp_avgs", exp_avgs), ("exp_avg_sqs", exp_avg_sqs)):
        _flat_f32(ts, f"adam_step: {name}")
    for i in range(n):
        if not (params[i].shape == grads[i].shape == exp_avgs[i].shape == exp_avg_sqs[i].shape):
            raise RuntimeError(f"adam_step: tensor {i}: shapes differ")
    if n == 0:
        return torch.zeros(0, dtype=torch.float32)
    dev = params[0].device
    if sumsq is None:
        sumsq = torch.empty(n, dtype=torch.float32, device=dev)
    coefs = np.ascontiguousarray(coefs, dtype=np.float32).reshape(n, 7)
    for a in range(0, n, ADAM_MAX_TENSORS):
        b = min(n, a + ADAM_MAX_TENSORS)
        numel = [t.numel() for t in params[a:b]]
        ws = _adam_workspace(numel, dev)
        _check(lib().vfr_adam_step_f32(b - a, _ptr_array(params[a:b]), _ptr_array(grads[a:b]), _ptr_array(exp_avgs[a:b]),
                                       _ptr_array(exp_avg_sqs[a:b]), (ctypes.c_int64 * (b - a))(*numel),
                                       coefs[a:b].ctypes.data, sumsq[a:].data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "vfr_adam_step_f32")
    return sumsq


def grad_sumsq(grads) -> torch.Tensor:
    """Sums of squares of the given gradients [n] f32 on the device (include/vfr.h vfr_grad_sumsq_f32), one launch per
    ``ADAM_MAX_TENSORS`` tensors; deterministic."""
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
    _flat_f32(grads, "grad_sumsq")
    n = len(grads)
    if n == 0:
        return torch.zeros(0, dtype=torch.float32)
    dev = grads[0].device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    for a in range(0, n, ADAM_MAX_TENSORS):
        b = min(n, a + ADAM_MAX_TENSORS)
        numel = [t.numel() for t in grads[a:b]]
        ws = _adam_workspace(numel, dev)
        _check(lib().vfr_grad_sumsq_f32(b - a, _ptr_array(grads[a:b]), (ctypes.c_int64 * (b - a))(*numel), out[a:].data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "vfr_grad_sumsq_f32")
    return out
