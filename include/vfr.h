/*
 * vfr.h -- C ABI of libvfr.so: the MI355X (gfx950) cross-modal scoring hot path of
 * video-fragments-retrieval.  Plain pointers and sizes only; no torch / C++ types.
 *
 * The reference has no FFI layer: its operator surface is Python (nn.Module calls and two
 * evaluate() functions) and all arithmetic runs in implicit torch / torchvision / numpy vendor
 * kernels.  Each entry point below replaces one such implicit call site; the citation names the
 * reference file:line (relative to the reference repo root) whose arithmetic it takes over.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; row-major, fp32 unless typed
 *   - the caller owns all memory, workspaces included (vfr_*_workspace_bytes tells how much);
 *     the library never allocates or frees device memory and keeps no pointer after return
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no entry point synchronises with the host
 *   - return 0 on success, a negative VFR_E* code otherwise; vfr_last_error() gives the message
 *     (thread-local).  No exception, exit or abort crosses the boundary.
 *   - no model state: weights are passed per call (no hidden model handle), so load_state_dict()/.to()
 *     on the Python side keep working.  Compute entry points are re-entrant: any number of host threads
 *     may call them concurrently (each on its own stream or sharing one).  The process-wide state is:
 *     the tuning options (vfr_set_option: PROCESS-GLOBAL atomic ints, read at the start of a call -- a
 *     knob for tests and sweeps, every setting gives the same bits; do NOT change one while calls are in
 *     flight on other threads: a call may then see the old value for one of its launches and the new
 *     one for the next, which is harmless for the results but not a per-call setting), the fault word
 *     registered with vfr_set_fault_word, and the launch-site profiler (off by default; event pairs
 *     are owned by the calling scope, the totals are folded under a mutex)
 *   - numerics: every contraction is one k-ascending fp32 fma chain (what the fp32 MFMAs
 *     compute), so results are bit-identical to oracle/vfr_oracle.c on any input
 */
#ifndef VFR_H
#define VFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library itself is built with -fvisibility=hidden */
#endif

#define VFR_OK 0
#define VFR_EINVAL (-1)       /* null pointer, negative size, misaligned buffer                 */
#define VFR_EUNSUPPORTED (-2) /* shape outside what the kernels are built for (message says)    */
#define VFR_EHIP (-3)         /* a HIP runtime call failed; hipGetErrorString in the message    */
#define VFR_EWORKSPACE (-4)   /* workspace smaller than vfr_*_workspace_bytes                   */

typedef void *vfr_stream_t; /* hipStream_t */

int vfr_version(void);
const char *vfr_last_error(void);

/* ---- a3  clip pooling: CustomDataset.load_video_features, model/data.py:163-181 -------------
 * frames [T,F] -> seg [ceil(T/seg_len), F], ctx [F].  mode 0 = avg (np.mean), 1 = max (np.max);
 * pooled row / (||pooled row||_2 + 1e-5).  F must be a multiple of 4.                           */
int vfr_segment_pool_norm_f32(const float *frames, int T, int F, int seg_len, int mode, float *seg, float *ctx,
                              vfr_stream_t stream);
/* many videos at once: frames [sum T, F], frame_offsets [Nv+1] (int32, device),
 * seg_offsets [Nv+1] = prefix sums of ceil(T_v/seg_len), total_segments = its last entry (host
 * copy); seg [total_segments, F], ctx [Nv, F]                                                   */
int vfr_segment_pool_norm_batch_f32(const float *frames, const int32_t *frame_offsets, const int32_t *seg_offsets,
                                    int Nv, int total_segments, int F, int seg_len, int mode, float *seg,
                                    float *ctx, vfr_stream_t stream);

/* ---- a4 + a7  clip encoder: make_visual_features model/data.py:204-213 + CALModel visual
 * branch model/models.py:21-26,55-56.  Row t of video v is [seg_t | ctx_v | t/n | (t+1)/n] x
 * W1[hid, 2F+2] -> ReLU -> W2[D, hid]; the 2F+2 concat is never materialised and the context
 * half of W1 is applied once per video.  clip_offsets [Nv+1] int32; out [total_clips, D].       */
size_t vfr_visual_mlp_workspace_bytes(int total_clips, int Nv, int F, int hid);
int vfr_visual_mlp_f32(const float *seg, const float *ctx, const int32_t *clip_offsets, int Nv, int total_clips,
                       int F, const float *W1, const float *b1, const float *W2, const float *b2, int hid, int D,
                       float *out, void *workspace, size_t workspace_bytes, vfr_stream_t stream);

/* ---- generic Linear (+ReLU): nn.Linear at model/models.py:31,59 (BERT branch) and the VGG
 * classifier[0], classifier[3] (get_rgb_features.py:126).  out[M,N] = A[M,K] W[N,K]^T + b      */
int vfr_linear_f32(const float *A, int64_t M, int K, const float *W, const float *b, int N, int relu, float *out,
                   vfr_stream_t stream);

/* ---- a8  query encoder: CALModel GloVe branch model/models.py:61-66 (+ init_hidden :50-52):
 * Embedding gather [-> unit-norm x learnable length when len_tab != NULL, :62-64] -> BiLSTM(H),
 * h0 = c0 = 0, all T steps including pads -> h_n [fwd|bwd] -> Linear(2H, D).
 * tokens [B,T] int64; emb [vocab,E]; W_ih [4H,E], W_hh [4H,H], b_* [4H] (gate order i,f,g,o)
 * for the forward (_f) and reverse (_b) directions; Wfc [D,2H]; out [B,D].
 * The workspace also holds the per-vocabulary input-projection table (emb x W_ih^T, both directions) that the
 * recurrent steps start their gate chains from when vocab <= 32768 -- hence `vocab` in its size.
 * B <= 2 at a shape whose 32-column weight slices fit a CU's LDS (E + H <= 1170, H <= 1024, 2 * ceil(H / 8) <= CUs), and
 * 3 <= B <= 32 at E = 100, H = 1000 (weights resident in registers as MFMA fragments): the
 * whole sequence and the Linear run as ONE launch of 2 * ceil(H / 8) workgroups that wait on each other's h every step, so
 * ALL of them must be resident: do not run two such calls concurrently on one device (two streams / processes can starve
 * each other of CUs -- the host checks the grid against the device's CU count, it cannot see what else is running).  The
 * waits are bounded, and a give-up is REPAIRED inside the same call: behind every such launch a rescue kernel is enqueued
 * that returns at once in the normal case and otherwise re-encodes the batch without any cross-workgroup dependency (one
 * workgroup per query; milliseconds) -- `out` never holds NaN from a give-up and the return code stays VFR_OK because the
 * result is right.  The event is reported through the fault word: vfr_set_fault_word / vfr_poll_faults below.
 * vfr_set_option("lstm_persist", 0) selects one launch per step instead.                                            */
size_t vfr_bilstm_workspace_bytes(int64_t B, int T, int E, int H, int vocab);
/* Tests only: byte offset, inside that workspace, of two uint32 counters [forward, reverse].  With option "lstm_live_blocks"
 * bit 1 set, the fused MFMA steps of a call add the (16-row x 16-unit) blocks they issued matrix work for; the call zeroes
 * them first.  No output is computed from them.                                                                       */
size_t vfr_bilstm_debug_offset(int64_t B, int T, int E, int H, int vocab);
/* Introspection (no device needed): the form the fused BiLSTM steps of `rows` GEMM rows (queries + 1) take under the current
 * options on a device of `cus` compute units.  *one_launch: 1 = the one-launch kernel is selected ("lstm_multi"), 0 = one launch
 * per step; *tile: rows per tile as "lstm_tile" numbers them (1 = 64, 2 = 128, 3 = 32); *slots: the one-launch grid (0 otherwise).
 * A selected one-launch form still falls back to the per-step launches when its grid is not resident at once.
 * CONSTRAINT of the one-launch form (the default from 2500 rows on): its workgroups wait for each other, so run ONE such encode
 * per device at a time.  Two concurrent large vfr_bilstm_final_f32 calls, or another process filling the device, can leave each
 * with part of its grid resident; the waits are bounded (seconds), the batch is then re-encoded by the rescue kernel and the
 * event reported through the fault word -- results stay right, the call is slow.  "lstm_multi" 0 removes the constraint.  */
int vfr_lstm_plan(int64_t rows, int H, int T, int cus, int *one_launch, int *tile, int64_t *slots);
int vfr_bilstm_final_f32(const int64_t *tokens, int64_t B, int T, const float *emb, int vocab, const float *len_tab,
                         const float *Wih_f, const float *Whh_f, const float *bih_f, const float *bhh_f,
                         const float *Wih_b, const float *Whh_b, const float *bih_b, const float *bhh_b, int E,
                         int H, const float *Wfc, const float *bfc, int D, float *out, void *workspace,
                         size_t workspace_bytes, vfr_stream_t stream);

/* Fault word: kernels cannot return codes, and no entry point synchronises.  A caller that wants to HEAR about device-side
 * recoveries registers one device-accessible HOST word (page-locked: hipHostMalloc / torch pin_memory; process-wide, any
 * device; NULL unregisters; it must outlive every call made while registered).  Kernels raise bits in it with system-scope
 * atomics; vfr_poll_faults() (host only, no synchronisation: poll after the caller's own sync point) returns and clears the
 * bits raised since the last poll and leaves the explanation in vfr_last_error().
 *   VFR_FAULT_SEQ_RESCUED  a single-launch sequence encoder gave up and the batch was re-encoded by the rescue kernel     */
#define VFR_FAULT_SEQ_RESCUED 1
int vfr_set_fault_word(uint32_t *word_host);
int vfr_poll_faults(void);

/* ---- a10  scoring core: model/evaluate.py:49-58 (same code evaluate_single.py:48-53,
 * main.py:148-157).  dist[c] = ||(V[c] - q) + eps||_2 (F.pairwise_distance), score of moment
 * (s,e) = mean(dist[s..e]); moments of a video in utils.generate_moments order
 * (model/utils.py:71-75), videos concatenated in clip_offsets order.
 * moment_offsets [Nv+1] int64 = prefix sums of n_v(n_v+1)/2.                                    */
/* dense: scores [Nq, moment_offsets[Nv]]                                                        */
int vfr_score_moments_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                          const int64_t *moment_offsets, int Nv, int max_clips, int64_t total_moments, int D,
                          float eps, float *scores, vfr_stream_t stream);
/* each query against ONE video own[q] (evaluate_single.py:48-53): scores [Nq, Mmax], tail +inf  */
int vfr_score_own_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int32_t *own,
                      int max_clips, int D, float eps, int Mmax, float *scores, vfr_stream_t stream);

/* ---- a12  ranking: np.argsort over all moments of all videos + R@k / MR, evaluate.py:67-80.
 * Fused scoring + selection: never materialises the [Nq, sum M] score matrix.  Order is
 * (distance, global moment id) ascending (the stable argsort).
 *   k > 0 : out_dist [Nq,k] / out_idx [Nq,k] (int64 global moment ids) = the k best, padded
 *           with (+inf, -1) when fewer than k moments exist
 *   num_rank > 0 (<= 4) : rank_dist / rank_idx / count_lt are [num_rank, Nq]; count_lt[r][q] (int64)
 *           += number of moments that sort strictly before (rank_dist[r][q], rank_idx[r][q]) --
 *           evaluate.py:77's MR when that pair is the best ground-truth-positive moment of IoU
 *           threshold r.  Counts are ADDED (zero the array first, or chain shards).
 * thr_seed (nullable, [Nq] packed keys (fp32 bits of distance << 32 | id)): an upper bound on each query's k-th best
 *           key, known to the caller (the merged sample of all shards, 8e).  Only keys below it are collected and the
 *           internal sample pre-pass is skipped; results are exact for any valid bound.
 * id_base is added to every emitted / compared moment id (shard offset for multi-GPU, 8e).
 * min_clips / max_clips: smallest / largest clip count in the bank (min_clips 0 = unknown; when
 * min == max the kernels drop their per-video length guards).
 * Limits: max_clips <= 64, k <= 448, id_base + total moments < 2^32.                           */
size_t vfr_score_topk_workspace_bytes(int64_t Nq, int Nv, int k);
int vfr_score_topk_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                       const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips, int D,
                       float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx, int num_rank,
                       const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, const int64_t *thr_seed,
                       void *workspace, size_t workspace_bytes, vfr_stream_t stream);
/* The same pass with the clip distances taken from the GEMM form |v|^2 + |q|^2 - 2 v.q on the matrix cores
 * (model/evaluate.py:53-58 as north_star's "MFMA batched query x clip GEMM"; csrc/score_mfma.h):
 *   dtype VFR_MFMA_F32  fp32 MFMA pre-filter with a rigorous error margin; whatever the margin cannot decide is
 *                       re-scored with the exact chain, so every output is BIT-IDENTICAL to vfr_score_topk_f32
 *                       (shapes the pre-filter is not built for are simply handed to vfr_score_topk_f32; 1-8 queries -- a
 *                       serving request -- take a path of their own with lanes = clips / videos, equally exact);
 *   dtype VFR_MFMA_BF16 bf16 operands, fp32 accumulate: count_lt from the approximate
 *                       distances, top-k = exact re-rank of the k + 28 best approximate candidates.  Needs D = 100,
 *                       max_clips <= 21, num_rank in {0, 2}, k <= 253; VFR_EUNSUPPORTED otherwise.
 * Arguments as vfr_score_topk_f32.
 * dtype | VFR_MFMA_BANK_READY: the caller states that `workspace` was last used by a pre-filter call (one for which
 * vfr_score_topk_mfma_prefilter returned 1) on this bank and has not been written since: the bank-side products (mean,
 * centred rows, norms; they sit at the front of the workspace at offsets that depend on total_clips alone) are reused
 * instead of recomputed.  For serving many query batches against one resident bank (~0.1 ms per call at 210 000 clips).
 * CHECKED ON THE DEVICE: every call hashes all of V and the clip offsets (64-bit position-weighted sum, ~20 us at 84 MB)
 * and compares {hash, total_clips, Nv, D, eps, bf16 copy present} with the signature stored next to the products; on any
 * difference the products are recomputed inside the same call (the pre-pass kernels are always enqueued and return at once
 * when the signature matches -- no host decision, no synchronisation).  A bank rewritten through a raw pointer therefore
 * costs a recomputation, never a wrong result.  (The hash is a position-weighted 64-bit sum: it catches accidental rewrites,
 * it is not collision-resistant against an adversary who chooses the bank.)  NOT checked: that the product region of `workspace` itself is intact --
 * that part stays the caller's statement (do not set the flag for a workspace other code has used in between).
 * vfr_score_topk_mfma_prefilter: 1 if a call with these shapes runs the pre-filter (and therefore leaves the bank-side
 * products in its workspace), 0 if it is handed to the exact kernels.                            */
#define VFR_MFMA_F32 0
#define VFR_MFMA_BF16 1
#define VFR_MFMA_BANK_READY 0x100
size_t vfr_score_topk_mfma_workspace_bytes(int64_t Nq, int Nv, int total_clips, int k);
int vfr_score_topk_mfma_prefilter(int64_t Nq, int Nv, int total_clips, int max_clips, int D, int num_rank, int k, int dtype);
int vfr_score_topk_mfma(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                        const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips, int D,
                        float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx, int num_rank,
                        const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, const int64_t *thr_seed,
                        int dtype, void *workspace, size_t workspace_bytes, vfr_stream_t stream);
/* measurement hook (SYNCHRONISES the stream): what the last f32 call on `workspace` (same Nq, Nv, total_clips, k) left to
 * the exact kernels.  stats_host[4] = {query groups of 64, groups handed to the exact fallback, (query, video) pairs
 * re-scored exactly, pairs the (video, group) bitmap can mark = Nq * Nv}.                                             */
int vfr_score_topk_mfma_stats(const void *workspace, int64_t Nq, int Nv, int total_clips, int k, int64_t *stats_host,
                              vfr_stream_t stream);
/* ---- video-level retrieval: which VIDEOS match a query.  Keys as vfr_score_topk_f32 ((distance, global moment id) ascending).
 * The best key of a video is the smallest key among its moments (its first moment in the moment ranking; the WHOLE triangle
 * decides it: an fp32 mean of several clips can round below the video's smallest clip distance).
 *   k > 0 : out_dist [Nq,k] / out_idx [Nq,k] = the k smallest best keys over the bank's videos, as (distance, global moment id of
 *           the video's best moment), i.e. the moment ranking reduced to the first moment of each video; video order is therefore
 *           (best distance, video index).  Padded with (+inf, -1) when the bank has fewer than k videos.  k = 0: counts only.
 *   own_dist / own_idx / video_count_lt [Nq] (nullable, together): video_count_lt[q] (int64) += number of this bank's videos
 *           whose best key sorts strictly before (own_dist[q], own_idx[q]) -- the 0-based video rank of the query's own video
 *           when that pair is its best key.  ADDED, so shards chain like count_lt.
 *   dtype VFR_MFMA_F32    D = 100 and <= 21 clips per video (banks of at least score_mfma_min videos): per-(query, video) bounds
 *                         of the smallest clip distance from the fp32 MFMA GEMM form with a rigorous margin exclude or count
 *                         almost every video; the rest get their whole triangle with the canonical chain.  BIT-IDENTICAL to
 *                         VFR_SCORE_EXACT; other shapes take the exact path.  | VFR_MFMA_BANK_READY: as vfr_score_topk_mfma (the
 *                         bank-side products sit at the same workspace offsets and are checked by the same device hash).
 *   dtype VFR_SCORE_EXACT every video's triangle with the canonical chain (any shape).
 * Other arguments and limits as vfr_score_topk_f32 (max_clips <= 64, k <= 448, id_base + total moments < 2^32).
 * vfr_score_video_topk_stats (measurement hook, SYNCHRONISES the stream): what the last VFR_MFMA_F32 fast-path call on `workspace`
 * (same Nq, Nv, total_clips) re-scored exactly: stats_host [Nq, 2] = {videos given a triangle, of them rank-undecided}. */
#define VFR_SCORE_EXACT 2
size_t vfr_score_video_topk_workspace_bytes(int64_t Nq, int Nv, int total_clips, int k);
int vfr_score_video_topk_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                             const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips,
                             int D, float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx,
                             const float *own_dist, const int64_t *own_idx, int64_t *video_count_lt,
                             int dtype, void *workspace, size_t workspace_bytes, vfr_stream_t stream);
int vfr_score_video_topk_stats(const void *workspace, int64_t Nq, int Nv, int total_clips, int64_t *stats_host,
                               vfr_stream_t stream);
/* ---- diversified moment retrieval: the k best MOMENTS, at most per_video per video and no two of a video overlapping more
 * than nms_iou.  Keys, ids and scores as vfr_score_topk_f32 ((distance, global moment id) ascending).  Per query and video, the
 * video's moments are taken in key order and accepted greedily: a moment is suppressed when its IoU (utils.get_iou on the
 * inclusive clip spans, float64) with an already accepted moment of the same video is > nms_iou; at most per_video are
 * accepted (0 = no cap, values >= k act as k).  nms_iou >= 1 suppresses nothing, nms_iou = 0 keeps disjoint spans only.
 *   out_dist [Nq,k] / out_idx [Nq,k] = the k smallest accepted keys over the bank, padded with (+inf, -1).
 *   per_video = 1 gives exactly vfr_score_video_topk_f32's (dist, idx); per_video in {0, >= k} with nms_iou >= 1 gives exactly
 *   vfr_score_topk_f32's top-k.  Every listed moment belongs to one of the query's k best videos, and a video never spans
 *   shards: per-shard lists merge with vfr_topk_merge_f32.
 *   dtype VFR_MFMA_F32 (| VFR_MFMA_BANK_READY) or VFR_SCORE_EXACT, as vfr_score_video_topk_f32 (its launch sequence finds the
 *   k best videos; the workspace front is the same, so BANK_READY and the device hash work alike); BIT-IDENTICAL outputs.
 * Limits as vfr_score_video_topk_f32 (k <= 448, max_clips <= 64, id_base + total moments < 2^32), Nq * k < 2^31; per_video >= 0;
 * nms_iou >= 0 and not NaN.  Bad arguments: VFR_EINVAL.
 * vfr_nms_inter_table (host only, no GPU): min_inter[0..max_len] = for each union length u the smallest integer intersection
 * with (double)inter / u > nms_iou (u + 1 when none; entry 0 is 1) -- the exact, integer form of the IoU test the kernels use. */
size_t vfr_score_moment_nms_workspace_bytes(int64_t Nq, int Nv, int total_clips, int k, int per_video);
int vfr_score_moment_nms_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                             const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips,
                             int D, float eps, int64_t id_base, int k, int per_video, double nms_iou,
                             float *out_dist, int64_t *out_idx, int dtype, void *workspace, size_t workspace_bytes,
                             vfr_stream_t stream);
int vfr_nms_inter_table(double nms_iou, int max_len, int32_t *min_inter);
/* ---- candidate-restricted retrieval: search only the videos each query lists ("these videos": a per-user library or a metadata
 * filter, a first-stage shortlist, the candidate-pool evaluation protocol).  Keys, ids and scores as vfr_score_topk_f32.
 * cand_off [Nq+1] int64 / cand_vid [nnz] int32: CSR lists of CORPUS-GLOBAL video indices, strictly ascending per query;
 * vid_base = global index of the bank's first video: entries outside [vid_base, vid_base + Nv) are skipped, so every shard takes
 * the same lists (a video never spans shards).  max_list (host) = the longest list: it sizes the grid without a synchronisation.
 *   level VFR_SUBSET_MOMENTS: out_dist / out_idx [Nq,k] = the k smallest keys over all moments of the query's listed videos of this
 *           bank, padded with (+inf, -1); count_lt[r][q] += number of those moments whose key sorts strictly before
 *           (rank_dist[r][q], rank_idx[r][q]), as vfr_score_topk_f32 counts.
 *   level VFR_SUBSET_VIDEOS: out_* = the k smallest BEST keys of the listed videos, as (best distance, id of the best moment);
 *           count_lt[r][q] += number of listed videos whose best key sorts strictly before the rank key, as video_count_lt.
 *   Every list = every video of the bank gives exactly vfr_score_topk_f32 (moments) and vfr_score_video_topk_f32 (videos).
 * num_rank <= 4 ([num_rank, Nq] rank_dist / rank_idx / count_lt, ADDED); k = 0 with counts only is allowed.  An empty list gives
 * padding and adds nothing.  Cost scales with the listed (query, video) pairs, not with Nq x Nv; the result is exact (the
 * canonical chain and the whole triangle of every listed video).
 * bad (nullable, device int): set to 1 when a list is not strictly ascending, holds an index < 0, is longer than max_list, or
 * cand_off is not a non-decreasing run from 0 to nnz (results for such lists are unspecified; nothing is read or written out of
 * bounds).  Limits as vfr_score_video_topk_f32 (k <= 448, max_clips <= 64, id_base + total moments < 2^32), Nq * k < 2^31,
 * nnz < 2^31.  Bad host-side arguments: VFR_EINVAL before anything is enqueued.
 * vfr_score_subset_workspace_bytes: O((nnz / 64 + Nq) k) for moments, O(nnz) for videos (0 for a bad argument).        */
#define VFR_SUBSET_MOMENTS 0
#define VFR_SUBSET_VIDEOS 1
size_t vfr_score_subset_workspace_bytes(int64_t Nq, int64_t nnz, int64_t max_list, int k, int level);
int vfr_score_subset_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                         const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips, int D,
                         float eps, int64_t id_base, int64_t vid_base, const int64_t *cand_off, const int32_t *cand_vid,
                         int64_t nnz, int64_t max_list, int level, int k, float *out_dist, int64_t *out_idx, int num_rank,
                         const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, int *bad, void *workspace,
                         size_t workspace_bytes, vfr_stream_t stream);
/* ---- sentence retrieval for moments (the reverse direction): which SENTENCES of a bank describe a probe moment best, and where
 * a given sentence ranks among them -- the moment->sentence half of a two-way retrieval report, "describe / tag this moment" by
 * nearest stored captions, the sentence-side hard-negative search.  S [Ns, D] = the sentence bank (the rows the other entry points
 * take as queries); probes int32 [Nm, 3] = (video, start_t, end_t): CORPUS-GLOBAL video index and the inclusive clip span in
 * utils.generate_moments units.  Probes need not be sorted, may repeat and may share videos; outputs are in the caller's order.
 *   score(m, j) = (dist[s] + .. + dist[e]) / (e - s + 1), dist[c] = ||(V[c] - S[j]) + eps||_2: the canonical chain, BIT-IDENTICAL
 *           to what vfr_score_moments_f32 writes at [j, moment id of m].  key = (fp32 bits of the score << 32) | (sent_base + j),
 *           order (distance, sentence id) ascending.
 *   k > 0 : out_dist / out_idx [Nm,k] = the k smallest keys over the bank's sentences as (distance, sent_base + j), padded with
 *           (+inf, -1) when Ns < k.  k = 0 with counts only is allowed.
 *   num_rank > 0 (<= 4): rank_dist / rank_idx / count_lt are [num_rank, Nm]; count_lt[r][m] (int64) += number of sentences of this
 *           bank whose key sorts strictly before (rank_dist[r][m], rank_idx[r][m]).  ADDED, so sentence-bank shards chain, and their
 *           lists merge with vfr_topk_merge_f32 (sent_base = the shard's first sentence id).
 *   vid_base = global index of the clip bank's first video.  A probe whose video lies outside [vid_base, vid_base + Nv) belongs to
 *           another shard and is skipped (padding, nothing added): every shard of a video-sharded bank takes the same probes.
 *   bad (nullable, device int): set to 1 for a probe with video < 0, start_t < 0, end_t < start_t (on any shard) or end_t >= the
 *           video's clip count (on the shard that holds the video); such a probe gives padding and adds nothing; nothing is read
 *           or written out of bounds.
 * Consecutive probes that name the same video share their clip distances (each (clip, sentence) distance is computed once per
 * group of 8 probes; the sum order s -> e is fixed, so the bits do not depend on it): sort the probes by video for speed.
 * Any D (D = 100 with 16-byte aligned S and V takes the register-resident fast path).
 * Limits: max_clips <= 64, k <= 448, sent_base + Ns < 2^32, Nm * k < 2^31.  Bad host-side arguments: VFR_EINVAL before anything is
 * enqueued.
 * vfr_score_sentences_workspace_bytes = 256 + 8 k Nm C, C = min(ceil(2048 / ceil(Nm / 8)), ceil(Ns / 64), 256) >= 1 = the bound on
 * the chunks the sentence axis is cut into (enough to fill the device when Nm is small): O(Nm k), no Nm x Ns term (0 for a bad
 * argument).                                                                                                             */
size_t vfr_score_sentences_workspace_bytes(int64_t Nm, int64_t Ns, int k);
int vfr_score_sentences_f32(const float *S, int64_t Ns, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                            int max_clips, int D, float eps, const int32_t *probes, int64_t Nm, int64_t vid_base,
                            int64_t sent_base, int k, float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist,
                            const int64_t *rank_idx, int64_t *count_lt, int *bad, void *workspace, size_t workspace_bytes,
                            vfr_stream_t stream);
/* ---- video-to-sentence retrieval (the reverse direction at the video level): which SENTENCES of a bank describe a whole VIDEO, and
 * where its own sentences rank among them -- the video->text half of a two-way retrieval table, "caption / tag this video" from
 * stored sentences.  S [Ns, D] = the sentence bank; videos int32 [Np] = CORPUS-GLOBAL video indices: they need not be sorted and
 * may repeat; outputs are in the caller's order.
 *   score(p, j) = b(j, v_p), the quantity of vfr_score_video_topk_f32 and vfr_score_paragraph_pairs_f32: the smallest moment score
 *           over the WHOLE triangle of video v_p for sentence j, every moment score the canonical chain (k-ascending fp32 fma chain
 *           of ((V - S) + eps)^2, IEEE sqrt, sequential fp32 sum s -> e, one IEEE division by (float)(e - s + 1)).  BIT-IDENTICAL to
 *           the minimum over video v_p's block of row j of vfr_score_moments_f32(S, ..).  The moment that attains it, m(j, v) (the
 *           smallest (distance, moment id) key, as in the video top-k), is NOT returned here: vfr_score_paragraph_pairs_f32 with
 *           groups of length 1 gives it for named (sentence, video) pairs.
 *           key = (fp32 bits of the score << 32) | (sent_base + j), order (distance, sentence id) ascending.
 *   k > 0 : out_dist / out_idx [Np,k] = the k smallest keys over the bank's sentences as (distance, sent_base + j), padded with
 *           (+inf, -1) when Ns < k.  k = 0 with counts only is allowed.
 *   num_rank > 0 (<= 4): rank_dist / rank_idx / count_lt are [num_rank, Np]; count_lt[r][p] (int64) += number of sentences of this
 *           bank whose key sorts strictly before (rank_dist[r][p], rank_idx[r][p]).  ADDED, so sentence-bank shards chain through
 *           sent_base (the shard's first sentence id), and their lists merge with vfr_topk_merge_f32.
 *   vid_base = global index of the clip bank's first video.  A probe whose video lies outside [vid_base, vid_base + Nv) belongs to
 *           another shard and is skipped (padding, nothing added): every shard of a video-sharded bank takes the same probes.  A
 *           video without clips gives padding, adds nothing and is not bad.
 *   bad (nullable, device int): set to 1 for a probe with video < 0 (on any shard); such a probe gives padding and adds nothing.
 *           Nothing is read before it is checked; nothing is read or written out of bounds.
 * Exact arithmetic only: every (probe, sentence) pair gets its whole triangle.  An MFMA bounds pre-filter as the sentence->video
 * direction has is not built for this one.  Any D (D = 100 with 16-byte aligned S and V takes the register-resident fast path).
 * Np = 0, and k = 0 without rank keys and without bad, return without a launch.
 * Limits: max_clips <= 64, k <= 448, sent_base + Ns < 2^32, Np * k < 2^31.  Bad host-side arguments: VFR_EINVAL before anything is
 * enqueued; a short workspace: VFR_EWORKSPACE.
 * vfr_score_video_sentences_workspace_bytes = 256 + 8 k Np C, C = min(ceil(2048 / Np), ceil(Ns / 64), 256) >= 1 = the bound on the
 * chunks the sentence axis is cut into: O(Np k), no Np x Ns term (0 for a bad argument).                                  */
size_t vfr_score_video_sentences_workspace_bytes(int64_t Np, int64_t Ns, int k);
int vfr_score_video_sentences_f32(const float *S, int64_t Ns, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                                  int max_clips, int D, float eps, const int32_t *videos, int64_t Np, int64_t vid_base,
                                  int64_t sent_base, int k, float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist,
                                  const int64_t *rank_idx, int64_t *count_lt, int *bad, void *workspace, size_t workspace_bytes,
                                  vfr_stream_t stream);
/* ---- paragraph-to-video retrieval: which VIDEO does a group of sentences describe (the paragraph-to-video protocol of datasets
 * with several descriptions per video).  Q [Nq, D] = the sentences; a paragraph is a run of consecutive rows: grp_off [Ng+1]
 * (device int64, non-decreasing from 0 to Nq); max_len (host) = the longest run, <= 64.
 *   b(j, v)     = the distance of video v's best key for sentence j, exactly vfr_score_video_topk_f32's (the smallest (distance,
 *           global moment id) key over the whole triangle, canonical chain); m(j, v) = that key's moment id.
 *   score(g, v) = (b(j0, v) + b(j0+1, v) + .. + b(j0+L-1, v)) / (float)L: one fp32 left-to-right chain in sentence order starting
 *           from b(j0, v), then one correctly rounded fp32 division; nothing is contracted into an fma.
 *   key = (fp32 bits of score << 32) | (vid_base + v), order (score, global video index) ascending.  A video without clips is never
 *           ranked; an empty group gives padding and adds nothing.  With every group of length 1 out_dist equals
 *           vfr_score_video_topk_f32's out_dist bit for bit and the videos are those of its out_idx, in the same order.
 * vfr_score_paragraphs_f32:
 *   k > 0 : out_dist / out_idx [Ng,k] = the k smallest keys over the bank's videos as (score, global video index), padded with
 *           (+inf, -1).  k = 0 with counts only is allowed.
 *   own_dist / own_idx / count_lt [Ng] (nullable, together): count_lt[g] (int64) += number of this bank's videos whose key sorts
 *           strictly before (own_dist[g], own_idx[g]).  ADDED, so shards chain; the lists merge with vfr_topk_merge_f32.
 *   dtype VFR_SCORE_EXACT or VFR_MFMA_F32 (| VFR_MFMA_BANK_READY), as vfr_score_video_topk_f32: the fast path (D = 100, <= 21 clips,
 *           banks of at least score_mfma_min videos) runs the score's own chain on rigorous per-(sentence, video) bounds, keeps the
 *           videos the bounds cannot exclude or count, and gives those the exact chain.  BIT-IDENTICAL outputs.  The workspace front
 *           is vfr_score_video_topk_f32's, so BANK_READY and the device hash work alike.
 *   bad (nullable, device int): set to 1 when grp_off is not a non-decreasing run from 0 to Nq or a group is longer than max_len
 *           (results for such input are unspecified; nothing is read or written out of bounds).
 * vfr_score_paragraph_pairs_f32: pairs int32 [Np,2] = (group, GLOBAL video).  out_score [Np] = score(group, video);
 *   out_moments int64 [Np,max_len] (nullable) = m(j, video) per sentence of the group, -1 past the group's length.  A pair whose
 *   video lies outside [vid_base, vid_base + Nv) is left untouched: pre-fill +inf / -1 and reduce MIN / MAX over shards.  A pair on a
 *   video without clips or an empty group gets (+inf, -1); a group index outside [0, Ng) sets bad and is left untouched.  Serves the
 *   own video's rank key and the grounding of returned videos (where in video v each sentence lands).
 * Limits: k <= 448, max_clips <= 64, max_len <= 64, Ng * k < 2^31, vid_base + Nv < 2^32, id_base + total moments < 2^32.  Bad host
 * arguments: VFR_EINVAL before anything is enqueued.  The kernels keep one sentence row and the lanes' clip distances in 64 KB of
 * LDS: 4 * (round_up(D, 4) + 64 * max(max_clips, 1)) bytes for vfr_score_paragraphs_f32 (D <= 12288 at max_clips = 64, more for
 * shorter videos) and 4 * (round_up(D, 4) + 64) bytes for the pairs call must fit; VFR_EUNSUPPORTED otherwise, before anything is
 * enqueued.  vfr_score_paragraphs_workspace_bytes: O((Nq + Ng) Nv) (0 for a bad argument).
 * vfr_score_paragraphs_stats (measurement hook, SYNCHRONISES the stream): what the last VFR_MFMA_F32 fast-path call on `workspace`
 * (same Nq, Ng, Nv, total_clips) re-scored exactly: stats_host [Ng, 2] = {videos given the exact chain, of them rank-undecided}. */
size_t vfr_score_paragraphs_workspace_bytes(int64_t Nq, int64_t Ng, int Nv, int total_clips, int k);
int vfr_score_paragraphs_f32(const float *Q, int64_t Nq, const int64_t *grp_off, int64_t Ng, int max_len, const float *V,
                             const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips, int min_clips,
                             int max_clips, int D, float eps, int64_t vid_base, int k, float *out_dist, int64_t *out_idx,
                             const float *own_dist, const int64_t *own_idx, int64_t *count_lt, int dtype, int *bad,
                             void *workspace, size_t workspace_bytes, vfr_stream_t stream);
int vfr_score_paragraph_pairs_f32(const float *Q, int64_t Nq, const int64_t *grp_off, int64_t Ng, int max_len, const float *V,
                                  const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips, int min_clips,
                                  int max_clips, int D, float eps, int64_t id_base, int64_t vid_base, const int32_t *pairs, int64_t Np,
                                  float *out_score, int64_t *out_moments, int *bad, vfr_stream_t stream);
int vfr_score_paragraphs_stats(const void *workspace, int64_t Nq, int64_t Ng, int Nv, int total_clips, int64_t *stats_host,
                               vfr_stream_t stream);
/* ---- hard-negative mining for the ranking loss: the training loss IS the retrieval score (F.pairwise_distance(..., eps).mean()
 * over a span's clips = score(q, video, s, e)), so the hardest negatives of a training span are keys the scorer defines exactly.
 * items int32 [N, 4] = (query row of Q, CORPUS-GLOBAL video, start_t, end_t): inclusive clip span in utils.generate_moments units.
 * Items need not be sorted, may repeat and may share query rows; outputs are in the caller's order.
 *   score(q, v, s, e) = (dist[s] + .. + dist[e]) / (float)(e - s + 1), dist[c] = ||(V[c] - Q[q]) + eps||_2: the canonical chain
 *           (k-ascending fp32 fma chain, IEEE sqrt, fp32 sum s -> e, one correctly rounded division), BIT-IDENTICAL to what
 *           vfr_score_moments_f32 writes at [q, moment id of (v, s, e)].
 *   bad (nullable, device int): set to 1 for an item with query row outside [0, Nq), video < 0, start_t < 0, end_t < start_t (on any
 *           shard) or end_t >= the video's clip count (on the shard that holds the video); nothing is read or written out of bounds.
 * vfr_score_spans_f32: out[p] = score of item p.  An item whose video lies outside [vid_base, vid_base + Nv) belongs to another shard
 *   and is left untouched, as is a malformed one: pre-fill +inf and reduce MIN over shards.  Serves the positives of the miner.
 * vfr_mine_negatives_f32: an item is a training span (query row, OWN video, positive span).  h >= 0 entries per list:
 *   inter_dist / inter_vid [Nm,h] (nullable, together): the h smallest keys (fp32 bits of score << 32) | (vid_base + v) over the bank's
 *           eligible videos v -- global index != the own video and at least end_t + 1 clips -- with score(q, v, start_t, end_t): the
 *           positive's span applied to the other video, the loss's inter term.  Order (score, global video index) ascending, padded
 *           with (+inf, -1).  Every shard takes the same items; the lists merge with vfr_topk_merge_f32.
 *   intra_dist / intra_idx [Nm,h] (nullable, together): the h smallest keys over the eligible moments (s', e') of the own video, id =
 *           id_base + moment_offsets[v] + position in utils.generate_moments order.  intra_mode VFR_MINE_SAME_LENGTH: e' - s' ==
 *           end_t - start_t and (s', e') != (start_t, end_t) (CustomBatchSampler, same_length=True); VFR_MINE_ANY: every moment but
 *           (start_t, end_t) and the spans of excl int32 [Nm, X, 2] (X <= 8 host int, rows padded with (-1, -1); same_length=False:
 *           none of the annotated spans).  WRITTEN ONLY by the shard that holds the own video (sorted, padded with (+inf, -1)); other
 *           shards and malformed items leave the rows untouched: pre-fill (+inf, -1) and reduce MIN / MAX over shards.
 *   floor_dist [Nm] (nullable): an eligible negative with score <= floor_dist[m] is not listed (the positive's own score as the floor:
 *           semi-hard mining).
 *   thr_dist [Nm] (nullable) comes with count_inter / count_intra [Nm] int64 (at least one): += the eligible negatives with score <
 *           thr_dist[m], whatever the floor.  ADDED, so shards chain.  thr = fp32(positive + margin): the number of margin violators.
 *   A malformed item gives inter padding and adds nothing.  h = 0 with counts only is allowed.  Exact arithmetic only; any D (D = 100
 *   with 16-byte aligned Q and V takes the register-resident fast path).
 * Limits: h <= 448, max_clips <= 64, Nm * h < 2^31, vid_base + Nv < 2^32, id_base + total moments < 2^32.  Bad host-side arguments:
 * VFR_EINVAL before anything is enqueued.
 * vfr_mine_negatives_workspace_bytes = 256 + 8 h Nm C, C = min(ceil(4096 / Nm), ceil(Nv / 64), 256) >= 1 = the bound on the chunks the
 * video axis is cut into: O(Nm h), no Nm x Nv term (0 for a bad argument).                                                  */
#define VFR_MINE_SAME_LENGTH 0
#define VFR_MINE_ANY 1
int vfr_score_spans_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                        int max_clips, int D, float eps, int64_t vid_base, const int32_t *items, int64_t Np, float *out, int *bad,
                        vfr_stream_t stream);
size_t vfr_mine_negatives_workspace_bytes(int64_t Nm, int Nv, int h);
int vfr_mine_negatives_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets,
                           int Nv, int total_clips, int max_clips, int D, float eps, int64_t id_base, int64_t vid_base,
                           const int32_t *items, int64_t Nm, int h, int intra_mode, const int32_t *excl, int X,
                           const float *floor_dist, const float *thr_dist, float *inter_dist, int64_t *inter_vid, float *intra_dist,
                           int64_t *intra_idx, int64_t *count_inter, int64_t *count_intra, int *bad, void *workspace,
                           size_t workspace_bytes, vfr_stream_t stream);
/* ---- late-fusion retrieval: rank by a weighted sum over S streams (two feature extractors, RGB + flow, several seeds) that describe
 * the SAME videos: one clip_offsets / moment_offsets, per stream s a clip bank V_s [total_clips, D_s], a query matrix Q_s [Nq, D_s]
 * and a weight w_s (fp32, finite, >= 0).  The streams are HOST arrays of S device pointers / widths / weights (Q_host, V_host,
 * D_host, w_host), handed to the kernels by value like vfr_adam_step_f32's pointer arrays; 1 <= S <= VFR_FUSION_MAX_STREAMS.
 *   stream clip distance  d_s[q, c] = ||(V_s[c] - Q_s[q]) + eps||_2, the canonical chain: the bits of vfr_score_moments_f32 on
 *           stream s at the single-clip moment (c, c).
 *   fused clip distance   f = fl(w_0 d_0); f = fl(f + fl(w_s d_s)) for s = 1 .. S-1: fp32, every operation rounded, no fma.
 *   fused moment score    the moment chain on f: sequential fp32 sum of f[s..e] started at f[s], one IEEE division by
 *           (float)(e - s + 1), utils.generate_moments order.  (In real arithmetic: the weighted sum of the per-stream moment
 *           scores -- the mean is linear -- with one triangle per (query, video), not S.)
 *   keys    (fused score, id_base + moment_offsets[v] + j) ascending, padding (+inf, -1), as vfr_score_topk_f32.
 * S = 1 with w = (1), and w = (1, 0, ..) for any S (finite distances), give vfr_score_topk_f32 / vfr_score_video_topk_f32
 * (VFR_SCORE_EXACT) on stream 0 BIT FOR BIT.
 * vfr_score_fusion_own_f32: each query against ONE video own[q] (local index; outside [0, Nv): the row is all +inf): fused scores
 *   [Nq, Mmax], tail +inf -- layout and meaning of vfr_score_own_f32, so the rows feed vfr_gt_best_keys_f32 / vfr_gt_rank_keys_f32.
 * vfr_score_fusion_f32: level VFR_FUSION_MOMENTS: out_dist / out_idx [Nq,k] = the k smallest keys over all moments; count_lt[r][q]
 *   += the moments whose key sorts strictly before (rank_dist[r][q], rank_idx[r][q]).  VFR_FUSION_VIDEOS: the k smallest BEST
 *   keys of the videos (the whole triangle decides a video's best key) as (best score, id of the best moment); count_lt[r][q] +=
 *   the videos whose best key sorts before the rank key.  num_rank <= 4, counts are ADDED (shards chain; lists merge with
 *   vfr_topk_merge_f32); k = 0 with counts only is allowed.  min_clips is accepted for the shared argument list and unused.
 * Limits: max_clips <= 64, k <= 448, id_base + total moments < 2^32, Nq * k < 2^31, and the query rows of all streams must fit the
 * kernels' LDS plan: sum over s of round_up(D_s, 4) <= VFR_FUSION_MAX_SUM_D (32 KB of rows + 16 KB of clip distances + 4 KB of keys
 * in a 64 KB workgroup), VFR_EUNSUPPORTED above it.  VFR_EINVAL before anything is enqueued for S outside 1 .. 4, a null stream
 * array or stream pointer, D_s < 1, a weight that is negative, NaN or infinite, and the other bad host-side arguments.  Exact
 * arithmetic only (no MFMA bounds pre-filter: per-stream margins would have to be combined through the weighted sum).
 * vfr_score_fusion_workspace_bytes = 256 + 8 k Nq C, C = min(ceil(4096 / Nq), ceil(Nv / 64), 256) >= 1 = the bound on the chunks the
 * video axis is cut into: O(Nq k), no Nq x Nv term (0 for a bad argument).                                                   */
#define VFR_FUSION_MAX_STREAMS 4
#define VFR_FUSION_MAX_SUM_D 8192
#define VFR_FUSION_MOMENTS 0
#define VFR_FUSION_VIDEOS 1
int vfr_score_fusion_own_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int S,
                             int64_t Nq, const int32_t *clip_offsets, const int32_t *own, int Nv, int max_clips, float eps, int Mmax,
                             float *scores, vfr_stream_t stream);
size_t vfr_score_fusion_workspace_bytes(int64_t Nq, int Nv, int k);
int vfr_score_fusion_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int S,
                         int64_t Nq, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips,
                         int min_clips, int max_clips, float eps, int64_t id_base, int level, int k, float *out_dist,
                         int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt,
                         void *workspace, size_t workspace_bytes, vfr_stream_t stream);
/* ---- fusion weight sweep: the two calls above for a GRID of W weight vectors (w_host [W][S] row-major, host, every weight finite
 * and >= 0; 1 <= W <= VFR_FUSION_MAX_SWEEP) over the same streams in one pass -- what tuning the weights on a validation split
 * needs.  The stream clip distances d_s[q, c] do not depend on the weights: they are computed once, and per weight vector only the
 * fuse and the moment chain are repeated.  For every row w of the grid, BIT FOR BIT:
 *   vfr_score_fusion_sweep_own_f32: scores[w] [Nq, Mmax] = what vfr_score_fusion_own_f32 writes at w (scores is [W, Nq, Mmax]).
 *   vfr_score_fusion_sweep_f32:     count_lt[w] [num_rank, Nq] += what vfr_score_fusion_f32 adds at w with k = 0 and the rank keys
 *                                   rank_dist[w] / rank_idx[w] (all three [W, num_rank, Nq]).  Counts only: no lists, no workspace.
 * Stream arrays, level, num_rank <= 4, max_clips <= 64, id_base and the ADDED counts (shards chain) are as in the single-weight
 * calls; the grid travels by value in the kernel arguments; nothing waits for the host.  Nq = 0, Nv = 0 or num_rank = 0: VFR_OK,
 * nothing written (sweep_own still fills +inf when Nq > 0).
 * LDS of a vfr_score_fusion_sweep_f32 wave, in bytes, rows = max(max_clips, 1):
 *     4 * (sum over s of round_up(D_s, 4))       the query rows
 *   + 4 * 64 * rows * S                          the per-stream clip distances of a block of 64 videos
 *   + 4 * 64 * rows                              the fused clip distances of the current weight vector
 *   + 16 * W * num_rank                          the rank keys and the wave's 64-bit counts
 * must not exceed 65536: VFR_EUNSUPPORTED (the message states the bytes) otherwise -- S = 4 at max_clips = 64 never fits, S = 2 at
 * max_clips = 64 does for query rows of up to 3 840 floats in all.  VFR_EINVAL before anything is enqueued for W outside 1 .. 16, a null
 * array, a bad weight anywhere in the grid (the message names the row) and the bad arguments of the single-weight calls.      */
#define VFR_FUSION_MAX_SWEEP 16
int vfr_score_fusion_sweep_own_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int W,
                                   int S, int64_t Nq, const int32_t *clip_offsets, const int32_t *own, int Nv, int max_clips, float eps,
                                   int Mmax, float *scores, vfr_stream_t stream);
int vfr_score_fusion_sweep_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int W,
                               int S, int64_t Nq, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips,
                               int max_clips, float eps, int64_t id_base, int level, int num_rank, const float *rank_dist,
                               const int64_t *rank_idx, int64_t *count_lt, vfr_stream_t stream);
/* ---- prior-aware retrieval: a MOMENT TABLE gives every moment position an additive bias or excludes it -- a temporal prior
 * ("prior + model": how often training annotators chose a span), a proposal set (sliding windows of given lengths and stride), a
 * length limit ("at most 3 clips").  The first variant that changes the moment score inside a video.
 *   moment table  for every clip count n in 0 .. max_clips and every local moment j in utils.generate_moments(n) order one fp32
 *           entry: table_off int32 [max_clips + 2] = prefix sums of n (n + 1) / 2 (table_off[n] = where the row of n-clip videos
 *           starts, table_off[max_clips + 1] = all entries, at most 45 760 at 64 clips), table fp32 [table_off[max_clips + 1]].
 *           Both are device arrays, the same on every shard.  An entry is a finite bias >= 0 or +inf = excluded.
 *   biased score  g(q, v, j) = fl(score(q, v, j) + T[n_v][j]): score is the canonical chain, BIT-IDENTICAL to what
 *           vfr_score_moments_f32 writes; then ONE rounded fp32 addition, contracted with nothing.  A moment is a candidate iff
 *           g < +inf.
 *   keys    (fp32 bits of g << 32) | (id_base + moment_offsets[v] + j) ascending, padding (+inf, -1), as vfr_score_topk_f32.
 *           (Negative biases are not allowed: they would break the unsigned key order.)
 *   bad     (nullable, device int) is set to 1 when an entry that was read is NaN or < 0, or a table_off entry that was read points
 *           outside the table; such a moment (video) is treated as excluded.  Nothing is read or written out of bounds.
 * A table of zeros gives vfr_score_topk_f32 / vfr_score_video_topk_f32 (VFR_SCORE_EXACT) BIT FOR BIT: distances are >= 0 and
 * fl(x + 0) = x.
 * vfr_score_prior_own_f32: each query against ONE video own[q] (local index; outside [0, Nv): the row is all +inf): biased scores
 *   [Nq, Mmax], +inf at excluded moments and in the tail -- layout and meaning of vfr_score_own_f32, so the rows feed
 *   vfr_gt_best_keys_f32 / vfr_gt_rank_keys_f32 unchanged.
 * vfr_score_prior_f32: level VFR_PRIOR_MOMENTS: out_dist / out_idx [Nq,k] = the k smallest CANDIDATE keys; count_lt[r][q] += the
 *   candidates that sort strictly before (rank_dist[r][q], rank_idx[r][q]).  VFR_PRIOR_VIDEOS: the k smallest best candidate keys
 *   of the videos as (best g, id of that moment); a video without a candidate is never ranked or counted; count_lt[r][q] += the
 *   videos whose best key sorts before the rank key.  num_rank <= 4, counts are ADDED (shards chain; lists merge with
 *   vfr_topk_merge_f32); k = 0 with counts only is allowed.  The rank key (+inf, -1) counts every candidate (every video with one).
 *   Nq = 0: nothing is written.  Nv = 0: the lists are padding, the counts stay.  min_clips is accepted for the shared argument
 *   list and unused.
 * Limits: max_clips <= 64, k <= 448, id_base + total moments < 2^32, Nq * k < 2^31, any D (D = 100 with 16-byte aligned Q and V
 * takes the register-resident fast path).  VFR_EINVAL before anything is enqueued for the bad host-side arguments.  Exact arithmetic
 * only (an MFMA bounds pre-filter would be sound -- a bias >= 0 keeps lower bounds valid -- and is not built).
 * LDS of a vfr_score_prior_f32 wave, in bytes: 416 (the query row; fast path only) + 256 max(max_clips, 1) (the clip distances of a
 * block of 64 videos) + 8 slots(k) (the key list: 128 / 256 / 512 slots for k <= 64 / 192 / 448): at most 20 896 at max_clips = 64.
 * vfr_score_prior_workspace_bytes = 256 + 8 k Nq C, C = min(ceil(4096 / Nq), ceil(Nv / 64), 256) >= 1 = the bound on the chunks the
 * video axis is cut into: O(Nq k), no Nq x Nv term (0 for a bad argument).                                                   */
#define VFR_PRIOR_MOMENTS 0
#define VFR_PRIOR_VIDEOS 1
int vfr_score_prior_own_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int32_t *own, int Nv,
                            int max_clips, int D, float eps, int Mmax, const int32_t *table_off, const float *table, float *scores,
                            int *bad, vfr_stream_t stream);
size_t vfr_score_prior_workspace_bytes(int64_t Nq, int Nv, int k);
int vfr_score_prior_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
                        int total_clips, int min_clips, int max_clips, int D, float eps, int64_t id_base, int level, int k,
                        float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx,
                        int64_t *count_lt, const int32_t *table_off, const float *table, int *bad, void *workspace,
                        size_t workspace_bytes, vfr_stream_t stream);
/* ---- windowed retrieval for long videos: the candidate set is every window of at most max_len clips, whatever the length of a
 * video -- the proposal set long-video corpora (Charades-STA, ActivityNet Captions, TACoS) are searched over.  Every other scoring
 * entry point puts one whole video on a lane and refuses max_clips > 64; this one scans the FLAT clip axis (lane = start clip, a
 * running sum over the next max_len end clips), so nothing in it is sized by a video.
 *   candidates  every moment (video v, start s, end e) with 0 <= s <= e < n_v and e - s + 1 <= max_len, 1 <= max_len <= 64.
 *   score   the canonical chain, BIT-IDENTICAL to what vfr_score_moments_f32 writes (k-ascending fp32 fma chain of ((v - q) + eps)^2,
 *           IEEE sqrt, sequential fp32 sum s -> e, one IEEE division by (float)(e - s + 1)).
 *   keys    (fp32 bits of the score << 32) | (id_base + moment_offsets[v] + j), j = the moment's position in utils.generate_moments(n_v)
 *           order: the ids stay canonical, so max_len >= max_clips gives vfr_score_topk_f32 (VFR_SCORE_EXACT) BIT FOR BIT and every
 *           decoder of ids still works.  Ascending, padding (+inf, -1).
 * vfr_score_window_f32: out_dist / out_idx [Nq,k] = the k smallest candidate keys; count_lt[r][q] += the candidates that sort
 *   strictly before (rank_dist[r][q], rank_idx[r][q]).  num_rank <= 4, counts are ADDED (shards chain; lists merge with
 *   vfr_topk_merge_f32); k = 0 with counts only is allowed.  Nq = 0: nothing is written.  Nv = 0 or total_clips = 0: the lists are
 *   padding, the counts stay.  Videos without clips own no candidate.
 * vfr_score_window_span_keys_f32: items int32 [Np, 4] = (query row, corpus-global video, start, end) -> out_keys[p] = the key of that
 *   span (what a rank key of a ground-truth span is, without an own-video row of n^2 entries).  An item whose video lies outside
 *   [vid_base, vid_base + Nv) is left untouched: pre-fill VFR_KEY_EMPTY and reduce MIN over the shards.  A malformed item (query row
 *   outside [0, Nq), start < 0, end < start, end >= n_v, end - start + 1 > 64) sets *bad (nullable, device int) and is left untouched.
 * Limits: 1 <= max_len <= 64, k <= 448, id_base + total moments <= 2^32 (bounded as total_clips (max_clips + 1) / 2), Nq * k < 2^31,
 * any D (D = 100 with 16-byte aligned Q and V takes the fast path of the scan), and max_clips <= 1024: the longest video the CPU
 * oracle (vfo_score_moments) can check -- the kernels keep nothing that is sized by a video (their int32 moment positions would hold
 * up to 32 767 clips).  VFR_EINVAL before
 * anything is enqueued for the bad host-side arguments, a workspace shorter than vfr_score_window_workspace_bytes among them.  Exact
 * arithmetic only (no MFMA pre-filter), stride 1.
 * LDS of a vfr_score_window_f32 wave, in bytes: 416 (the query row; fast path only) + 512 (the clip distances of a tile of 64 flat
 * clips and its halo of max_len - 1) + 8 slots(k) (the key list: 128 / 256 / 512 slots for k <= 64 / 192 / 448): at most 5 024,
 * whatever the clip counts are.
 * vfr_score_window_workspace_bytes = 256 + 8 k Nq C, C = min(ceil(4096 / Nq), ceil(total_clips / 64), 256) >= 1 = the bound on the
 * chunks the flat clip axis is cut into: O(Nq k) (0 for a bad argument).                                                       */
size_t vfr_score_window_workspace_bytes(int64_t Nq, int total_clips, int k);
int vfr_score_window_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
                         int total_clips, int max_clips, int D, float eps, int64_t id_base, int max_len, int k, float *out_dist,
                         int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt,
                         void *workspace, size_t workspace_bytes, vfr_stream_t stream);
int vfr_score_window_span_keys_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                                   const int64_t *moment_offsets, int Nv, int total_clips, int D, float eps, int64_t id_base,
                                   int64_t vid_base, const int32_t *items, int64_t Np, int64_t *out_keys, int *bad,
                                   vfr_stream_t stream);
/* Device self-check of the arithmetic model the pre-filter's margins and the MFMA GEMMs' bit-exactness assume: a
 * v_mfma_f32_16x16x4_f32 = four fp32 fmas, k ascending, on its accumulator (denormals kept).  A, B [16, K] device rows
 * (K % 4 == 0; make them adversarial: wide exponent range, cancellation, denormals): C = A B^T by the matrix pipe against an
 * explicit fmaf chain per element; *mismatches (device int) = elements whose bits differ -- 0 on a conforming device.
 * reversed != 0 runs the reference chain k-descending (what a failing check looks like).  The Python layer runs it once per
 * process before the first "mfma" / "bf16" scoring call and falls back to the exact kernels if it fails.          */
int vfr_mfma_selfcheck(const float *A, const float *B, int K, int reversed, int *mismatches, vfr_stream_t stream);
/* int8 arm of the self-check: what the int8 operand mode of the pre-filter ("score_i8") assumes about v_mfma_i32_16x16x64_i8 --
 * its lane map and exact, accumulated products.  A, B: device [16, 128] int8 (16-byte aligned; make them asymmetric): C = A B^T
 * over two chained k-steps on the matrix pipe against integer dot products on the vector ALU; *mismatches (device int) = elements
 * that differ.  permuted != 0 compares with the TRANSPOSED product (what a wrong lane map looks like).  The Python layer runs it
 * with the fp32 arm; a device that fails only this arm scores with the fp32 operands ("score_i8" 0) and a warning.          */
int vfr_mfma_selfcheck_i8(const int8_t *A, const int8_t *B, int permuted, int *mismatches, vfr_stream_t stream);
/* TEST HOOK of the int8 operand mode (not on any hot path): runs the mode's pre-passes on (Q, V) in `workspace`
 * (>= vfr_score_topk_mfma_workspace_bytes(Nq, Nv, total_clips, 0)) and copies out, all device pointers: the limb planes
 * vlimbs [total_clips, 3, 128] / qlimbs [Nq, 3, 128] (digit i of X = sum digit_i 256^i; bytes 100 .. 127 zero), bank_const [4] =
 * {s_v, max |v - X / s_v|, max |X_v|_1 / s_v, max |v_k - mu_k|}, query_const [Nq, 2] = {|q - mu|_1, max |q - X / s_q|},
 * query_scale [groups] = s_q and query_factor [groups] = fl(-512 / (s_q s_v)) per 64-query group, qmeta [Nq, 4] = {b_q, 0, E2,
 * R + |q|}, va [total_clips] = a_c, mu [128], and ring [Nq, total_clips] = the approximate d^2 - b_q of every (query, clip) as
 * the scoring kernel's device functions compute them (16-clip tiles from clip 0).  D = 100.                                 */
int vfr_score_i8_debug(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, int Nv, int total_clips, int D,
                       float eps, void *workspace, size_t workspace_bytes, int8_t *vlimbs, int8_t *qlimbs, double *bank_const,
                       double *query_const, double *query_scale, float *query_factor, float *qmeta, float *va, float *mu,
                       float *ring, vfr_stream_t stream);
/* merge G per-shard top-k lists (after the RCCL all-gather): part_dist/part_idx
 * [G, Nq, k] -> out [Nq, k], same (distance, id) order.                                        */
int vfr_topk_merge_f32(const float *part_dist, const int64_t *part_idx, int G, int64_t Nq, int k, float *out_dist,
                       int64_t *out_idx, vfr_stream_t stream);
/* The same exchange with the lists in the form the ranks send them: one int64 key per entry,
 * (fp32 bits of the distance << 32) | moment id, whose signed order is the (distance, id) order;
 * VFR_KEY_EMPTY = (+inf, 0xffffffff) marks an unused slot.  pack: (dist, idx) [n] -> keys [n]
 * (idx < 0 -> empty).  merge: part_keys [G, Nq, k] -> out_dist/out_idx [Nq, k] (both or neither)
 * and/or out_keys [Nq, k] (nullable) -- the merged list as keys, whose column k-1 is the
 * threshold seed of the next pass and which can be merged again without repacking.  _strided: slot
 * g starts at part_keys + g * slot_stride (>= Nq * k int64 elements) -- the lists as they lie inside
 * the rows of a packed exchange buffer, merged in place.                                          */
#define VFR_KEY_EMPTY 0x7F800000FFFFFFFFll
int vfr_topk_pack_keys(const float *dist, const int64_t *idx, int64_t n, int64_t *keys, vfr_stream_t stream);
int vfr_topk_merge_keys(const int64_t *part_keys, int G, int64_t Nq, int k, float *out_dist, int64_t *out_idx,
                        int64_t *out_keys, vfr_stream_t stream);
int vfr_topk_merge_keys_strided(const int64_t *part_keys, int64_t slot_stride, int G, int64_t Nq, int k, float *out_dist,
                                int64_t *out_idx, int64_t *out_keys, vfr_stream_t stream);
/* a12  position of the first ground-truth-positive moment (model/evaluate.py:67-77,
 * np.where(labels[order])[0][0]) needs that moment's key: keys[r, sel[s]] = min over m < M with
 * labels[r, s, m] != 0 of (own_scores[s, m], id_base[s] + m); every other entry of keys [R, Nq]
 * (queries whose video lives on another rank, queries without a positive) = VFR_KEY_EMPTY.
 * own_scores [n_sel, score_stride] from vfr_score_own_f32, labels uint8 [R, n_sel, label_stride]. */
int vfr_gt_best_keys_f32(const float *own_scores, int64_t n_sel, int M, int score_stride, const uint8_t *labels, int R,
                         int label_stride, const int64_t *id_base, const int64_t *sel, int64_t Nq, int64_t *keys,
                         vfr_stream_t stream);
/* The same, plus what a single-shard caller does with the keys next, in the same two launches (a serving request is a chain
 * of short dependent launches: every one saved is ~10 us of its latency): rank_dist / rank_idx [R, Nq] (nullable, together) =
 * the keys unpacked into the rank-key arguments of vfr_score_topk_* ((+inf, 0xffffffff) where there is none); count_zero
 * [R, Nq] int64 (nullable) is zeroed (the count_lt argument those entry points ADD to); *missing (device int, nullable) = 1 iff
 * some (threshold, selected query) has no positive moment, else 0 -- model/evaluate.py:77's IndexError condition.          */
int vfr_gt_rank_keys_f32(const float *own_scores, int64_t n_sel, int M, int score_stride, const uint8_t *labels, int R,
                         int label_stride, const int64_t *id_base, const int64_t *sel, int64_t Nq, int64_t *keys,
                         float *rank_dist, int64_t *rank_idx, int64_t *count_zero, int *missing, vfr_stream_t stream);

/* a11  ground-truth labels (model/evaluate.py:59-62 with utils.get_iou, model/utils.py:78-82; main.py:161 uses >=):
 * labels[r][q][m] = 1 iff >= 2 annotators of query q have IoU > thr[r] (strict != 0) or >= thr[r] with local moment m
 * (utils.generate_moments order) of the query's own video of n_own[q] clips; IoU = float64 intersection / union of the
 * inclusive clip spans.  times int32 [Nq, A, 2] (rows >= nannot[q] unused), thresholds_host: R <= 16 doubles (HOST).
 * labels uint8 [R, Nq, Mmax], zero for m >= n(n+1)/2.                                           */
int vfr_gt_labels_u8(const int32_t *times, const int32_t *nannot, const int32_t *n_own, int64_t Nq, int A,
                     const double *thresholds_host, int R, int strict, int Mmax, uint8_t *labels, vfr_stream_t stream);

/* ---- a1  frame normalisation: DiDeMoDataset.__getitem__ tail, get_rgb_features.py:64-69
 * THWC uint8 -> TCHW fp32, ((x/255) - mean[c]) / std[c] with the ImageNet constants (:34-35)    */
int vfr_frames_normalize_f32(const uint8_t *frames_thwc, int T, int H, int W, float *out_tchw, vfr_stream_t stream);

/* ---- a2  VGG-19 "E" up to fc7: torchvision vgg19.features/avgpool/classifier[0..4],
 * get_rgb_features.py:122-126,145-147.  Layer primitives (NCHW fp32):                           */
int vfr_conv3x3_relu_f32(const float *x, int B, int Cin, int H, int W, const float *w /*[Cout,Cin,3,3]*/,
                         const float *b, int Cout, float *y, vfr_stream_t stream);
int vfr_maxpool2_f32(const float *x, int B, int C, int H, int W, float *y, vfr_stream_t stream);
int vfr_adaptive_avgpool7_f32(const float *x, int B, int C, int H, int W, float *y, vfr_stream_t stream);
/* whole stack: frames [T,H,W,3] u8 -> out [T, fc_dim].  cfg_host: ncfg ints, >0 = conv width,
 * 0 = maxpool (VGG-19: 64,64,0,128,128,0,256x4,0,512x4,0,512x4,0).  conv_w/conv_b: HOST arrays
 * of DEVICE pointers, one per conv.  fc6 [fc_dim, C_last*49], fc7 [fc_dim, fc_dim].             */
size_t vfr_vgg_fc7_workspace_bytes(int T, int H, int W, const int *cfg_host, int ncfg, int fc_dim);
int vfr_vgg_fc7_f32(const uint8_t *frames_thwc, int T, int H, int W, const int *cfg_host, int ncfg,
                    const float *const *conv_w_host, const float *const *conv_b_host, const float *fc6_w,
                    const float *fc6_b, const float *fc7_w, const float *fc7_b, int fc_dim, float *out,
                    void *workspace, size_t workspace_bytes, vfr_stream_t stream);

/* ---- f4  ResNet-152 variant of the extractor: torchvision resnet152 without its fc head, get_rgb_features.py:127-131
 * (conv1 / bn1 / relu / maxpool, Bottleneck layers, global average pool) -> out [T, 32 * width] (2048 at width 64).
 * blocks_host [4] = Bottleneck blocks per layer ({3, 8, 36, 3}); width = 64.  conv_w_host / bn_host: HOST arrays of DEVICE
 * pointers, one per convolution in EXECUTION order -- the stem, then per block conv1 (1x1), conv2 (3x3, carries the
 * stride), conv3 (1x1) and, for the first block of a layer, the 1x1 downsample convolution: conv weight [Cout, Cin, k, k]
 * (torchvision layout) and its BatchNorm as one packed [4, Cout] tensor (weight, bias, running_mean, running_var).  Eval-mode
 * BatchNorm is folded into the convolution (csrc/resnet.hip); bn_eps = 1e-5 for torchvision's modules.                    */
size_t vfr_resnet_pool_workspace_bytes(int T, int H, int W, const int *blocks_host, int width);
int vfr_resnet_pool_f32(const uint8_t *frames_thwc, int T, int H, int W, const int *blocks_host, int width,
                        const float *const *conv_w_host, const float *const *bn_host, float bn_eps, float *out, void *workspace,
                        size_t workspace_bytes, vfr_stream_t stream);
/* The same with the BatchNorm folding and tap-major repacking of the 155 convolutions done ONCE per model instead of once per
 * call (0.6 ms of a 36 ms video): vfr_resnet_fold_f32 writes the folded weights and betas into a caller-owned buffer of
 * vfr_resnet_folded_bytes; vfr_resnet_pool_folded_f32 runs the stack on it (same workspace size, same bits).                */
size_t vfr_resnet_folded_bytes(const int *blocks_host, int width);
int vfr_resnet_fold_f32(const int *blocks_host, int width, const float *const *conv_w_host, const float *const *bn_host, float bn_eps,
                        void *folded, size_t folded_bytes, vfr_stream_t stream);
int vfr_resnet_pool_folded_f32(const uint8_t *frames_thwc, int T, int H, int W, const int *blocks_host, int width, const void *folded,
                               size_t folded_bytes, float *out, void *workspace, size_t workspace_bytes, vfr_stream_t stream);

/* ---- f2  training / test loss: Trainer.ranking_loss, model/main.py:214-232 (called from train_epoch :63 and
 * test_epoch :102).  posit, inter [P,D], intra [Nn,D], lang [S,D]; maskp [P], maskn [Nn] int64 sample ids (rows whose id
 * is outside [0,S) belong to no sample).  loss[0] = sum_i relu(c_posit - c_intra + b) + lamb*relu(c_posit - c_inter + b),
 * c_x = mean pairwise_distance(x rows of sample i, lang[i]).  The optional normalize_loss row scaling (:219-223) is the
 * caller's (it is plain differentiable arithmetic on the inputs).  The workspace written by the forward call (row distances,
 * per-sample terms) is what the backward call reads; grad_loss is the upstream scalar gradient on the device.            */
size_t vfr_ranking_loss_workspace_bytes(int64_t P, int64_t Nn, int S);
int vfr_ranking_loss_f32(const float *posit, const float *intra, const float *inter, const float *lang, const int64_t *maskp,
                         const int64_t *maskn, int64_t P, int64_t Nn, int S, int D, float b, float lamb, float eps,
                         float *loss, void *workspace, size_t workspace_bytes, vfr_stream_t stream);
int vfr_ranking_loss_grad_f32(const float *posit, const float *intra, const float *inter, const float *lang,
                              const int64_t *maskp, const int64_t *maskn, int64_t P, int64_t Nn, int S, int D, float lamb,
                              float eps, const float *grad_loss, const void *workspace, float *grad_posit, float *grad_intra,
                              float *grad_inter, float *grad_lang, vfr_stream_t stream);

/* ---- f2 (second half)  the encoders' backward: loss.backward() through CALModel.forward, model/main.py:58-67 with
 * model/models.py:21-26 (visual_fc) and :40-47,61-66 (lstm, lang_fc).  The gradient contractions are vfr_linear_f32 on
 * transposed operands (dX = dY W, dW = dY^T X); these are the pieces around them (train.py wires them into autograd):
 *   transpose      out [cols, rows] = in [rows, cols]^T
 *   colsum         out[c] = sum_r in[r][c] in a fixed order (16 row phases, then the phases; bias gradients; deterministic)
 *   relu_backward  out = act > 0 ? grad : 0
 *   lstm_cell_forward   one step of nn.LSTM's cell (gates i, f, g, o): pre [B,4H] = h_prev W_hh^T + b_hh, the input part
 *                  x_t W_ih^T + b_ih of batch row b at xproj + b * x_stride; writes the ACTIVATED gates [B,4H], c, h [B,H]
 *   lstm_cell_backward  one step of BPTT: (dh [B,H], dc [B,H] in/out) + the step's gates and cell states -> dpre [B,4H]
 *   bilstm_train_forward   the whole recurrence of both directions over dense inputs X [B,T,E] (E, H multiples of 4): T
 *                  launches of the inference path's fused step, which here also stores the activated gates.  Buffers are
 *                  [direction][step]-major: gates [2][T][B][4H], cs / hs [2][T+1][B][H] (slot 0 = the zero initial state,
 *                  written here; step s of the reverse direction read time T-1-s); h_n = hs[d][T].
 *   bilstm_train_backward  BPTT for both directions: gout [B,2H] = gradient of [h_fwd | h_bwd]; WhhT_d [H,4H] = W_hh,d^T;
 *                  dpre [2][T][B][4H] = gradient of every step's gate pre-activations (the weight gradients are GEMMs over
 *                  it).  Per step one cell-backward launch and one GEMM grid for both directions, K cut into ranges whose
 *                  partial products the next cell-backward adds in a fixed order (deterministic).                          */
int vfr_transpose_f32(const float *in, int64_t rows, int64_t cols, float *out, vfr_stream_t stream);
int vfr_colsum_f32(const float *in, int64_t rows, int cols, float *out, vfr_stream_t stream);
int vfr_relu_backward_f32(const float *grad, const float *act, int64_t n, float *out, vfr_stream_t stream);
int vfr_lstm_cell_forward_f32(const float *pre, const float *xproj, int64_t x_stride, const float *c_prev, int64_t B, int H,
                              float *gates, float *c, float *h, vfr_stream_t stream);
int vfr_lstm_cell_backward_f32(const float *dh, float *dc, const float *gates, const float *c_prev, const float *c_cur, int64_t B,
                               int H, float *dpre, vfr_stream_t stream);
int vfr_bilstm_train_forward_f32(const float *X, int64_t B, int T, int E, int H, const float *Wih_f, const float *Whh_f,
                                 const float *bih_f, const float *bhh_f, const float *Wih_b, const float *Whh_b,
                                 const float *bih_b, const float *bhh_b, float *gates, float *cs, float *hs, vfr_stream_t stream);
size_t vfr_bilstm_train_backward_workspace_bytes(int64_t B, int H);
int vfr_bilstm_train_backward_f32(const float *gout, const float *gates, const float *cs, const float *WhhT_f, const float *WhhT_b,
                                  int64_t B, int T, int H, float *dpre, void *workspace, size_t workspace_bytes, vfr_stream_t stream);

/* ---- f2  the training driver: Trainer.train_epoch's data path and optimizer step, model/main.py:43-80 ---------------
 * triplet_gather  one batch of CustomBatchSampler triplets (model/data.py:249-343) -> custom_collate's tensors (:346-356) from
 *                 the resident bank (seg [sum n, F], ctx [Nv, F], clip_off [Nv+1] int32) and token table tokens [A, Tq] int64.
 *                 plan_host [S][7] int32 (HOST memory, read before return): video_pos, video_neg, start_t, end_t, start_tn,
 *                 end_tn, token row.  Writes posit / inter [P, 2F+2] (rows (video_pos | video_neg, start_t..end_t)), intra
 *                 [Nn, 2F+2] (video_pos, start_tn..end_tn), each row [seg[off[v] + t] | ctx[v] | t/n | (t+1)/n] (IEEE fp32
 *                 division, make_visual_features :204-213); maskp [P], maskn [Nn] int64 = sample index; lang [S, Tq] int64.
 *                 P and Nn must equal the plan's row totals; clip spans must be < 256.  One launch per 128 samples: the plan
 *                 travels in the kernel arguments (no staging buffer to race on).  Outputs 8-byte aligned (rows are).
 * adam_step       torch.optim.Adam(amsgrad=False, maximize=False) with L2 (not decoupled) weight decay over n <=
 *                 VFR_ADAM_MAX_TENSORS fp32 tensors in ONE launch; host arrays of device pointers param / grad / exp_avg /
 *                 exp_avg_sq, numel_host [n], coef_host [n][7] = fp32 {weight_decay, 1-beta1, beta2, 1-beta2, eps, -step_size,
 *                 1/bias_correction2_sqrt} (the caller computes step_size and bias_correction2_sqrt in double from the step count,
 *                 as torch does, and the reciprocal in fp32).  Per element, each op rounded: g' = g + wd p (wd != 0);
 *                 m = lerp(m, g', 1-beta1); v = v beta2; v = v + (1-beta2) (g' g'); p = p + (-step_size) (m / (sqrt(v) *
 *                 (1/bc2_sqrt) + eps)).  Also writes grad_sumsq[n] = sum of squares of every RAW gradient (before weight
 *                 decay): fixed-order partials per 4096-element chunk, then a fixed-order reduce by the launch's last block
 *                 (deterministic, no float atomics).  float4 where all four pointers of a tensor are 16-byte aligned.
 * grad_sumsq      the same sums of squares without the update (utils.grad_norm's input for any optimizer).
 * The workspace (vfr_adam_workspace_bytes, shared by both) must be ZERO before its first use; every call leaves it so.      */
#define VFR_ADAM_MAX_TENSORS 32
int vfr_triplet_gather_f32(const float *seg, const float *ctx, const int *clip_off, int num_videos, int F, const int64_t *tokens,
                           int num_tokens_rows, int Tq, const int *plan_host, int S, int64_t P, int64_t Nn, float *posit,
                           float *intra, float *inter, int64_t *maskp, int64_t *maskn, int64_t *lang, vfr_stream_t stream);
size_t vfr_adam_workspace_bytes(const int64_t *numel_host, int n);
int vfr_adam_step_f32(int n, float *const *param_host, const float *const *grad_host, float *const *exp_avg_host,
                      float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_host, float *grad_sumsq,
                      void *workspace, size_t workspace_bytes, vfr_stream_t stream);
int vfr_grad_sumsq_f32(int n, const float *const *grad_host, const int64_t *numel_host, float *grad_sumsq, void *workspace,
                       size_t workspace_bytes, vfr_stream_t stream);

/* ---- parity probe: elementwise canonical math (0 exp, 1 sigmoid, 2 tanh, 3 x/y, 4 sqrt,
 * 5 fma(x,y,x)) so tests can pin the device's transcendental forms against the oracle's.        */
int vfr_math_f32(int op, const float *x, const float *y, float *out, int64_t n, vfr_stream_t stream);

/* ---- tuning / introspection (tests and bench only) -------------------------------------------
 * vfr_set_option("gemm", 0|1): 0 = LDS-tiled VALU chain kernels, 1 = MFMA kernels (default).
 * Both produce identical bits; the switch exists so tests can prove that on the device.
 * "score_fast" 0|1 (the fused D=100 scorer vs the generic one), "score_split" 0|1 (top-k and rank keys in separate
 * launches), "lstm_tile" 0|1|2|3 (fused LSTM step tile rows: automatic | 64 | 128 | 32), "score_pre_b" N (videos in the top-k threshold ladder's stage B; 0 = Nv/16
 * capped at 640), "score_tasks" N (wave-tasks the fused scorer's plan aims for; 0 = automatic), "lstm_skip0" 1|0 (the first LSTM step
 * skips its recurrent segment because h_0 = 0 | runs it), "score_smallq" N (vfr_score_topk_mfma, f32: batches of up to N <= 64 queries against banks of <= 21 clips per video are scored with lanes = clips / videos, the top-k by video selection, default 64; 0: always the fused kernels), "lstm_small" N (batches of up to N <= 4 queries take the vector-chain LSTM step, default 2; 0: always the MFMA tiles), "score_mfma_min" N (vfr_score_topk_mfma hands banks of fewer than N videos to the exact kernels, default 128), "gemm_small" 0|64 (GEMMs of under 384 128-row tiles: 32-row tiles |
 * 64-row tiles), "lstm_xcd" 1|0 (XCD-aware workgroup order of the fused LSTM step | launch order), "lstm_persist" 1|0 (up to 32
 * queries: the whole BiLSTM sequence in ONE launch -- one or two queries: weight slices resident in LDS, vector chains; above
 * "lstm_persist_min" (default 2) at the model's shape: weights resident in registers as MFMA fragments -- with h handed between
 * workgroups as tagged granules | one launch per step), "score_smallq_select" 1|0 (few-queries top-k by video selection | key
 * array + selection tree), "vgg_fuse_pool" 1|0 (a 2x2 max-pool behind a VGG convolution runs in that convolution's epilogue |
 * its own kernel), "vgg_direct1" 1|0 (first VGG convolution as the direct kernel | the implicit-GEMM MFMA kernel), "vgg_halo" 1|0 (the VGG stack on
 * halo-padded activations where its shape allows: convolution loader without tap masks | unpadded), "lstm_fast" 1|0 (the
 * select-free instantiation of the table-start LSTM step where the launch qualifies | always the general form),
 * "lstm_multi" 2|1|0 (all T LSTM steps of both directions in one launch -- ordered task lists per XCD group, completion counters,
 * agent-scope state traffic: automatic, i.e. from "lstm_multi_min" GEMM rows on (default 2500) at H >= 512 with 128-row tiles while
 * "lstm_tile" is 0 | always, tile height by "lstm_tile" | never: one launch per step; a give-up is repaired by a
 * rescue kernel and reported through the fault word like the sequence kernels'; it needs its whole grid resident at once, which
 * is checked at launch -- occupancy x CUs -- and the per-step launches are taken when it is not; "lstm_multi_taken" is READ-ONLY
 * (vfr_set_option refuses it) and written by every vfr_bilstm_final_f32: 1 = the call ran the one-launch kernel, 2 = selected but
 * not resident at once, per-step launches taken, 0 = any other path),
 * "lstm_live_blocks" 1|0 (fused LSTM step: a wave issues fragment reads, MFMAs, table gather and gate epilogue only for its 16-row
 * blocks that hold a row below the direction's active count and a unit below H | for every block of its tile -- same bits; +2:
 * count the issued blocks, see vfr_bilstm_debug_offset),
 * "score_kth_seed" 1|0 (stage A of the top-k threshold ladder takes its seed by bisection on the candidates' score bits | by the merge kernel),
 * "score_smallq_rank" N (few-queries path with video selection: from N queries on -- default 8 -- the rank counts run with lane = video,
 * straight-line triangle, 3-instruction exact quotient; 0: always the 16-threads-per-video moment kernel),
 * "score_defer" N (vfr_score_topk_mfma, f32: whole-video early-out of the rank half of the moment triangle when at most N lanes of
 * a wave are left undecided by the video's smallest / largest clip distance -- those are re-counted exactly; default 8, -1: off),
 * "score_sort" 1|0|2 (the pre-filter pass with rank keys runs on the batch sorted by difficulty from 1024 queries x 4096 videos
 * on | caller's order | sorted whatever the size), "score_hist" 1|0 (the main top-k launch tightens its threshold from a histogram
 * of the candidates found so far | stage B's threshold throughout), "score_i8" 1|0 (vfr_score_topk_mfma, f32: the pre-filter's
 * approximate GEMM runs on int8 limbs of the centred rows -- exact integer products on v_mfma_i32_16x16x64_i8, the margin built
 * from the computed quantisation error | on the fp32 rows, v_mfma_f32_16x16x4_f32; the bank-side products of one form are
 * recomputed when the other is asked for) -- same bits either way.  Options are process-global (see Conventions).        */
int vfr_set_option(const char *name, int value);
int vfr_get_option(const char *name);
/* vfr_set_option("profile", 1): every instrumented launch is bracketed by two hipEvents recorded on
 * the launch stream.  After the caller has synchronised the device, vfr_profile_read(site, ...) folds
 * the finished pairs and returns the site's accumulated device time and launch count (reset != 0
 * clears all sites afterwards).  Sites are 1 .. vfr_profile_sites()-1, named by
 * vfr_profile_site_name().  This is how bench.py measures the dominant kernel's launch duration.   */
int vfr_profile_sites(void);
const char *vfr_profile_site_name(int site);
int vfr_profile_read(int site, double *total_ms, int64_t *launches, int reset);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* VFR_H */
