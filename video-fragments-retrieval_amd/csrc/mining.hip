// Hard-negative mining for the ranking loss: vfr_score_spans_f32 and vfr_mine_negatives_f32 (include/vfr.h).
//
// The training loss IS the retrieval score: F.pairwise_distance(..., eps).mean() over a span's clips = score(q, video, s, e), the
// canonical chain of vfr_score_moments_f32 (k-ascending fp32 fma chain over D, IEEE sqrt, sequential fp32 sum s -> e, one IEEE
// division); its clip distances come from scan_common.h, not from the headers of score.o, so the code objects of score.o do not
// change.  An item is a training span (query row, own video, s, e):
//   inter negatives  the span (s, e) applied to every OTHER video of at least e + 1 clips, key = (score bits << 32) | global video
//   intra negatives  the other moments of the own video (same length, or any but the annotated spans), key = (score bits << 32) |
//                    global moment id
// Kernels (a translation unit of its own):
//   mine_spans_kernel  one wave per item: lane = clip of the span, its distance into LDS, lane 0 sums s -> e and divides.
//   mine_inter_kernel  one wave per (item, chunk of the video axis).  lane = video: the wave-uniform query row sits in LDS, each lane
//                      reads only rows s..e of its video (16-byte loads, two clips = two independent chains at a time) and carries the
//                      sum in a register; ineligible lanes (own video, shorter than e + 1 clips, past the bank) are masked.  Counts by
//                      compare + ballot + popcount, one atomic per wave; the h smallest keys are collected under a running threshold
//                      into an LDS list that is sorted and cut back to h when it fills; the chunk's list goes to ws[chunk][item][0..h).
//   mine_intra_kernel  one wave per item, on the shard that holds the own video: lane = clip (its distance into LDS), then lane =
//                      start clip with a running sum over the end clip, the same list and count; writes the sorted, padded list.
//   The per-chunk inter lists are merged by vfr_topk_merge_keys (one launch), which also pads with (+inf, -1).
// The chunk plan (scan_plan: at most SCAN_MAX_CHUNKS chunks, just enough for about SCAN_TARGET_WAVES waves: one item against 10 000
// videos fills the device, 5 000 items run long streams -- a running threshold wants them), the list's capacity and sort and the
// clip-distance helpers are those of scan_common.h.
// Workspace: chunks x Nm x h keys, chunks <= SCAN_MAX_CHUNKS whatever Nv is.  Nothing is of size Nm x Nv, nothing waits for the host.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int MINE_MAX_CLIPS = 64;                   // as the fused scorer
constexpr int MINE_MAX_X = 8;                        // excluded spans per item
constexpr int MINE_INTRA_BUF = 1024;                 // key buffer of the intra scan (>= h + 64)

struct MineItem { int q, gv, s, e, lown, nown; bool wrong; };

// the item's row, checked: lown = the own video's local index (-1: another shard's), nown = its clip count (at most 64)
__device__ __forceinline__ MineItem mine_item(const int32_t *__restrict__ items, int64_t m, int64_t Nq,
                                              const int32_t *__restrict__ clip_off, int Nv, int64_t vid_base)
{
    MineItem it;
    it.q = items[4 * m]; it.gv = items[4 * m + 1]; it.s = items[4 * m + 2]; it.e = items[4 * m + 3];
    it.wrong = it.q < 0 || it.q >= Nq || it.gv < 0 || it.s < 0 || it.e < it.s;
    it.lown = -1; it.nown = 0;
    const int64_t l = (int64_t)it.gv - vid_base;
    if (it.gv >= 0 && l >= 0 && l < Nv) {
        int n = clip_off[l + 1] - clip_off[l];
        n = n > MINE_MAX_CLIPS ? MINE_MAX_CLIPS : n;
        it.lown = (int)l; it.nown = n;
        it.wrong |= it.e >= n;
    }
    return it;
}

// ---- score of named (query, video, span) items: one wave per item ----
template <bool FAST>
__global__ __launch_bounds__(64) void mine_spans_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                        const int32_t *__restrict__ clip_off, int Nv, int D, float eps,
                                                        int64_t vid_base, const int32_t *__restrict__ items, int64_t Np,
                                                        float *__restrict__ out, int *__restrict__ bad)
{
    __shared__ __attribute__((aligned(16))) float qs[FAST ? SCAN_FAST_D + 4 : 4];
    __shared__ float ds[MINE_MAX_CLIPS];
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const MineItem it = mine_item(items, p, Nq, clip_off, Nv, vid_base);
    if (it.wrong) {
        if (bad && lane == 0) *bad = 1;
        return;
    }
    if (it.lown < 0) return;                                   // another shard's video: untouched
    const float *qr = query_row<FAST>(Q, it.q, D, qs, lane);
    const int len = it.e - it.s + 1;                           // <= nown <= 64
    if (lane < len) {
        const float *vr = V + (int64_t)(clip_off[it.lown] + it.s + lane) * D;
        float d;
        if constexpr (FAST) clip_dist_fast<1>(vr, qr, eps, &d);
        else d = clip_dist_any(vr, qr, D, eps);
        ds[lane] = d;
    }
    __syncthreads();
    if (lane == 0) {
        float sum = ds[0];
        for (int c = 1; c < len; ++c) sum = sum + ds[c];
        out[p] = sum / (float)len;
    }
}

// ---- inter negatives: one wave per (item, chunk of the video axis), lane = video ----
template <bool FAST>
__global__ __launch_bounds__(64) void mine_inter_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                        const int32_t *__restrict__ clip_off, int Nv, int D, float eps,
                                                        int64_t vid_base, const int32_t *__restrict__ items, int64_t Nm, int h, int cap,
                                                        const float *__restrict__ floor_dist, const float *__restrict__ thr_dist,
                                                        int64_t *__restrict__ count_inter, int chunks, int64_t per,
                                                        int *__restrict__ bad, unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float *qs = ssm;                                                                       // [104] (fast path)
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ssm + (FAST ? SCAN_FAST_D + 4 : 0));   // [cap]
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - m * chunks);
    const MineItem it = mine_item(items, m, Nq, clip_off, Nv, vid_base);
    unsigned long long *out = ws + ((size_t)ch * Nm + m) * h;
    if (it.wrong) {                                            // padding, nothing added
        if (bad && lane == 0 && ch == 0) *bad = 1;
        for (int i = lane; i < h; i += 64) out[i] = SCAN_KEY_EMPTY;
        return;
    }
    const float *qr = query_row<FAST>(Q, it.q, D, qs, lane);
    const int s = it.s, e = it.e;
    const int len = e - s < MINE_MAX_CLIPS ? e - s + 1 : MINE_MAX_CLIPS + 1;   // a longer span fits no video (no e - s + 1 overflow)
    const float flen = (float)len;
    const bool has_floor = floor_dist != nullptr, has_thr = thr_dist != nullptr && count_inter != nullptr;
    const float floor = has_floor ? floor_dist[m] : 0.0f, tdist = has_thr ? thr_dist[m] : 0.0f;
    const int64_t v0 = (int64_t)ch * per;
    const int64_t v1 = v0 + per < Nv ? v0 + per : Nv;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned long long thr = SCAN_KEY_MAX;                     // keys >= thr cannot be among the chunk's h smallest
    int cnt = 0;                                               // keys in buf (wave-uniform)
    unsigned nlt = 0u;

    for (int64_t vb = v0; vb < v1; vb += 64) {
        const int64_t l = vb + lane;
        const int64_t gvl = vid_base + l;
        bool elig = l < v1 && gvl != (int64_t)it.gv;
        float sc = 0.0f;
        if (elig) {
            const int c0 = clip_off[l];
            elig = clip_off[l + 1] - c0 > e;                   // at least e + 1 clips: the span lies inside the video
            if (elig) {
                const float *vr = V + (int64_t)(c0 + s) * D;
                float sum = 0.0f;
                int c = 0;
                if constexpr (FAST) {
                    for (; c + 2 <= len; c += 2) {
                        float d[2];
                        clip_dist_fast<2>(vr + (int64_t)c * SCAN_FAST_D, qr, eps, d);
                        sum = c == 0 ? d[0] : sum + d[0];
                        sum = sum + d[1];
                    }
                    if (c < len) {
                        float d;
                        clip_dist_fast<1>(vr + (int64_t)c * SCAN_FAST_D, qr, eps, &d);
                        sum = c == 0 ? d : sum + d;
                    }
                } else {
                    for (; c < len; ++c) {
                        const float d = clip_dist_any(vr + (int64_t)c * D, qr, D, eps);
                        sum = c == 0 ? d : sum + d;
                    }
                }
                sc = sum / flen;
            }
        }
        if (has_thr) {
            const unsigned long long mlt = __ballot(elig && sc < tdist);
            nlt += (unsigned)__popcll(mlt);
        }
        if (h > 0) {
            const unsigned long long key = make_key(sc, (unsigned)gvl);
            const bool take = elig && !(has_floor && sc <= floor) && key < thr;
            const unsigned long long mt = __ballot(take);
            if (mt) {
                if (take) buf[cnt + __popcll(mt & below)] = key;
                cnt += __popcll(mt);
                if (cnt > cap - 64) {
                    __syncthreads();
                    wave_sort_keys(buf, cnt, cap, lane);
                    if (cnt >= h) { thr = buf[h - 1]; cnt = h; }
                    __syncthreads();
                }
            }
        }
    }
    if (h > 0) {                                               // the merge sorts: a list of at most h keys goes out as it stands
        __syncthreads();
        if (cnt > h) {
            wave_sort_keys(buf, cnt, cap, lane);
            cnt = h;
        }
        for (int i = lane; i < h; i += 64) out[i] = i < cnt ? buf[i] : SCAN_KEY_EMPTY;
    }
    if (has_thr && lane == 0 && nlt)
        atomicAdd(reinterpret_cast<unsigned long long *>(count_inter + m), (unsigned long long)nlt);
}

// ---- intra negatives: one wave per item on the shard of the own video; lane = clip, then lane = start clip ----
template <bool FAST>
__global__ __launch_bounds__(64) void mine_intra_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                        const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                        int Nv, int D, float eps, int64_t id_base, int64_t vid_base,
                                                        const int32_t *__restrict__ items, int64_t Nm, int h, int mode,
                                                        const int32_t *__restrict__ excl, int X, const float *__restrict__ floor_dist,
                                                        const float *__restrict__ thr_dist, float *__restrict__ intra_dist,
                                                        int64_t *__restrict__ intra_idx, int64_t *__restrict__ count_intra,
                                                        int *__restrict__ bad)
{
    __shared__ __attribute__((aligned(16))) float qs[FAST ? SCAN_FAST_D + 4 : 4];
    __shared__ float ds[MINE_MAX_CLIPS];
    __shared__ unsigned long long buf[MINE_INTRA_BUF];
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    const MineItem it = mine_item(items, m, Nq, clip_off, Nv, vid_base);
    if (it.wrong) {
        if (bad && lane == 0) *bad = 1;
        return;
    }
    if (it.lown < 0) return;                                   // the shard of the own video writes the intra list
    const float *qr = query_row<FAST>(Q, it.q, D, qs, lane);
    const int n = it.nown, s = it.s, e = it.e;
    if (lane < n) {
        const float *vr = V + (int64_t)(clip_off[it.lown] + lane) * D;
        float d;
        if constexpr (FAST) clip_dist_fast<1>(vr, qr, eps, &d);
        else d = clip_dist_any(vr, qr, D, eps);
        ds[lane] = d;
    }
    __syncthreads();
    const bool any = mode == VFR_MINE_ANY;
    int xs[MINE_MAX_X], xe[MINE_MAX_X];
#pragma unroll
    for (int j = 0; j < MINE_MAX_X; ++j) {
        const bool on = any && j < X;
        xs[j] = on ? excl[(m * X + j) * 2] : -1;
        xe[j] = on ? excl[(m * X + j) * 2 + 1] : -1;
    }
    const bool lists = h > 0 && intra_dist != nullptr;
    const bool has_floor = floor_dist != nullptr, has_thr = thr_dist != nullptr && count_intra != nullptr;
    const float floor = has_floor ? floor_dist[m] : 0.0f, tdist = has_thr ? thr_dist[m] : 0.0f;
    const int64_t mbase = id_base + mom_off[it.lown];
    const int L = e - s, Lmax = any ? n - 1 : L;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned long long thr = SCAN_KEY_MAX;
    int cnt = 0, nlt = 0;
    float sum = 0.0f;
    for (int Lp = 0; Lp <= Lmax; ++Lp) {                       // lane = start clip s', end clip e' = s' + Lp: the sum runs s' -> e'
        const int e2 = lane + Lp;
        const bool live = e2 < n;
        const float de = live ? ds[e2] : 0.0f;
        sum = Lp == 0 ? de : sum + de;
        if (!any && Lp != L) continue;
        bool emit = live && !(lane == s && e2 == e);
#pragma unroll
        for (int j = 0; j < MINE_MAX_X; ++j) emit = emit && !(lane == xs[j] && e2 == xe[j]);
        const float sc = sum / (float)(Lp + 1);
        if (has_thr) nlt += (emit && sc < tdist) ? 1 : 0;
        if (lists) {
            const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, lane, e2)));
            const bool take = emit && !(has_floor && sc <= floor) && key < thr;
            const unsigned long long mt = __ballot(take);
            if (mt) {
                if (take) buf[cnt + __popcll(mt & below)] = key;
                cnt += __popcll(mt);
                if (cnt > MINE_INTRA_BUF - 64) {
                    __syncthreads();
                    wave_sort_keys(buf, cnt, MINE_INTRA_BUF, lane);
                    if (cnt >= h) { thr = buf[h - 1]; cnt = h; }
                    __syncthreads();
                }
            }
        }
    }
    if (lists) {
        __syncthreads();
        int size = 64;
        while (size < cnt) size <<= 1;
        wave_sort_keys(buf, cnt, size, lane);
        cnt = cnt > h ? h : cnt;
        for (int i = lane; i < h; i += 64) {
            const unsigned long long x = i < cnt ? buf[i] : 0ull;
            intra_dist[m * h + i] = i < cnt ? __uint_as_float((unsigned)(x >> 32)) : __builtin_inff();
            intra_idx[m * h + i] = i < cnt ? (int64_t)(unsigned)x : -1;
        }
    }
    if (has_thr) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nlt += __shfl_xor(nlt, o, 64);
        if (lane == 0 && nlt) atomicAdd(reinterpret_cast<unsigned long long *>(count_intra + m), (unsigned long long)nlt);
    }
}

}  // namespace
}  // namespace vfr

extern "C" {

int vfr_score_spans_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                        int max_clips, int D, float eps, int64_t vid_base, const int32_t *items, int64_t Np, float *out, int *bad,
                        vfr_stream_t stream)
{
    VFR_REQUIRE(Nq >= 0 && Np >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && max_clips >= 0 && max_clips <= vfr::MINE_MAX_CLIPS &&
                vid_base >= 0, VFR_EINVAL, "vfr_score_spans_f32: bad shape (max_clips <= 64, sizes, vid_base >= 0)");
    VFR_REQUIRE(vid_base + Nv < (int64_t(1) << 32), VFR_EINVAL, "vfr_score_spans_f32: vid_base + Nv must stay below 2^32");
    VFR_REQUIRE(Np <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_spans_f32: Np must stay below 2^31");
    VFR_REQUIRE(Np == 0 || (items && out), VFR_EINVAL, "vfr_score_spans_f32: items / out is null");
    VFR_REQUIRE(Np == 0 || Nq == 0 || Q, VFR_EINVAL, "vfr_score_spans_f32: Q is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && (V || total_clips == 0)), VFR_EINVAL, "vfr_score_spans_f32: null clip bank");
    if (Np == 0) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, st);
    const dim3 grid((unsigned)Np), block(64);
    if (vfr::rows_fast(Q, V, D))
        hipLaunchKernelGGL((vfr::mine_spans_kernel<true>), grid, block, 0, st, Q, Nq, V, clip_offsets, Nv, D, eps, vid_base, items, Np, out,
                           bad);
    else
        hipLaunchKernelGGL((vfr::mine_spans_kernel<false>), grid, block, 0, st, Q, Nq, V, clip_offsets, Nv, D, eps, vid_base, items, Np, out,
                           bad);
    VFR_CHECK_LAUNCH("mine_spans_kernel");
    return VFR_OK;
}

size_t vfr_mine_negatives_workspace_bytes(int64_t Nm, int Nv, int h)
{
    if (Nm < 0 || Nv < 0 || h < 0 || h > vfr::SCAN_MAX_K || Nm * (int64_t)(h > 0 ? h : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(Nm, Nv, vfr::SCAN_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Nm * (size_t)h * 8 + 256, 256);
}

int vfr_mine_negatives_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets,
                           int Nv, int total_clips, int max_clips, int D, float eps, int64_t id_base, int64_t vid_base,
                           const int32_t *items, int64_t Nm, int h, int intra_mode, const int32_t *excl, int X,
                           const float *floor_dist, const float *thr_dist, float *inter_dist, int64_t *inter_vid, float *intra_dist,
                           int64_t *intra_idx, int64_t *count_inter, int64_t *count_intra, int *bad, void *workspace,
                           size_t workspace_bytes, vfr_stream_t stream)
{
    VFR_REQUIRE(Nq >= 0 && Nm >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && h >= 0 && h <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::MINE_MAX_CLIPS && id_base >= 0 && vid_base >= 0, VFR_EINVAL,
                "vfr_mine_negatives_f32: bad shape (h <= 448, max_clips <= 64, sizes, id_base, vid_base >= 0)");
    VFR_REQUIRE(intra_mode == VFR_MINE_SAME_LENGTH || intra_mode == VFR_MINE_ANY, VFR_EINVAL,
                "vfr_mine_negatives_f32: intra_mode %d (0 = same length, 1 = any)", intra_mode);
    VFR_REQUIRE(X >= 0 && X <= vfr::MINE_MAX_X, VFR_EINVAL, "vfr_mine_negatives_f32: X = %d excluded spans per item (0 .. 8)", X);
    VFR_REQUIRE(vid_base + Nv < (int64_t(1) << 32), VFR_EINVAL, "vfr_mine_negatives_f32: vid_base + Nv must stay below 2^32");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_mine_negatives_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(Nm * (int64_t)(h > 0 ? h : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_mine_negatives_f32: Nm * h must stay below 2^31");
    VFR_REQUIRE((inter_dist == nullptr) == (inter_vid == nullptr) && (intra_dist == nullptr) == (intra_idx == nullptr), VFR_EINVAL,
                "vfr_mine_negatives_f32: a list needs both of its arrays");
    VFR_REQUIRE((count_inter == nullptr && count_intra == nullptr) == (thr_dist == nullptr), VFR_EINVAL,
                "vfr_mine_negatives_f32: thr_dist comes with count_inter / count_intra");
    VFR_REQUIRE(Nm == 0 || items, VFR_EINVAL, "vfr_mine_negatives_f32: items is null");
    VFR_REQUIRE(Nm == 0 || Nq == 0 || Q, VFR_EINVAL, "vfr_mine_negatives_f32: Q is null");
    VFR_REQUIRE(intra_mode != VFR_MINE_ANY || X == 0 || Nm == 0 || excl, VFR_EINVAL, "vfr_mine_negatives_f32: excl is null with X > 0");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets && (V || total_clips == 0)), VFR_EINVAL,
                "vfr_mine_negatives_f32: null clip bank");
    const vfr::ScanPlan plan = vfr::scan_plan(Nm, Nv, vfr::SCAN_TARGET_WAVES);
    VFR_REQUIRE(Nm * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_mine_negatives_f32: too many (item, chunk) waves");
    const size_t need = vfr_mine_negatives_workspace_bytes(Nm, Nv, h);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_mine_negatives_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    if (Nm == 0) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    const bool fast = vfr::rows_fast(Q, V, D);
    const bool inter_lists = h > 0 && inter_dist != nullptr, intra_lists = h > 0 && intra_dist != nullptr;
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    if (intra_lists || count_intra || (bad && !inter_lists && !count_inter)) {
        vfr::ProfScope prof(vfr::SITE_SCORE_OWN, st);
        const dim3 grid((unsigned)Nm), block(64);
        if (fast)
            hipLaunchKernelGGL((vfr::mine_intra_kernel<true>), grid, block, 0, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps,
                               id_base, vid_base, items, Nm, h, intra_mode, excl, X, floor_dist, thr_dist, intra_dist, intra_idx,
                               count_intra, bad);
        else
            hipLaunchKernelGGL((vfr::mine_intra_kernel<false>), grid, block, 0, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps,
                               id_base, vid_base, items, Nm, h, intra_mode, excl, X, floor_dist, thr_dist, intra_dist, intra_idx,
                               count_intra, bad);
        VFR_CHECK_LAUNCH("mine_intra_kernel");
    }
    if (inter_lists || count_inter) {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        const int hh = inter_lists ? h : 0;
        const int cap = vfr::scan_cap(hh);
        const size_t lds = (fast ? (size_t)(vfr::SCAN_FAST_D + 4) * 4 : 0) + (size_t)cap * 8;
        const dim3 grid((unsigned)(Nm * plan.chunks)), block(64);
        if (fast)
            hipLaunchKernelGGL((vfr::mine_inter_kernel<true>), grid, block, lds, st, Q, Nq, V, clip_offsets, Nv, D, eps, vid_base, items,
                               Nm, hh, cap, floor_dist, thr_dist, count_inter, plan.chunks, plan.per, bad, keys);
        else
            hipLaunchKernelGGL((vfr::mine_inter_kernel<false>), grid, block, lds, st, Q, Nq, V, clip_offsets, Nv, D, eps, vid_base, items,
                               Nm, hh, cap, floor_dist, thr_dist, count_inter, plan.chunks, plan.per, bad, keys);
        VFR_CHECK_LAUNCH("mine_inter_kernel");
        if (inter_lists)
            return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Nm, h, inter_dist, inter_vid, nullptr, stream);
    }
    return VFR_OK;
}

}  // extern "C"
