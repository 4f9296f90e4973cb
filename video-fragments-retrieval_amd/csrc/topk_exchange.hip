// What a multi-GPU evaluation runs around the scorer: the merge of the per-shard top-k lists after the all-gather and the packed
// int64 keys the ranks exchange (topk_*), the labels of the annotated moments (a11) and the best ground-truth-positive key per
// (threshold, query) -- the rank keys of vfr_score_topk_* (gt_*).  Keys are (fp32 bits of score << 32 | moment id), as in score.hip.
#include "score_device.h"
#include "score_internal.h"

namespace vfr {

// merge G shard lists [G, Nq, k] -> [Nq, k] (after the all-gather, 8e).  Lists arrive either as (dist, idx) arrays or as
// the packed int64 keys the ranks exchange (KEY_EMPTY = (+inf, 0xffffffff) marks an unused slot).  Same LDS pool as the
// task merge: all G*k keys are read as one flat sequence, CAP per round with the loads in flight together, and a key is
// appended only if it beats the running k-th key -- after the first round almost nothing is, so a query costs ~2 sorts.
template <int KPL, bool PACKED>
__global__ __launch_bounds__(256) void topk_merge_parts_kernel(const float *__restrict__ pd,
                                                               const int64_t *__restrict__ pi, int64_t slot_stride,
                                                               int64_t q_stride, int G, int64_t Nq, int k,
                                                               float *__restrict__ out_dist,
                                                               int64_t *__restrict__ out_idx,
                                                               int64_t *__restrict__ out_keys)
{
    constexpr int CAP = KPL * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wv;
    if (q >= Nq) return;
    __shared__ unsigned long long pool_s[4][CAP];
    unsigned long long *pool = pool_s[wv];
    unsigned long long key[KPL];
    unsigned long long thr = KEY_MAX;
    int fill = 0;
    auto lds_sync = [&]() { __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_wave_barrier(); };
    auto sort_pool = [&](bool final_pass) {
        lds_sync();
#pragma unroll
        for (int i = 0; i < KPL; ++i) { const int e = i * 64 + lane; key[i] = e < fill ? pool[e] : KEY_MAX; }
        wave_sort<KPL>(key, lane);
        if (final_pass) return;
        lds_sync();
#pragma unroll
        for (int i = 0; i < KPL; ++i) { const int e = i * 64 + lane; if (e < k) pool[e] = key[i]; }
        if (fill >= k) thr = key_at<KPL>(key, k - 1);
        fill = fill < k ? fill : k;
    };
    const int total = G * k;
    for (int done = 0; done < total; done += CAP) {
        unsigned long long x[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int gi = done + i * 64 + lane;
            x[i] = KEY_MAX;
            if (gi < total) {
                const int g = gi / k, off = gi - g * k;
                const int64_t at = (int64_t)g * slot_stride + q * q_stride + off;  // [G, Nq, k]: slot_stride = Nq * k, q_stride = k
                if constexpr (PACKED) {
                    const unsigned long long v = (unsigned long long)pi[at];
                    x[i] = v >= KEY_EMPTY ? KEY_MAX : v;
                } else {
                    const int64_t id = pi[at];
                    x[i] = id < 0 ? KEY_MAX : make_key(pd[at], (unsigned)id);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            if (fill + 64 > CAP) sort_pool(false);
            const bool pass = x[i] < thr;                        // KEY_MAX (empty) never passes
            const unsigned long long m = __ballot(pass);
            if (pass) pool[fill + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = x[i];
            fill += __builtin_popcountll(m);
        }
    }
    sort_pool(true);
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        int e = i * 64 + lane;
        if (e < k) {
            const bool ok = key[i] != KEY_MAX;
            if (out_dist) {
                out_dist[q * k + e] = ok ? __uint_as_float((unsigned)(key[i] >> 32)) : __builtin_inff();
                out_idx[q * k + e] = ok ? (int64_t)(key[i] & 0xffffffffull) : -1;
            }
            if (out_keys) out_keys[q * k + e] = (int64_t)(ok ? key[i] : KEY_EMPTY);
        }
    }
}

// (dist, idx) lists -> the packed int64 keys the ranks exchange (one collective instead of two); idx < 0 -> KEY_EMPTY
__global__ __launch_bounds__(256) void topk_pack_keys_kernel(const float *__restrict__ d, const int64_t *__restrict__ ix,
                                                             int64_t n, int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ix[i];
    keys[i] = (int64_t)(id < 0 ? KEY_EMPTY : make_key(d[i], (unsigned)id));
}

// best ground-truth-positive key per (threshold, query):  min over the labelled moments of the query's own video of
// (score, global id)  (evaluate.py:67-77: the first positive in the sorted order).  One wave per selected query.
__global__ __launch_bounds__(256) void gt_fill_keys_kernel(int64_t n, int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = (int64_t)KEY_EMPTY;
}
// the same initialisation with the unpacked forms of vfr_gt_rank_keys_f32: distance +inf, id 0xffffffff, counts 0, flag 0
__global__ __launch_bounds__(256) void gt_fill_rank_kernel(int64_t n, int64_t *__restrict__ keys, float *__restrict__ rank_dist,
                                                           int64_t *__restrict__ rank_idx, int64_t *__restrict__ count0,
                                                           int *__restrict__ missing)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && missing) *missing = 0;
    if (i >= n) return;
    keys[i] = (int64_t)KEY_EMPTY;
    if (rank_dist) { rank_dist[i] = __builtin_inff(); rank_idx[i] = 0xFFFFFFFFll; }
    if (count0) count0[i] = 0;
}
__global__ __launch_bounds__(256) void gt_best_keys_kernel(const float *__restrict__ sc, int64_t n_sel, int M,
                                                           int score_stride, const uint8_t *__restrict__ labels, int R,
                                                           int label_stride, const int64_t *__restrict__ id_base,
                                                           const int64_t *__restrict__ sel, int64_t Nq,
                                                           int64_t *__restrict__ keys, float *__restrict__ rank_dist = nullptr,
                                                           int64_t *__restrict__ rank_idx = nullptr, int *__restrict__ missing = nullptr)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_sel) return;
    const int64_t base = id_base[s], q = sel[s];
    for (int r = 0; r < R; ++r) {
        unsigned long long best = KEY_MAX;
        const uint8_t *lab = labels + ((int64_t)r * n_sel + s) * label_stride;
        for (int m = lane; m < M; m += 64)
            if (lab[m]) {
                const unsigned long long kk = make_key(sc[s * score_stride + m], (unsigned)(base + m));
                best = kk < best ? kk : best;
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) {
            const unsigned long long kq = best >= KEY_EMPTY ? KEY_EMPTY : best;
            keys[(int64_t)r * Nq + q] = (int64_t)kq;
            if (rank_dist) {
                rank_dist[(int64_t)r * Nq + q] = __uint_as_float((unsigned)(kq >> 32));
                rank_idx[(int64_t)r * Nq + q] = (int64_t)(kq & 0xffffffffull);
            }
            if (missing && kq == KEY_EMPTY) atomicOr(missing, 1);
        }
    }
}

// a11 (model/evaluate.py:59-62, utils.get_iou model/utils.py:78-82): labels[r][q][m] = 1 iff at least two annotators have
// IoU > (or >=) thr[r] with local moment m of the query's own video.  One thread per (query, moment); the IoU is the
// reference's float64 intersection / union (IEEE division: the same bits as numpy's).
constexpr int MAX_LABEL_THR = 16;
struct LabelThr { double t[MAX_LABEL_THR]; };
__global__ __launch_bounds__(256) void gt_labels_kernel(const int32_t *__restrict__ times, const int32_t *__restrict__ nannot,
                                                        const int32_t *__restrict__ n_own, int64_t Nq, int A, int R,
                                                        LabelThr thr, int strict, int Mmax, uint8_t *__restrict__ labels)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq * Mmax) return;
    const int64_t q = i / Mmax;
    const int m = (int)(i - q * Mmax), n = n_own[q];
    int s = m, e = m;                                     // generate_moments order: (j, j) first, then combinations
    bool real = m < n * (n + 1) / 2;
    if (real && m >= n) {
        int rest = m - n;
        s = 0;
        while (rest >= n - 1 - s) { rest -= n - 1 - s; ++s; }
        e = s + 1 + rest;
    }
    int cnt[MAX_LABEL_THR];
#pragma unroll
    for (int r = 0; r < MAX_LABEL_THR; ++r) cnt[r] = 0;
    const int na = nannot[q];
    for (int a = 0; a < na && real; ++a) {
        const int ts = times[(q * A + a) * 2], te = times[(q * A + a) * 2 + 1];
        const int inter = max(min(te, e) + 1 - max(ts, s), 0), uni = max(te, e) + 1 - min(ts, s);
        const double iou = (double)inter / (double)uni;
#pragma unroll
        for (int r = 0; r < MAX_LABEL_THR; ++r)
            if (r < R) cnt[r] += (strict ? iou > thr.t[r] : iou >= thr.t[r]) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < MAX_LABEL_THR; ++r)
        if (r < R) labels[((int64_t)r * Nq + q) * Mmax + m] = cnt[r] >= 2 ? 1 : 0;
}

}  // namespace vfr

extern "C" {

static int launch_merge_parts(const float *pd, const int64_t *pi, bool packed, int G, int64_t Nq, int k, float *od,
                              int64_t *oi, int64_t *okeys, vfr_stream_t stream, int64_t slot_stride = 0, int64_t q_stride = 0)
{
    if (slot_stride == 0) slot_stride = Nq * k;
    if (q_stride == 0) q_stride = k;
    dim3 grid((unsigned)vfr::cdiv(Nq, 4)), block(256);
    const int kpl = vfr::kpl_for(k);
    vfr::ProfScope prof(vfr::SITE_EXCHANGE, vfr::as_stream(stream));
#define VFR_MERGE(KPL, PACKED) hipLaunchKernelGGL((vfr::topk_merge_parts_kernel<KPL, PACKED>), grid, block, 0, \
                                                  vfr::as_stream(stream), pd, pi, slot_stride, q_stride, G, Nq, k, od, oi, okeys)
    if (packed) { if (kpl == 4) VFR_MERGE(4, true); else VFR_MERGE(8, true); }
    else        { if (kpl == 4) VFR_MERGE(4, false); else VFR_MERGE(8, false); }
#undef VFR_MERGE
    VFR_CHECK_LAUNCH("topk_merge_parts_kernel");
    return VFR_OK;
}

int vfr_topk_merge_f32(const float *part_dist, const int64_t *part_idx, int G, int64_t Nq, int k, float *out_dist,
                       int64_t *out_idx, vfr_stream_t stream)
{
    VFR_REQUIRE(part_dist && part_idx && out_dist && out_idx && G > 0 && Nq >= 0 && k > 0, VFR_EINVAL,
                "vfr_topk_merge_f32: bad argument");
    VFR_REQUIRE(k <= 448, VFR_EUNSUPPORTED, "vfr_topk_merge_f32: k=%d > 448", k);
    VFR_REQUIRE((int64_t)G * k < (1ll << 31), VFR_EUNSUPPORTED, "vfr_topk_merge_f32: G*k too large");
    if (Nq == 0) return VFR_OK;
    return launch_merge_parts(part_dist, part_idx, false, G, Nq, k, out_dist, out_idx, nullptr, stream);
}

int vfr_topk_pack_keys(const float *dist, const int64_t *idx, int64_t n, int64_t *keys, vfr_stream_t stream)
{
    VFR_REQUIRE(n >= 0 && (n == 0 || (dist && idx && keys)), VFR_EINVAL, "vfr_topk_pack_keys: bad argument");
    if (n == 0) return VFR_OK;
    vfr::ProfScope prof(vfr::SITE_EXCHANGE, vfr::as_stream(stream));
    hipLaunchKernelGGL(vfr::topk_pack_keys_kernel, dim3((unsigned)vfr::cdiv(n, 256)), dim3(256), 0,
                       vfr::as_stream(stream), dist, idx, n, keys);
    VFR_CHECK_LAUNCH("topk_pack_keys_kernel");
    return VFR_OK;
}

int vfr_topk_merge_keys_strided(const int64_t *part_keys, int64_t slot_stride, int G, int64_t Nq, int k, float *out_dist,
                                int64_t *out_idx, int64_t *out_keys, vfr_stream_t stream)
{
    VFR_REQUIRE(part_keys && G > 0 && Nq >= 0 && k > 0 && ((out_dist && out_idx) || out_keys) &&
                (out_dist == nullptr) == (out_idx == nullptr) && slot_stride >= Nq * k, VFR_EINVAL,
                "vfr_topk_merge_keys: bad argument");
    VFR_REQUIRE(k <= 448, VFR_EUNSUPPORTED, "vfr_topk_merge_keys: k=%d > 448", k);
    VFR_REQUIRE((int64_t)G * k < (1ll << 31), VFR_EUNSUPPORTED, "vfr_topk_merge_keys: G*k too large");
    if (Nq == 0) return VFR_OK;
    return launch_merge_parts(nullptr, part_keys, true, G, Nq, k, out_dist, out_idx, out_keys, stream, slot_stride);
}

int vfr_topk_merge_keys(const int64_t *part_keys, int G, int64_t Nq, int k, float *out_dist, int64_t *out_idx,
                        int64_t *out_keys, vfr_stream_t stream)
{
    return vfr_topk_merge_keys_strided(part_keys, Nq * k, G, Nq, k, out_dist, out_idx, out_keys, stream);
}

int vfr_gt_best_keys_f32(const float *own_scores, int64_t n_sel, int M, int score_stride, const uint8_t *labels, int R,
                         int label_stride, const int64_t *id_base, const int64_t *sel, int64_t Nq, int64_t *keys,
                         vfr_stream_t stream)
{
    VFR_REQUIRE(keys && R > 0 && Nq >= 0 && n_sel >= 0 && M >= 0 && score_stride >= M && label_stride >= M, VFR_EINVAL,
                "vfr_gt_best_keys_f32: bad argument");
    VFR_REQUIRE(n_sel == 0 || (own_scores && labels && id_base && sel), VFR_EINVAL, "vfr_gt_best_keys_f32: null input");
    if (Nq == 0) return VFR_OK;
    vfr::ProfScope prof(vfr::SITE_EXCHANGE, vfr::as_stream(stream));
    hipLaunchKernelGGL(vfr::gt_fill_keys_kernel, dim3((unsigned)vfr::cdiv((int64_t)R * Nq, 256)), dim3(256), 0,
                       vfr::as_stream(stream), (int64_t)R * Nq, keys);
    VFR_CHECK_LAUNCH("gt_fill_keys_kernel");
    if (n_sel == 0) return VFR_OK;
    hipLaunchKernelGGL(vfr::gt_best_keys_kernel, dim3((unsigned)vfr::cdiv(n_sel, 4)), dim3(256), 0, vfr::as_stream(stream),
                       own_scores, n_sel, M, score_stride, labels, R, label_stride, id_base, sel, Nq, keys);
    VFR_CHECK_LAUNCH("gt_best_keys_kernel");
    return VFR_OK;
}

int vfr_gt_rank_keys_f32(const float *own_scores, int64_t n_sel, int M, int score_stride, const uint8_t *labels, int R,
                         int label_stride, const int64_t *id_base, const int64_t *sel, int64_t Nq, int64_t *keys,
                         float *rank_dist, int64_t *rank_idx, int64_t *count_zero, int *missing, vfr_stream_t stream)
{
    VFR_REQUIRE(keys && R > 0 && Nq >= 0 && n_sel >= 0 && M >= 0 && score_stride >= M && label_stride >= M, VFR_EINVAL,
                "vfr_gt_rank_keys_f32: bad argument");
    VFR_REQUIRE(n_sel == 0 || (own_scores && labels && id_base && sel), VFR_EINVAL, "vfr_gt_rank_keys_f32: null input");
    VFR_REQUIRE((rank_dist == nullptr) == (rank_idx == nullptr), VFR_EINVAL, "vfr_gt_rank_keys_f32: rank_dist and rank_idx go together");
    if (Nq == 0) return VFR_OK;
    vfr::ProfScope prof(vfr::SITE_EXCHANGE, vfr::as_stream(stream));
    hipLaunchKernelGGL(vfr::gt_fill_rank_kernel, dim3((unsigned)vfr::cdiv((int64_t)R * Nq, 256)), dim3(256), 0, vfr::as_stream(stream),
                       (int64_t)R * Nq, keys, rank_dist, rank_idx, count_zero, missing);
    VFR_CHECK_LAUNCH("gt_fill_rank_kernel");
    if (n_sel == 0) return VFR_OK;
    hipLaunchKernelGGL(vfr::gt_best_keys_kernel, dim3((unsigned)vfr::cdiv(n_sel, 4)), dim3(256), 0, vfr::as_stream(stream),
                       own_scores, n_sel, M, score_stride, labels, R, label_stride, id_base, sel, Nq, keys, rank_dist, rank_idx, missing);
    VFR_CHECK_LAUNCH("gt_best_keys_kernel");
    return VFR_OK;
}

int vfr_gt_labels_u8(const int32_t *times, const int32_t *nannot, const int32_t *n_own, int64_t Nq, int A,
                     const double *thresholds_host, int R, int strict, int Mmax, uint8_t *labels, vfr_stream_t stream)
{
    VFR_REQUIRE(Nq >= 0 && A >= 0 && Mmax >= 0 && R > 0 && thresholds_host, VFR_EINVAL, "vfr_gt_labels_u8: bad argument");
    VFR_REQUIRE(R <= vfr::MAX_LABEL_THR, VFR_EUNSUPPORTED, "vfr_gt_labels_u8: R=%d > %d thresholds", R, vfr::MAX_LABEL_THR);
    if (Nq == 0 || Mmax == 0) return VFR_OK;
    VFR_REQUIRE(times && nannot && n_own && labels, VFR_EINVAL, "vfr_gt_labels_u8: null pointer");
    vfr::LabelThr t{};
    for (int r = 0; r < R; ++r) t.t[r] = thresholds_host[r];
    vfr::ProfScope prof(vfr::SITE_EXCHANGE, vfr::as_stream(stream));
    hipLaunchKernelGGL(vfr::gt_labels_kernel, dim3((unsigned)vfr::cdiv(Nq * Mmax, 256)), dim3(256), 0, vfr::as_stream(stream),
                       times, nannot, n_own, Nq, A, R, t, strict, Mmax, labels);
    VFR_CHECK_LAUNCH("gt_labels_kernel");
    return VFR_OK;
}

}  // extern "C"
