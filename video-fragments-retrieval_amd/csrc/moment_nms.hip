// Diversified moment retrieval (on top of video_topk.hip: phase 1 IS the video top-k call).
//
// Question: the k best MOMENTS of a query, but not k shifted copies of one span of one strong video.  Keys, ids and scores are
// exactly those of vfr_score_topk_f32: key = (fp32 distance, global moment id) ascending, id = id_base + mom_off[v] + j, j the
// position in utils.generate_moments(n_v); moment j of video v covers the inclusive clip span (s_j, e_j).
//
// Rule.  Per query and per video v, v's moments are taken in ascending key order and accepted greedily:
//   * b is SUPPRESSED when IoU(a, b) > nms_iou for an already accepted moment a of the same video;  IoU = utils.get_iou on the
//     inclusive spans, in float64:  inter = max(min(e_a, e_b) + 1 - max(s_a, s_b), 0),  union = max(e_a, e_b) + 1 - min(s_a, s_b);
//   * at most per_video moments are accepted (0 = no cap; values >= k act as k).
// nms_iou >= 1 suppresses nothing (distinct spans have IoU < 1); nms_iou = 0 keeps disjoint spans only.  Result: the k smallest
// accepted keys over the bank, padded with (+inf, -1).
//
// Exact IoU test.  inter / u > nms_iou is monotone in the integer inter for a fixed union u, so the host turns the double
// nms_iou into min_inter[u] = the smallest inter with (double)inter / u > nms_iou (u + 1 when there is none,
// vfr_nms_inter_table) and the kernel compares integers: suppressed <=> inter >= min_inter[union].  (An fp32 comparison is
// wrong at the boundary: 7/10 > 0.69999999 in double, not once both sides are rounded to fp32.)
//
// Consequences used here:
//   * a video's best key is always accepted (nothing precedes it), so per_video = 1 is the video top-k (identity A), and with
//     no cap (or a cap >= k) and nms_iou >= 1 every moment is accepted: the moment top-k (identity B);
//   * every accepted key x in the top-k belongs to one of the query's k best videos: each video ranked ahead of x's video puts
//     its (accepted) best key ahead of x, and fewer than k accepted keys precede x.  More sharply: with T* = the k-th best video
//     key (KEY_MAX when the bank has fewer than k videos), the k best videos hold k accepted keys <= T*, so every key of the
//     top-k is <= T*;
//   * NMS never crosses a video, and a video never spans shards: per-shard lists merge with the moment-key merge.
//
// Kernels (two phases):
//   phase 1   vfr_score_video_topk_f32 unchanged (bounds / select / exact / top-k, or the exact path), into the workspace:
//             each query's k best videos as (best distance, best moment id), hence T*
//   mnms_scan_kernel   one wave per (query, listed video): the video's clip distances with the canonical chain of
//             vtk_exact_kernel (k-ascending fmaf of ((v - q) + eps)^2, IEEE sqrt), its whole triangle (running sums,
//             IEEE divide), then the greedy loop: each round drops what the last accepted moment suppresses and takes the
//             smallest live key; it stops at min(per_video, k) accepted, at a key > T*, or when nothing is live.
//             Buffer: Nq x k x min(per_video, k) keys, KEY_MAX padded.  The bound is exact (only the k best videos can hold a
//             key <= T*, and none can contribute more than min(per_video, k) keys to a top-k).
//   mnms_topk_kernel   per query: the k smallest keys of its k x P buffer row (radix threshold on the high then the low word,
//             then a bitonic sort of <= k keys), padded with (+inf, -1)
#include "video_topk.h"

namespace vfr {

constexpr int MNMS_SORT = 512;                         // >= k (k <= 448)

struct MnmsTab { int min_inter[NMAX_FUSED + 1]; };     // suppressed <=> inter >= min_inter[union], union <= 64
constexpr int MNMS_TAB = (NMAX_FUSED + 1 + 3) & ~3;   // its LDS copy, 16-byte multiple

// ---- phase 2: one wave per (query, slot of the query's video top-k list) ----
// LDS: qs [D, rounded to 4] | ds [64] clip distances | min_inter [68] | keys [Mmax] | spans [Mmax] (s | e << 8)
__global__ __launch_bounds__(64) void mnms_scan_kernel(const float *__restrict__ Q, const float *__restrict__ V,
                                                       const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                       int Nv, int D, float eps, int64_t id_base, int k, int P, int Mmax,
                                                       MnmsTab tab, const float *__restrict__ vd, const int64_t *__restrict__ vi,
                                                       unsigned long long *__restrict__ buf)
{
    extern __shared__ __attribute__((aligned(16))) float msm[];
    float *qs = msm;
    float *ds = msm + ((D + 3) & ~3);
    int *min_inter = reinterpret_cast<int *>(ds + 64);
    unsigned long long *mk = reinterpret_cast<unsigned long long *>(min_inter + MNMS_TAB);
    unsigned short *msp = reinterpret_cast<unsigned short *>(mk + Mmax);
    const int lane = threadIdx.x;
    const int64_t item = blockIdx.x, q = item / k;
    unsigned long long *out = buf + item * P;
    const int64_t g = vi[item];
    if (g < 0) {                                        // fewer than k videos in the bank
        for (int r = lane; r < P; r += 64) out[r] = KEY_MAX;
        return;
    }
    const int64_t glast = vi[q * k + k - 1];
    const unsigned long long T = glast < 0 ? KEY_MAX : make_key(vd[q * k + k - 1], (unsigned)glast);
    // the video of global moment id g: the last v with mom_off[v] <= g - id_base (never an empty video: its successor starts there)
    const int64_t local = g - id_base;
    int lo = 0, hi = Nv - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mom_off[mid] <= local) lo = mid; else hi = mid - 1;
    }
    const int v = lo;
    const int c0 = clip_off[v], n = clip_off[v + 1] - c0;
    const int M = n * (n + 1) / 2;
    for (int i = lane; i < D; i += 64) qs[i] = Q[q * D + i];
    for (int i = lane; i <= NMAX_FUSED; i += 64) min_inter[i] = tab.min_inter[i];
    __syncthreads();
    if (lane < n) {                                     // clip distance: the canonical chain of vtk_exact_kernel
        const float *vr = V + (int64_t)(c0 + lane) * D;
        float acc = 0.0f;
        if ((D & 3) == 0 && (((uintptr_t)V) & 15) == 0) {
            for (int k4 = 0; k4 < D; k4 += 4) {
                const float4 x = *reinterpret_cast<const float4 *>(vr + k4), y = *reinterpret_cast<const float4 *>(qs + k4);
                float t = (x.x - y.x) + eps; acc = __builtin_fmaf(t, t, acc);
                t = (x.y - y.y) + eps; acc = __builtin_fmaf(t, t, acc);
                t = (x.z - y.z) + eps; acc = __builtin_fmaf(t, t, acc);
                t = (x.w - y.w) + eps; acc = __builtin_fmaf(t, t, acc);
            }
        } else {
            for (int kk = 0; kk < D; ++kk) {
                const float t = (vr[kk] - qs[kk]) + eps;
                acc = __builtin_fmaf(t, t, acc);
            }
        }
        ds[lane] = __builtin_sqrtf(acc);
    }
    __syncthreads();
    const int64_t mbase = id_base + mom_off[v];
    if (lane < n) {                                     // lane = start clip s: row s of the triangle at s n - s (s - 1) / 2
        const int s = lane, ro = s * n - s * (s - 1) / 2;
        float sum = 0.0f;
        for (int e = s; e < n; ++e) {
            const float de = ds[e];
            sum = e == s ? de : sum + de;
            const float sc = sum / (float)(e - s + 1);
            mk[ro + e - s] = make_key(sc, (unsigned)(mbase + moment_index(n, s, e)));
            msp[ro + e - s] = (unsigned short)(s | (e << 8));
        }
    }
    __syncthreads();
    // greedy accept loop; entry i is owned by lane i % 64 for the whole loop (no barrier between rounds)
    int na = 0, as = 0, ae = -1;
    unsigned long long last = KEY_MAX;
    while (na < P) {
        unsigned long long mine = KEY_MAX;
        int mi = -1;
        for (int i = lane; i < M; i += 64) {
            const unsigned long long x = mk[i];
            if (x == KEY_MAX) continue;
            if (ae >= 0) {
                const int sp = msp[i], s = sp & 255, e = sp >> 8;
                const int inter = (e < ae ? e : ae) + 1 - (s > as ? s : as);
                const int uni = (e > ae ? e : ae) + 1 - (s < as ? s : as);
                if (x == last || inter >= min_inter[uni]) { mk[i] = KEY_MAX; continue; }
            }
            if (x < mine) { mine = x; mi = i; }
        }
        unsigned long long best = mine;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long y = __shfl_xor(best, o, 64);
            best = y < best ? y : best;
        }
        if (best >= KEY_EMPTY || best > T) break;       // nothing live (KEY_MAX), an inf / NaN score, or past T*
        const unsigned long long owner = __ballot(mine == best);
        const int bi = __shfl(mi, __ffsll((long long)owner) - 1, 64);
        const int sp = msp[bi];
        as = sp & 255;
        ae = sp >> 8;
        last = best;
        if (lane == 0) out[na] = best;
        ++na;
    }
    for (int r = na + lane; r < P; r += 64) out[r] = KEY_MAX;
}

// ---- per query: the k smallest keys of its k x P buffer row, sorted; (+inf, -1) past the accepted keys ----
__global__ __launch_bounds__(256) void mnms_topk_kernel(const unsigned long long *__restrict__ buf, int L, int k,
                                                        float *__restrict__ out_dist, int64_t *__restrict__ out_idx)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sw[2];
    __shared__ unsigned long long pool[MNMS_SORT];
    __shared__ int npool;
    __shared__ int bsum[4];
    const int64_t q = blockIdx.x;
    const unsigned long long *row = buf + q * L;
    // threshold = the k-th smallest entry (KEY_MAX padding included; real keys are distinct: ids are): high word, then low word
    unsigned long long thr = KEY_MAX;
    if (k < L) {
        const unsigned hi = vtk_radix_kth32([&](int i) { return (unsigned)(row[i] >> 32); }, L, k, hist, sw);
        int below = 0;
        for (int i = threadIdx.x; i < L; i += 256) below += (unsigned)(row[i] >> 32) < hi ? 1 : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) below += __shfl_xor(below, o, 64);
        if ((threadIdx.x & 63) == 0) bsum[threadIdx.x >> 6] = below;
        __syncthreads();
        below = bsum[0] + bsum[1] + bsum[2] + bsum[3];
        const unsigned lo = vtk_radix_kth32([&](int i) { const unsigned long long x = row[i]; return (unsigned)(x >> 32) == hi ? (unsigned)x : 0xFFFFFFFFu; },
                                            L, k - below, hist, sw);
        thr = ((unsigned long long)hi << 32) | lo;
    }
    if (threadIdx.x == 0) npool = 0;
    for (int i = threadIdx.x; i < MNMS_SORT; i += 256) pool[i] = KEY_MAX;
    __syncthreads();
    // at most k real keys are <= thr (k of them when thr is a real key, fewer when it is the padding)
    for (int i = threadIdx.x; i < L; i += 256) {
        const unsigned long long x = row[i];
        if (x != KEY_MAX && x <= thr) { const int s = atomicAdd(&npool, 1); if (s < MNMS_SORT) pool[s] = x; }
    }
    __syncthreads();
    for (int size = 2; size <= MNMS_SORT; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < MNMS_SORT; i += 256) {
                const int p = i ^ stride;
                if (p > i) {
                    const bool asc = (i & size) == 0;
                    const unsigned long long a = pool[i], b = pool[p];
                    if ((a > b) == asc) { pool[i] = b; pool[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    const int take = npool;
    for (int i = threadIdx.x; i < k; i += 256) {
        const unsigned long long x = pool[i];
        const bool empty = i >= take;
        out_dist[q * k + i] = empty ? __builtin_inff() : __uint_as_float((unsigned)(x >> 32));
        out_idx[q * k + i] = empty ? -1 : (int64_t)(unsigned)x;
    }
}

struct MnmsWs {
    VtkWs vtk;                                         // phase 1's workspace, unchanged at the front (BANK_READY, device hash)
    size_t vtk_bytes;
    float *vd; int64_t *vi; unsigned long long *buf;
    size_t total;
};
static inline int mnms_per_video(int k, int per_video) { return per_video == 0 || per_video > k ? k : per_video; }
static MnmsWs carve_mnms(void *base, int64_t Nq, int Nv, int total_clips, int k, int per_video)
{
    MnmsWs w{};
    w.vtk = carve_vtk(base, Nq, Nv, total_clips);
    w.vtk_bytes = w.vtk.total;
    size_t off = w.vtk.total;
    auto take = [&](size_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes, 256); return p; };
    const size_t items = (size_t)Nq * (size_t)k;
    w.vd = reinterpret_cast<float *>(take(items * 4));
    w.vi = reinterpret_cast<int64_t *>(take(items * 8));
    w.buf = reinterpret_cast<unsigned long long *>(take(items * (size_t)mnms_per_video(k, per_video) * 8));
    w.total = off;
    return w;
}

}  // namespace vfr

extern "C" {

int vfr_nms_inter_table(double nms_iou, int max_len, int32_t *min_inter)
{
    VFR_REQUIRE(min_inter && max_len >= 0 && !(nms_iou != nms_iou) && nms_iou >= 0.0, VFR_EINVAL,
                "vfr_nms_inter_table: bad argument (nms_iou must be >= 0 and not NaN, max_len >= 0)");
    min_inter[0] = 1;                                  // no span has union 0
    for (int u = 1; u <= max_len; ++u) {
        int m = 0;
        while (m <= u && !((double)m / (double)u > nms_iou)) ++m;
        min_inter[u] = m;                              // u + 1: nothing of this union length is suppressed
    }
    return VFR_OK;
}

size_t vfr_score_moment_nms_workspace_bytes(int64_t Nq, int Nv, int total_clips, int k, int per_video)
{
    if (Nq < 0 || Nv < 0 || total_clips < 0 || k < 0 || per_video < 0) return 0;
    return vfr::carve_mnms(nullptr, Nq, Nv, total_clips, k, per_video).total;
}

int vfr_score_moment_nms_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                             const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips,
                             int D, float eps, int64_t id_base, int k, int per_video, double nms_iou,
                             float *out_dist, int64_t *out_idx, int dtype, void *workspace, size_t workspace_bytes,
                             vfr_stream_t stream)
{
    const int base_dtype = dtype & ~VFR_MFMA_BANK_READY;
    VFR_REQUIRE(base_dtype == VFR_MFMA_F32 || base_dtype == VFR_SCORE_EXACT, VFR_EINVAL,
                "vfr_score_moment_nms_f32: dtype %d (0 = f32 MFMA bounds, 2 = exact; | VFR_MFMA_BANK_READY)", dtype);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= 448 && max_clips >= 0 && max_clips <= vfr::NMAX_FUSED &&
                id_base >= 0, VFR_EINVAL, "vfr_score_moment_nms_f32: bad shape (k <= 448, max_clips <= 64, id_base >= 0)");
    // every global moment id fits 32 bits: total moments <= total_clips (max_clips + 1) / 2
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_moment_nms_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(per_video >= 0, VFR_EINVAL, "vfr_score_moment_nms_f32: per_video %d < 0", per_video);
    VFR_REQUIRE(!(nms_iou != nms_iou) && nms_iou >= 0.0, VFR_EINVAL, "vfr_score_moment_nms_f32: nms_iou must be >= 0 and not NaN");
    VFR_REQUIRE(k == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_moment_nms_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nq * (int64_t)k <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_moment_nms_f32: Nq * k must stay below 2^31");
    const size_t need = vfr_score_moment_nms_workspace_bytes(Nq, Nv, total_clips, k, per_video);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_moment_nms_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    if (Nq == 0 || k == 0) return VFR_OK;
    VFR_REQUIRE(Q && V && clip_offsets && moment_offsets, VFR_EINVAL, "vfr_score_moment_nms_f32: null input");
    vfr::MnmsTab tab{};
    if (int rc = vfr_nms_inter_table(nms_iou, vfr::NMAX_FUSED, tab.min_inter)) return rc;
    vfr::MnmsWs w = vfr::carve_mnms(workspace, Nq, Nv, total_clips, k, per_video);
    const int P = vfr::mnms_per_video(k, per_video);
    // phase 1: the query's k best videos and their best keys (the video top-k launch sequence, unchanged)
    if (int rc = vfr_score_video_topk_f32(Q, Nq, V, clip_offsets, moment_offsets, Nv, total_clips, min_clips, max_clips, D, eps, id_base, k,
                                          w.vd, w.vi, nullptr, nullptr, nullptr, dtype, workspace, w.vtk_bytes, stream))
        return rc;
    hipStream_t st = vfr::as_stream(stream);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        const int rows = max_clips < 1 ? 1 : max_clips;
        const int Mmax = rows * (rows + 1) / 2;
        const size_t lds = ((size_t)((D + 3) & ~3) + 64 + vfr::MNMS_TAB) * 4 + vfr::align_up((size_t)Mmax * 10, 16);
        VFR_REQUIRE(lds <= 64 * 1024, VFR_EUNSUPPORTED, "vfr_score_moment_nms_f32: D = %d too wide for the NMS kernel", D);
        hipLaunchKernelGGL(vfr::mnms_scan_kernel, dim3((unsigned)(Nq * k)), dim3(64), lds, st, Q, V, clip_offsets, moment_offsets, Nv, D,
                           eps, id_base, k, P, Mmax, tab, w.vd, w.vi, w.buf);
        VFR_CHECK_LAUNCH("mnms_scan_kernel");
    }
    {
        vfr::ProfScope prof(vfr::SITE_TOPK_MERGE, st);
        hipLaunchKernelGGL(vfr::mnms_topk_kernel, dim3((unsigned)Nq), dim3(256), 0, st, w.buf, k * P, k, out_dist, out_idx);
        VFR_CHECK_LAUNCH("mnms_topk_kernel");
    }
    return VFR_OK;
}

}  // extern "C"
