// Video-level retrieval (its fast path reuses the MFMA pre-filter's bank-side pre-pass: vtk_prepass, score_internal.h).
//
// Question: which VIDEOS match a query?  Semantics, from the moment ranking of vfr_score_topk_* (keys = (distance, global moment
// id), ascending):
//   best key of video v   = the smallest key among v's moments (its first moment in the moment ranking)
//   video top-k           = the k smallest best keys over the bank's videos, emitted as (distance, moment id of the best moment)
//   video rank count      = number of videos whose best key < a given key (the query's own video's best key)
//
// Every best key comes from the WHOLE moment triangle of its video with the canonical chain.  A tempting shortcut is wrong: a
// one-clip moment's score is its clip distance, so best <= dmin_v (the smallest clip distance), and every moment score is
// >= dmin_v (1 - 22 u) (score.hip, whole-video bounds) -- but the best moment need NOT be the arg-min clip: an fp32 mean of
// L equal distances d can round strictly below d (a quarter of the (d, L) cases).  So dmin may only EXCLUDE or COUNT a
// video; it never picks the moment.
//
// Kernels:
//   vtk_bounds_kernel   (fast path: D = 100, <= 21 clips)  m2[q][v] = min over v's clips of d~^2 = a_c + b_q - 2 v_c.q, the
//                       GEMM form on the matrix cores on centred rows (the pre-filter's products: mfma_prep_*), one wave = 64
//                       queries x a run of whole videos, per-video minima by LDS atomics
//   vtk_select_kernel   per query: T = the k-th smallest upper bound of dmin (radix select on the bits of m2: the bound is
//                       monotone in m2); lists the videos that may hold a top-k key or whose rank count is undecided
//   vtk_exact_kernel    lane = listed video: its clip distances with the canonical chain, its whole triangle, its best key
//                       (exact path: every video is listed)
//   vtk_topk_kernel     per query: the k smallest keys of its list, sorted, padded with (+inf, -1)
//
// Margins (fast path).  Notation of score_mfma.h: E2 = 20 u G bounds the pre-filter's BLOCKED chain, W = R + |q| (centred norms).
//   * Here the K = 100 chain is ONE k-ordered fma chain of 25 v_mfma_f32_16x16x4_f32 (any order of the k's is a recursive sum):
//     |err| <= 100 u sum|2 q_k v_k| <= 100 u |q||v|·2 <= 50 u G; the adds of a_c and b_q (partial sums <= 2 G) and their two
//     roundings from fp64 add <= 6 u G.  E2m := 8 E2 = 160 u G covers it with a factor of 2.8.  The minimum over clips commutes
//     with the monotone bound functions, so for the centred distances d':  sqrt(max(0, m2 - E2m)) <= min_c d'_c <= sqrt(m2 + E2m).
//   * centring moves a distance by <= u W (score_mfma.h); taken as 4 u W.
//   * the exact-path distance d obeys |d - d*| <= 53.5 u d* (score_mfma.h); taken as 128 u.
//   * the fp32 evaluation of the bounds themselves (one subtraction, one sqrt, one add, one product): <= 4 u relative, absorbed
//     by an extra factor (1 -/+ 8 u).
//   =>  dlo := (sqrt(max(0, m2 - E2m)) - 4 u W)(1 - 136 u) <= dmin_v <= (sqrt(m2 + E2m) + 4 u W)(1 + 136 u) =: dhi
//   best key of v: best_dist <= dmin_v <= dhi (a one-clip moment) and best_dist >= dmin_v (1 - 22 u) >= dlo (1 - 32 u) =: blo.
//   top-k:  T = k-th smallest dhi.  The k videos with the smallest dhi all have best_dist <= T, so the k-th best video has
//           best_dist <= T: a video with blo > T cannot be in the top-k.  Every other video is listed (ties at T included).
//   rank:   dhi < own_dist  => best_dist < own_dist: counted without a triangle;  blo > own_dist => not counted;  otherwise the
//           video is listed and counted from its exact best key.  NaN anywhere lands on "listed" (every test is written so).
#include <vector>

#include "video_topk.h"

namespace vfr {

// ---- fast path: per (query, video) minimum of the approximate squared distance ----
__global__ __launch_bounds__(64) void vtk_bounds_kernel(const float *__restrict__ qc, int64_t Nq, const float *__restrict__ vc,
                                                        const float *__restrict__ va, const float4 *__restrict__ qmeta,
                                                        const int32_t *__restrict__ clip_off, int Nv, int total_clips,
                                                        float *__restrict__ m2)
{
    __shared__ unsigned mins[64 * VTK_VIDEOS];
    __shared__ unsigned char lvid[VTK_CLIPS];
    const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
    const int v0 = blockIdx.x * VTK_VIDEOS, v1 = v0 + VTK_VIDEOS < Nv ? v0 + VTK_VIDEOS : Nv;
    const int nv = v1 - v0;
    const int64_t q0 = (int64_t)blockIdx.y * 64;
    const int c_lo = clip_off[v0], c_hi = clip_off[v1];
    for (int i = lane; i < 64 * VTK_VIDEOS; i += 64) mins[i] = 0x7F800000u;            // +inf
    for (int lv = 0; lv < nv; ++lv) {
        const int a = clip_off[v0 + lv] - c_lo, b = clip_off[v0 + lv + 1] - c_lo;
        for (int c = a + lane; c < b; c += 64) lvid[c] = (unsigned char)lv;
    }
    // A operand: -2 (q - mu), k permuted exactly like the B loads (step s = 4 b + s4 takes k = 24 g + 4 b + s4, step 24 k = 96 + g)
    float Af[4][25];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        int64_t q = q0 + 16 * t + j;
        q = q < Nq ? q : Nq - 1;
        const float *p = qc + q * FAST_D;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const float4 x = *reinterpret_cast<const float4 *>(p + 24 * g + 4 * b);
            Af[t][4 * b + 0] = -2.0f * x.x; Af[t][4 * b + 1] = -2.0f * x.y; Af[t][4 * b + 2] = -2.0f * x.z; Af[t][4 * b + 3] = -2.0f * x.w;
        }
        Af[t][24] = -2.0f * p[96 + g];
    }
    float bq[4][4];                                                       // b_q of the accumulator rows this lane holds
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t q = q0 + 16 * t + 4 * g + i;
            bq[t][i] = qmeta[q < Nq ? q : Nq - 1].x;
        }
    __syncthreads();
    const int last_row = total_clips - 1;
    // B operand (clip j of the tile, this lane's k-quarter g) and a_c: the next tile's requested before this tile's MFMAs
    float4 Bq_n[6];
    float Bl_n, acv_n;
    auto bload = [&](int c_tile) {
        const int c = c_tile + j;
        const int row = c < last_row ? c : last_row;
        const float *vr = vc + (int64_t)row * FAST_D;
#pragma unroll
        for (int b = 0; b < 6; ++b) Bq_n[b] = *reinterpret_cast<const float4 *>(vr + 24 * g + 4 * b);
        Bl_n = vr[96 + g];
        acv_n = va[row];
    };
    bload(c_lo);
    for (int c_tile = c_lo; c_tile < c_hi; c_tile += 16) {
        const int c = c_tile + j;
        float4 Bq[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) Bq[b] = Bq_n[b];
        const float Bl = Bl_n, acv = acv_n;
        if (c_tile + 16 < c_hi) bload(c_tile + 16);
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const float bs[4] = {Bq[b].x, Bq[b].y, Bq[b].z, Bq[b].w};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Af[t][4 * b + s4], bs[s4], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Af[t][24], Bl, acc[t], 0, 0, 0);
        if (c < c_hi) {
            // lane holds clip j of the tile for queries 16 t + 4 g + i
            unsigned *mrow = mins + lvid[c - c_lo];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float x = (acc[t][i] + acv) + bq[t][i];    // d~^2 (a_c - 2 v.q alone can be negative: b_q before the clamp)
                    x = x < 0.0f ? 0.0f : x;                   // (a NaN loses every atomicMin: its bits sort above +inf)
                    atomicMin(mrow + (16 * t + 4 * g + i) * VTK_VIDEOS, __float_as_uint(x));
                }
        }
    }
    __syncthreads();
    for (int i = lane; i < 64 * nv; i += 64) {
        const int ql = i / nv, lv = i - ql * nv;
        const int64_t q = q0 + ql;
        if (q >= Nq) continue;
        m2[q * Nv + v0 + lv] = __uint_as_float(mins[ql * VTK_VIDEOS + lv]);
    }
}

// ---- fast path: per query, the threshold, the list, the counts decided by the bounds ----
__global__ __launch_bounds__(256) void vtk_select_kernel(const float *__restrict__ m2, int64_t Nq, int Nv, int k,
                                                         const float4 *__restrict__ qmeta, const float *__restrict__ own_dist,
                                                         int64_t *__restrict__ count_lt, unsigned *__restrict__ list,
                                                         int *__restrict__ list_len, int *__restrict__ n_undecided)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sw[2];
    __shared__ int nlist, nund;
    __shared__ int ncount[4];
    const int64_t q = blockIdx.x;
    const float *row = m2 + q * Nv;
    const float4 qm = qmeta[q];
    const float E2m = 8.0f * qm.z, W = qm.w;
    float T = -1.0f;                                                   // k = 0: no top-k list
    if (k > 0) {
        if (Nv <= k) T = __builtin_inff();
        else {
            const unsigned b = vtk_radix_kth32([&](int i) { return __float_as_uint(row[i]); }, Nv, k, hist, sw);
            T = vtk_dhi(__uint_as_float(b), E2m, W);                   // dhi is monotone in m2: the k-th smallest dhi
        }
    }
    const bool rank = own_dist != nullptr;
    const float od = rank ? own_dist[q] : 0.0f;
    if (threadIdx.x == 0) { nlist = 0; nund = 0; }
    __syncthreads();
    unsigned *out = list + q * Nv;
    int cnt = 0;
    for (int v = threadIdx.x; v < Nv; v += 256) {
        const float x = row[v];
        const float blo = vtk_blo(x, E2m, W);
        const bool cand = k > 0 && !(blo > T);
        bool undecided = false;
        if (rank) {
            if (vtk_dhi(x, E2m, W) < od) ++cnt;
            else undecided = !(blo > od);
        }
        if (cand || undecided) {
            const int slot = atomicAdd(&nlist, 1);
            out[slot] = (unsigned)v | (undecided ? VTK_UNDECIDED : 0u);
            if (undecided) atomicAdd(&nund, 1);
        }
    }
    if (rank) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if ((threadIdx.x & 63) == 0) ncount[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        list_len[q] = nlist;
        n_undecided[q] = nund;
        if (rank) {
            const long long t = (long long)ncount[0] + ncount[1] + ncount[2] + ncount[3];
            if (t) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + q), (unsigned long long)t);
        }
    }
}

// ---- exact best key of each listed (query, video): lane = video, the canonical chain and the whole triangle ----
// list == nullptr: every video of the bank is listed (exact path), rank-undecided when own keys are given.
// keys[q * Nv + slot] = the best key of the slot's video (KEY_EMPTY for a video without clips).
__global__ __launch_bounds__(64) void vtk_exact_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                       const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                       int Nv, int D, float eps, int64_t id_base, int ds_rows,
                                                       const unsigned *__restrict__ list, const int *__restrict__ list_len,
                                                       const float *__restrict__ own_dist, const int64_t *__restrict__ own_idx,
                                                       int64_t *__restrict__ count_lt, unsigned long long *__restrict__ keys)
{
    extern __shared__ __attribute__((aligned(16))) float vsm[];
    float *qs = vsm;                                      // [D]
    float *ds = vsm + ((D + 3) & ~3);                     // [ds_rows][64]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int i = lane; i < D; i += 64) qs[i] = Q[q * D + i];
    __syncthreads();
    const int len = list ? list_len[q] : Nv;
    const bool vec4 = (D & 3) == 0 && (((uintptr_t)V) & 15) == 0;
    const bool rank = own_dist != nullptr;
    const unsigned long long own = rank ? make_key(own_dist[q], (unsigned)own_idx[q]) : 0ull;
    int nlt = 0;
    for (int base = (int)blockIdx.y * 64; base < len; base += 64 * (int)gridDim.y) {
        const int slot = base + lane;
        if (slot >= len) break;
        const unsigned e = list ? list[q * Nv + slot] : ((unsigned)slot | (rank ? VTK_UNDECIDED : 0u));
        const int v = (int)(e & ~VTK_UNDECIDED);
        const int c0 = clip_off[v], n = clip_off[v + 1] - c0;
        for (int c = 0; c < n; ++c) {
            const float *vr = V + (int64_t)(c0 + c) * D;
            float acc = 0.0f;
            if (D == FAST_D && vec4) {                    // the whole row requested at once (25 loads in flight), then the chain
                float4 x[FAST_D / 4];
#pragma unroll
                for (int k4 = 0; k4 < FAST_D / 4; ++k4) x[k4] = *reinterpret_cast<const float4 *>(vr + 4 * k4);
#pragma unroll
                for (int k4 = 0; k4 < FAST_D / 4; ++k4) {
                    const float4 y = *reinterpret_cast<const float4 *>(qs + 4 * k4);
                    float t = (x[k4].x - y.x) + eps; acc = __builtin_fmaf(t, t, acc);
                    t = (x[k4].y - y.y) + eps; acc = __builtin_fmaf(t, t, acc);
                    t = (x[k4].z - y.z) + eps; acc = __builtin_fmaf(t, t, acc);
                    t = (x[k4].w - y.w) + eps; acc = __builtin_fmaf(t, t, acc);
                }
            } else if (vec4) {                            // the same k-ascending chain, rows read 16 bytes at a time
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
            ds[c * 64 + lane] = __builtin_sqrtf(acc);
        }
        const int64_t mbase = id_base + mom_off[v];
        unsigned long long best = KEY_EMPTY;
        for (int s = 0; s < n; ++s) {
            float sum = 0.0f;
            for (int e2 = s; e2 < n; ++e2) {
                const float de = ds[e2 * 64 + lane];
                sum = e2 == s ? de : sum + de;
                const float sc = sum / (float)(e2 - s + 1);
                const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e2)));
                best = key < best ? key : best;
            }
        }
        keys[q * Nv + slot] = best;
        if ((e & VTK_UNDECIDED) && n > 0 && best < own) ++nlt;
    }
    if (rank) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nlt += __shfl_xor(nlt, o, 64);
        if (lane == 0 && nlt) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + q), (unsigned long long)nlt);
    }
}

// ---- per query: the k smallest keys of the list, sorted; (+inf, -1) past the list's end ----
constexpr int VTK_SORT = 512;                          // >= k (k <= 448)
__global__ __launch_bounds__(256) void vtk_topk_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ list_len,
                                                       int Nv, int k, float *__restrict__ out_dist, int64_t *__restrict__ out_idx)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sw[2];
    __shared__ unsigned long long pool[VTK_SORT];
    __shared__ int npool;
    const int64_t q = blockIdx.x;
    const unsigned long long *row = keys + q * Nv;
    const int len = list_len ? list_len[q] : Nv;
    const int take = len < k ? len : k;
    // threshold = the take-th smallest key (keys are distinct: ids are): high word, then low word
    unsigned long long thr = KEY_MAX;
    if (take > 0 && take < len) {
        const unsigned hi = vtk_radix_kth32([&](int i) { return (unsigned)(row[i] >> 32); }, len, take, hist, sw);
        // rank of the first key with high word == hi
        int below = 0;
        for (int i = threadIdx.x; i < len; i += 256) below += (unsigned)(row[i] >> 32) < hi ? 1 : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) below += __shfl_xor(below, o, 64);
        __shared__ int bsum[4];
        if ((threadIdx.x & 63) == 0) bsum[threadIdx.x >> 6] = below;
        __syncthreads();
        below = bsum[0] + bsum[1] + bsum[2] + bsum[3];
        const unsigned lo = vtk_radix_kth32([&](int i) { const unsigned long long x = row[i]; return (unsigned)(x >> 32) == hi ? (unsigned)x : 0xFFFFFFFFu; },
                                            len, take - below, hist, sw);
        thr = ((unsigned long long)hi << 32) | lo;
    }
    if (threadIdx.x == 0) npool = 0;
    for (int i = threadIdx.x; i < VTK_SORT; i += 256) pool[i] = KEY_MAX;
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += 256) {
        const unsigned long long x = row[i];
        if (x <= thr) { const int s = atomicAdd(&npool, 1); if (s < VTK_SORT) pool[s] = x; }
    }
    __syncthreads();
    // bitonic sort of the pool, ascending
    for (int size = 2; size <= VTK_SORT; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < VTK_SORT; i += 256) {
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
    for (int i = threadIdx.x; i < k; i += 256) {
        const unsigned long long x = i < take ? pool[i] : KEY_EMPTY;
        const bool empty = i >= take || x >= KEY_EMPTY;
        out_dist[q * k + i] = empty ? __builtin_inff() : __uint_as_float((unsigned)(x >> 32));
        out_idx[q * k + i] = empty ? -1 : (int64_t)(unsigned)x;
    }
}

void vtk_launch_bounds(const float *qc, int64_t Nq, const MfmaWs &mw, const float4 *qmeta, const int32_t *clip_offsets, int Nv, int total_clips, float *m2, hipStream_t st)
{
    hipLaunchKernelGGL(vtk_bounds_kernel, dim3((unsigned)cdiv(Nv, VTK_VIDEOS), (unsigned)cdiv(Nq, 64)), dim3(64), 0, st, qc, Nq, mw.vc, mw.va, qmeta, clip_offsets, Nv, total_clips, m2);
}
void vtk_launch_topk(const unsigned long long *keys, const int *list_len, int64_t rows, int Nv, int k, float *out_dist, int64_t *out_idx, hipStream_t st)
{
    hipLaunchKernelGGL(vtk_topk_kernel, dim3((unsigned)rows), dim3(256), 0, st, keys, list_len, Nv, k, out_dist, out_idx);
}

}  // namespace vfr

extern "C" {

size_t vfr_score_video_topk_workspace_bytes(int64_t Nq, int Nv, int total_clips, int k)
{
    if (Nq < 0 || Nv < 0 || total_clips < 0 || k < 0) return 0;
    return vfr::carve_vtk(nullptr, Nq, Nv, total_clips).total;
}

int vfr_score_video_topk_stats(const void *workspace, int64_t Nq, int Nv, int total_clips, int64_t *stats_host, vfr_stream_t stream)
{
    VFR_REQUIRE(workspace && stats_host && Nq >= 0, VFR_EINVAL, "vfr_score_video_topk_stats: bad argument");
    vfr::VtkWs w = vfr::carve_vtk(const_cast<void *>(workspace), Nq, Nv, total_clips);
    hipStream_t st = vfr::as_stream(stream);
    std::vector<int> a((size_t)Nq), b((size_t)Nq);
    if (Nq > 0 && (hipMemcpyAsync(a.data(), w.list_len, (size_t)Nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                   hipMemcpyAsync(b.data(), w.n_undecided, (size_t)Nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                   hipStreamSynchronize(st) != hipSuccess))
        return vfr::fail(VFR_EHIP, "vfr_score_video_topk_stats: copy failed");
    for (int64_t i = 0; i < Nq; ++i) { stats_host[2 * i] = a[(size_t)i]; stats_host[2 * i + 1] = b[(size_t)i]; }
    return VFR_OK;
}

int vfr_score_video_topk_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                             const int64_t *moment_offsets, int Nv, int total_clips, int min_clips, int max_clips,
                             int D, float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx,
                             const float *own_dist, const int64_t *own_idx, int64_t *video_count_lt,
                             int dtype, void *workspace, size_t workspace_bytes, vfr_stream_t stream)
{
    (void)min_clips;
    const bool bank_ready = (dtype & VFR_MFMA_BANK_READY) != 0;
    dtype &= ~VFR_MFMA_BANK_READY;
    VFR_REQUIRE(dtype == VFR_MFMA_F32 || dtype == VFR_SCORE_EXACT, VFR_EUNSUPPORTED,
                "vfr_score_video_topk_f32: dtype %d (0 = f32 MFMA bounds, 2 = exact)", dtype);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= 448 && max_clips >= 0 && max_clips <= vfr::NMAX_FUSED &&
                id_base >= 0, VFR_EINVAL, "vfr_score_video_topk_f32: bad shape (k <= 448, max_clips <= 64, id_base >= 0)");
    VFR_REQUIRE(k == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_video_topk_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE((own_dist == nullptr) == (own_idx == nullptr) && (own_dist == nullptr) == (video_count_lt == nullptr), VFR_EINVAL,
                "vfr_score_video_topk_f32: own_dist, own_idx and video_count_lt are given together or not at all");
    VFR_REQUIRE(workspace && workspace_bytes >= vfr_score_video_topk_workspace_bytes(Nq, Nv, total_clips, k), VFR_EWORKSPACE,
                "vfr_score_video_topk_f32: workspace %zu < %zu bytes", workspace_bytes,
                vfr_score_video_topk_workspace_bytes(Nq, Nv, total_clips, k));
    if (Nq == 0 || (k == 0 && !own_dist)) return VFR_OK;
    VFR_REQUIRE(Q && V && clip_offsets && moment_offsets, VFR_EINVAL, "vfr_score_video_topk_f32: null input");
    hipStream_t st = vfr::as_stream(stream);
    vfr::VtkWs w = vfr::carve_vtk(workspace, Nq, Nv, total_clips);
    if (Nv == 0) {
        if (k > 0) {
            const vfr::FillJob jobs[2] = {{out_dist, nullptr, (size_t)Nq * k * 4, 0x7F800000u}, {out_idx, nullptr, (size_t)Nq * k * 8, 0xFFFFFFFFu}};
            return vfr::fill_regions(jobs, 2, st);
        }
        return VFR_OK;
    }
    const bool fast = dtype == VFR_MFMA_F32 && D == vfr::FAST_D && max_clips <= 21 && total_clips > 0 && Nv >= vfr::opt_mfma_min() &&
                      ((((uintptr_t)Q) | ((uintptr_t)V)) & 15) == 0;
    const unsigned *list = nullptr;
    const int *list_len = nullptr;
    if (fast)
        if (int rc = vfr::vtk_prepass(w.mw, w.qc, w.qmeta, Q, Nq, V, clip_offsets, Nv, total_clips, D, eps, bank_ready, st)) return rc;
    if (fast) {
        vfr::ProfScope prof(vfr::SITE_SCORE_FUSED, st);
        vfr::vtk_launch_bounds(w.qc, Nq, w.mw, w.qmeta, clip_offsets, Nv, total_clips, w.m2, st);
        hipLaunchKernelGGL(vfr::vtk_select_kernel, dim3((unsigned)Nq), dim3(256), 0, st, w.m2, Nq, Nv, k, w.qmeta, own_dist, video_count_lt,
                           w.list, w.list_len, w.n_undecided);
        VFR_CHECK_LAUNCH("vtk_bounds_kernel / vtk_select_kernel");
        list = w.list;
        list_len = w.list_len;
    }
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        const int rows = max_clips < 1 ? 1 : max_clips;
        const size_t lds = ((size_t)((D + 3) & ~3) + (size_t)rows * 64) * 4;
        VFR_REQUIRE(lds <= 64 * 1024, VFR_EUNSUPPORTED, "vfr_score_video_topk_f32: D = %d too wide for the exact kernel", D);
        // a query's list split over `split` waves: few queries (a serving request) still fill the device
        const unsigned split = Nq >= 2048 ? 1u : (Nq >= 256 ? 2u : 8u);
        hipLaunchKernelGGL(vfr::vtk_exact_kernel, dim3((unsigned)Nq, split), dim3(64), lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps,
                           id_base, rows, list, list_len, own_dist, own_idx, video_count_lt, w.keys);
        VFR_CHECK_LAUNCH("vtk_exact_kernel");
    }
    if (k > 0) {
        vfr::ProfScope prof(vfr::SITE_TOPK_MERGE, st);
        vfr::vtk_launch_topk(w.keys, list_len, Nq, Nv, k, out_dist, out_idx, st);
        VFR_CHECK_LAUNCH("vtk_topk_kernel");
    }
    return VFR_OK;
}

}  // extern "C"
