// Paragraph-to-video retrieval (it builds on the video top-k's workspace front, pre-pass, bounds kernel, bound functions and
// top-k kernel: video_topk.h).
//
// Question: which VIDEO does a GROUP of sentences describe?  Q [Nq, D] holds the sentences, a paragraph is a run of consecutive
// rows given by grp_off [Ng + 1] (non-decreasing from 0 to Nq, runs of at most max_len <= 64 rows).
//   b(j, v)      = the distance part of video v's best key for sentence j, exactly vfr_score_video_topk_f32's: the smallest
//                  (distance, global moment id) key over the WHOLE triangle, canonical chain;  m(j, v) = that key's moment id
//   score(g, v)  = (b(j0, v) + b(j0 + 1, v) + .. + b(j0 + L - 1, v)) / (float)L: ONE fp32 left-to-right chain in sentence order
//                  starting from b(j0, v), then one correctly rounded fp32 division -- the moment score's own form (clips ->
//                  moment) one level up (sentences -> paragraph).  Additions and a division only: nothing contracts into an fma.
//   key          = (fp32 bits of score << 32) | (vid_base + v), order (score, global video index) ascending
// A video without clips is never ranked; an empty group yields padding and adds nothing to any count.  With every group of
// length 1 the score is b(j, v) / 1.0f = b(j, v): vfr_score_video_topk_f32's distances, bit for bit, and its video order.
//
// Kernels:
//   par_check_kernel    grp_off is a non-decreasing run from 0 to Nq with runs <= max_len, else *bad = 1.  Every other kernel
//                       CLAMPS a run into [0, Nq] and to max_len rows (par_group), so a bad grp_off never leads out of bounds
//   par_select_kernel   (fast path) per group: lo / hi of every video from m2 [Nq, Nv] of vtk_bounds_kernel, T = the k-th
//                       smallest hi (radix select), the list of videos that may hold a top-k key or whose rank count is undecided
//   par_exact_kernel    one wave per (group, chunk of 64 listed videos), lane = video: per sentence (staged in LDS, wave-uniform)
//                       the lane's clip distances with the canonical chain, its whole triangle by running sums, the best key;
//                       the fp32 chain over the sentences stays in a register; one key per (group, video); rank counts with
//                       one atomic per wave.  Exact path: every video is listed
//   vtk_topk_kernel     per group: the k smallest keys of its list (video_topk.h, unchanged: the key layout is the same)
//   par_pairs_kernel    one wave per named (group, video) pair, lane = clip / start clip: score and m(j, v) per sentence
//
// Bounds of the fast path.  video_topk.h gives, per (sentence j, video v), blo_j <= b(j, v) <= dhi_j as fp32 numbers
// (vtk_blo / vtk_dhi of m2[j][v], margins derived there).  Here
//   lo(g, v) = (blo_j0 + blo_j0+1 + .. ) / (float)L      hi(g, v) = (dhi_j0 + dhi_j0+1 + .. ) / (float)L
// evaluated in fp32 with the SAME left-to-right order and the same single division as the score.  Claim: lo <= score <= hi, with
// no further margin.  Proof: round-to-nearest is monotone (x <= y => fl(x) <= fl(y)), so fl(a + b) is non-decreasing in a and in
// b, and fl(s / c) is non-decreasing in s for a constant c > 0.  By induction over the chain, the partial sums of the componentwise
// smaller inputs are <= those of the larger ones at every step, and the final division keeps the order.  The ONE condition: the
// three evaluations are the identical expression -- same order, plain additions, no fma (an fma would round a different real
// number).  The chain holds additions and one division only, and the library is built with contraction off.
//   top-k:  T = k-th smallest hi.  The k videos with the smallest hi all have score <= T, so the k-th best video has score <= T: a
//           video with lo > T cannot be in the top-k.  Every other video is listed (ties at T included).
//   rank:   hi < own score => counted without a triangle;  lo > own score => not counted;  otherwise listed as undecided and
//           counted from its exact key (which also settles score == own by the video index).  NaN anywhere lands on "listed".
#include <vector>

#include "video_topk.h"

namespace vfr {

constexpr int PAR_MAX_LEN = 64;                        // sentences per paragraph

// the run of group g, clamped: rows [j0, j0 + L) lie inside [0, Nq) and L <= max_len whatever grp_off holds
__device__ __forceinline__ void par_group(const int64_t *__restrict__ grp_off, int64_t g, int64_t Nq, int max_len, int64_t *j0, int *L)
{
    int64_t a = grp_off[g], b = grp_off[g + 1];
    a = a < 0 ? 0 : (a > Nq ? Nq : a);
    b = b < a ? a : (b > Nq ? Nq : b);
    if (b - a > max_len) b = a + max_len;
    *j0 = a;
    *L = (int)(b - a);
}

__global__ __launch_bounds__(256) void par_check_kernel(const int64_t *__restrict__ grp_off, int64_t Ng, int64_t Nq, int max_len,
                                                        int *__restrict__ bad)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > Ng) return;
    bool wrong = false;
    if (g == 0) wrong = grp_off[0] != 0;
    if (g == Ng) wrong = wrong || grp_off[Ng] != Nq;
    if (g < Ng) {
        const int64_t a = grp_off[g], b = grp_off[g + 1];
        wrong = wrong || b < a || b - a > max_len;
    }
    if (wrong) atomicOr(bad, 1);
}

// ||(vr - qs) + eps||_2 with the canonical chain of vtk_exact_kernel (k-ascending fmaf, IEEE sqrt); qs = the sentence row in LDS
__device__ __forceinline__ float par_clip_dist(const float *__restrict__ vr, const float *qs, int D, float eps, bool vec4)
{
    float acc = 0.0f;
    if (D == FAST_D && vec4) {                            // the whole row requested at once (25 loads in flight), then the chain
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
    } else if (vec4) {
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
    return __builtin_sqrtf(acc);
}

// best key of one video (clips [c0, c0 + n), n >= 1) for the sentence row qs: lane-private, distances in column `lane` of ds
__device__ __forceinline__ unsigned long long par_best_key(const float *qs, const float *__restrict__ V, int c0, int n, int D, float eps,
                                                           bool vec4, float *ds, int lane, int64_t mbase)
{
    for (int c = 0; c < n; ++c) ds[c * 64 + lane] = par_clip_dist(V + (int64_t)(c0 + c) * D, qs, D, eps, vec4);
    unsigned long long best = KEY_EMPTY;
    for (int s = 0; s < n; ++s) {
        float sum = 0.0f;
        for (int e = s; e < n; ++e) {
            const float de = ds[e * 64 + lane];
            sum = e == s ? de : sum + de;
            const float sc = sum / (float)(e - s + 1);
            const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e)));
            best = key < best ? key : best;
        }
    }
    return best;
}

// ---- fast path: per group the two bounds of every video, the threshold, the list, the counts the bounds decide ----
__global__ __launch_bounds__(256) void par_select_kernel(const float *__restrict__ m2, int64_t Nq, const int64_t *__restrict__ grp_off,
                                                         int max_len, int Nv, int k, const float4 *__restrict__ qmeta,
                                                         const float *__restrict__ own_dist, int64_t *__restrict__ count_lt,
                                                         float *__restrict__ glo, float *__restrict__ ghi, unsigned *__restrict__ list,
                                                         int *__restrict__ list_len, int *__restrict__ n_undecided)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sw[2];
    __shared__ int nlist, nund;
    __shared__ int ncount[4];
    __shared__ float sE[PAR_MAX_LEN], sW[PAR_MAX_LEN];
    const int64_t g = blockIdx.x;
    int64_t j0;
    int L;
    par_group(grp_off, g, Nq, max_len < PAR_MAX_LEN ? max_len : PAR_MAX_LEN, &j0, &L);
    if (L == 0) {                                                      // an empty group: no list, nothing counted
        if (threadIdx.x == 0) { list_len[g] = 0; n_undecided[g] = 0; }
        return;
    }
    for (int t = threadIdx.x; t < L; t += 256) {
        const float4 qm = qmeta[j0 + t];
        sE[t] = 8.0f * qm.z;
        sW[t] = qm.w;
    }
    if (threadIdx.x == 0) { nlist = 0; nund = 0; }
    __syncthreads();
    float *lo_row = glo + g * Nv, *hi_row = ghi + g * Nv;
    const float fl = (float)L;
    for (int v = threadIdx.x; v < Nv; v += 256) {
        float lo = 0.0f, hi = 0.0f;
        for (int t = 0; t < L; ++t) {                                  // the score's own chain on the two bounds of b(j, v)
            const float x = m2[(j0 + t) * Nv + v];
            const float bl = vtk_blo(x, sE[t], sW[t]), dh = vtk_dhi(x, sE[t], sW[t]);
            lo = t == 0 ? bl : lo + bl;
            hi = t == 0 ? dh : hi + dh;
        }
        lo_row[v] = lo / fl;
        hi_row[v] = hi / fl;
    }
    __syncthreads();
    float T = -1.0f;                                                   // k = 0: no top-k list
    if (k > 0) {
        if (Nv <= k) T = __builtin_inff();
        else                                                           // hi >= 0 (or NaN, which sorts last): the bits order like the values
            T = __uint_as_float(vtk_radix_kth32([&](int i) { return __float_as_uint(hi_row[i]); }, Nv, k, hist, sw));
    }
    const bool rank = own_dist != nullptr;
    const float od = rank ? own_dist[g] : 0.0f;
    unsigned *out = list + g * Nv;
    int cnt = 0;
    for (int v = threadIdx.x; v < Nv; v += 256) {
        const float lo = lo_row[v];
        const bool cand = k > 0 && !(lo > T);
        bool undecided = false;
        if (rank) {
            if (hi_row[v] < od) ++cnt;
            else undecided = !(lo > od);
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
        list_len[g] = nlist;
        n_undecided[g] = nund;
        if (rank) {
            const long long t = (long long)ncount[0] + ncount[1] + ncount[2] + ncount[3];
            if (t) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + g), (unsigned long long)t);
        }
    }
}

// ---- exact key of each listed (group, video): lane = video, sentences one after the other through LDS ----
// list == nullptr: every video of the bank is listed (exact path), rank-undecided when own keys are given.
// keys[g * Nv + slot] = (score, vid_base + v) of the slot's video (KEY_EMPTY for a video without clips or an empty group).
__global__ __launch_bounds__(64) void par_exact_kernel(const float *__restrict__ Q, int64_t Nq, const int64_t *__restrict__ grp_off,
                                                       int max_len, const float *__restrict__ V, const int32_t *__restrict__ clip_off,
                                                       const int64_t *__restrict__ mom_off, int Nv, int D, float eps, int64_t vid_base,
                                                       int ds_rows, const unsigned *__restrict__ list, const int *__restrict__ list_len,
                                                       const float *__restrict__ own_dist, const int64_t *__restrict__ own_idx,
                                                       int64_t *__restrict__ count_lt, unsigned long long *__restrict__ keys)
{
    extern __shared__ __attribute__((aligned(16))) float psm[];
    float *qs = psm;                                      // [D] the current sentence
    float *ds = psm + ((D + 3) & ~3);                     // [ds_rows][64]
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t j0;
    int L;
    par_group(grp_off, g, Nq, max_len, &j0, &L);
    const int len = list ? list_len[g] : Nv;
    const bool vec4 = (D & 3) == 0 && ((((uintptr_t)V) | ((uintptr_t)Q)) & 15) == 0;
    const bool rank = own_dist != nullptr;
    const unsigned long long own = rank ? make_key(own_dist[g], (unsigned)own_idx[g]) : 0ull;
    int nlt = 0;
    for (int base = (int)blockIdx.y * 64; base < len; base += 64 * (int)gridDim.y) {      // wave-uniform trip count
        const int slot = base + lane;
        const bool active = slot < len;
        const unsigned e = !active ? 0u : (list ? list[g * Nv + slot] : ((unsigned)slot | (rank ? VTK_UNDECIDED : 0u)));
        const int v = (int)(e & ~VTK_UNDECIDED);
        const int c0 = clip_off[v];
        int n = active ? clip_off[v + 1] - c0 : 0;
        n = n < 0 ? 0 : (n > ds_rows ? ds_rows : n);
        // the moment id only breaks ties inside the video: the paragraph key carries the video index, so any base serves
        const int64_t mbase = mom_off[v];
        float sum = 0.0f;
        for (int t = 0; t < L; ++t) {
            __syncthreads();                              // every lane is done with the previous row
            for (int i = lane; i < D; i += 64) qs[i] = Q[(j0 + t) * D + i];
            __syncthreads();
            if (n > 0) {
                const float b = __uint_as_float((unsigned)(par_best_key(qs, V, c0, n, D, eps, vec4, ds, lane, mbase) >> 32));
                sum = t == 0 ? b : sum + b;
            }
        }
        if (active) {
            const bool ranked = n > 0 && L > 0;
            const unsigned long long key = ranked ? make_key(sum / (float)L, (unsigned)(vid_base + v)) : KEY_EMPTY;
            keys[g * Nv + slot] = key;
            if ((e & VTK_UNDECIDED) && ranked && key < own) ++nlt;
        }
    }
    if (rank) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nlt += __shfl_xor(nlt, o, 64);
        if (lane == 0 && nlt) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + g), (unsigned long long)nlt);
    }
}

// ---- named (group, global video) pairs: the score and, per sentence, the moment id of the video's best key ----
// One wave per pair; lane = clip for the distances, lane = start clip for its row of the triangle.
__global__ __launch_bounds__(64) void par_pairs_kernel(const float *__restrict__ Q, int64_t Nq, const int64_t *__restrict__ grp_off,
                                                       int64_t Ng, int max_len, const float *__restrict__ V,
                                                       const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off, int Nv,
                                                       int D, float eps, int64_t id_base, int64_t vid_base,
                                                       const int32_t *__restrict__ pairs, float *__restrict__ out_score,
                                                       int64_t *__restrict__ out_moments, int *__restrict__ bad)
{
    extern __shared__ __attribute__((aligned(16))) float psm[];
    float *qs = psm;
    float *ds = psm + ((D + 3) & ~3);                     // [64]
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int64_t gi = pairs[2 * p], lv = (int64_t)pairs[2 * p + 1] - vid_base;
    if (gi < 0 || gi >= Ng) {                             // not a group: flagged, left untouched
        if (lane == 0 && bad) atomicOr(bad, 1);
        return;
    }
    if (lv < 0 || lv >= Nv) return;                       // another shard's video: left untouched
    int64_t j0;
    int L;
    par_group(grp_off, gi, Nq, max_len, &j0, &L);
    const int v = (int)lv, c0 = clip_off[v];
    int n = clip_off[v + 1] - c0;
    n = n < 0 ? 0 : (n > NMAX_FUSED ? NMAX_FUSED : n);
    const int64_t mbase = id_base + mom_off[v];
    const bool vec4 = (D & 3) == 0 && ((((uintptr_t)V) | ((uintptr_t)Q)) & 15) == 0;
    int64_t *mrow = out_moments ? out_moments + p * max_len : nullptr;
    float sum = 0.0f;
    for (int t = 0; t < L; ++t) {
        __syncthreads();
        for (int i = lane; i < D; i += 64) qs[i] = Q[(j0 + t) * D + i];
        __syncthreads();
        if (lane < n) ds[lane] = par_clip_dist(V + (int64_t)(c0 + lane) * D, qs, D, eps, vec4);
        __syncthreads();
        unsigned long long best = KEY_EMPTY;
        if (lane < n) {
            const int s = lane;
            float rs = 0.0f;
            for (int e = s; e < n; ++e) {
                const float de = ds[e];
                rs = e == s ? de : rs + de;
                const unsigned long long key = make_key(rs / (float)(e - s + 1), (unsigned)(mbase + moment_index(n, s, e)));
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long y = __shfl_xor(best, o, 64);
            best = y < best ? y : best;
        }
        const float b = __uint_as_float((unsigned)(best >> 32));
        sum = t == 0 ? b : sum + b;
        if (lane == 0 && mrow) mrow[t] = n > 0 ? (int64_t)(unsigned)best : -1;
    }
    if (lane == 0) out_score[p] = (n > 0 && L > 0) ? sum / (float)L : __builtin_inff();
    if (mrow)
        for (int t = L + lane; t < max_len; t += 64) mrow[t] = -1;
}

struct ParWs {
    MfmaWs mw;                                         // bank-side products at the pre-filter's offsets, as carve_vtk
    float4 *qmeta; float *qc; float *m2; float *glo, *ghi; unsigned *list; int *list_len, *n_undecided; unsigned long long *keys;
    size_t total;
};
static ParWs carve_par(void *base, int64_t Nq, int64_t Ng, int Nv, int total_clips)
{
    ParWs w{};
    w.mw = carve_bank_front(base, total_clips);
    size_t off = (size_t)(reinterpret_cast<char *>(w.mw.stale) - static_cast<char *>(base)) + 256;
    auto take = [&](size_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes, 256); return p; };
    w.qmeta = reinterpret_cast<float4 *>(take((size_t)Nq * 16));
    w.qc = reinterpret_cast<float *>(take((size_t)Nq * FAST_D * 4));
    w.m2 = reinterpret_cast<float *>(take((size_t)Nq * Nv * 4));
    w.glo = reinterpret_cast<float *>(take((size_t)Ng * Nv * 4));
    w.ghi = reinterpret_cast<float *>(take((size_t)Ng * Nv * 4));
    w.list = reinterpret_cast<unsigned *>(take((size_t)Ng * Nv * 4));
    w.list_len = reinterpret_cast<int *>(take((size_t)Ng * 4));
    w.n_undecided = reinterpret_cast<int *>(take((size_t)Ng * 4));
    w.keys = reinterpret_cast<unsigned long long *>(take((size_t)Ng * Nv * 8));
    w.total = off;
    return w;
}

}  // namespace vfr

extern "C" {

size_t vfr_score_paragraphs_workspace_bytes(int64_t Nq, int64_t Ng, int Nv, int total_clips, int k)
{
    if (Nq < 0 || Ng < 0 || Nv < 0 || total_clips < 0 || k < 0) return 0;
    return vfr::carve_par(nullptr, Nq, Ng, Nv, total_clips).total;
}

int vfr_score_paragraphs_stats(const void *workspace, int64_t Nq, int64_t Ng, int Nv, int total_clips, int64_t *stats_host,
                               vfr_stream_t stream)
{
    VFR_REQUIRE(workspace && stats_host && Nq >= 0 && Ng >= 0 && Nv >= 0 && total_clips >= 0, VFR_EINVAL,
                "vfr_score_paragraphs_stats: bad argument");
    vfr::ParWs w = vfr::carve_par(const_cast<void *>(workspace), Nq, Ng, Nv, total_clips);
    hipStream_t st = vfr::as_stream(stream);
    std::vector<int> a((size_t)Ng), b((size_t)Ng);
    if (Ng > 0 && (hipMemcpyAsync(a.data(), w.list_len, (size_t)Ng * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                   hipMemcpyAsync(b.data(), w.n_undecided, (size_t)Ng * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                   hipStreamSynchronize(st) != hipSuccess))
        return vfr::fail(VFR_EHIP, "vfr_score_paragraphs_stats: copy failed");
    for (int64_t i = 0; i < Ng; ++i) { stats_host[2 * i] = a[(size_t)i]; stats_host[2 * i + 1] = b[(size_t)i]; }
    return VFR_OK;
}

int vfr_score_paragraphs_f32(const float *Q, int64_t Nq, const int64_t *grp_off, int64_t Ng, int max_len, const float *V,
                             const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips, int min_clips,
                             int max_clips, int D, float eps, int64_t vid_base, int k, float *out_dist, int64_t *out_idx,
                             const float *own_dist, const int64_t *own_idx, int64_t *count_lt, int dtype, int *bad,
                             void *workspace, size_t workspace_bytes, vfr_stream_t stream)
{
    (void)min_clips;
    const bool bank_ready = (dtype & VFR_MFMA_BANK_READY) != 0;
    dtype &= ~VFR_MFMA_BANK_READY;
    VFR_REQUIRE(dtype == VFR_MFMA_F32 || dtype == VFR_SCORE_EXACT, VFR_EINVAL,
                "vfr_score_paragraphs_f32: dtype %d (0 = f32 MFMA bounds, 2 = exact; | VFR_MFMA_BANK_READY)", dtype);
    VFR_REQUIRE(Nq >= 0 && Ng >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= 448 && max_clips >= 0 &&
                max_clips <= vfr::NMAX_FUSED && max_len >= 0 && max_len <= vfr::PAR_MAX_LEN && vid_base >= 0 &&
                vid_base + (int64_t)Nv <= 0xFFFFFFFFll, VFR_EINVAL,
                "vfr_score_paragraphs_f32: bad shape (k <= 448, max_clips <= 64, max_len <= 64, 0 <= vid_base, vid_base + Nv < 2^32)");
    VFR_REQUIRE(Ng * (int64_t)k <= 0x7FFFFFFF && Ng <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_paragraphs_f32: Ng * k must stay below 2^31");
    VFR_REQUIRE(grp_off, VFR_EINVAL, "vfr_score_paragraphs_f32: null grp_off");
    VFR_REQUIRE(k == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_paragraphs_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE((own_dist == nullptr) == (own_idx == nullptr) && (own_dist == nullptr) == (count_lt == nullptr), VFR_EINVAL,
                "vfr_score_paragraphs_f32: own_dist, own_idx and count_lt are given together or not at all");
    VFR_REQUIRE(Nq == 0 || Nv == 0 || (Q && V && clip_offsets && moment_offsets), VFR_EINVAL, "vfr_score_paragraphs_f32: null input");
    const size_t need = vfr_score_paragraphs_workspace_bytes(Nq, Ng, Nv, total_clips, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_paragraphs_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    const int rows = max_clips < 1 ? 1 : max_clips;
    const size_t lds = ((size_t)((D + 3) & ~3) + (size_t)rows * 64) * 4;
    VFR_REQUIRE(lds <= 64 * 1024, VFR_EUNSUPPORTED, "vfr_score_paragraphs_f32: D = %d too wide for the exact kernel", D);
    hipStream_t st = vfr::as_stream(stream);
    if (bad) {
        hipLaunchKernelGGL(vfr::par_check_kernel, dim3((unsigned)vfr::cdiv(Ng + 1, 256)), dim3(256), 0, st, grp_off, Ng, Nq, max_len, bad);
        VFR_CHECK_LAUNCH("par_check_kernel");
    }
    if (Ng == 0 || (k == 0 && !own_dist)) return VFR_OK;
    if (Nv == 0 || Nq == 0 || max_len == 0) {             // nothing to rank: padding, nothing counted
        if (k > 0) {
            const vfr::FillJob jobs[2] = {{out_dist, nullptr, (size_t)Ng * k * 4, 0x7F800000u}, {out_idx, nullptr, (size_t)Ng * k * 8, 0xFFFFFFFFu}};
            return vfr::fill_regions(jobs, 2, st);
        }
        return VFR_OK;
    }
    vfr::ParWs w = vfr::carve_par(workspace, Nq, Ng, Nv, total_clips);
    const bool fast = dtype == VFR_MFMA_F32 && D == vfr::FAST_D && max_clips <= 21 && total_clips > 0 && Nv >= vfr::opt_mfma_min() &&
                      ((((uintptr_t)Q) | ((uintptr_t)V)) & 15) == 0;
    const unsigned *list = nullptr;
    const int *list_len = nullptr;
    if (fast) {
        if (int rc = vfr::vtk_prepass(w.mw, w.qc, w.qmeta, Q, Nq, V, clip_offsets, Nv, total_clips, D, eps, bank_ready, st)) return rc;
        vfr::ProfScope prof(vfr::SITE_SCORE_FUSED, st);
        vfr::vtk_launch_bounds(w.qc, Nq, w.mw, w.qmeta, clip_offsets, Nv, total_clips, w.m2, st);
        hipLaunchKernelGGL(vfr::par_select_kernel, dim3((unsigned)Ng), dim3(256), 0, st, w.m2, Nq, grp_off, max_len, Nv, k, w.qmeta, own_dist,
                           count_lt, w.glo, w.ghi, w.list, w.list_len, w.n_undecided);
        VFR_CHECK_LAUNCH("vtk_bounds_kernel / par_select_kernel");
        list = w.list;
        list_len = w.list_len;
    }
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        // a group's list split over `split` waves: few paragraphs (a serving request) still fill the device
        const int64_t chunks = vfr::cdiv(Nv, 64);
        int64_t split = vfr::cdiv(4096, Ng);
        split = split > chunks ? chunks : split;
        split = split < 1 ? 1 : (split > 1024 ? 1024 : split);
        hipLaunchKernelGGL(vfr::par_exact_kernel, dim3((unsigned)Ng, (unsigned)split), dim3(64), lds, st, Q, Nq, grp_off, max_len, V, clip_offsets,
                           moment_offsets, Nv, D, eps, vid_base, rows, list, list_len, own_dist, own_idx, count_lt, w.keys);
        VFR_CHECK_LAUNCH("par_exact_kernel");
    }
    if (k > 0) {
        vfr::ProfScope prof(vfr::SITE_TOPK_MERGE, st);
        vfr::vtk_launch_topk(w.keys, list_len, Ng, Nv, k, out_dist, out_idx, st);
        VFR_CHECK_LAUNCH("vtk_topk_kernel");
    }
    return VFR_OK;
}

int vfr_score_paragraph_pairs_f32(const float *Q, int64_t Nq, const int64_t *grp_off, int64_t Ng, int max_len, const float *V,
                                  const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips, int min_clips,
                                  int max_clips, int D, float eps, int64_t id_base, int64_t vid_base, const int32_t *pairs, int64_t Np,
                                  float *out_score, int64_t *out_moments, int *bad, vfr_stream_t stream)
{
    (void)min_clips;
    VFR_REQUIRE(Nq >= 0 && Ng >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && Np >= 0 && Np <= 0x7FFFFFFF && max_clips >= 0 &&
                max_clips <= vfr::NMAX_FUSED && max_len >= 0 && max_len <= vfr::PAR_MAX_LEN && id_base >= 0 && vid_base >= 0, VFR_EINVAL,
                "vfr_score_paragraph_pairs_f32: bad shape (max_clips <= 64, max_len <= 64, Np < 2^31, id_base >= 0, vid_base >= 0)");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_paragraph_pairs_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(grp_off, VFR_EINVAL, "vfr_score_paragraph_pairs_f32: null grp_off");
    VFR_REQUIRE(Np == 0 || (pairs && out_score), VFR_EINVAL, "vfr_score_paragraph_pairs_f32: null pairs / out_score");
    VFR_REQUIRE(Nq == 0 || Nv == 0 || (Q && V && clip_offsets && moment_offsets), VFR_EINVAL, "vfr_score_paragraph_pairs_f32: null input");
    const size_t lds = ((size_t)((D + 3) & ~3) + 64) * 4;
    VFR_REQUIRE(lds <= 64 * 1024, VFR_EUNSUPPORTED, "vfr_score_paragraph_pairs_f32: D = %d too wide", D);
    hipStream_t st = vfr::as_stream(stream);
    if (bad) {
        hipLaunchKernelGGL(vfr::par_check_kernel, dim3((unsigned)vfr::cdiv(Ng + 1, 256)), dim3(256), 0, st, grp_off, Ng, Nq, max_len, bad);
        VFR_CHECK_LAUNCH("par_check_kernel");
    }
    if (Np == 0 || Nv == 0) return VFR_OK;
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, st);
    hipLaunchKernelGGL(vfr::par_pairs_kernel, dim3((unsigned)Np), dim3(64), lds, st, Q, Nq, grp_off, Ng, max_len, V, clip_offsets, moment_offsets,
                       Nv, D, eps, id_base, vid_base, pairs, out_score, out_moments, bad);
    VFR_CHECK_LAUNCH("par_pairs_kernel");
    return VFR_OK;
}

}  // extern "C"
