// Late-fusion retrieval: vfr_score_fusion_f32 and vfr_score_fusion_own_f32 (include/vfr.h).
//
// S <= 4 streams (feature types, modalities, seeds) describe the same videos: stream s has its own clip bank V_s [total_clips, D_s],
// its own query matrix Q_s [Nq, D_s] and a weight w_s >= 0; clip_offsets / moment_offsets are shared.  The ranking key changes at
// the CLIP: d_s[q, c] is the canonical chain of vfr_score_moments_f32 (k-ascending fp32 fma chain of ((v - q) + eps)^2, IEEE sqrt),
// written out in fus_dist (not taken from the headers of score.o, so its code objects do not change); the fused clip distance is
//     f = fl(w_0 d_0);  f = fl(f + fl(w_s d_s)), s = 1 .. S-1          (__fmul_rn / __fadd_rn: every operation rounded, no fma)
// and everything downstream is the existing moment chain on f: sequential fp32 sum s -> e started at f[s], one IEEE division by
// (float)(e - s + 1), key = (score bits << 32) | (id_base + moment_offsets[v] + position in utils.generate_moments order).  The
// mean is linear, so in real arithmetic this is the weighted sum of the per-stream moment scores -- with ONE triangle per (query,
// video) instead of S.  S = 1, w = (1) and w = (1, 0, ..) give the bits of vfr_score_topk_f32 / vfr_score_video_topk_f32 on
// stream 0 (fl(1 d) = d, d + fl(0 d') = d for finite d').
// Kernels (a translation unit of its own):
//   fusion_own_kernel   one wave per query: lane = clip of own[q] (its S chains, fused, into LDS), then lane = start clip with a
//                       running sum over the end clip; the row layout of vfr_score_own_f32 (tail +inf).
//   fusion_scan_kernel  one wave per (query, chunk of the video axis), lane = video.  The S query rows sit wave-uniform in LDS; per
//                       block of 64 videos each lane runs the S chains of its clips, fuses them and writes f to its LDS column, then
//                       walks its triangle by running sums and IEEE division.  Rank counts: per-lane counters, one atomic per wave
//                       and rank.  The chunk's k smallest keys (moments: every key; videos: the lane's best key over its WHOLE
//                       triangle) are collected under a running threshold into an LDS list of 128 / 256 / 512 keys that is sorted
//                       and cut back to k when it fills; the chunk's list goes to ws[chunk][query][0..k).
//   The per-chunk lists are merged by vfr_topk_merge_keys (one launch), which also pads with (+inf, -1).
// The chunk plan (scan_plan: at most SCAN_MAX_CHUNKS chunks, just enough for about SCAN_TARGET_WAVES waves -- one query against
// 10 000 videos fills the device, 5 000 queries run whole-bank streams: a running threshold wants long streams), the list's
// capacity and sort and the scan kernel's rank-key counters are those of scan_common.h.
// Workspace: chunks x Nq x k keys, chunks <= SCAN_MAX_CHUNKS whatever Nv is.  Nothing is of size Nq x Nv, nothing waits for the host.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int FUS_MAX_S = VFR_FUSION_MAX_STREAMS;
constexpr int FUS_MAX_CLIPS = 64;                    // as the fused scorer
constexpr int FUS_MAX_SUM_D = VFR_FUSION_MAX_SUM_D;  // floats of query rows in LDS (each D_s rounded up to 4)

// the streams, by value in the kernel arguments: device pointers, widths, weights, where each query row starts in LDS
struct FusStreams {
    const float *Q[FUS_MAX_S];
    const float *V[FUS_MAX_S];
    int D[FUS_MAX_S];
    int qo[FUS_MAX_S];           // offset of the stream's query row in the LDS block (multiples of 4 floats)
    int vec[FUS_MAX_S];          // D % 4 == 0 and both pointers 16-byte aligned: 16-byte loads
    float w[FUS_MAX_S];
    int S;
    int qs_floats;               // sum of the rows, each rounded up to 4 floats
};

// one clip row against the query row in LDS: the canonical chain
__device__ __forceinline__ float fus_dist(const float *__restrict__ vr, const float *qs, int D, bool vec, float eps)
{
    float acc = 0.0f;
    if (vec) {
#pragma unroll 5
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

// fused distance of clip row c (index into every stream's bank): f = fl(w_0 d_0), f = fl(f + fl(w_s d_s))
__device__ __forceinline__ float fus_clip(const FusStreams &st, const float *qs, int64_t c, float eps)
{
    float f = 0.0f;
#pragma unroll
    for (int s = 0; s < FUS_MAX_S; ++s) {
        if (s < st.S) {
            const float d = fus_dist(st.V[s] + c * st.D[s], qs + st.qo[s], st.D[s], st.vec[s] != 0, eps);
            const float t = __fmul_rn(st.w[s], d);
            f = s == 0 ? t : __fadd_rn(f, t);
        }
    }
    return f;
}

// the S wave-uniform query rows of query q into LDS
__device__ __forceinline__ void fus_query_rows(const FusStreams &st, int64_t q, float *qs, int lane)
{
#pragma unroll
    for (int s = 0; s < FUS_MAX_S; ++s) {
        if (s < st.S) {
            const float *qg = st.Q[s] + q * st.D[s];
            for (int i = lane; i < st.D[s]; i += 64) qs[st.qo[s] + i] = qg[i];
        }
    }
    __syncthreads();
}

// ---- each query against ONE video own[q]: one wave per query; lane = clip, then lane = start clip ----
__global__ __launch_bounds__(64) void fusion_own_kernel(const FusStreams st, int64_t Nq, const int32_t *__restrict__ clip_off,
                                                        const int32_t *__restrict__ own, int Nv, float eps, int Mmax,
                                                        float *__restrict__ scores)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    __shared__ float ds[FUS_MAX_CLIPS];
    float *qs = ssm;                                           // [qs_floats]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    float *out = scores + q * Mmax;
    const int v = own[q];
    int c0 = 0, n = 0;
    if (v >= 0 && v < Nv) {
        c0 = clip_off[v];
        n = clip_off[v + 1] - c0;
        n = n > FUS_MAX_CLIPS ? FUS_MAX_CLIPS : (n < 0 ? 0 : n);
    }
    int M = n * (n + 1) / 2;
    if (M > Mmax) { M = 0; n = 0; }                            // cannot happen with Mmax >= max_clips (max_clips + 1) / 2
    for (int m = M + lane; m < Mmax; m += 64) out[m] = __builtin_inff();      // slots past this video's moments
    fus_query_rows(st, q, qs, lane);
    if (lane < n) ds[lane] = fus_clip(st, qs, (int64_t)c0 + lane, eps);
    __syncthreads();
    if (lane < n) {
        float sum = 0.0f;
        for (int e = lane; e < n; ++e) {
            const float de = ds[e];
            sum = e == lane ? de : sum + de;
            out[moment_index(n, lane, e)] = sum / (float)(e - lane + 1);
        }
    }
}

// ---- one wave per (query, chunk of the video axis), lane = video ----
__global__ __launch_bounds__(64) void fusion_scan_kernel(const FusStreams st, int64_t Nq, const int32_t *__restrict__ clip_off,
                                                         const int64_t *__restrict__ mom_off, int Nv, float eps, int64_t id_base,
                                                         int level, int k, int cap, ScanRank rk, int ds_rows, int chunks, int64_t per,
                                                         unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float *qs = ssm;                                                                        // [qs_floats]
    float *ds = ssm + st.qs_floats;                                                         // [ds_rows][64] fused clip distances, lane-minor
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ds + (size_t)ds_rows * 64);   // [cap]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - q * chunks);
    fus_query_rows(st, q, qs, lane);

    unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r)
        rkey[r] = r < rk.num_rank ? make_key(rk.dist[r * Nq + q], (unsigned)rk.idx[r * Nq + q]) : 0ull;
    int nlt[SCAN_MAX_RANK] = {0, 0, 0, 0};

    const int64_t v0 = (int64_t)ch * per;
    const int64_t v1 = v0 + per < Nv ? v0 + per : Nv;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned long long thr = SCAN_KEY_MAX;                     // keys >= thr cannot be among the chunk's k smallest
    int cnt = 0;                                               // keys in buf (wave-uniform)
    // a wave-uniform append of the lanes' keys under the threshold; the list is sorted and cut back to k when it may overflow
    auto append = [&](bool take, unsigned long long key) {
        const unsigned long long mt = __ballot(take);
        if (mt) {
            if (take) buf[cnt + __popcll(mt & below)] = key;
            cnt += __popcll(mt);
            if (cnt > cap - 64) {
                __syncthreads();
                wave_sort_keys(buf, cnt, cap, lane);
                if (cnt >= k) { thr = buf[k - 1]; cnt = k; }
                __syncthreads();
            }
        }
    };

    for (int64_t vb = v0; vb < v1; vb += 64) {
        const int64_t l = vb + lane;
        int n = 0;
        int64_t mbase = 0;
        if (l < v1) {
            const int c0 = clip_off[l];
            n = clip_off[l + 1] - c0;
            n = n > ds_rows ? ds_rows : (n < 0 ? 0 : n);
            mbase = id_base + mom_off[l];
            for (int c = 0; c < n; ++c) ds[c * 64 + lane] = fus_clip(st, qs, (int64_t)c0 + c, eps);   // the lane's own column
        }
        if (level == VFR_FUSION_VIDEOS) {
            unsigned long long best = SCAN_KEY_EMPTY;
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
            if (n > 0) scan_rank_count(rk.num_rank, rkey, best, nlt);
            if (k > 0) append(n > 0 && best < thr, best);
        } else {
            // the wave-uniform loop over the widest triangle of the block: a lane past its own video's end takes no part
            int nmax = n;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(nmax, o, 64); nmax = x > nmax ? x : nmax; }
            for (int s = 0; s < nmax; ++s) {
                float sum = 0.0f;
                for (int e2 = s; e2 < nmax; ++e2) {
                    const bool live = e2 < n;
                    const float de = live ? ds[e2 * 64 + lane] : 0.0f;
                    sum = e2 == s ? de : sum + de;
                    const float sc = sum / (float)(e2 - s + 1);
                    const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e2)));
                    if (live) scan_rank_count(rk.num_rank, rkey, key, nlt);
                    if (k > 0) append(live && key < thr, key);
                }
            }
        }
    }
    if (k > 0) {
        __syncthreads();
        int size = 64;
        while (size < cnt) size <<= 1;                         // cnt <= cap, a power of two
        wave_sort_keys(buf, cnt, size, lane);
        cnt = cnt > k ? k : cnt;
        unsigned long long *out = ws + ((size_t)ch * Nq + q) * k;
        for (int i = lane; i < k; i += 64) out[i] = i < cnt ? buf[i] : SCAN_KEY_EMPTY;
    }
    if (rk.num_rank > 0) {
#pragma unroll
        for (int r = 0; r < SCAN_MAX_RANK; ++r) {
            // a lane counts at most its share of the 2^32 ids, the wave's sum needs 64 bits (one wave may stream the whole bank)
            unsigned long long x = (unsigned long long)(unsigned)nlt[r];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
            if (r < rk.num_rank && lane == 0 && x)
                atomicAdd(reinterpret_cast<unsigned long long *>(rk.count_lt + (int64_t)r * Nq + q), x);
        }
    }
}

// The host arrays of a call, checked -> the by-value kernel argument.  need_q / need_v: the matrices are read at all.
int fus_streams(const char *who, const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int S,
                bool need_q, bool need_v, FusStreams *out)
{
    VFR_REQUIRE(S >= 1 && S <= FUS_MAX_S, VFR_EINVAL, "%s: S = %d streams (1 .. %d)", who, S, FUS_MAX_S);
    VFR_REQUIRE(Q_host && V_host && D_host && w_host, VFR_EINVAL, "%s: null stream array (Q_host, V_host, D_host, w_host)", who);
    FusStreams st{};
    st.S = S;
    int64_t floats = 0;
    for (int s = 0; s < S; ++s) {
        VFR_REQUIRE(D_host[s] >= 1, VFR_EINVAL, "%s: stream %d: D = %d", who, s, D_host[s]);
        const float w = w_host[s];
        VFR_REQUIRE(w >= 0.0f && w <= 3.402823466e38f, VFR_EINVAL, "%s: stream %d: weight %g (finite, >= 0)", who, s, (double)w);
        VFR_REQUIRE(!need_q || Q_host[s], VFR_EINVAL, "%s: stream %d: Q is null", who, s);
        VFR_REQUIRE(!need_v || V_host[s], VFR_EINVAL, "%s: stream %d: V is null", who, s);
        st.Q[s] = Q_host[s]; st.V[s] = V_host[s]; st.D[s] = D_host[s]; st.w[s] = w;
        st.vec[s] = (D_host[s] & 3) == 0 && ((((uintptr_t)Q_host[s]) | ((uintptr_t)V_host[s])) & 15) == 0;
        st.qo[s] = (int)floats;
        floats += ((int64_t)D_host[s] + 3) & ~int64_t(3);
    }
    VFR_REQUIRE(floats <= FUS_MAX_SUM_D, VFR_EUNSUPPORTED,
                "%s: the query rows of all streams take %lld floats of LDS (each D rounded up to 4), limit VFR_FUSION_MAX_SUM_D = %d", who,
                (long long)floats, FUS_MAX_SUM_D);
    st.qs_floats = (int)floats;
    *out = st;
    return VFR_OK;
}

// ---- the weight sweep: vfr_score_fusion_sweep_own_f32 / vfr_score_fusion_sweep_f32 (include/vfr.h) ----
// A grid of W <= VFR_FUSION_MAX_SWEEP weight vectors over the SAME streams.  The stream clip distances d_s[q, c] do not depend on the
// weights, so each kernel runs the S chains (fus_dist) ONCE and repeats, per weight vector, only what the weights enter: the fuse
// (__fmul_rn / __fadd_rn, the sequence of fus_clip) and the triangle (running fp32 sum, one IEEE division).  Bits per weight vector =
// the single-weight kernels' at that vector.
//   fusion_sweep_own_kernel  one wave per query, lane = clip of own[q]: its S distances stay in registers; per weight vector the lane
//                            fuses them into an LDS row and, as start clip, walks the end clips (fusion_own_kernel's triangle).
//   fusion_sweep_kernel      one wave per (query, chunk of the video axis) with the chunk plan of scan_plan, lane = video.  Per block
//                            of 64 videos the lane writes the PER-STREAM distances of its clips to LDS columns [S][rows][64]; then
//                            the weight loop: fuse into one more column block [rows][64], walk the triangle, count the keys before
//                            that weight's rank keys in num_rank <= 4 REGISTER counters, and flush them -- wave sum by shuffles,
//                            lane 0 adds it to the wave's 64-bit total of (weight, rank) in LDS.  So no lane holds W x num_rank
//                            counters (no scratch), and after the last block there is one atomic per (wave, weight, rank) with a
//                            non-zero total.  No lists, no workspace.
//   LDS of a sweep wave = 4 (sum of round_up(D_s, 4)) + 4 * 64 * rows * (S + 1) + 16 * W * num_rank bytes, rows = max(max_clips, 1):
//   query rows, S + 1 column blocks, the rank keys and totals of every (weight, rank); it must fit FUS_SWEEP_LDS.
constexpr int FUS_MAX_SWEEP = VFR_FUSION_MAX_SWEEP;
constexpr size_t FUS_SWEEP_LDS = 65536;              // what a workgroup gets without asking the runtime for more

struct FusGrid {
    float w[FUS_MAX_SWEEP * FUS_MAX_S];              // [W][S] row-major
    int W;
};

size_t fus_sweep_lds(const FusStreams &st, int rows, int W, int num_rank)
{
    return ((size_t)st.qs_floats + (size_t)64 * rows * (st.S + 1)) * 4 + (size_t)16 * W * num_rank;
}

// f = fl(w_0 d_0), f = fl(f + fl(w_s d_s)) for weight vector wi of the grid: the operations of fus_clip on distances already there
__device__ __forceinline__ float fus_fuse(const FusGrid &grid, int wi, int S, const float (&d)[FUS_MAX_S])
{
    float f = 0.0f;
#pragma unroll
    for (int s = 0; s < FUS_MAX_S; ++s) {
        if (s < S) {
            const float t = __fmul_rn(grid.w[wi * S + s], d[s]);
            f = s == 0 ? t : __fadd_rn(f, t);
        }
    }
    return f;
}

__global__ __launch_bounds__(64) void fusion_sweep_own_kernel(const FusStreams st, const FusGrid grid, int64_t Nq,
                                                              const int32_t *__restrict__ clip_off, const int32_t *__restrict__ own,
                                                              int Nv, float eps, int Mmax, float *__restrict__ scores)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    __shared__ float fs[FUS_MAX_CLIPS];
    float *qs = ssm;                                           // [qs_floats]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int v = own[q];
    int c0 = 0, n = 0;
    if (v >= 0 && v < Nv) {
        c0 = clip_off[v];
        n = clip_off[v + 1] - c0;
        n = n > FUS_MAX_CLIPS ? FUS_MAX_CLIPS : (n < 0 ? 0 : n);
    }
    int M = n * (n + 1) / 2;
    if (M > Mmax) { M = 0; n = 0; }                            // cannot happen with Mmax >= max_clips (max_clips + 1) / 2
    fus_query_rows(st, q, qs, lane);
    float d[FUS_MAX_S] = {0.0f, 0.0f, 0.0f, 0.0f};             // the lane's clip against every stream, once
    if (lane < n) {
#pragma unroll
        for (int s = 0; s < FUS_MAX_S; ++s)
            if (s < st.S)
                d[s] = fus_dist(st.V[s] + ((int64_t)c0 + lane) * st.D[s], qs + st.qo[s], st.D[s], st.vec[s] != 0, eps);
    }
    for (int wi = 0; wi < grid.W; ++wi) {
        float *out = scores + ((int64_t)wi * Nq + q) * Mmax;
        for (int m = M + lane; m < Mmax; m += 64) out[m] = __builtin_inff();  // slots past this video's moments
        __syncthreads();                                       // the previous weight's triangle has read fs
        if (lane < n) fs[lane] = fus_fuse(grid, wi, st.S, d);
        __syncthreads();
        if (lane < n) {
            float sum = 0.0f;
            for (int e = lane; e < n; ++e) {
                const float de = fs[e];
                sum = e == lane ? de : sum + de;
                out[moment_index(n, lane, e)] = sum / (float)(e - lane + 1);
            }
        }
    }
}

__global__ __launch_bounds__(64) void fusion_sweep_kernel(const FusStreams st, const FusGrid grid, int64_t Nq,
                                                          const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                          int Nv, float eps, int64_t id_base, int level, ScanRank rk, int ds_rows,
                                                          int chunks, int64_t per)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    const int blk = ds_rows * 64;                                                           // floats of one column block
    float *qs = ssm;                                                                        // [qs_floats]
    float *ds = ssm + st.qs_floats;                                                         // [S][ds_rows][64] stream clip distances
    float *fs = ds + (size_t)st.S * blk;                                                    // [ds_rows][64] fused, of the current weight
    const int slots = grid.W * rk.num_rank;                                                 // (weight, rank) pairs, weight-major
    unsigned long long *rkeys = reinterpret_cast<unsigned long long *>(fs + blk);          // [slots] rank keys
    unsigned long long *tot = rkeys + slots;                                                // [slots] the wave's counts
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - q * chunks);
    for (int i = lane; i < slots; i += 64) {
        rkeys[i] = make_key(rk.dist[(int64_t)i * Nq + q], (unsigned)rk.idx[(int64_t)i * Nq + q]);
        tot[i] = 0ull;
    }
    fus_query_rows(st, q, qs, lane);                           // (ends in a barrier: rkeys / tot are visible too)

    const int64_t v0 = (int64_t)ch * per;
    const int64_t v1 = v0 + per < Nv ? v0 + per : Nv;
    for (int64_t vb = v0; vb < v1; vb += 64) {
        const int64_t l = vb + lane;
        int n = 0;
        int64_t mbase = 0;
        if (l < v1) {
            const int c0 = clip_off[l];
            n = clip_off[l + 1] - c0;
            n = n > ds_rows ? ds_rows : (n < 0 ? 0 : n);
            mbase = id_base + mom_off[l];
            for (int c = 0; c < n; ++c) {                      // the lane's own columns, one per stream
#pragma unroll
                for (int s = 0; s < FUS_MAX_S; ++s)
                    if (s < st.S)
                        ds[s * blk + c * 64 + lane] =
                            fus_dist(st.V[s] + ((int64_t)c0 + c) * st.D[s], qs + st.qo[s], st.D[s], st.vec[s] != 0, eps);
            }
        }
        for (int wi = 0; wi < grid.W; ++wi) {
            for (int c = 0; c < n; ++c) {
                float d[FUS_MAX_S] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < FUS_MAX_S; ++s)
                    if (s < st.S) d[s] = ds[s * blk + c * 64 + lane];
                fs[c * 64 + lane] = fus_fuse(grid, wi, st.S, d);
            }
            unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
            for (int r = 0; r < SCAN_MAX_RANK; ++r) rkey[r] = r < rk.num_rank ? rkeys[wi * rk.num_rank + r] : 0ull;
            int nlt[SCAN_MAX_RANK] = {0, 0, 0, 0};
            // no list, so no wave-uniform step: every lane walks its own triangle
            if (level == VFR_FUSION_VIDEOS) {
                unsigned long long best = SCAN_KEY_EMPTY;
                for (int s = 0; s < n; ++s) {
                    float sum = 0.0f;
                    for (int e2 = s; e2 < n; ++e2) {
                        const float de = fs[e2 * 64 + lane];
                        sum = e2 == s ? de : sum + de;
                        const float sc = sum / (float)(e2 - s + 1);
                        const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e2)));
                        best = key < best ? key : best;
                    }
                }
                if (n > 0) {
#pragma unroll
                    for (int r = 0; r < SCAN_MAX_RANK; ++r) nlt[r] += (r < rk.num_rank && best < rkey[r]) ? 1 : 0;
                }
            } else {
                for (int s = 0; s < n; ++s) {
                    float sum = 0.0f;
                    for (int e2 = s; e2 < n; ++e2) {
                        const float de = fs[e2 * 64 + lane];
                        sum = e2 == s ? de : sum + de;
                        const float sc = sum / (float)(e2 - s + 1);
                        const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e2)));
#pragma unroll
                        for (int r = 0; r < SCAN_MAX_RANK; ++r) nlt[r] += (r < rk.num_rank && key < rkey[r]) ? 1 : 0;
                    }
                }
            }
            // flush: a block adds at most 64 x 2080 per (weight, rank), the totals are 64-bit (one wave may stream the whole bank)
#pragma unroll
            for (int r = 0; r < SCAN_MAX_RANK; ++r) {
                if (r < rk.num_rank) {
                    int x = nlt[r];
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
                    if (lane == 0 && x) tot[wi * rk.num_rank + r] += (unsigned long long)(unsigned)x;
                }
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < slots; i += 64) {
        const unsigned long long x = tot[i];
        if (x) atomicAdd(reinterpret_cast<unsigned long long *>(rk.count_lt + (int64_t)i * Nq + q), x);
    }
}

// the grid of a sweep call, checked -> the by-value kernel argument (before fus_streams, which then sees row 0 as its weights)
int fus_grid(const char *who, const float *w_host, int W, int S, FusGrid *out)
{
    VFR_REQUIRE(W >= 1 && W <= FUS_MAX_SWEEP, VFR_EINVAL, "%s: W = %d weight vectors (1 .. %d = VFR_FUSION_MAX_SWEEP)", who, W,
                FUS_MAX_SWEEP);
    VFR_REQUIRE(S >= 1 && S <= FUS_MAX_S, VFR_EINVAL, "%s: S = %d streams (1 .. %d)", who, S, FUS_MAX_S);
    VFR_REQUIRE(w_host, VFR_EINVAL, "%s: null stream array (Q_host, V_host, D_host, w_host)", who);
    FusGrid g{};
    g.W = W;
    for (int i = 0; i < W; ++i)
        for (int s = 0; s < S; ++s) {
            const float w = w_host[i * S + s];
            VFR_REQUIRE(w >= 0.0f && w <= 3.402823466e38f, VFR_EINVAL, "%s: grid row %d, stream %d: weight %g (finite, >= 0)", who, i, s,
                        (double)w);
            g.w[i * S + s] = w;
        }
    *out = g;
    return VFR_OK;
}

}  // namespace
}  // namespace vfr

extern "C" {

int vfr_score_fusion_own_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int S,
                             int64_t Nq, const int32_t *clip_offsets, const int32_t *own, int Nv, int max_clips, float eps, int Mmax,
                             float *scores, vfr_stream_t stream)
{
    vfr::FusStreams st;
    const int rc = vfr::fus_streams("vfr_score_fusion_own_f32", Q_host, V_host, D_host, w_host, S, Nq > 0, Nq > 0 && Nv > 0, &st);
    if (rc != VFR_OK) return rc;
    VFR_REQUIRE(Nq >= 0 && Nq <= 0x7FFFFFFF && Nv >= 0 && Mmax >= 0 && max_clips >= 0 && max_clips <= vfr::FUS_MAX_CLIPS, VFR_EINVAL,
                "vfr_score_fusion_own_f32: bad shape (max_clips <= 64, Nq < 2^31, sizes >= 0)");
    VFR_REQUIRE(Mmax >= max_clips * (max_clips + 1) / 2, VFR_EINVAL, "vfr_score_fusion_own_f32: max_clips = %d needs Mmax >= %d, got %d",
                max_clips, max_clips * (max_clips + 1) / 2, Mmax);
    VFR_REQUIRE(Nq == 0 || (own && (scores || Mmax == 0) && (clip_offsets || Nv == 0)), VFR_EINVAL,
                "vfr_score_fusion_own_f32: null own / scores / clip_offsets");
    if (Nq == 0 || Mmax == 0) return VFR_OK;
    hipStream_t stq = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, stq);
    hipLaunchKernelGGL(vfr::fusion_own_kernel, dim3((unsigned)Nq), dim3(64), (size_t)st.qs_floats * 4, stq, st, Nq, clip_offsets, own, Nv,
                       eps, Mmax, scores);
    VFR_CHECK_LAUNCH("fusion_own_kernel");
    return VFR_OK;
}

size_t vfr_score_fusion_workspace_bytes(int64_t Nq, int Nv, int k)
{
    if (Nq < 0 || Nv < 0 || k < 0 || k > vfr::SCAN_MAX_K || Nq * (int64_t)(k > 0 ? k : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(Nq, Nv, vfr::SCAN_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Nq * (size_t)k * 8 + 256, 256);
}

int vfr_score_fusion_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int S,
                         int64_t Nq, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips, int min_clips,
                         int max_clips, float eps, int64_t id_base, int level, int k, float *out_dist, int64_t *out_idx, int num_rank,
                         const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, void *workspace, size_t workspace_bytes,
                         vfr_stream_t stream)
{
    (void)min_clips;
    vfr::FusStreams st;
    const int rc = vfr::fus_streams("vfr_score_fusion_f32", Q_host, V_host, D_host, w_host, S, Nq > 0, total_clips > 0, &st);
    if (rc != VFR_OK) return rc;
    VFR_REQUIRE(level == VFR_FUSION_MOMENTS || level == VFR_FUSION_VIDEOS, VFR_EINVAL,
                "vfr_score_fusion_f32: level %d (0 = moments, 1 = videos)", level);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::FUS_MAX_CLIPS && id_base >= 0, VFR_EINVAL,
                "vfr_score_fusion_f32: bad shape (k <= 448, max_clips <= 64, sizes, id_base >= 0)");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_fusion_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(Nq * (int64_t)(k > 0 ? k : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_fusion_f32: Nq * k must stay below 2^31");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_fusion_f32: num_rank %d (0 .. 4)", num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_fusion_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || Nq == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_fusion_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets), VFR_EINVAL, "vfr_score_fusion_f32: null clip_offsets / moment_offsets");
    const vfr::ScanPlan plan = vfr::scan_plan(Nq, Nv, vfr::SCAN_TARGET_WAVES);
    VFR_REQUIRE(Nq * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_fusion_f32: too many (query, chunk) waves");
    const size_t need = vfr_score_fusion_workspace_bytes(Nq, Nv, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_fusion_f32: workspace %zu < %zu bytes", workspace_bytes,
                need);
    if (Nq == 0 || (k == 0 && num_rank == 0)) return VFR_OK;
    hipStream_t stq = vfr::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, stq);
        const int rows = max_clips < 1 ? 1 : max_clips;
        const int cap = vfr::scan_cap(k);
        const size_t lds = ((size_t)st.qs_floats + (size_t)rows * 64) * 4 + (size_t)cap * 8;     // <= 32 + 16 + 4 KB
        vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        hipLaunchKernelGGL(vfr::fusion_scan_kernel, dim3((unsigned)(Nq * plan.chunks)), dim3(64), lds, stq, st, Nq, clip_offsets,
                           moment_offsets, Nv, eps, id_base, level, k, cap, rk, rows, plan.chunks, plan.per, keys);
        VFR_CHECK_LAUNCH("fusion_scan_kernel");
    }
    if (k > 0)
        return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Nq, k, out_dist, out_idx, nullptr, stream);
    return VFR_OK;
}

int vfr_score_fusion_sweep_own_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int W,
                                   int S, int64_t Nq, const int32_t *clip_offsets, const int32_t *own, int Nv, int max_clips, float eps,
                                   int Mmax, float *scores, vfr_stream_t stream)
{
    static const char who[] = "vfr_score_fusion_sweep_own_f32";
    vfr::FusGrid grid;
    int rc = vfr::fus_grid(who, w_host, W, S, &grid);
    if (rc != VFR_OK) return rc;
    vfr::FusStreams st;
    rc = vfr::fus_streams(who, Q_host, V_host, D_host, w_host, S, Nq > 0, Nq > 0 && Nv > 0, &st);
    if (rc != VFR_OK) return rc;
    VFR_REQUIRE(Nq >= 0 && Nq <= 0x7FFFFFFF && Nv >= 0 && Mmax >= 0 && max_clips >= 0 && max_clips <= vfr::FUS_MAX_CLIPS, VFR_EINVAL,
                "%s: bad shape (max_clips <= 64, Nq < 2^31, sizes >= 0)", who);
    VFR_REQUIRE(Mmax >= max_clips * (max_clips + 1) / 2, VFR_EINVAL, "%s: max_clips = %d needs Mmax >= %d, got %d", who, max_clips,
                max_clips * (max_clips + 1) / 2, Mmax);
    VFR_REQUIRE(Nq == 0 || (own && (scores || Mmax == 0) && (clip_offsets || Nv == 0)), VFR_EINVAL,
                "%s: null own / scores / clip_offsets", who);
    if (Nq == 0 || Mmax == 0) return VFR_OK;
    hipStream_t stq = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, stq);
    hipLaunchKernelGGL(vfr::fusion_sweep_own_kernel, dim3((unsigned)Nq), dim3(64), (size_t)st.qs_floats * 4, stq, st, grid, Nq,
                       clip_offsets, own, Nv, eps, Mmax, scores);
    VFR_CHECK_LAUNCH("fusion_sweep_own_kernel");
    return VFR_OK;
}

int vfr_score_fusion_sweep_f32(const float *const *Q_host, const float *const *V_host, const int *D_host, const float *w_host, int W,
                               int S, int64_t Nq, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv, int total_clips,
                               int max_clips, float eps, int64_t id_base, int level, int num_rank, const float *rank_dist,
                               const int64_t *rank_idx, int64_t *count_lt, vfr_stream_t stream)
{
    static const char who[] = "vfr_score_fusion_sweep_f32";
    vfr::FusGrid grid;
    int rc = vfr::fus_grid(who, w_host, W, S, &grid);
    if (rc != VFR_OK) return rc;
    vfr::FusStreams st;
    rc = vfr::fus_streams(who, Q_host, V_host, D_host, w_host, S, Nq > 0, total_clips > 0, &st);
    if (rc != VFR_OK) return rc;
    VFR_REQUIRE(level == VFR_FUSION_MOMENTS || level == VFR_FUSION_VIDEOS, VFR_EINVAL, "%s: level %d (0 = moments, 1 = videos)", who,
                level);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && max_clips >= 0 && max_clips <= vfr::FUS_MAX_CLIPS && id_base >= 0, VFR_EINVAL,
                "%s: bad shape (max_clips <= 64, sizes, id_base >= 0)", who);
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "%s: id_base + moments must stay below 2^32", who);
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "%s: num_rank %d (0 .. 4)", who, num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL, "%s: num_rank > 0 needs rank_dist, rank_idx and count_lt",
                who);
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets), VFR_EINVAL, "%s: null clip_offsets / moment_offsets", who);
    const vfr::ScanPlan plan = vfr::scan_plan(Nq, Nv, vfr::SCAN_TARGET_WAVES);
    VFR_REQUIRE(Nq * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "%s: too many (query, chunk) waves", who);
    const int rows = max_clips < 1 ? 1 : max_clips;
    const size_t lds = vfr::fus_sweep_lds(st, rows, W, num_rank);
    VFR_REQUIRE(lds <= vfr::FUS_SWEEP_LDS, VFR_EUNSUPPORTED,
                "%s: a wave needs %zu bytes of LDS (4 x %d floats of query rows + 256 x max_clips x (S + 1) + 16 x W x num_rank with "
                "max_clips = %d, S = %d, W = %d, num_rank = %d), limit %zu", who, lds, st.qs_floats, max_clips, S, W, num_rank,
                vfr::FUS_SWEEP_LDS);
    if (Nq == 0 || Nv == 0 || num_rank == 0) return VFR_OK;
    hipStream_t stq = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, stq);
    vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
    hipLaunchKernelGGL(vfr::fusion_sweep_kernel, dim3((unsigned)(Nq * plan.chunks)), dim3(64), lds, stq, st, grid, Nq, clip_offsets,
                       moment_offsets, Nv, eps, id_base, level, rk, rows, plan.chunks, plan.per);
    VFR_CHECK_LAUNCH("fusion_sweep_kernel");
    return VFR_OK;
}

}  // extern "C"
