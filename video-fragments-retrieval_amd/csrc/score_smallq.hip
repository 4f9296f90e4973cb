// The scorer's few-queries path (one serving request: 1 .. 64 queries), behind vfr_score_topk_mfma in f32 mode (score.hip
// decides with smallq_applicable and hands the whole call to run_smallq).  Exact like every f32 path.
#include "score_device.h"
#include "score_internal.h"

namespace vfr {

// ---- a handful of queries (one serving request) ---------------------------------------------------------------------
constexpr int SMALLQ_CLIPS_MAX = 21;
// The fused kernels put QUERIES on the lanes: with 1-8 queries a wave is 2-12 % full and the pass costs 0.55 ms however
// little there is to score.  Here the lanes are clips and videos: every clip distance once (lane = clip, the canonical chain
// against all NQ queries while the row streams past), then lane = video writes the keys of its moments -- the canonical sums
// and IEEE quotients of the dense kernel -- and counts them against the rank keys; the top-k is two rounds of the pool
// selection of topk_merge_parts_kernel over the key array (P ranges per query, then the P lists).  Exact like every f32 path.
template <int NQ>
__global__ __launch_bounds__(256) void smallq_dist_kernel(const float *__restrict__ Q, int Nq, const float *__restrict__ V,
                                                          int total_clips, int D, float eps, float *__restrict__ dist)
{
    // D = 100 (the model's embedding width; other widths take the general loop below): the lane's whole row is requested at
    // once (25 loads in flight), the queries sit in LDS and are read as broadcasts
    __shared__ __attribute__((aligned(16))) float qs[NQ][FAST_D];
    // blockIdx.y = group of NQ queries: all groups of a request in ONE launch (eight launches of 27 us each were 12 us of
    // arithmetic and 15 of launch gap, ramp and a 3.2-blocks-per-CU round each)
    Q += (int64_t)blockIdx.y * NQ * D;
    dist += (int64_t)blockIdx.y * NQ * total_clips;
    Nq = Nq - (int)blockIdx.y * NQ < NQ ? Nq - (int)blockIdx.y * NQ : NQ;
    const int c = blockIdx.x * 256 + threadIdx.x;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0f;
    if (D == FAST_D) {
        for (int i = threadIdx.x; i < NQ * FAST_D; i += 256) qs[i / FAST_D][i % FAST_D] = Q[(int64_t)(i / FAST_D < Nq ? i / FAST_D : 0) * FAST_D + i % FAST_D];
        float4 row[FAST_D / 4];
        const float4 *v4 = reinterpret_cast<const float4 *>(V + (int64_t)(c < total_clips ? c : total_clips - 1) * FAST_D);
#pragma unroll
        for (int k4 = 0; k4 < FAST_D / 4; ++k4) row[k4] = v4[k4];
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < FAST_D / 4; ++k4) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float4 qq = *reinterpret_cast<const float4 *>(&qs[q][4 * k4]);
                float t = (row[k4].x - qq.x) + eps; acc[q] = __builtin_fmaf(t, t, acc[q]);
                t = (row[k4].y - qq.y) + eps; acc[q] = __builtin_fmaf(t, t, acc[q]);
                t = (row[k4].z - qq.z) + eps; acc[q] = __builtin_fmaf(t, t, acc[q]);
                t = (row[k4].w - qq.w) + eps; acc[q] = __builtin_fmaf(t, t, acc[q]);
            }
        }
    } else if (c < total_clips) {
        const float *v = V + (int64_t)c * D;
        for (int k = 0; k < D; ++k) {
            const float vk = v[k];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float t = (vk - Q[(int64_t)(q < Nq ? q : 0) * D + k]) + eps;
                acc[q] = __builtin_fmaf(t, t, acc[q]);
            }
        }
    }
    if (c >= total_clips) return;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q < Nq) dist[(int64_t)q * total_clips + c] = __builtin_sqrtf(acc[q]);
}

// 16 videos per block, 16 threads per video (thread = the moments starting at clip s, s + 16, ...): canonical sums and
// quotients, keys staged in LDS at their moment index and written out as one contiguous run (the videos' moments are
// adjacent), rank counts reduced over the block
constexpr int SQ_VIDEOS = 16, SQ_MOM = SMALLQ_CLIPS_MAX * (SMALLQ_CLIPS_MAX + 1) / 2;
__global__ __launch_bounds__(256) void smallq_moments_kernel(const float *__restrict__ dist, int Nq, const int32_t *__restrict__ clip_off,
                                                             const int64_t *__restrict__ mom_off, int Nv, int total_clips, int64_t id_base,
                                                             unsigned long long *__restrict__ keys, int64_t Mpad, int num_rank,
                                                             const float *__restrict__ rank_dist, const int64_t *__restrict__ rank_idx,
                                                             int64_t *__restrict__ count_lt, float *__restrict__ dmin)
{
    __shared__ unsigned long long stage[SQ_VIDEOS * SQ_MOM];
    __shared__ float ds[SQ_VIDEOS][SMALLQ_CLIPS_MAX + 3];
    __shared__ int red[MAX_RANK][4];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int vl = threadIdx.x >> 4, sl = threadIdx.x & 15;                   // video within the block, first start clip
    const int v0 = blockIdx.x * SQ_VIDEOS, v = v0 + vl;
    unsigned long long kstar[MAX_RANK] = {0, 0, 0, 0};
    for (int r = 0; r < num_rank; ++r) kstar[r] = make_key(rank_dist[(int64_t)r * Nq + q], (unsigned)rank_idx[(int64_t)r * Nq + q]);
    int nlt[MAX_RANK] = {0, 0, 0, 0};
    const int vhi = v0 + SQ_VIDEOS < Nv ? v0 + SQ_VIDEOS : Nv;
    const int64_t mb0 = mom_off[v0], mb1 = mom_off[vhi];                      // the block's run of moments
    int n = 0, c0 = 0;
    int64_t m0 = 0;
    if (v < Nv) { c0 = clip_off[v]; n = clip_off[v + 1] - c0; m0 = mom_off[v]; }
    float dm = __builtin_inff();
    for (int c = sl; c < n; c += 16) { const float dv = dist[(int64_t)q * total_clips + c0 + c]; ds[vl][c] = dv; dm = dv < dm ? dv : dm; }
    if (dmin) {           // the video's smallest clip distance = the score of its best one-clip moment (top-k selection below)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { const float t = __shfl_xor(dm, o, 64); dm = t < dm ? t : dm; }
        if (sl == 0 && v < Nv) dmin[(int64_t)q * Nv + v] = dm;
    }
    __syncthreads();
    for (int s = sl; s < n; s += 16) {
        float sum = 0.0f;
        for (int e = s; e < n; ++e) {
            const float de = ds[vl][e];
            sum = e == s ? de : sum + de;
            const float sc = sum / (float)(e - s + 1);
            const int64_t m = m0 + moment_index(n, s, e);
            const unsigned long long key = make_key(sc, (unsigned)(id_base + m));
            stage[m - mb0] = key;
#pragma unroll
            for (int r = 0; r < MAX_RANK; ++r) nlt[r] += key < kstar[r] ? 1 : 0;     // kstar = 0 when unused
        }
    }
    for (int r = 0; r < num_rank; ++r) {
        int x = nlt[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) red[r][wv] = x;
    }
    __syncthreads();
    if (keys)
        for (int64_t i = threadIdx.x; i < mb1 - mb0; i += 256) keys[(int64_t)q * Mpad + mb0 + i] = stage[i];
    if ((int)threadIdx.x < num_rank) {
        const int r = threadIdx.x;
        const long long t = (long long)red[r][0] + red[r][1] + red[r][2] + red[r][3];
        if (t) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + (int64_t)r * Nq + q), (unsigned long long)t);
    }
}

// Rank counts + per-video smallest clip distance for the video-selection form (no key array wanted): lane = VIDEO.  The moment
// kernel above gives a video to 16 threads by start clip -- thread 0 of a 21-clip video walks 26 moments, thread 15 six, and every
// moment pays an LDS key store, four 64-bit compares, a run-time moment index and an 11-instruction IEEE division: 0.32 ms at 64
// queries x 10 000 videos, a quarter of that request.  Here a lane keeps its video's distances in registers (+inf past its clip
// count: such moments compare false), the triangle is straight-line code -- the canonical sum (clips left to right from the start
// clip), the quotient by a compile-time length as c_div_small (3 instructions, the IEEE quotient for every sum in [2^-60, 2^100]:
// vfr_math.h), two float compares per rank key -- and the moment id only exists on the slow path: a lane whose score EQUALS a rank
// distance somewhere (the id decides), or whose distances leave that range, redoes its video with keys and IEEE divisions.
// One wave per 64 videos and query; from `score_smallq_rank` (8) queries on -- below, the 16-threads-per-video form has more waves
// in flight for the same work and finishes sooner.
template <int NT, int NR>
__global__ __launch_bounds__(64) void smallq_rank_kernel(const float *__restrict__ dist, int Nq, const int32_t *__restrict__ clip_off,
                                                         const int64_t *__restrict__ mom_off, int Nv, int total_clips, int64_t id_base,
                                                         int num_rank, const float *__restrict__ rank_dist, const int64_t *__restrict__ rank_idx,
                                                         int64_t *__restrict__ count_lt, float *__restrict__ dmin)
{
    const int q = blockIdx.y, lane = threadIdx.x;
    const int v = blockIdx.x * 64 + lane;
    int n = 0, c0 = 0;
    if (v < Nv) { c0 = clip_off[v]; n = clip_off[v + 1] - c0; }
    float d[NT];
    float dm = __builtin_inff(), dx = 0.0f;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const float x = c < n ? dist[(int64_t)q * total_clips + c0 + c] : 0.0f;
        dm = c < n && x < dm ? x : dm;
        dx = x > dx ? x : dx;
        d[c] = c < n ? x : __builtin_inff();
    }
    if (dmin && v < Nv) dmin[(int64_t)q * Nv + v] = dm;
    if (num_rank == 0) return;
    float kd[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) kd[r] = r < num_rank ? rank_dist[(int64_t)r * Nq + q] : -1.0f;     // (scores are >= 0: an unused key counts nothing)
    int nlt[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) nlt[r] = 0;
    // every sum of this video lies in [smallest distance, NT x largest]: inside c_div_small's range?
    bool slow = n > 0 && (dm < C_DIV_SMALL_LO || dx > C_DIV_SMALL_HI / 32.0f);
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        float sum = d[s];
#pragma unroll
        for (int e = s; e < NT; ++e) {
            if (e > s) sum = sum + d[e];
            const float sc = c_div_small(sum, e - s + 1);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                nlt[r] += sc < kd[r] ? 1 : 0;
                slow = slow || sc == kd[r];
            }
        }
    }
    if (slow) {
        unsigned long long kstar[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) { nlt[r] = 0; kstar[r] = r < num_rank ? make_key(kd[r], (unsigned)rank_idx[(int64_t)r * Nq + q]) : 0ull; }
        const int64_t m0 = mom_off[v < Nv ? v : 0];
        for (int s = 0; s < n; ++s) {
            float sum = 0.0f;
            for (int e = s; e < n; ++e) {
                const float de = dist[(int64_t)q * total_clips + c0 + e];
                sum = e == s ? de : sum + de;
                const unsigned long long key = make_key(sum / (float)(e - s + 1), (unsigned)(id_base + m0 + moment_index(n, s, e)));
#pragma unroll
                for (int r = 0; r < NR; ++r) nlt[r] += key < kstar[r] ? 1 : 0;
            }
        }
    }
    for (int r = 0; r < NR; ++r) {
        if (r >= num_rank) break;
        int x = nlt[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0 && x) atomicAdd(reinterpret_cast<unsigned long long *>(count_lt + (int64_t)r * Nq + q), (unsigned long long)x);
    }
}

// One level of the selection tree over key lists [q][Pin][k]: wave (q, r) reads lists r*F .. r*F + F - 1 of query q as one
// flat range -- the next round's keys requested before the current round is filtered -- keeps the k smallest in the LDS
// pool of the merge kernels and writes them as list r of [q][Pout][k] (or, at the root, as the query's (dist, idx) rows).
template <int KPL>
__global__ __launch_bounds__(256) void topk_tree_kernel(const unsigned long long *__restrict__ in, int64_t Pin, int F, int64_t Pout,
                                                        int64_t n_vq, int k, unsigned long long *__restrict__ out_keys,
                                                        float *__restrict__ out_dist, int64_t *__restrict__ out_idx)
{
    constexpr int CAP = KPL * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t vq = (int64_t)blockIdx.x * 4 + wv;
    if (vq >= n_vq) return;
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
    const int64_t q = vq / Pout, r = vq - q * Pout, first = r * F;
    const int64_t nl = Pin - first < F ? Pin - first : F;
    const unsigned long long *src = in + (q * Pin + first) * k;
    const int64_t total = nl * k;
    // NB rounds of CAP keys are requested together and the next NB before these are filtered: a wave is alone with its
    // range, so the memory latency it pays is per batch of requests, not per round
    constexpr int NB = 4;
    unsigned long long x[NB][KPL], xn[NB][KPL];
    auto load = [&](unsigned long long (&dst)[NB][KPL], int64_t done) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int64_t gi = done + (b * KPL + i) * 64 + lane;
                const unsigned long long vv = src[gi < total ? gi : total - 1];
                dst[b][i] = (gi < total && vv < KEY_EMPTY) ? vv : KEY_MAX;
            }
    };
    load(x, 0);
    for (int64_t done = 0; done < total; done += NB * CAP) {
        load(xn, done + NB * CAP);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                if (fill + 64 > CAP) sort_pool(false);
                const bool pass = x[b][i] < thr;                 // KEY_MAX (empty) never passes
                const unsigned long long m = __ballot(pass);
                if (pass) pool[fill + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = x[b][i];
                fill += __builtin_popcountll(m);
            }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < KPL; ++i) x[b][i] = xn[b][i];
    }
    sort_pool(true);
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int e = i * 64 + lane;
        if (e < k) {
            const bool ok = key[i] != KEY_MAX;
            if (out_dist) {
                out_dist[vq * k + e] = ok ? __uint_as_float((unsigned)(key[i] >> 32)) : __builtin_inff();
                out_idx[vq * k + e] = ok ? (int64_t)(key[i] & 0xffffffffull) : -1;
            } else {
                out_keys[vq * k + e] = ok ? key[i] : KEY_EMPTY;
            }
        }
    }
}

// Top-k of a handful of queries WITHOUT the key array and the selection tree (three latency-bound levels: 0.09 ms at one
// query).  Every moment's score is a mean of its video's clip distances, so score >= dmin_v * (1 - 22 u) (dmin_v = the
// video's smallest clip distance; each rounding is monotone), and dmin_v itself is the score of a one-clip moment.  Hence any
// thr that is >= the k-th smallest dmin over the videos bounds the k-th best moment, and only videos with
// dmin_v <= thr * (1 + 32 u) can hold a moment of the top-k.  One 1024-thread workgroup per query:
//   A  thr: min / max of the dmin row, a 2048-bin histogram over [min, max], the first bin b* at which the running count
//      reaches k; thr = the largest dmin in bins <= b* (>= k videos lie at or below it).  Nv <= k: thr = +inf (everything);
//   B  the videos passing the margin test are listed in LDS (4096 at a time);
//   C  thread = (listed video, start clip): the canonical sums and IEEE quotients of smallq_moments_kernel, keys <= (thr, max id)
//      appended to the query's candidate run in global memory (the slot from an LDS counter: one workgroup owns the query);
//   D  wave 0 runs the pool selection of the merge kernels over the candidates (typically a few hundred) and writes the rows.
// Exact: the candidates are a superset of the top-k with the dense kernel's keys.
constexpr int SQS_BINS = 2048, SQS_LIST = 4096, SQS_THREADS = 1024;
static_assert(SQS_BINS == 2 * SQS_THREADS, "the bin scan gives every thread two bins");
static_assert(SQS_LIST >= 2 * SQS_THREADS, "the video list must take at least one full chunk of candidates after a partial one");
template <int KPL>
__global__ __launch_bounds__(SQS_THREADS) void smallq_select_kernel(const float *__restrict__ dist, const float *__restrict__ dmin,
                                                                    const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                                    int Nv, int total_clips, int64_t id_base, int k,
                                                                    unsigned long long *__restrict__ cand, int64_t cand_stride,
                                                                    float *__restrict__ out_dist, int64_t *__restrict__ out_idx)
{
    constexpr int CAP = KPL * 64;
    __shared__ int hist[SQS_BINS];
    __shared__ int vlist[SQS_LIST];
    __shared__ float redf[2][SQS_THREADS / 64];
    __shared__ int redi[SQS_THREADS / 64];
    __shared__ int s_bstar, s_nlist, s_ncand;
    __shared__ unsigned long long pool[CAP];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *dq = dmin + (int64_t)q * Nv;
    unsigned long long *cq = cand + (int64_t)q * cand_stride;
    // ---- A: threshold ----
    float mn = __builtin_inff(), mx = 0.0f;
    for (int v = tid; v < Nv; v += SQS_THREADS) { const float x = dq[v]; mn = x < mn ? x : mn; mx = (x > mx && x < __builtin_inff()) ? x : mx; }   // (a video without clips: +inf)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
    if (lane == 0) { redf[0][wv] = mn; redf[1][wv] = mx; }
    for (int i = tid; i < SQS_BINS; i += SQS_THREADS) hist[i] = 0;
    if (tid == 0) { s_nlist = 0; s_ncand = 0; s_bstar = SQS_BINS - 1; }
    __syncthreads();
    mn = redf[0][0]; mx = redf[1][0];
#pragma unroll
    for (int i = 1; i < SQS_THREADS / 64; ++i) { mn = redf[0][i] < mn ? redf[0][i] : mn; mx = redf[1][i] > mx ? redf[1][i] : mx; }
    const float scale = mx > mn ? (float)(SQS_BINS - 1) / (mx - mn) : 0.0f;
    auto bin_of = [&](float x) {
        if (!(x < __builtin_inff())) return SQS_BINS - 1;
        const int b = (int)((x - mn) * scale);
        return b < 0 ? 0 : (b > SQS_BINS - 1 ? SQS_BINS - 1 : b);
    };
    float thr = __builtin_inff();
    if (Nv > k) {
        for (int v = tid; v < Nv; v += SQS_THREADS) atomicAdd(&hist[bin_of(dq[v])], 1);
        __syncthreads();
        // running count over the bins: thread t owns bins 2t, 2t + 1
        const int h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
        int part = h0 + h1, incl = part;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63) redi[wv] = incl;
        __syncthreads();
        int before = 0;
        for (int i = 0; i < wv; ++i) before += redi[i];
        const int excl = before + incl - part;                              // videos in bins < 2t
        if (excl < k && excl + h0 >= k) s_bstar = 2 * tid;
        else if (excl + h0 < k && excl + part >= k) s_bstar = 2 * tid + 1;
        __syncthreads();
        const int bstar = s_bstar;
        float tm = 0.0f;
        for (int v = tid; v < Nv; v += SQS_THREADS) { const float x = dq[v]; if (bin_of(x) <= bstar) tm = x > tm ? x : tm; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const float a = __shfl_xor(tm, o, 64); tm = a > tm ? a : tm; }
        if (lane == 0) redf[0][wv] = tm;
        __syncthreads();
        tm = redf[0][0];
#pragma unroll
        for (int i = 1; i < SQS_THREADS / 64; ++i) tm = redf[0][i] > tm ? redf[0][i] : tm;
        thr = tm;
    }
    const unsigned long long thrkey = thr < __builtin_inff() ? (((unsigned long long)__float_as_uint(thr) << 32) | 0xFFFFFFFFull) : KEY_MAX;
    const float vthr = thr < __builtin_inff() ? thr * (1.0f + 32.0f * 5.9604645e-8f) : thr;
    // ---- B + C: listed videos, SQS_LIST at a time ----
    for (int vbase = 0; vbase < Nv; ) {
        __syncthreads();
        if (tid == 0) s_nlist = 0;
        __syncthreads();
        // fill the list from vbase on; stop at the chunk of SQS_THREADS videos that would overflow it
        int vend = vbase;
        while (vend < Nv) {
            const int v = vend + tid;
            const bool sel = v < Nv && dq[v] <= vthr;
            if (sel) { const int slot = atomicAdd(&s_nlist, 1); if (slot < SQS_LIST) vlist[slot] = v; }
            vend += SQS_THREADS;
            __syncthreads();
            if (s_nlist + SQS_THREADS > SQS_LIST) break;                     // uniform: the next chunk might not fit
            __syncthreads();
        }
        __syncthreads();
        const int nlist = s_nlist < SQS_LIST ? s_nlist : SQS_LIST;          // (never exceeds: checked before every chunk)
        for (int it = tid; it < nlist * SMALLQ_CLIPS_MAX; it += SQS_THREADS) {
            const int v = vlist[it / SMALLQ_CLIPS_MAX], s0 = it % SMALLQ_CLIPS_MAX;
            const int c0 = clip_off[v], n = clip_off[v + 1] - c0;
            if (s0 >= n) continue;
            const int64_t m0 = mom_off[v];
            const float *dv = dist + (int64_t)q * total_clips + c0;
            float sum = 0.0f;
            for (int e = s0; e < n; ++e) {
                const float de = dv[e];
                sum = e == s0 ? de : sum + de;
                const float sc = sum / (float)(e - s0 + 1);
                const unsigned long long key = make_key(sc, (unsigned)(id_base + m0 + moment_index(n, s0, e)));
                if (key <= thrkey) cq[atomicAdd(&s_ncand, 1)] = key;
            }
        }
        vbase = vend < Nv ? vend : Nv;
    }
    __threadfence_block();
    __syncthreads();
    if (wv != 0) return;
    // ---- D: wave 0 selects the k best of the candidates ----
    const int64_t total = s_ncand;
    unsigned long long key[KPL];
    unsigned long long pthr = KEY_MAX;
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
        if (fill >= k) pthr = key_at<KPL>(key, k - 1);
        fill = fill < k ? fill : k;
    };
    for (int64_t done = 0; done < total; done += CAP) {
        unsigned long long x[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int64_t gi = done + i * 64 + lane;
            const unsigned long long vv = cq[gi < total ? gi : total - 1];
            x[i] = gi < total ? vv : KEY_MAX;
        }
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            if (fill + 64 > CAP) sort_pool(false);
            const bool pass = x[i] < pthr;
            const unsigned long long m = __ballot(pass);
            if (pass) pool[fill + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = x[i];
            fill += __builtin_popcountll(m);
        }
    }
    sort_pool(true);
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int e = i * 64 + lane;
        if (e < k) {
            const bool ok = key[i] != KEY_MAX;
            out_dist[(int64_t)q * k + e] = ok ? __uint_as_float((unsigned)(key[i] >> 32)) : __builtin_inff();
            out_idx[(int64_t)q * k + e] = ok ? (int64_t)(key[i] & 0xffffffffull) : -1;
        }
    }
}

constexpr int SMALLQ_MAX = 64, SMALLQ_CLIPS = SMALLQ_CLIPS_MAX;
struct SmallqWs { float *dist; unsigned long long *keys, *bufa, *bufb; float *dmin; int64_t Mpad, P0, P1; size_t total; };
constexpr int SQ_F1 = 20, SQ_F = 32;        // lists of k per first-level range; fan-in of the later levels
static SmallqWs carve_smallq(void *base, int64_t Nq, int total_clips, int k)
{
    SmallqWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes, 256); return p; };
    const int64_t Mb = (int64_t)total_clips * (SMALLQ_CLIPS + 1) / 2 + 1;            // >= total moments when every video has <= 21 clips
    w.dist = reinterpret_cast<float *>(take((size_t)Nq * total_clips * 4));
    if (k > 0) {
        w.P0 = cdiv(Mb, k);                                                           // the key array as lists of k
        w.Mpad = w.P0 * k;
        w.P1 = cdiv(w.P0, SQ_F1);
        w.keys = reinterpret_cast<unsigned long long *>(take((size_t)Nq * w.Mpad * 8));
        w.bufa = reinterpret_cast<unsigned long long *>(take((size_t)Nq * w.P1 * k * 8));
        w.bufb = reinterpret_cast<unsigned long long *>(take((size_t)Nq * cdiv(w.P1, SQ_F) * k * 8));
        w.dmin = reinterpret_cast<float *>(take((size_t)Nq * total_clips * 4));           // (Nv <= total_clips)
    }
    w.total = off;
    return w;
}
size_t smallq_workspace_bytes(int64_t Nq, int total_clips, int k)
{
    return Nq <= SMALLQ_MAX ? carve_smallq(nullptr, Nq, total_clips, k).total : 0;
}
bool smallq_applicable(int64_t Nq, int Nv, int total_clips, int max_clips, int num_rank, int k)
{
    const int lim = opt_score_smallq() < SMALLQ_MAX ? opt_score_smallq() : SMALLQ_MAX;
    return Nq > 0 && Nq <= lim && Nv > 0 && total_clips > 0 && max_clips <= SMALLQ_CLIPS && num_rank <= MAX_RANK && k <= 448;
}
int run_smallq(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
               int total_clips, int max_clips, int D, float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx, int num_rank,
               const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, void *workspace, vfr_stream_t stream)
{
    hipStream_t st = as_stream(stream);
    SmallqWs w = carve_smallq(workspace, Nq, total_clips, k);
    {
        ProfScope prof(SITE_SCORE_FUSED, st);
        const dim3 grid((unsigned)cdiv(total_clips, 256));
        // eight queries per pass over the bank (sixteen were measured: 0.574 against 0.542 ms at 64 queries, 0.194 against 0.184 at
        // 16 -- the kernel is bound by its 3 VALU issues per (query, clip, dimension), not by the row reads, and the wider
        // form's registers cost a wave of occupancy)
        {
            const dim3 g8(grid.x, (unsigned)cdiv(Nq, 8));
            if (Nq == 1)      hipLaunchKernelGGL(smallq_dist_kernel<1>, grid, dim3(256), 0, st, Q, (int)Nq, V, total_clips, D, eps, w.dist);
            else if (Nq == 2) hipLaunchKernelGGL(smallq_dist_kernel<2>, grid, dim3(256), 0, st, Q, (int)Nq, V, total_clips, D, eps, w.dist);
            else if (Nq <= 4) hipLaunchKernelGGL(smallq_dist_kernel<4>, grid, dim3(256), 0, st, Q, (int)Nq, V, total_clips, D, eps, w.dist);
            else              hipLaunchKernelGGL(smallq_dist_kernel<8>, g8, dim3(256), 0, st, Q, (int)Nq, V, total_clips, D, eps, w.dist);
        }
        // top-k by video selection (smallq_select_kernel) unless switched off: then the key array + selection tree
        const bool select = k > 0 && opt_score_smallq_select();
        // unwritten key slots (the padding past the last moment) must read as empty: any value >= KEY_EMPTY does
        if (k > 0 && !select && hipMemsetAsync(w.keys, 0xFF, (size_t)Nq * w.Mpad * 8, st) != hipSuccess)
            return fail(VFR_EHIP, "vfr_score_topk_mfma: hipMemsetAsync failed");
        if (select && opt_score_smallq_rank() > 0 && Nq >= opt_score_smallq_rank()) {
            // video-selection form: no key array -- rank counts and the per-video smallest distance with lane = video
            const dim3 rgrid((unsigned)cdiv(Nv, 64), (unsigned)Nq);
#define VFR_SQR(NTV, NRV) hipLaunchKernelGGL((smallq_rank_kernel<NTV, NRV>), rgrid, dim3(64), 0, st, w.dist, (int)Nq, clip_offsets, moment_offsets, Nv, total_clips, \
                                             id_base, num_rank, rank_dist, rank_idx, count_lt, w.dmin)
            if (max_clips <= 6) { if (num_rank <= 2) VFR_SQR(6, 2); else VFR_SQR(6, MAX_RANK); }
            else                { if (num_rank <= 2) VFR_SQR(SMALLQ_CLIPS_MAX, 2); else VFR_SQR(SMALLQ_CLIPS_MAX, MAX_RANK); }
#undef VFR_SQR
        } else
        if (k > 0 || num_rank > 0)
            hipLaunchKernelGGL(smallq_moments_kernel, dim3((unsigned)cdiv(Nv, SQ_VIDEOS), (unsigned)Nq), dim3(256), 0, st, w.dist, (int)Nq, clip_offsets,
                               moment_offsets, Nv, total_clips, id_base, (k > 0 && !select) ? w.keys : nullptr, w.Mpad, num_rank, rank_dist, rank_idx,
                               count_lt, select ? w.dmin : nullptr);
        VFR_CHECK_LAUNCH("smallq kernels");
    }
    {
        const bool select = k > 0 && opt_score_smallq_select();
        if (select) {
            ProfScope prof2(SITE_TOPK_MERGE, st);
            if (kpl_for(k) == 4)
                hipLaunchKernelGGL(smallq_select_kernel<4>, dim3((unsigned)Nq), dim3(SQS_THREADS), 0, st, w.dist, w.dmin, clip_offsets, moment_offsets,
                                   Nv, total_clips, id_base, k, w.keys, w.Mpad, out_dist, out_idx);
            else
                hipLaunchKernelGGL(smallq_select_kernel<8>, dim3((unsigned)Nq), dim3(SQS_THREADS), 0, st, w.dist, w.dmin, clip_offsets, moment_offsets,
                                   Nv, total_clips, id_base, k, w.keys, w.Mpad, out_dist, out_idx);
            VFR_CHECK_LAUNCH("smallq_select_kernel");
            return VFR_OK;
        }
    }
    if (k == 0) return VFR_OK;
    // selection tree: ranges of SQ_F1 lists of k keys -> lists of k, then SQ_F lists at a time until one list per query is left
    ProfScope prof(SITE_TOPK_MERGE, st);
    const int kpl = kpl_for(k);
    const unsigned long long *in = w.keys;
    int64_t Pin = w.P0;
    int F = SQ_F1;
    unsigned long long *bufs[2] = {w.bufa, w.bufb};
    for (int level = 0;; ++level) {
        const int64_t Pout = cdiv(Pin, F), n_vq = Nq * Pout;
        const bool root = Pout == 1;
        unsigned long long *out = root ? nullptr : bufs[level & 1];
        const dim3 grid((unsigned)cdiv(n_vq, 4));
        if (kpl == 4) hipLaunchKernelGGL(topk_tree_kernel<4>, grid, dim3(256), 0, st, in, Pin, F, Pout, n_vq, k, out, root ? out_dist : nullptr, root ? out_idx : nullptr);
        else          hipLaunchKernelGGL(topk_tree_kernel<8>, grid, dim3(256), 0, st, in, Pin, F, Pout, n_vq, k, out, root ? out_dist : nullptr, root ? out_idx : nullptr);
        if (root) break;
        in = out; Pin = Pout; F = Pin <= 2 * SQ_F ? (int)Pin : SQ_F;
    }
    VFR_CHECK_LAUNCH("topk_tree_kernel");
    return VFR_OK;
}

}  // namespace vfr
