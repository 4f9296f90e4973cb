// Candidate-restricted retrieval ("search only these videos"): vfr_score_subset_f32 (include/vfr.h).
//
// Semantics are those of the full-corpus entry points restricted to a per-query list of videos: key = (fp32 distance, global
// moment id) ascending, id = id_base + mom_off[v] + j (j = position in utils.generate_moments(n_v)), the best key of a video is
// the smallest key over its WHOLE triangle (csrc/video_topk.hip explains why the triangle is needed).  Lists are CSR over queries
// (cand_off [Nq+1] int64, cand_vid [nnz] int32, corpus-global video indices, strictly ascending per query); entries outside
// [vid_base, vid_base + Nv) belong to another shard and are skipped, so every shard takes the same lists.
//
// Kernels (a translation unit of its own: the arithmetic is the canonical chain of vtk_exact_kernel, written out here, so the code
// objects of score.o do not change; the key constants, the rank-key counters and the sort of the key buffer are those of
// scan_common.h):
//   subset_plan_kernel   one workgroup: chunk_off[q] = sum over q' < q of ceil(len_q' / 64) (a list is cut into chunks of 64
//                        entries), clamped to the host's bound on the chunk count; flags lists longer than max_list
//   subset_scan_kernel   one wave per chunk (a flattened grid: a query with 10 000 candidates and 4 999 with 10 cost 157 + 4 999
//                        waves, not Nq x 157), lane = listed video: its clip distances with the canonical chain into LDS, its
//                        whole triangle by running sums and IEEE division, the <= 4 rank counts (one atomic per wave and rank);
//                          moments: the chunk's k smallest keys, collected under a running threshold into an LDS buffer that is
//                                   sorted and cut back to k when it fills, written sorted to ws[chunk][0..k) (KEY_MAX padded)
//                          videos:  one best key per entry, ws[entry] (KEY_MAX for an entry of another shard)
//                        each lane compares its entry with its predecessor: a list that is not strictly ascending, or holds an
//                        index < 0, raises *bad
//   subset_topk_kernel   per query: the k smallest keys of its segment of ws (radix select on the key bits, bitonic sort),
//                        padded with (+inf, -1)
// Workspace: chunk_off [Nq+1] and the keys: (nnz + 63 Nq) / 64 chunks x k for moments (no more than Nq ceil(max_list / 64)),
// nnz for videos.  Nothing is of size Nq x Nv and nothing waits for the host.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int SUB_LANES = 64;                       // list entries per chunk (= wave lanes)
constexpr int SUB_MAX_CLIPS = 64;                   // as the fused scorer (NMAX_FUSED)
constexpr int SUB_BUF = 1024;                       // per-wave key buffer of the moment level (>= k + 64)
constexpr int SUB_SORT = 512;                       // pool of the top-k kernel (>= k)

// the host's bound on the total number of chunks: sum ceil(len / 64) <= (nnz + 63 Nq) / 64, and <= Nq ceil(max_list / 64)
int64_t sub_chunk_bound(int64_t Nq, int64_t nnz, int64_t max_list)
{
    const int64_t a = (nnz + 63 * Nq) / SUB_LANES, b = Nq * ((max_list + SUB_LANES - 1) / SUB_LANES);
    return a < b ? a : b;
}

__device__ __forceinline__ void sub_segment(const int64_t *cand_off, int64_t nnz, int64_t q, int64_t &lo, int64_t &hi)
{
    lo = cand_off[q];
    hi = cand_off[q + 1];
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
}

// ---- chunk offsets (one workgroup of 1024): each thread sums a run of queries, then a scan of the 1024 run totals ----
__global__ __launch_bounds__(1024) void subset_plan_kernel(const int64_t *__restrict__ cand_off, int64_t Nq, int64_t nnz, int64_t max_list,
                                                           int64_t bound, int *__restrict__ chunk_off, int *__restrict__ bad)
{
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (Nq + 1023) / 1024, q0 = t * per, q1 = q0 + per < Nq ? q0 + per : Nq;
    int64_t sum = 0;
    bool wrong = false;
    for (int64_t q = q0; q < q1; ++q) {
        const int64_t a = cand_off[q], b = cand_off[q + 1];
        wrong |= a < 0 || b < a || b > nnz || b - a > max_list;
        int64_t lo, hi;
        sub_segment(cand_off, nnz, q, lo, hi);
        int64_t len = hi - lo;
        len = len > max_list ? max_list : len;
        sum += (len + SUB_LANES - 1) / SUB_LANES;
    }
    if (Nq > 0 && t == 0 && cand_off[0] != 0) wrong = true;
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                 // inclusive Hillis-Steele scan
        const int64_t x = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int64_t run = t > 0 ? part[t - 1] : 0;
    for (int64_t q = q0; q < q1; ++q) {
        chunk_off[q] = (int)(run < bound ? run : bound);
        int64_t lo, hi;
        sub_segment(cand_off, nnz, q, lo, hi);
        int64_t len = hi - lo;
        len = len > max_list ? max_list : len;
        run += (len + SUB_LANES - 1) / SUB_LANES;
    }
    if (t == 1023) chunk_off[Nq] = (int)(part[1023] < bound ? part[1023] : bound);
    if (wrong && bad) *bad = 1;
}

// ---- one wave per (query, chunk of 64 list entries) ----
__global__ __launch_bounds__(64) void subset_scan_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                         const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                         int Nv, int D, float eps, int64_t id_base, int64_t vid_base,
                                                         const int64_t *__restrict__ cand_off, const int32_t *__restrict__ cand_vid,
                                                         int64_t nnz, int64_t max_list, const int *__restrict__ chunk_off,
                                                         int level, int k, ScanRank rk, int ds_rows, int *__restrict__ bad,
                                                         unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    const int lane = threadIdx.x;
    const int chunk = (int)blockIdx.x;
    if (chunk >= chunk_off[Nq]) return;
    // the query whose chunk this is: the last q with chunk_off[q] <= chunk (chunk_off is non-decreasing)
    int64_t a = 0, b = Nq;
    while (b - a > 1) {
        const int64_t m = (a + b) >> 1;
        if (chunk_off[m] <= chunk) a = m; else b = m;
    }
    const int64_t q = a;
    int64_t lo, hi;
    sub_segment(cand_off, nnz, q, lo, hi);
    if (hi - lo > max_list) hi = lo + max_list;
    const int64_t e = lo + (int64_t)(chunk - chunk_off[q]) * SUB_LANES + lane;
    const bool listed = e < hi;
    int v = -1;
    if (listed) {
        const int gv = cand_vid[e];
        if (gv < 0 || (e > lo && cand_vid[e - 1] >= gv)) { if (bad) *bad = 1; }
        const int64_t lv = (int64_t)gv - vid_base;
        v = (gv >= 0 && lv >= 0 && lv < Nv) ? (int)lv : -1;
    }

    float *qs = ssm;                                      // [D]
    float *ds = ssm + ((D + 3) & ~3);                     // [ds_rows][64] clip distances, lane-minor
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ds + (size_t)ds_rows * 64);   // [SUB_BUF] (moments, k > 0)
    for (int i = lane; i < D; i += 64) qs[i] = Q[q * D + i];
    __syncthreads();

    int n = 0;
    int64_t mbase = 0;
    if (v >= 0) {
        const int c0 = clip_off[v];
        n = clip_off[v + 1] - c0;
        n = n > ds_rows ? ds_rows : n;
        mbase = id_base + mom_off[v];
        const bool vec4 = (D & 3) == 0 && (((uintptr_t)V) & 15) == 0;
        for (int c = 0; c < n; ++c) {
            const float *vr = V + (int64_t)(c0 + c) * D;
            float acc = 0.0f;
            if (D == SCAN_FAST_D && vec4) {                // the whole row requested at once, then the k-ascending chain
                float4 x[SCAN_FAST_D / 4];
#pragma unroll
                for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) x[k4] = *reinterpret_cast<const float4 *>(vr + 4 * k4);
#pragma unroll
                for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) {
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
            ds[c * 64 + lane] = __builtin_sqrtf(acc);
        }
    }
    unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r)
        rkey[r] = r < rk.num_rank ? make_key(rk.dist[r * Nq + q], (unsigned)rk.idx[r * Nq + q]) : 0ull;
    int nlt[SCAN_MAX_RANK] = {0, 0, 0, 0};

    if (level == VFR_SUBSET_VIDEOS) {
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
        if (listed) ws[e] = v >= 0 ? best : SCAN_KEY_MAX;
    } else {
        // the wave-uniform loop over the widest triangle of the chunk: a lane past its own video's end takes no part
        int nmax = n;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(nmax, o, 64); nmax = x > nmax ? x : nmax; }
        unsigned long long thr = SCAN_KEY_MAX;             // keys >= thr cannot be among the chunk's k smallest
        int cnt = 0;                                      // keys in buf (wave-uniform)
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        auto compact = [&]() {
            // buf[0..SUB_BUF) sorted, keep the k smallest
            wave_sort_keys(buf, cnt, SUB_BUF, lane);
            if (cnt >= k) { thr = buf[k - 1]; cnt = k; }
        };
        for (int s = 0; s < nmax; ++s) {
            float sum = 0.0f;
            for (int e2 = s; e2 < nmax; ++e2) {
                const bool live = e2 < n;
                const float de = live ? ds[e2 * 64 + lane] : 0.0f;
                sum = e2 == s ? de : sum + de;
                const float sc = sum / (float)(e2 - s + 1);
                const unsigned long long key = make_key(sc, (unsigned)(mbase + moment_index(n, s, e2)));
                if (live) scan_rank_count(rk.num_rank, rkey, key, nlt);
                if (k > 0) {
                    const bool take = live && key < thr;
                    const unsigned long long m = __ballot(take);
                    if (take) buf[cnt + __popcll(m & below)] = key;
                    cnt += __popcll(m);
                    if (cnt > SUB_BUF - 64) { __syncthreads(); compact(); }
                }
            }
        }
        if (k > 0) {
            __syncthreads();
            compact();
            unsigned long long *out = ws + (size_t)chunk * k;
            for (int i = lane; i < k; i += 64) out[i] = i < cnt ? buf[i] : SCAN_KEY_MAX;
        }
    }
    if (rk.num_rank > 0) {
#pragma unroll
        for (int r = 0; r < SCAN_MAX_RANK; ++r) {
            int x = nlt[r];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
            if (r < rk.num_rank && lane == 0 && x)
                atomicAdd(reinterpret_cast<unsigned long long *>(rk.count_lt + (int64_t)r * Nq + q), (unsigned long long)x);
        }
    }
}

// k-th smallest (1-based) of the 32-bit patterns x[0..n) (all threads of the block get it): four passes of 256 bins
template <typename LOAD>
__device__ unsigned sub_radix_kth32(LOAD load, int n, int kth, unsigned *hist, unsigned *shared_word)
{
    unsigned prefix = 0u, mask = 0u;
    int need = kth;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0u;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned x = load(i);
            if ((x & mask) == prefix) atomicAdd(hist + ((x >> shift) & 255u), 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned cum = 0u, b = 0u;
            for (; b < 255u; ++b) {
                if (cum + hist[b] >= (unsigned)need) break;
                cum += hist[b];
            }
            shared_word[0] = b;
            shared_word[1] = cum;
        }
        __syncthreads();
        prefix |= shared_word[0] << shift;
        mask |= 255u << shift;
        need -= (int)shared_word[1];
        __syncthreads();
    }
    return prefix;
}

// ---- per query: the k smallest keys of its segment of ws, sorted; (+inf, -1) past the real keys ----
__global__ __launch_bounds__(256) void subset_topk_kernel(const unsigned long long *__restrict__ ws, const int64_t *__restrict__ cand_off,
                                                          int64_t nnz, int64_t max_list, const int *__restrict__ chunk_off, int level,
                                                          int k, float *__restrict__ out_dist, int64_t *__restrict__ out_idx)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sw[2];
    __shared__ unsigned long long pool[SUB_SORT];
    __shared__ int npool;
    __shared__ int bsum[4];
    const int64_t q = blockIdx.x;
    const unsigned long long *row;
    int len;
    if (level == VFR_SUBSET_VIDEOS) {
        int64_t lo, hi;
        sub_segment(cand_off, nnz, q, lo, hi);
        const int64_t cap = (int64_t)(chunk_off[q + 1] - chunk_off[q]) * SUB_LANES;   // entries the scan reached
        const int64_t n = hi - lo < cap ? hi - lo : cap;
        row = ws + lo;
        len = (int)n;
    } else {
        row = ws + (size_t)chunk_off[q] * k;
        len = (chunk_off[q + 1] - chunk_off[q]) * k;
    }
    // threshold = the k-th smallest entry (KEY_MAX padding included; real keys of a valid list are distinct: ids are)
    unsigned long long thr = SCAN_KEY_MAX;
    if (len > k) {
        const unsigned hi = sub_radix_kth32([&](int i) { return (unsigned)(row[i] >> 32); }, len, k, hist, sw);
        int below = 0;
        for (int i = threadIdx.x; i < len; i += 256) below += (unsigned)(row[i] >> 32) < hi ? 1 : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) below += __shfl_xor(below, o, 64);
        if ((threadIdx.x & 63) == 0) bsum[threadIdx.x >> 6] = below;
        __syncthreads();
        below = bsum[0] + bsum[1] + bsum[2] + bsum[3];
        const unsigned lo = sub_radix_kth32([&](int i) { const unsigned long long x = row[i]; return (unsigned)(x >> 32) == hi ? (unsigned)x : 0xFFFFFFFFu; },
                                            len, k - below, hist, sw);
        thr = ((unsigned long long)hi << 32) | lo;
    }
    if (threadIdx.x == 0) npool = 0;
    for (int i = threadIdx.x; i < SUB_SORT; i += 256) pool[i] = SCAN_KEY_MAX;
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += 256) {
        const unsigned long long x = row[i];
        if (x < SCAN_KEY_EMPTY && x <= thr) { const int s = atomicAdd(&npool, 1); if (s < SUB_SORT) pool[s] = x; }
    }
    __syncthreads();
    for (int size = 2; size <= SUB_SORT; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < SUB_SORT; i += 256) {
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

struct SubWs { int *chunk_off; unsigned long long *keys; size_t total; };
SubWs carve_subset(void *base, int64_t Nq, int64_t nnz, int64_t max_list, int k, int level)
{
    SubWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes, 256); return p; };
    w.chunk_off = reinterpret_cast<int *>(take((size_t)(Nq + 1) * 4));
    const size_t nkeys = level == VFR_SUBSET_VIDEOS ? (size_t)nnz : (size_t)sub_chunk_bound(Nq, nnz, max_list) * (size_t)k;
    w.keys = reinterpret_cast<unsigned long long *>(take(nkeys * 8));
    w.total = off;
    return w;
}

}  // namespace
}  // namespace vfr

extern "C" {

size_t vfr_score_subset_workspace_bytes(int64_t Nq, int64_t nnz, int64_t max_list, int k, int level)
{
    if (Nq < 0 || nnz < 0 || max_list < 0 || k < 0 || k > vfr::SCAN_MAX_K || (level != VFR_SUBSET_MOMENTS && level != VFR_SUBSET_VIDEOS))
        return 0;
    return vfr::carve_subset(nullptr, Nq, nnz, max_list, k, level).total;
}

int vfr_score_subset_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets,
                         int Nv, int total_clips, int min_clips, int max_clips, int D, float eps, int64_t id_base,
                         int64_t vid_base, const int64_t *cand_off, const int32_t *cand_vid, int64_t nnz, int64_t max_list,
                         int level, int k, float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist,
                         const int64_t *rank_idx, int64_t *count_lt, int *bad, void *workspace, size_t workspace_bytes,
                         vfr_stream_t stream)
{
    (void)min_clips;
    VFR_REQUIRE(level == VFR_SUBSET_MOMENTS || level == VFR_SUBSET_VIDEOS, VFR_EINVAL,
                "vfr_score_subset_f32: level %d (0 = moments, 1 = videos)", level);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::SUB_MAX_CLIPS && id_base >= 0 && vid_base >= 0 && nnz >= 0 && max_list >= 0, VFR_EINVAL,
                "vfr_score_subset_f32: bad shape (k <= 448, max_clips <= 64, id_base, vid_base, nnz, max_list >= 0)");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_subset_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(Nq * (int64_t)k <= 0x7FFFFFFF && nnz <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_subset_f32: Nq * k and nnz must stay below 2^31");
    VFR_REQUIRE(vfr::sub_chunk_bound(Nq, nnz, max_list) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_subset_f32: too many list chunks");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_subset_f32: num_rank %d (0 .. 4)", num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_subset_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_subset_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nq == 0 || cand_off, VFR_EINVAL, "vfr_score_subset_f32: cand_off is null");
    VFR_REQUIRE(nnz == 0 || cand_vid, VFR_EINVAL, "vfr_score_subset_f32: cand_vid is null with nnz > 0");
    VFR_REQUIRE(Nq == 0 || Nv == 0 || (Q && V && clip_offsets && moment_offsets), VFR_EINVAL, "vfr_score_subset_f32: null input");
    const int rows = max_clips < 1 ? 1 : max_clips;
    const size_t lds = ((size_t)((D + 3) & ~3) + (size_t)rows * 64) * 4 +
                       (level == VFR_SUBSET_MOMENTS && k > 0 ? (size_t)vfr::SUB_BUF * 8 : 0);
    VFR_REQUIRE(lds <= 64 * 1024, VFR_EINVAL, "vfr_score_subset_f32: D = %d too wide for the subset kernel", D);
    const size_t need = vfr_score_subset_workspace_bytes(Nq, nnz, max_list, k, level);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_subset_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    if (Nq == 0 || (k == 0 && num_rank == 0)) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    vfr::SubWs w = vfr::carve_subset(workspace, Nq, nnz, max_list, k, level);
    const int64_t bound = vfr::sub_chunk_bound(Nq, nnz, max_list);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PREP, st);
        hipLaunchKernelGGL(vfr::subset_plan_kernel, dim3(1), dim3(1024), 0, st, cand_off, Nq, nnz, max_list, bound, w.chunk_off, bad);
        VFR_CHECK_LAUNCH("subset_plan_kernel");
    }
    if (bound > 0 && Nv > 0) {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        hipLaunchKernelGGL(vfr::subset_scan_kernel, dim3((unsigned)bound), dim3(64), lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D,
                           eps, id_base, vid_base, cand_off, cand_vid, nnz, max_list, w.chunk_off, level, k, rk, rows, bad, w.keys);
        VFR_CHECK_LAUNCH("subset_scan_kernel");
    }
    if (k > 0) {
        vfr::ProfScope prof(vfr::SITE_TOPK_MERGE, st);
        if (Nv == 0) {     // nothing scored: every row is padding (the scan did not write the keys)
            const vfr::FillJob jobs[2] = {{out_dist, nullptr, (size_t)Nq * k * 4, 0x7F800000u}, {out_idx, nullptr, (size_t)Nq * k * 8, 0xFFFFFFFFu}};
            return vfr::fill_regions(jobs, 2, st);
        }
        hipLaunchKernelGGL(vfr::subset_topk_kernel, dim3((unsigned)Nq), dim3(256), 0, st, w.keys, cand_off, nnz, max_list, w.chunk_off, level, k,
                           out_dist, out_idx);
        VFR_CHECK_LAUNCH("subset_topk_kernel");
    }
    return VFR_OK;
}

}  // extern "C"
