// Prior-aware retrieval: vfr_score_prior_f32 and vfr_score_prior_own_f32 (include/vfr.h).
//
// A moment table T gives every (clip count n, local moment j in utils.generate_moments order) one fp32 entry: a finite bias >= 0 or
// +inf = excluded.  table_off [max_clips + 2] = prefix sums of n (n + 1) / 2, table [table_off[max_clips + 1]].  The ranking key
// changes at the MOMENT: score(q, v, j) is the canonical chain of vfr_score_moments_f32 (k-ascending fp32 fma chain of
// ((v - q) + eps)^2, IEEE sqrt, sequential fp32 sum s -> e, one IEEE division); its clip distances come from scan_common.h, not
// from the headers of score.o, so the code objects of score.o do not change, and
//     g(q, v, j) = fl(score(q, v, j) + T[n_v][j])                       (__fadd_rn: one rounded addition, contracted with nothing)
// is what the key carries: key = (bits of g << 32) | (id_base + moment_offsets[v] + j).  A moment is a candidate iff g < +inf; an
// entry that is NaN or < 0 sets *bad and excludes its moment.  A table of zeros gives the bits of vfr_score_topk_f32 /
// vfr_score_video_topk_f32 (fl(x + 0) = x for x >= 0).
// Kernels (a translation unit of its own), each in two forms: FAST = D == 100 with 16-byte aligned Q and V (the query row in LDS, the
// chain unrolled over 16-byte loads, two clips = two independent chains at a time), and any D (the query row read from global at a
// wave-uniform address):
//   prior_own_kernel   one wave per query: lane = clip of own[q] (its distance into LDS), then lane = start clip with a running sum
//                      over the end clip; the row layout of vfr_score_own_f32 (excluded moments and the tail +inf).
//   prior_scan_kernel  one wave per (query, chunk of the video axis), lane = video.  Per block of 64 videos each lane writes the
//                      distances of its clips to its LDS column, then walks its triangle by running sums and IEEE division and adds
//                      the entry of ITS table row (table + table_off[n_lane]: a gather, the lanes' videos differ in length; the
//                      table is at most 183 KB and stays in L2).  g < +inf is tested before anything is done with the key.  Rank
//                      counts: per-lane counters, one atomic per wave and rank.  The chunk's k smallest candidate keys (moments:
//                      every candidate; videos: the lane's best candidate over its WHOLE triangle, none = the video is neither listed
//                      nor counted) are collected under a running threshold into an LDS list of 128 / 256 / 512 keys that is sorted and
//                      cut back to k when it fills; the chunk's list goes to ws[chunk][query][0..k).
//   The per-chunk lists are merged by vfr_topk_merge_keys (one launch), which also pads with (+inf, -1).
// The chunk plan, the list's capacity and sort, the rank-key counters and the clip-distance helpers are those of scan_common.h.
// LDS of a scan wave = 416 (FAST: the query row) + 256 max(max_clips, 1) + 8 slots(k) bytes <= 416 + 16 384 + 4 096.
// Workspace: chunks x Nq x k keys, chunks <= SCAN_MAX_CHUNKS whatever Nv is.  Nothing is of size Nq x Nv, nothing waits for the host.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int PRI_MAX_CLIPS = 64;                    // as the fused scorer
struct PriTable {
    const int32_t *off;          // [max_clips + 2]
    const float *val;            // [len]
    int len;                     // max_clips (max_clips + 1) (max_clips + 2) / 6: what the contract says `val` holds
    int max_clips;
    int *bad;                    // nullable
};

// the table row of an n-clip video (n <= max_clips, so table_off[n] exists); a row that would leave the table is refused: the video
// then has no candidate at all
__device__ __forceinline__ const float *pri_row(const PriTable &t, int n, bool &wrong)
{
    if (n <= 0) return t.val;
    const int base = t.off[n];
    if (base < 0 || base > t.len - n * (n + 1) / 2) {
        wrong = true;
        return nullptr;
    }
    return t.val + base;
}

// g = fl(score + entry); an entry that is NaN or < 0 excludes its moment (+inf) and is reported
__device__ __forceinline__ float pri_biased(float sc, float b, bool &wrong)
{
    if (!(b >= 0.0f)) {
        wrong = true;
        return __builtin_inff();
    }
    return __fadd_rn(sc, b);
}

// ---- each query against ONE video own[q]: one wave per query; lane = clip, then lane = start clip ----
template <bool FAST>
__global__ __launch_bounds__(64) void prior_own_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                       const int32_t *__restrict__ clip_off, const int32_t *__restrict__ own, int Nv,
                                                       int D, float eps, int Mmax, const PriTable tb, float *__restrict__ scores)
{
    __shared__ __attribute__((aligned(16))) float qs[FAST ? SCAN_FAST_D + 4 : 4];
    __shared__ float ds[PRI_MAX_CLIPS];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    float *out = scores + q * Mmax;
    const int v = own[q];
    int64_t c0 = 0;
    int n = 0;
    if (v >= 0 && v < Nv) {
        c0 = clip_off[v];
        n = clip_off[v + 1] - (int)c0;
        n = n > tb.max_clips ? tb.max_clips : (n < 0 ? 0 : n);
    }
    bool wrong = false;
    const float *row = pri_row(tb, n, wrong);
    if (row == nullptr) n = 0;
    const int M = n * (n + 1) / 2;                             // <= Mmax: Mmax >= max_clips (max_clips + 1) / 2
    for (int m = M + lane; m < Mmax; m += 64) out[m] = __builtin_inff();      // slots past this video's moments
    const float *qr = query_row<FAST>(Q, q, D, qs, lane);
    if (lane < n) clip_dists<FAST>(V, c0 + lane, 1, qr, D, eps, ds + lane, 1);
    __syncthreads();
    if (lane < n) {
        float sum = 0.0f;
        for (int e = lane; e < n; ++e) {
            const float de = ds[e];
            sum = e == lane ? de : sum + de;
            const int j = moment_index(n, lane, e);
            out[j] = pri_biased(sum / (float)(e - lane + 1), row[j], wrong);
        }
    }
    if (tb.bad && wrong) *tb.bad = 1;
}

// ---- one wave per (query, chunk of the video axis), lane = video ----
template <bool FAST>
__global__ __launch_bounds__(64) void prior_scan_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                        const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                        int Nv, int D, float eps, int64_t id_base, int level, int k, int cap,
                                                        ScanRank rk, int ds_rows, int chunks, int64_t per, const PriTable tb,
                                                        unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float *qs = ssm;                                                                        // [104] (fast path)
    float *ds = ssm + (FAST ? SCAN_FAST_D + 4 : 0);                                          // [ds_rows][64] clip distances, lane-minor
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ds + (size_t)ds_rows * 64);   // [cap]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - q * chunks);
    const float *qr = query_row<FAST>(Q, q, D, qs, lane);

    unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r)
        rkey[r] = r < rk.num_rank ? make_key(rk.dist[r * Nq + q], (unsigned)rk.idx[r * Nq + q]) : 0ull;
    int nlt[SCAN_MAX_RANK] = {0, 0, 0, 0};

    const int64_t v0 = (int64_t)ch * per;
    const int64_t v1 = v0 + per < Nv ? v0 + per : Nv;
    const float inf = __builtin_inff();
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
    bool wrong = false;

    for (int64_t vb = v0; vb < v1; vb += 64) {
        const int64_t l = vb + lane;
        int n = 0;
        int64_t mbase = 0;
        const float *row = tb.val;
        if (l < v1) {
            const int c0 = clip_off[l];
            n = clip_off[l + 1] - c0;
            n = n > tb.max_clips ? tb.max_clips : (n < 0 ? 0 : n);   // max_clips <= ds_rows: the lane's LDS column and table row exist
            row = pri_row(tb, n, wrong);
            if (row == nullptr) n = 0;
            mbase = id_base + mom_off[l];
            clip_dists<FAST>(V, (int64_t)c0, n, qr, D, eps, ds + lane, 64);                  // the lane's own column
        }
        if (level == VFR_PRIOR_VIDEOS) {
            unsigned long long best = SCAN_KEY_EMPTY;
            for (int s = 0; s < n; ++s) {
                float sum = 0.0f;
                const int jrow = n + (s * (2 * n - s - 1)) / 2 - s - 1;               // moment_index(n, s, e) = jrow + e for e > s
                for (int e2 = s; e2 < n; ++e2) {
                    const float de = ds[e2 * 64 + lane];
                    sum = e2 == s ? de : sum + de;
                    const int j = e2 == s ? s : jrow + e2;
                    const float g = pri_biased(sum / (float)(e2 - s + 1), row[j], wrong);
                    if (g < inf) {
                        const unsigned long long key = make_key(g, (unsigned)(mbase + j));
                        best = key < best ? key : best;
                    }
                }
            }
            const bool has = best != SCAN_KEY_EMPTY;            // a video without a candidate is neither counted nor listed
            if (has) scan_rank_count(rk.num_rank, rkey, best, nlt);
            if (k > 0) append(has && best < thr, best);
        } else {
            // the wave-uniform loop over the widest triangle of the block: a lane past its own video's end takes no part
            int nmax = n;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(nmax, o, 64); nmax = x > nmax ? x : nmax; }
            for (int s = 0; s < nmax; ++s) {
                float sum = 0.0f;
                const int jrow = n + (s * (2 * n - s - 1)) / 2 - s - 1;
                for (int e2 = s; e2 < nmax; ++e2) {
                    const bool live = e2 < n;
                    const float de = live ? ds[e2 * 64 + lane] : 0.0f;
                    sum = e2 == s ? de : sum + de;
                    const int j = e2 == s ? s : jrow + e2;
                    const float g = live ? pri_biased(sum / (float)(e2 - s + 1), row[j], wrong) : inf;
                    const bool cand = g < inf;                 // excluded moments stop here: no key, no count, no insert
                    const unsigned long long key = make_key(g, (unsigned)(mbase + j));
                    if (cand) scan_rank_count(rk.num_rank, rkey, key, nlt);
                    if (k > 0) append(cand && key < thr, key);
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
    if (tb.bad && wrong) *tb.bad = 1;
}

PriTable pri_table(const int32_t *table_off, const float *table, int max_clips, int *bad)
{
    return PriTable{table_off, table, max_clips * (max_clips + 1) * (max_clips + 2) / 6, max_clips, bad};
}

}  // namespace
}  // namespace vfr

extern "C" {

int vfr_score_prior_own_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int32_t *own, int Nv,
                            int max_clips, int D, float eps, int Mmax, const int32_t *table_off, const float *table, float *scores,
                            int *bad, vfr_stream_t stream)
{
    VFR_REQUIRE(Nq >= 0 && Nq <= 0x7FFFFFFF && Nv >= 0 && Mmax >= 0 && D > 0 && max_clips >= 0 && max_clips <= vfr::PRI_MAX_CLIPS,
                VFR_EINVAL, "vfr_score_prior_own_f32: bad shape (max_clips <= 64, Nq < 2^31, D >= 1, sizes >= 0)");
    VFR_REQUIRE(Mmax >= max_clips * (max_clips + 1) / 2, VFR_EINVAL, "vfr_score_prior_own_f32: max_clips = %d needs Mmax >= %d, got %d",
                max_clips, max_clips * (max_clips + 1) / 2, Mmax);
    VFR_REQUIRE(Nq == 0 || (Q && own && (scores || Mmax == 0) && (clip_offsets || Nv == 0)), VFR_EINVAL,
                "vfr_score_prior_own_f32: null Q / own / scores / clip_offsets");
    VFR_REQUIRE(Nq == 0 || Nv == 0 || max_clips == 0 || (V && table_off && table), VFR_EINVAL,
                "vfr_score_prior_own_f32: null V / table_off / table");
    if (Nq == 0 || Mmax == 0) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, st);
    const vfr::PriTable tb = vfr::pri_table(table_off, table, max_clips, bad);
    const dim3 grid((unsigned)Nq), block(64);
    if (vfr::rows_fast(Q, V, D))
        hipLaunchKernelGGL((vfr::prior_own_kernel<true>), grid, block, 0, st, Q, Nq, V, clip_offsets, own, Nv, D, eps, Mmax, tb, scores);
    else
        hipLaunchKernelGGL((vfr::prior_own_kernel<false>), grid, block, 0, st, Q, Nq, V, clip_offsets, own, Nv, D, eps, Mmax, tb, scores);
    VFR_CHECK_LAUNCH("prior_own_kernel");
    return VFR_OK;
}

size_t vfr_score_prior_workspace_bytes(int64_t Nq, int Nv, int k)
{
    if (Nq < 0 || Nv < 0 || k < 0 || k > vfr::SCAN_MAX_K || Nq * (int64_t)(k > 0 ? k : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(Nq, Nv, vfr::SCAN_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Nq * (size_t)k * 8 + 256, 256);
}

int vfr_score_prior_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
                        int total_clips, int min_clips, int max_clips, int D, float eps, int64_t id_base, int level, int k,
                        float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx,
                        int64_t *count_lt, const int32_t *table_off, const float *table, int *bad, void *workspace,
                        size_t workspace_bytes, vfr_stream_t stream)
{
    (void)min_clips;
    VFR_REQUIRE(level == VFR_PRIOR_MOMENTS || level == VFR_PRIOR_VIDEOS, VFR_EINVAL,
                "vfr_score_prior_f32: level %d (0 = moments, 1 = videos)", level);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::PRI_MAX_CLIPS && id_base >= 0, VFR_EINVAL,
                "vfr_score_prior_f32: bad shape (k <= 448, max_clips <= 64, D >= 1, sizes, id_base >= 0)");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_prior_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(Nq * (int64_t)(k > 0 ? k : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_prior_f32: Nq * k must stay below 2^31");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_prior_f32: num_rank %d (0 .. 4)", num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_prior_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || Nq == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_prior_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nq == 0 || Q, VFR_EINVAL, "vfr_score_prior_f32: Q is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets && (V || total_clips == 0)), VFR_EINVAL,
                "vfr_score_prior_f32: null clip bank (V, clip_offsets, moment_offsets)");
    VFR_REQUIRE(Nv == 0 || max_clips == 0 || (table_off && table), VFR_EINVAL, "vfr_score_prior_f32: null table_off / table");
    const vfr::ScanPlan plan = vfr::scan_plan(Nq, Nv, vfr::SCAN_TARGET_WAVES);
    VFR_REQUIRE(Nq * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_prior_f32: too many (query, chunk) waves");
    const size_t need = vfr_score_prior_workspace_bytes(Nq, Nv, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_prior_f32: workspace %zu < %zu bytes", workspace_bytes,
                need);
    if (Nq == 0 || (k == 0 && (num_rank == 0 || Nv == 0))) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        const bool fast = vfr::rows_fast(Q, V, D);
        const int rows = max_clips < 1 ? 1 : max_clips;
        const int cap = vfr::scan_cap(k);
        const size_t lds = (fast ? (size_t)(vfr::SCAN_FAST_D + 4) * 4 : 0) + (size_t)rows * 64 * 4 + (size_t)cap * 8;   // <= 416 + 16 K + 4 K
        const vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        const vfr::PriTable tb = vfr::pri_table(table_off, table, max_clips, bad);
        const dim3 grid((unsigned)(Nq * plan.chunks)), block(64);
        if (fast)
            hipLaunchKernelGGL((vfr::prior_scan_kernel<true>), grid, block, lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps,
                               id_base, level, k, cap, rk, rows, plan.chunks, plan.per, tb, keys);
        else
            hipLaunchKernelGGL((vfr::prior_scan_kernel<false>), grid, block, lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps,
                               id_base, level, k, cap, rk, rows, plan.chunks, plan.per, tb, keys);
        VFR_CHECK_LAUNCH("prior_scan_kernel");
    }
    if (k > 0)
        return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Nq, k, out_dist, out_idx, nullptr, stream);
    return VFR_OK;
}

}  // extern "C"
