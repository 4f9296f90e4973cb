// Windowed retrieval for long videos: vfr_score_window_f32 and vfr_score_window_span_keys_f32 (include/vfr.h).
//
// The candidate set of a window max_len = L (1 <= L <= 64): every moment (video v, start s, end e) with 0 <= s <= e < n_v and
// e - s + 1 <= L -- the sliding-window proposal set long-video corpora are searched over.  The score is the canonical chain of
// vfr_score_moments_f32 (k-ascending fp32 fma chain of ((v - q) + eps)^2, IEEE sqrt, sequential fp32 sum s -> e, one IEEE division);
// the id stays canonical: id_base + moment_offsets[v] + moment_index(n_v, s, e), so with L >= max_clips the keys are those of
// vfr_score_topk_f32 and every decoder of ids still works.  key = (score bits << 32) | id.
// Kernels (a translation unit of its own over scan_common.h):
//   window_scan_kernel  one wave per (query, chunk of the FLAT clip axis); chunk boundaries ignore video boundaries, a moment belongs
//                      to the chunk that holds its start clip.  Per tile of 64 consecutive flat clips from T0: lane l writes the
//                      distance of clip T0 + l to LDS, lanes l < L - 1 also that of clip T0 + 64 + l (the halo; both guarded by
//                      total_clips).  The lane finds the video of ITS start clip by an upper-bound search in clip_offsets (the
//                      offsets stay in L2), then a wave-uniform loop i = 0 .. L - 1 keeps the running sum over ds[l + i] (lane-
//                      consecutive addresses: conflict-free), divides, forms the key, counts it against the rank keys and appends it
//                      under the running threshold.  Two forms: FAST = D == 100 with 16-byte aligned Q and V (query row in LDS), and
//                      any D.  Nothing in it is sized by the length of a video.
//   window_span_keys_kernel  one lane per item (query row, corpus-global video, start, end): the key of that span -- the rank keys
//                      of ground-truth spans without an own-video row of n^2 entries.
// The per-chunk lists are merged by vfr_topk_merge_keys (one launch), which also pads with (+inf, -1).
// LDS of a scan wave = 416 (FAST: the query row) + 512 (two tiles of clip distances) + 8 slots(k) bytes <= 5 024.
// Workspace: chunks x Nq x k keys, chunks <= SCAN_MAX_CHUNKS whatever the bank holds.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int WIN_MAX_LEN = 64;                      // a lane's window: at most one tile ahead of its start clip
// what the CPU oracle can check.  The kernels keep no per-video storage; their positions inside a video (moment_index, jrow: products
// of about 2 n^2) are int32, which holds up to 32 767 clips -- a larger limit here needs them in int64 first
constexpr int WIN_MAX_CLIPS = 1024;

// the video that owns flat clip c (0 <= c < clip_off[Nv]): the last v with clip_off[v] <= c, so empty videos own nothing
__device__ __forceinline__ int win_video_of(const int32_t *__restrict__ clip_off, int Nv, int64_t c)
{
    int lo = 0, hi = Nv;                                       // clip_off[lo] <= c < clip_off[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (clip_off[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- one wave per (query, chunk of the flat clip axis), lane = start clip ----
template <bool FAST>
__global__ __launch_bounds__(64) void window_scan_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                         const int32_t *__restrict__ clip_off, const int64_t *__restrict__ mom_off,
                                                         int Nv, int total_clips, int D, float eps, int64_t id_base, int L, int k,
                                                         int cap, ScanRank rk, int chunks, int64_t per,
                                                         unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float *qs = ssm;                                                                        // [104] (fast path)
    float *ds = ssm + (FAST ? SCAN_FAST_D + 4 : 0);                                          // [128] clip distances: the tile, then its halo
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ds + 128);             // [cap]
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - q * chunks);
    const float *qr = query_row<FAST>(Q, q, D, qs, lane);

    unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r)
        rkey[r] = r < rk.num_rank ? make_key(rk.dist[r * Nq + q], (unsigned)rk.idx[r * Nq + q]) : 0ull;
    int nlt[SCAN_MAX_RANK] = {0, 0, 0, 0};

    const int64_t c0 = (int64_t)ch * per;
    const int64_t c1 = c0 + per < total_clips ? c0 + per : total_clips;
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
    auto dist_of = [&](int64_t c) {
        const float *vr = V + c * D;
        float d;
        if constexpr (FAST) clip_dist_fast<1>(vr, qr, eps, &d);
        else d = clip_dist_any(vr, qr, D, eps);
        return d;
    };

    for (int64_t T0 = c0; T0 < c1; T0 += 64) {
        const int64_t c = T0 + lane;
        __syncthreads();                                       // the previous tile's reads of ds are done
        ds[lane] = c < total_clips ? dist_of(c) : 0.0f;
        if (lane < L - 1) ds[64 + lane] = c + 64 < total_clips ? dist_of(c + 64) : 0.0f;   // read at ds[l + i] <= ds[62 + L] only
        __syncthreads();
        int s = 0, m = 0, n = 0;                               // local start clip, windows that start here, clips of the video
        int64_t mbase = 0;
        if (c < c1) {
            const int v = win_video_of(clip_off, Nv, c);
            const int o = clip_off[v];
            n = clip_off[v + 1] - o;
            s = (int)c - o;
            m = n - s < L ? n - s : L;                         // ends s .. min(n, s + L) - 1
            m = s < 0 || m < 0 ? 0 : m;                        // (offsets that are no prefix sums: the lane takes no part)
            mbase = id_base + mom_off[v];
        }
        // the wave-uniform loop over the longest window of the tile: a lane past its own video's end takes no part
        int mmax = m;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(mmax, o, 64); mmax = x > mmax ? x : mmax; }
        const int jrow = n + (s * (2 * n - s - 1)) / 2 - s - 1;                       // moment_index(n, s, e) = jrow + e for e > s
        float sum = 0.0f;
        for (int i = 0; i < mmax; ++i) {
            const bool live = i < m;
            const float de = ds[lane + i];
            sum = i == 0 ? de : sum + de;
            const int j = i == 0 ? s : jrow + s + i;
            const unsigned long long key = make_key(sum / (float)(i + 1), (unsigned)(mbase + j));
            if (live) scan_rank_count(rk.num_rank, rkey, key, nlt);
            if (k > 0) append(live && key < thr, key);
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

// ---- the key of named (query, video, span) items: one lane per item ----
__global__ __launch_bounds__(64) void window_span_keys_kernel(const float *__restrict__ Q, int64_t Nq, const float *__restrict__ V,
                                                              const int32_t *__restrict__ clip_off,
                                                              const int64_t *__restrict__ mom_off, int Nv, int D, float eps,
                                                              int64_t id_base, int64_t vid_base, const int32_t *__restrict__ items,
                                                              int64_t Np, unsigned long long *__restrict__ out_keys,
                                                              int *__restrict__ bad)
{
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= Np) return;
    const int q = items[4 * p], gv = items[4 * p + 1], s = items[4 * p + 2], e = items[4 * p + 3];
    bool wrong = q < 0 || q >= Nq || s < 0 || e < s || (int64_t)e - s + 1 > WIN_MAX_LEN;
    const int64_t l = (int64_t)gv - vid_base;
    const bool owned = l >= 0 && l < Nv;
    int o = 0, n = 0;
    if (owned) {
        o = clip_off[l];
        n = clip_off[l + 1] - o;
        wrong |= e >= n;
    }
    if (wrong) {
        if (bad) *bad = 1;
        return;
    }
    if (!owned) return;                                        // another shard's video: untouched
    const float *qr = Q + (int64_t)q * D;
    float sum = 0.0f;
    for (int c = s; c <= e; ++c) {                             // 0 <= s <= e < n: rows o + s .. o + e are this video's
        const float d = clip_dist_any(V + (int64_t)(o + c) * D, qr, D, eps);
        sum = c == s ? d : sum + d;
    }
    out_keys[p] = make_key(sum / (float)(e - s + 1), (unsigned)(id_base + mom_off[l] + moment_index(n, s, e)));
}

}  // namespace
}  // namespace vfr

extern "C" {

size_t vfr_score_window_workspace_bytes(int64_t Nq, int total_clips, int k)
{
    if (Nq < 0 || total_clips < 0 || k < 0 || k > vfr::SCAN_MAX_K || Nq * (int64_t)(k > 0 ? k : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(Nq, total_clips, vfr::SCAN_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Nq * (size_t)k * 8 + 256, 256);
}

int vfr_score_window_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
                         int total_clips, int max_clips, int D, float eps, int64_t id_base, int max_len, int k, float *out_dist,
                         int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt,
                         void *workspace, size_t workspace_bytes, vfr_stream_t stream)
{
    VFR_REQUIRE(max_len >= 1 && max_len <= vfr::WIN_MAX_LEN, VFR_EINVAL, "vfr_score_window_f32: max_len %d (1 .. 64)", max_len);
    VFR_REQUIRE(Nq >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::WIN_MAX_CLIPS && id_base >= 0, VFR_EINVAL,
                "vfr_score_window_f32: bad shape (k <= 448, max_clips <= 1024, D >= 1, sizes, id_base >= 0)");
    VFR_REQUIRE(id_base + (int64_t)total_clips * (max_clips + 1) / 2 <= (int64_t(1) << 32), VFR_EINVAL,
                "vfr_score_window_f32: id_base + moments must stay below 2^32");
    VFR_REQUIRE(Nq * (int64_t)(k > 0 ? k : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_window_f32: Nq * k must stay below 2^31");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_window_f32: num_rank %d (0 .. 4)", num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_window_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || Nq == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_window_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nq == 0 || Q, VFR_EINVAL, "vfr_score_window_f32: Q is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets && (V || total_clips == 0)), VFR_EINVAL,
                "vfr_score_window_f32: null clip bank (V, clip_offsets, moment_offsets)");
    const int clips = Nv == 0 ? 0 : total_clips;               // a bank without videos has no clip to start a window at
    const vfr::ScanPlan plan = vfr::scan_plan(Nq, clips, vfr::SCAN_TARGET_WAVES);
    VFR_REQUIRE(Nq * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_window_f32: too many (query, chunk) waves");
    const size_t need = vfr_score_window_workspace_bytes(Nq, total_clips, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EINVAL, "vfr_score_window_f32: workspace %zu < %zu bytes", workspace_bytes,
                need);
    if (Nq == 0 || (k == 0 && (num_rank == 0 || clips == 0))) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        const bool fast = vfr::rows_fast(Q, V, D);
        const int cap = vfr::scan_cap(k);
        const size_t lds = (fast ? (size_t)(vfr::SCAN_FAST_D + 4) * 4 : 0) + 128 * 4 + (size_t)cap * 8;   // <= 416 + 512 + 4 K
        const vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        const dim3 grid((unsigned)(Nq * plan.chunks)), block(64);
        if (fast)
            hipLaunchKernelGGL((vfr::window_scan_kernel<true>), grid, block, lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv,
                               clips, D, eps, id_base, max_len, k, cap, rk, plan.chunks, plan.per, keys);
        else
            hipLaunchKernelGGL((vfr::window_scan_kernel<false>), grid, block, lds, st, Q, Nq, V, clip_offsets, moment_offsets, Nv,
                               clips, D, eps, id_base, max_len, k, cap, rk, plan.chunks, plan.per, keys);
        VFR_CHECK_LAUNCH("window_scan_kernel");
    }
    if (k > 0)
        return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Nq, k, out_dist, out_idx, nullptr, stream);
    return VFR_OK;
}

int vfr_score_window_span_keys_f32(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                                   const int64_t *moment_offsets, int Nv, int total_clips, int D, float eps, int64_t id_base,
                                   int64_t vid_base, const int32_t *items, int64_t Np, int64_t *out_keys, int *bad,
                                   vfr_stream_t stream)
{
    VFR_REQUIRE(Nq >= 0 && Nq <= 0x7FFFFFFF && Nv >= 0 && total_clips >= 0 && D > 0 && Np >= 0 && id_base >= 0 && vid_base >= 0,
                VFR_EINVAL, "vfr_score_window_span_keys_f32: bad shape (Nq < 2^31, D >= 1, sizes, id_base >= 0, vid_base >= 0)");
    VFR_REQUIRE(vid_base + Nv < (int64_t(1) << 32), VFR_EINVAL, "vfr_score_window_span_keys_f32: vid_base + Nv must stay below 2^32");
    VFR_REQUIRE(Np <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_window_span_keys_f32: Np must stay below 2^31");
    VFR_REQUIRE(Np == 0 || (items && out_keys), VFR_EINVAL, "vfr_score_window_span_keys_f32: items / out_keys is null");
    VFR_REQUIRE(Np == 0 || Nq == 0 || Q, VFR_EINVAL, "vfr_score_window_span_keys_f32: Q is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && moment_offsets && (V || total_clips == 0)), VFR_EINVAL,
                "vfr_score_window_span_keys_f32: null clip bank (V, clip_offsets, moment_offsets)");
    if (Np == 0) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    vfr::ProfScope prof(vfr::SITE_SCORE_OWN, st);
    const dim3 grid((unsigned)vfr::cdiv(Np, 64)), block(64);
    hipLaunchKernelGGL(vfr::window_span_keys_kernel, grid, block, 0, st, Q, Nq, V, clip_offsets, moment_offsets, Nv, D, eps, id_base,
                       vid_base, items, Np, reinterpret_cast<unsigned long long *>(out_keys), bad);
    VFR_CHECK_LAUNCH("window_span_keys_kernel");
    return VFR_OK;
}

}  // extern "C"
