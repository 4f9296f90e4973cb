// The steps that the retrieval variants (subset.hip, sentences.hip, mining.hip, fusion.hip, prior.hip) have in common, once.
//
// Each variant is a translation unit of its own that scans a bank with one wave per (query, chunk of the scanned axis), counts the keys
// before up to four rank keys and keeps the chunk's k smallest keys in an LDS list; the per-chunk lists are merged by
// vfr_topk_merge_keys.  What is byte-for-byte the same in more than one of them lives here: the chunk plan, the list capacity, the key
// constants, the one-wave bitonic sort of a key list, the rank-key argument and its counters, and the canonical clip-distance chain at
// D = 100.  Anything that differs between the variants (their triangle walks, fus_dist, sen_dist_fast, the subset's chunk offsets)
// stays in its file.  So does the append under the running threshold (ballot, compacted store, wave_sort_keys and cut back to k above
// cap - 64 slots): the same text in mining.hip, fusion.hip and prior.hip, but as a struct or as a function taking thr / cnt by
// reference it changed the register allocation of the mining and fusion kernels.  Only those five files include this header:
// score.o and its headers restate nothing from here, so their code objects do not depend on it.
#pragma once
#include "vfr_common.h"
#include "vfr_math.h"

namespace vfr {

constexpr int SCAN_MAX_K = 448;                      // longest list: scan_cap(SCAN_MAX_K) - 64 slots
constexpr int SCAN_MAX_RANK = 4;
constexpr int SCAN_FAST_D = 100;
constexpr int SCAN_MAX_CHUNKS = 256;
constexpr int SCAN_TARGET_WAVES = 4096;              // of the lane = video scans (mining, fusion, prior)
constexpr unsigned long long SCAN_KEY_MAX = ~0ull;
constexpr unsigned long long SCAN_KEY_EMPTY = 0x7F800000FFFFFFFFull;   // VFR_KEY_EMPTY: an unused slot of a list; no candidate reaches it

// ---- host side ----

// slots of a scan wave's LDS list: a power of two >= k + 64 (a wave appends up to 64 keys before it looks at the fill)
inline int scan_cap(int k) { return k == 0 ? 0 : k <= 64 ? 128 : k <= 192 ? 256 : 512; }

struct ScanPlan { int chunks; int64_t per; int bound; };
// The scanned axis of n entries is cut into chunks of `per` entries (a multiple of 64): chunks = min(ceil(target_waves / waves),
// blocks of 64 entries, SCAN_MAX_CHUNKS), evened out, where `waves` is what one pass over the axis launches without chunks (queries,
// items, probe tiles).  `bound` (what the workspace is sized by) does not look at n beyond "fewer blocks than that".
inline ScanPlan scan_plan(int64_t waves, int64_t n, int target_waves)
{
    ScanPlan p{};
    const int64_t blocks = cdiv(n, 64);
    int64_t want = cdiv(target_waves, waves > 0 ? waves : 1);
    want = want > SCAN_MAX_CHUNKS ? SCAN_MAX_CHUNKS : want;
    int64_t c = want < blocks ? want : blocks;
    c = c < 1 ? 1 : c;
    p.bound = (int)c;
    p.per = cdiv(blocks > 0 ? blocks : 1, c) * 64;
    p.chunks = (int)cdiv(n > 0 ? n : 1, p.per);
    return p;
}

// the fast forms of the chain: D == 100 and 16-byte aligned rows on both sides
inline bool rows_fast(const float *Q, const float *V, int D)
{
    return D == SCAN_FAST_D && (((uintptr_t)Q) & 15) == 0 && (((uintptr_t)V) & 15) == 0;
}

// ---- the key list of one wave ----

// bitonic sort of b[0..size) (slots >= cnt filled with KEY_MAX first), one wave; size a power of two >= cnt
__device__ __forceinline__ void wave_sort_keys(unsigned long long *b, int cnt, int size, int lane)
{
    for (int i = cnt + lane; i < size; i += 64) b[i] = SCAN_KEY_MAX;
    __syncthreads();
    for (int sz = 2; sz <= size; sz <<= 1)
        for (int stride = sz >> 1; stride > 0; stride >>= 1) {
            for (int i = lane; i < size; i += 64) {
                const int o = i ^ stride;
                if (o > i) {
                    const bool asc = (i & sz) == 0;
                    const unsigned long long x = b[i], y = b[o];
                    if ((x > y) == asc) { b[i] = y; b[o] = x; }
                }
            }
            __syncthreads();
        }
}

// ---- rank keys: how many keys of the scan come before key r of query q ----
// The kernels load the keys (rkey[r] = r < num_rank ? make_key(dist[r * Nq + q], idx[r * Nq + q]) : 0) and flush the counters (64-bit
// wave sum by shuffles, one atomic per non-zero (wave, rank)) in their own bodies: as inline functions those two steps changed the
// register allocation of prior_scan_kernel.  fusion_sweep_kernel counts in its own body for the same reason.

struct ScanRank {
    int num_rank;
    const float *dist;           // [num_rank, Nq]
    const int64_t *idx;
    int64_t *count_lt;
};

// the lane's counters: key comes before rank key r
__device__ __forceinline__ void scan_rank_count(int num_rank, const unsigned long long (&rkey)[SCAN_MAX_RANK], unsigned long long key,
                                                int (&nlt)[SCAN_MAX_RANK])
{
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r) nlt[r] += (r < num_rank && key < rkey[r]) ? 1 : 0;
}

// ---- the canonical clip distance: k-ascending fp32 fma chain of ((v - q) + eps)^2, IEEE sqrt ----

// NC consecutive clip rows against the query row in LDS: NC independent canonical chains (D = 100, 16-byte aligned rows)
template <int NC>
__device__ __forceinline__ void clip_dist_fast(const float *__restrict__ vr, const float *qs, float eps, float *out)
{
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) {
        const float4 y = *reinterpret_cast<const float4 *>(qs + 4 * k4);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float4 x = *reinterpret_cast<const float4 *>(vr + i * SCAN_FAST_D + 4 * k4);
            float t = (x.x - y.x) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (x.y - y.y) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (x.z - y.z) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (x.w - y.w) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) out[i] = __builtin_sqrtf(acc[i]);
}

// one clip row, any D: qr is the query row in global memory (wave-uniform address)
__device__ __forceinline__ float clip_dist_any(const float *__restrict__ vr, const float *__restrict__ qr, int D, float eps)
{
    float acc = 0.0f;
    for (int kk = 0; kk < D; ++kk) {
        const float t = (vr[kk] - qr[kk]) + eps;
        acc = __builtin_fmaf(t, t, acc);
    }
    return __builtin_sqrtf(acc);
}

// the wave-uniform query row: LDS copy (qs, SCAN_FAST_D + 4 floats) for the fast path, the global row otherwise
template <bool FAST>
__device__ __forceinline__ const float *query_row(const float *__restrict__ Q, int64_t q, int D, float *qs, int lane)
{
    const float *qg = Q + q * D;
    if constexpr (FAST) {
        if (lane < SCAN_FAST_D / 4) reinterpret_cast<float4 *>(qs)[lane] = reinterpret_cast<const float4 *>(qg)[lane];
        __syncthreads();
        return qs;
    } else {
        return qg;
    }
}

// distances of the n clips from row c0 on, into dst[c * stride]: two clips = two independent chains at a time on the fast path
template <bool FAST>
__device__ __forceinline__ void clip_dists(const float *__restrict__ V, int64_t c0, int n, const float *qr, int D, float eps, float *dst,
                                           int stride)
{
    if constexpr (FAST) {
        const float *vr = V + c0 * SCAN_FAST_D;
        int c = 0;
        for (; c + 2 <= n; c += 2) {
            float d[2];
            clip_dist_fast<2>(vr + (int64_t)c * SCAN_FAST_D, qr, eps, d);
            dst[c * stride] = d[0];
            dst[(c + 1) * stride] = d[1];
        }
        if (c < n) {
            float d;
            clip_dist_fast<1>(vr + (int64_t)c * SCAN_FAST_D, qr, eps, &d);
            dst[c * stride] = d;
        }
    } else {
        for (int c = 0; c < n; ++c) dst[c * stride] = clip_dist_any(V + (c0 + c) * D, qr, D, eps);
    }
}

}  // namespace vfr
