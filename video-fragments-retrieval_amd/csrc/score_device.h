// Inline device helpers and constants shared by the scorer's translation units (score.hip, score_smallq.hip,
// topk_exchange.hip, video_topk.hip, moment_nms.hip, paragraphs.hip): the key and size constants, the clip-distance chain of
// the generic kernel, the cross-lane exchange and the wave-cooperative bitonic sort behind every top-k pool.
// (scan_common.h has its own wave_sort / clip_dist4 for the retrieval variants: different code, not merged.)
#pragma once
#include "vfr_common.h"
#include "vfr_math.h"

namespace vfr {

constexpr int NMAX_FUSED = 64;    // max clips per video on the fused path
constexpr int NMAX_DENSE = 128;   // max clips per video on the dense / own paths
constexpr unsigned long long KEY_MAX = ~0ull;
constexpr unsigned long long KEY_EMPTY = 0x7F800000FFFFFFFFull;   // (+inf, max id): an unused slot of an exchanged list
constexpr int MAX_RANK = 4;       // rank keys per query counted in one pass (IoU thresholds)
constexpr int FAST_D = 100;       // the model's embedding width: what every fast path is built for
typedef float f32x4 __attribute__((ext_vector_type(4)));   // an MFMA accumulator tile's four rows per lane

// ------------------------------------------------------------------------------------------------
// distance of NC (<= 4) clips to this lane's query: D is a template constant when DT > 0 (query in
// registers), runtime when DT == 0 (query re-read from global, L1-resident).
// ------------------------------------------------------------------------------------------------
template <int DT, int NC>
__device__ __forceinline__ void clip_dist4(const float *__restrict__ V, int64_t crow, int D, float eps,
                                           const float *qreg, const float *__restrict__ qrow, float *out)
{
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0f;
    const float *v = V + crow * (DT > 0 ? DT : D);
    if constexpr (DT > 0) {
#pragma unroll
        for (int k = 0; k < DT; ++k) {
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                float d = (v[i * DT + k] - qreg[k]) + eps;
                acc[i] = __builtin_fmaf(d, d, acc[i]);
            }
        }
    } else {
        for (int k = 0; k < D; ++k) {
            float qk = qrow[k];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                float d = (v[(int64_t)i * D + k] - qk) + eps;
                acc[i] = __builtin_fmaf(d, d, acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) out[i] = __builtin_sqrtf(acc[i]);
}

// all n clip distances of one video into the wave's LDS column ds[c*64 + lane]
template <int DT>
__device__ __forceinline__ void video_distances(const float *__restrict__ V, int c0, int n, int D, float eps,
                                                const float *qreg, const float *__restrict__ qrow, float *ds,
                                                int lane)
{
    int c = 0;
    for (; c + 4 <= n; c += 4) {
        float d[4];
        clip_dist4<DT, 4>(V, c0 + c, D, eps, qreg, qrow, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) ds[(c + i) * 64 + lane] = d[i];
    }
    for (; c < n; ++c) {
        float d[1];
        clip_dist4<DT, 1>(V, c0 + c, D, eps, qreg, qrow, d);
        ds[c * 64 + lane] = d[0];
    }
}

// value of lane (lane ^ STRIDE): within a row of 16 lanes through the DPP data path (one or two v_mov_b32_dpp per dword, a
// few cycles), across rows through ds_bpermute (an LDS round trip).  26 of the 33 cross-lane stages of the 256-key sort
// have STRIDE <= 8, and the stages depend on each other: the round trips were the sort's time.
template <int STRIDE>
__device__ __forceinline__ unsigned xor_lane_u32(unsigned x)
{
    if constexpr (STRIDE == 1) return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xF, 0xF, false);      // quad_perm [1,0,3,2]
    else if constexpr (STRIDE == 2) return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4E, 0xF, 0xF, false); // quad_perm [2,3,0,1]
    else if constexpr (STRIDE == 4) {
        const int t = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x104, 0xF, 0x5, false);       // row_shl:4 into banks 0, 2 (lane <- lane + 4)
        return (unsigned)__builtin_amdgcn_update_dpp(t, (int)x, 0x114, 0xF, 0xA, false);          // row_shr:4 into banks 1, 3 (lane <- lane - 4)
    } else if constexpr (STRIDE == 8) {
        const int t = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x108, 0xF, 0x3, false);       // row_shl:8 into banks 0, 1
        return (unsigned)__builtin_amdgcn_update_dpp(t, (int)x, 0x118, 0xF, 0xC, false);          // row_shr:8 into banks 2, 3
    } else return (unsigned)__shfl_xor((int)x, STRIDE, 64);
}
template <int STRIDE>
__device__ __forceinline__ unsigned long long xor_lane_u64(unsigned long long x)
{
    return ((unsigned long long)xor_lane_u32<STRIDE>((unsigned)(x >> 32)) << 32) | xor_lane_u32<STRIDE>((unsigned)x);
}

// ------------------------------------------------------------------------------------------------
// wave-cooperative bitonic sort of KPL*64 keys, element e = i*64 + lane, ascending
// ------------------------------------------------------------------------------------------------
template <int KPL>
__device__ __forceinline__ void wave_sort(unsigned long long (&key)[KPL], int lane)
{
    constexpr int CAP = KPL * 64;
#pragma unroll
    for (int size = 2; size <= CAP; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            if (stride >= 64) {
                const int j = stride >> 6;
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    if ((i & j) == 0) {
                        const bool asc = size >= CAP ? true : ((i & (size >> 6)) == 0);
                        unsigned long long a = key[i], b = key[i | j];
                        unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
                        key[i] = asc ? lo : hi;
                        key[i | j] = asc ? hi : lo;
                    }
                }
            } else {
                const bool lower = (lane & stride) == 0;
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    bool asc;
                    if (size >= CAP) asc = true;
                    else if (size >= 64) asc = (i & (size >> 6)) == 0;
                    else asc = (lane & size) == 0;
                    // the lane keeps its key when (it wants the smaller one) == (its key is the smaller one): one 64-bit
                    // compare and two selects (min / max / select took ten vector instructions per key and stage)
                    const unsigned long long other = stride == 1 ? xor_lane_u64<1>(key[i]) : stride == 2 ? xor_lane_u64<2>(key[i])
                                                   : stride == 4 ? xor_lane_u64<4>(key[i]) : stride == 8 ? xor_lane_u64<8>(key[i])
                                                   : stride == 16 ? xor_lane_u64<16>(key[i]) : xor_lane_u64<32>(key[i]);
                    const bool keep = (lower == asc) == (key[i] < other);
                    key[i] = keep ? key[i] : other;
                }
            }
        }
    }
}

template <int KPL>
__device__ __forceinline__ unsigned long long key_at(const unsigned long long (&key)[KPL], int e)
{
    unsigned long long r = 0;
    const int i = e >> 6, l = e & 63;
#pragma unroll
    for (int j = 0; j < KPL; ++j)
        if (j == i) r = __shfl(key[j], l, 64);
    return r;
}

// compact the candidate buffer of lane L (wave-uniform): keep the k smallest keys, sorted.
// returns the new count; *thr_out = k-th smallest key when at least k keys exist.
template <int KPL>
__device__ __attribute__((noinline)) int compact_buffer(unsigned long long *base, int cnt, int k, int lane,
                                              unsigned long long *thr_out)
{
    unsigned long long key[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        int e = i * 64 + lane;
        key[i] = e < cnt ? base[e] : KEY_MAX;
    }
    wave_sort<KPL>(key, lane);
    const int keep = cnt < k ? cnt : k;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        int e = i * 64 + lane;
        if (e < keep) base[e] = key[i];
    }
    if (cnt >= k) *thr_out = key_at<KPL>(key, k - 1);
    return keep;
}

}  // namespace vfr
