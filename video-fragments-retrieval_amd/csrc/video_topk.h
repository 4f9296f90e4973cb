// What the video-level units share (video_topk.hip defines it; moment_nms.hip and paragraphs.hip build on it): the list entry
// flag, the bound functions of the fast path (margins derived in video_topk.hip), the block-wide radix select, the workspace
// and the host launchers of the two kernels paragraphs.hip reuses.
#pragma once
#include "score_device.h"
#include "score_internal.h"

namespace vfr {

constexpr int VTK_VIDEOS = 32;                        // videos per wave of the bounds kernel (<= 32 x 21 clips)
constexpr int VTK_CLIPS = VTK_VIDEOS * 21;
constexpr unsigned VTK_UNDECIDED = 0x80000000u;       // list entry flag: the rank count of this video needs its exact key
constexpr float VTK_U = 5.9604645e-8f;                // 2^-24

__device__ __forceinline__ float vtk_dhi(float m2, float E2m, float W)
{
    return (__builtin_sqrtf(m2 + E2m) + 4.0f * VTK_U * W) * (1.0f + 136.0f * VTK_U);
}
__device__ __forceinline__ float vtk_blo(float m2, float E2m, float W)
{
    const float x = m2 - E2m;
    const float lo = (__builtin_sqrtf(x > 0.0f ? x : 0.0f) - 4.0f * VTK_U * W) * (1.0f - 136.0f * VTK_U);
    return lo * (1.0f - 32.0f * VTK_U);
}

// k-th smallest (1-based) of the 32-bit patterns x[0..n) (all threads of the block get it): four passes of 256 bins
template <typename LOAD>
__device__ unsigned vtk_radix_kth32(LOAD load, int n, int kth, unsigned *hist, unsigned *shared_word)
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

struct VtkWs {
    MfmaWs mw;                                         // bank-side products at the pre-filter's offsets (rv .. vb, hash, stale)
    float4 *qmeta; float *qc; float *m2; unsigned *list; int *list_len, *n_undecided; unsigned long long *keys;
    size_t total;
};
inline VtkWs carve_vtk(void *base, int64_t Nq, int Nv, int total_clips)
{
    VtkWs w{};
    w.mw = carve_bank_front(base, total_clips);
    size_t off = (size_t)(reinterpret_cast<char *>(w.mw.stale) - static_cast<char *>(base)) + 256;
    auto take = [&](size_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes, 256); return p; };
    w.qmeta = reinterpret_cast<float4 *>(take((size_t)Nq * 16));
    w.qc = reinterpret_cast<float *>(take((size_t)Nq * FAST_D * 4));
    w.m2 = reinterpret_cast<float *>(take((size_t)Nq * Nv * 4));
    w.list = reinterpret_cast<unsigned *>(take((size_t)Nq * Nv * 4));
    w.list_len = reinterpret_cast<int *>(take((size_t)Nq * 4));
    w.n_undecided = reinterpret_cast<int *>(take((size_t)Nq * 4));
    w.keys = reinterpret_cast<unsigned long long *>(take((size_t)Nq * Nv * 8));
    w.total = off;
    return w;
}

// launches only (profiler scope and launch check stay with the caller): m2 [Nq, Nv] from the products of vtk_prepass; per row of keys [rows, Nv] its k smallest, sorted, (+inf, -1) padded
void vtk_launch_bounds(const float *qc, int64_t Nq, const MfmaWs &mw, const float4 *qmeta, const int32_t *clip_offsets, int Nv, int total_clips, float *m2, hipStream_t st);
void vtk_launch_topk(const unsigned long long *keys, const int *list_len, int64_t rows, int Nv, int k, float *out_dist, int64_t *out_idx, hipStream_t st);

}  // namespace vfr
