// Sentence retrieval for moments ("which sentences describe this moment"): vfr_score_sentences_f32 (include/vfr.h), and for whole
// videos ("which sentences describe this video"): vfr_score_video_sentences_f32, vsent_scan_kernel further down.
//
// The reverse direction of the scorers of score.hip / subset.hip: the PROBE (video, start clip, end clip) owns the list and the
// sentences of the bank are ranked.  score(m, j) is the canonical chain of vfr_score_moments_f32 (k-ascending fp32 fma chain over
// D, sequential fp32 sum over the span, one IEEE division), written out here (not taken from the headers of score.o, so its code
// objects do not change); key = (fp32 bits of the score << 32) | (sent_base + j), order ascending.
//
// Kernel (a translation unit of its own):
//   sentences_scan_kernel  one wave per (tile of SEN_P consecutive probes, chunk of the sentence axis).  lane = sentence: its row
//                          sits in registers (D = 100, 16-byte aligned rows) while the wave-uniform clip rows of the tile's
//                          videos stream past it through the scalar cache, four clips (= four independent chains) at a time.
//                          Consecutive probes of a tile that name the same video form a RUN: dist[c] of the clips the run
//                          touches is computed once per (clip, sentence) into LDS (lane-minor, written and read by the same
//                          lane) and every span of the run is summed s -> e from those values -- callers that sort their
//                          probes by video (the Python wrapper does) get the sharing, any order gives the same bits.
//                          Per probe: rank counts by compare + ballot + popcount (one int64 atomic per probe, rank and chunk),
//                          and the k smallest keys collected under a running threshold into a per-probe LDS list that is
//                          sorted and cut back to k when it fills; the chunk's list goes to ws[chunk][probe][0..k).
//   The per-chunk lists are merged by vfr_topk_merge_keys (one launch), which also pads with (+inf, -1).
// The chunk plan is scan_plan of scan_common.h over probe tiles: at most SCAN_MAX_CHUNKS chunks of the sentence axis, just enough for
// about SEN_TARGET_WAVES waves: one probe against 33 000 sentences fills the device, 5 000 probes run long streams (a running
// threshold wants them).  The list capacity, the key constants and the sort inside `compact` are the shared ones as well; the
// per-probe list state lives in LDS (SenTile), so the append stays here.
// Workspace: chunks x Nm x k keys, chunks <= SCAN_MAX_CHUNKS whatever Ns is.  Nothing is of size Nm x Ns, nothing waits for the host.
#include "scan_common.h"

namespace vfr {
namespace {

constexpr int SEN_P = 8;                            // probes per tile
constexpr int SEN_MAX_CLIPS = 64;                   // as the fused scorer
constexpr int SEN_TARGET_WAVES = 2048;

// probe tiles = the waves of a pass without chunks: what scan_plan spreads over the sentence axis
int64_t sen_tiles(int64_t Nm) { return cdiv(Nm, SEN_P); }

struct SenTile {              // the tile's probes (lv < 0: nothing to score) and their running state
    int lv[SEN_P], s[SEN_P], e[SEN_P], c0[SEN_P], cnt[SEN_P];
    unsigned nlt[SEN_P][SCAN_MAX_RANK];
    unsigned long long thr[SEN_P];
    unsigned long long rkey[SEN_P][SCAN_MAX_RANK];
};

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// NC clips against the lane's sentence row x: NC independent canonical chains, clip rows wave-uniform
template <int NC>
__device__ __forceinline__ void sen_dist_fast(const float4 (&x)[SCAN_FAST_D / 4], const float *__restrict__ vb, float eps, float *out)
{
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float4 y = *reinterpret_cast<const float4 *>(vb + i * SCAN_FAST_D + 4 * k4);
            float t = (y.x - x[k4].x) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (y.y - x[k4].y) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (y.z - x[k4].z) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
            t = (y.w - x[k4].w) + eps; acc[i] = __builtin_fmaf(t, t, acc[i]);
        }
        __builtin_amdgcn_sched_barrier(0);     // one step of clip-row loads at a time: more in flight overruns the SGPR file
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) out[i * 64] = __builtin_sqrtf(acc[i]);
}

// FAST: D == 100 and 16-byte aligned rows of S and V
template <bool FAST>
__global__ __launch_bounds__(64) void sentences_scan_kernel(const float *__restrict__ S, int64_t Ns, const float *__restrict__ V,
                                                            const int32_t *__restrict__ clip_off, int Nv, int D, float eps,
                                                            const int32_t *__restrict__ probes, int64_t Nm, int64_t vid_base,
                                                            int64_t sent_base, int k, int cap, ScanRank rk, int rows, int chunks,
                                                            int64_t per, int *__restrict__ bad, unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    __shared__ SenTile T;
    float *ds = ssm;                                                                       // [rows][64] clip distances, lane-minor
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ssm + (size_t)rows * 64);   // [SEN_P][cap]
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - tile * chunks);
    const int64_t m0 = tile * SEN_P;
    const int64_t j0 = (int64_t)ch * per;
    const int64_t j1 = j0 + per < Ns ? j0 + per : Ns;

    if (lane < SEN_P) {
        const int64_t m = m0 + lane;
        int lv = -1, s = 0, e = 0, c0 = 0;
        if (m < Nm) {
            const int gv = probes[3 * m], ps = probes[3 * m + 1], pe = probes[3 * m + 2];
            bool wrong = gv < 0 || ps < 0 || pe < ps;
            const int64_t l = (int64_t)gv - vid_base;
            if (gv >= 0 && l >= 0 && l < Nv) {
                const int a = clip_off[l];
                int n = clip_off[l + 1] - a;
                n = n > rows ? rows : n;
                wrong |= pe >= n;
                if (!wrong) { lv = (int)l; s = ps; e = pe; c0 = a; }
            }
            if (wrong && bad) *bad = 1;
        }
        T.lv[lane] = lv; T.s[lane] = s; T.e[lane] = e; T.c0[lane] = c0; T.cnt[lane] = 0;
        T.thr[lane] = SCAN_KEY_MAX;
#pragma unroll
        for (int r = 0; r < SCAN_MAX_RANK; ++r) {
            T.nlt[lane][r] = 0u;
            T.rkey[lane][r] = (r < rk.num_rank && m < Nm) ? make_key(rk.dist[r * Nm + m], (unsigned)rk.idx[r * Nm + m]) : 0ull;
        }
    }
    __syncthreads();

    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    // list p sorted and cut back to the k smallest; returns the new fill
    auto compact = [&](int p, int cnt) -> int {
        unsigned long long *b = buf + (size_t)p * cap;
        wave_sort_keys(b, cnt, cap, lane);
        if (cnt >= k) {
            if (lane == 0) T.thr[p] = b[k - 1];
            cnt = k;
        }
        __syncthreads();
        return cnt;
    };

    for (int64_t jb = j0; jb < j1; jb += 64) {
        const int64_t j = jb + lane;
        const bool live = j < j1;
        const float *sr = S + (live ? j : j1 - 1) * D;
        float4 x[SCAN_FAST_D / 4];
        if constexpr (FAST) {
#pragma unroll
            for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) x[k4] = *reinterpret_cast<const float4 *>(sr + 4 * k4);
        }
        const unsigned sid = (unsigned)(sent_base + j);
        int p = 0;
        while (p < SEN_P) {
            const int lv = uni(T.lv[p]);
            if (lv < 0) { ++p; continue; }
            // the run of probes on this video and the clips it touches
            int q = p + 1, cmin = uni(T.s[p]), cmax = uni(T.e[p]);
            while (q < SEN_P && uni(T.lv[q]) == lv) {
                const int s2 = uni(T.s[q]), e2 = uni(T.e[q]);
                cmin = s2 < cmin ? s2 : cmin;
                cmax = e2 > cmax ? e2 : cmax;
                ++q;
            }
            const int nc = cmax - cmin + 1;                            // <= rows: every span lies inside its video
            const float *vb = V + (int64_t)(uni(T.c0[p]) + cmin) * D;
            int c = 0;
            if constexpr (FAST) {
                for (; c + 4 <= nc; c += 4) sen_dist_fast<4>(x, vb + (int64_t)c * SCAN_FAST_D, eps, ds + c * 64 + lane);
                for (; c < nc; ++c) sen_dist_fast<1>(x, vb + (int64_t)c * SCAN_FAST_D, eps, ds + c * 64 + lane);
            } else {
                for (; c < nc; ++c) {
                    const float *vr = vb + (int64_t)c * D;
                    float acc = 0.0f;
                    for (int kk = 0; kk < D; ++kk) {
                        const float t = (vr[kk] - sr[kk]) + eps;
                        acc = __builtin_fmaf(t, t, acc);
                    }
                    ds[c * 64 + lane] = __builtin_sqrtf(acc);
                }
            }
            for (int r = p; r < q; ++r) {
                const int s = uni(T.s[r]) - cmin, e = uni(T.e[r]) - cmin;
                float sum = ds[s * 64 + lane];
                for (int c2 = s + 1; c2 <= e; ++c2) sum = sum + ds[c2 * 64 + lane];
                const float sc = sum / (float)(e - s + 1);
                const unsigned long long key = make_key(sc, sid);
                for (int rr = 0; rr < rk.num_rank; ++rr) {
                    const unsigned long long mlt = __ballot(live && key < T.rkey[r][rr]);
                    if (lane == 0 && mlt) T.nlt[r][rr] += (unsigned)__popcll(mlt);
                }
                if (k > 0) {
                    const bool take = live && key < T.thr[r];
                    const unsigned long long mt = __ballot(take);
                    if (mt) {
                        int cnt = uni(T.cnt[r]);
                        if (take) buf[(size_t)r * cap + cnt + __popcll(mt & below)] = key;
                        cnt += __popcll(mt);
                        if (cnt > cap - 64) { __syncthreads(); cnt = compact(r, cnt); }
                        if (lane == 0) T.cnt[r] = cnt;
                    }
                }
            }
            p = q;
        }
    }
    __syncthreads();
    if (k > 0) {
        for (int r = 0; r < SEN_P; ++r) {
            const int64_t m = m0 + r;
            if (m >= Nm) break;
            int cnt = uni(T.cnt[r]);
            if (cnt > k) cnt = compact(r, cnt);
            unsigned long long *out = ws + ((size_t)ch * Nm + m) * k;
            for (int i = lane; i < k; i += 64) out[i] = i < cnt ? buf[(size_t)r * cap + i] : SCAN_KEY_EMPTY;
        }
    }
    if (lane < SEN_P * SCAN_MAX_RANK) {
        const int r = lane / SCAN_MAX_RANK, rr = lane % SCAN_MAX_RANK;
        const int64_t m = m0 + r;
        if (rr < rk.num_rank && m < Nm && T.nlt[r][rr])
            atomicAdd(reinterpret_cast<unsigned long long *>(rk.count_lt + (int64_t)rr * Nm + m), (unsigned long long)T.nlt[r][rr]);
    }
}

// ---- video -> sentences (vfr_score_video_sentences_f32): one wave per (probe video, chunk of the sentence axis), lane = sentence ----
// score(p, j) = b(j, v_p): the smallest moment score over the WHOLE triangle of the probe's video.  The lane's n clip distances go to its
// LDS column as above (sen_dist_fast: the row in registers, the clip rows wave-uniform), then the lane walks the triangle -- per start
// clip a running fp32 sum over the end clip and one IEEE division per moment -- and keeps the smallest score bits.  m(j, v), the moment
// that attains it, is not returned by this call, and among equal scores every moment gives the same sentence key, so no moment position
// is carried along.  Rank counts and the list state are wave-uniform and live in registers (one probe per wave).
constexpr int VSENT_TARGET_WAVES = 2048;            // a guess, as SEN_TARGET_WAVES

template <bool FAST>
__global__ __launch_bounds__(64) void vsent_scan_kernel(const float *__restrict__ S, int64_t Ns, const float *__restrict__ V,
                                                        const int32_t *__restrict__ clip_off, int Nv, int total_clips, int D, float eps,
                                                        const int32_t *__restrict__ videos, int64_t Np, int64_t vid_base,
                                                        int64_t sent_base, int k, int cap, ScanRank rk, int rows, int chunks,
                                                        int64_t per, int *__restrict__ bad, unsigned long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float *ds = ssm;                                                                       // [rows][64] clip distances, lane-minor
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(ssm + (size_t)rows * 64);   // [cap]
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x / chunks;
    const int ch = (int)(blockIdx.x - p * chunks);
    const int64_t j0 = (int64_t)ch * per;
    const int64_t j1 = j0 + per < Ns ? j0 + per : Ns;

    // the probe's video, checked before anything of the bank is read: n = 0 gives padding and adds nothing
    const int gv = uni(videos[p]);
    int n = 0, c0 = 0;
    const int64_t l = (int64_t)gv - vid_base;
    if (gv >= 0 && l >= 0 && l < Nv) {
        const int a = uni(clip_off[l]);
        int m = uni(clip_off[l + 1]) - a;
        m = m > rows ? rows : m;
        if (m > 0 && a >= 0 && a <= total_clips - m) { n = m; c0 = a; }     // the clip rows a .. a + m lie inside V
    }
    if (gv < 0 && bad && ch == 0 && lane == 0) *bad = 1;

    unsigned long long rkey[SCAN_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SCAN_MAX_RANK; ++r)
        rkey[r] = r < rk.num_rank ? make_key(rk.dist[r * Np + p], (unsigned)rk.idx[r * Np + p]) : 0ull;
    unsigned nlt[SCAN_MAX_RANK] = {0u, 0u, 0u, 0u};            // wave-uniform: a chunk holds fewer than 2^32 sentences

    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned long long thr = SCAN_KEY_MAX;                     // keys >= thr cannot be among the chunk's k smallest
    int cnt = 0;                                               // keys in buf (wave-uniform)
    const float *vb = V + (int64_t)c0 * D;

    for (int64_t jb = j0; jb < j1 && n > 0; jb += 64) {
        const int64_t j = jb + lane;
        const bool live = j < j1;
        const float *sr = S + (live ? j : j1 - 1) * D;
        int c = 0;
        if constexpr (FAST) {
            float4 x[SCAN_FAST_D / 4];
#pragma unroll
            for (int k4 = 0; k4 < SCAN_FAST_D / 4; ++k4) x[k4] = *reinterpret_cast<const float4 *>(sr + 4 * k4);
            for (; c + 4 <= n; c += 4) sen_dist_fast<4>(x, vb + (int64_t)c * SCAN_FAST_D, eps, ds + c * 64 + lane);
            for (; c < n; ++c) sen_dist_fast<1>(x, vb + (int64_t)c * SCAN_FAST_D, eps, ds + c * 64 + lane);
        } else {
            for (; c < n; ++c) {
                const float *vr = vb + (int64_t)c * D;
                float acc = 0.0f;
                for (int kk = 0; kk < D; ++kk) {
                    const float t = (vr[kk] - sr[kk]) + eps;
                    acc = __builtin_fmaf(t, t, acc);
                }
                ds[c * 64 + lane] = __builtin_sqrtf(acc);
            }
        }
        // the whole triangle from the lane's own column: scores are >= 0, so their bits order as they do
        unsigned best = 0xFFFFFFFFu;
        for (int s = 0; s < n; ++s) {
            float sum = 0.0f;
            for (int e = s; e < n; ++e) {
                const float de = ds[e * 64 + lane];
                sum = e == s ? de : sum + de;
                const unsigned b = __float_as_uint(sum / (float)(e - s + 1));
                best = b < best ? b : best;
            }
        }
        const unsigned long long key = ((unsigned long long)best << 32) | (unsigned)(sent_base + j);
#pragma unroll
        for (int r = 0; r < SCAN_MAX_RANK; ++r) {
            if (r < rk.num_rank) nlt[r] += (unsigned)__popcll(__ballot(live && key < rkey[r]));
        }
        if (k > 0) {
            const bool take = live && key < thr;
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
        }
    }
    if (k > 0) {
        __syncthreads();
        int size = 64;
        while (size < cnt) size <<= 1;                         // cnt <= cap, a power of two
        wave_sort_keys(buf, cnt, size, lane);
        cnt = cnt > k ? k : cnt;
        unsigned long long *out = ws + ((size_t)ch * Np + p) * k;
        for (int i = lane; i < k; i += 64) out[i] = i < cnt ? buf[i] : SCAN_KEY_EMPTY;
    }
    if (lane < rk.num_rank) {
        unsigned x = nlt[0];
#pragma unroll
        for (int r = 1; r < SCAN_MAX_RANK; ++r) x = lane == r ? nlt[r] : x;
        if (x) atomicAdd(reinterpret_cast<unsigned long long *>(rk.count_lt + (int64_t)lane * Np + p), (unsigned long long)x);
    }
}

}  // namespace
}  // namespace vfr

extern "C" {

size_t vfr_score_sentences_workspace_bytes(int64_t Nm, int64_t Ns, int k)
{
    if (Nm < 0 || Ns < 0 || k < 0 || k > vfr::SCAN_MAX_K || Nm * (int64_t)(k > 0 ? k : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(vfr::sen_tiles(Nm), Ns, vfr::SEN_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Nm * (size_t)k * 8 + 256, 256);
}

int vfr_score_sentences_f32(const float *S, int64_t Ns, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                            int max_clips, int D, float eps, const int32_t *probes, int64_t Nm, int64_t vid_base, int64_t sent_base,
                            int k, float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist, const int64_t *rank_idx,
                            int64_t *count_lt, int *bad, void *workspace, size_t workspace_bytes, vfr_stream_t stream)
{
    VFR_REQUIRE(Ns >= 0 && Nm >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::SEN_MAX_CLIPS && vid_base >= 0 && sent_base >= 0, VFR_EINVAL,
                "vfr_score_sentences_f32: bad shape (k <= 448, max_clips <= 64, sizes, vid_base, sent_base >= 0)");
    VFR_REQUIRE(sent_base + Ns < (int64_t(1) << 32), VFR_EINVAL, "vfr_score_sentences_f32: sent_base + Ns must stay below 2^32");
    VFR_REQUIRE(Nm * (int64_t)(k > 0 ? k : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_sentences_f32: Nm * k must stay below 2^31");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_sentences_f32: num_rank %d (0 .. 4)", num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_sentences_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_sentences_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Nm == 0 || probes, VFR_EINVAL, "vfr_score_sentences_f32: probes is null");
    VFR_REQUIRE(Ns == 0 || S, VFR_EINVAL, "vfr_score_sentences_f32: S is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && (V || total_clips == 0)), VFR_EINVAL, "vfr_score_sentences_f32: null clip bank");
    const int64_t tiles = vfr::sen_tiles(Nm);
    const vfr::ScanPlan plan = vfr::scan_plan(tiles, Ns, vfr::SEN_TARGET_WAVES);
    VFR_REQUIRE(tiles * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_sentences_f32: too many probe tiles");
    const size_t need = vfr_score_sentences_workspace_bytes(Nm, Ns, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_sentences_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    if (Nm == 0 || (k == 0 && num_rank == 0 && !bad)) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    const int rows = max_clips < 1 ? 1 : max_clips;
    const int cap = vfr::scan_cap(k);
    const size_t lds = (size_t)rows * 64 * 4 + (size_t)vfr::SEN_P * cap * 8;             // <= 16 KB + 32 KB
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        const dim3 grid((unsigned)(tiles * plan.chunks)), block(64);
        const bool fast = vfr::rows_fast(S, V, D);
        if (fast)
            hipLaunchKernelGGL((vfr::sentences_scan_kernel<true>), grid, block, lds, st, S, Ns, V, clip_offsets, Nv, D, eps, probes, Nm,
                               vid_base, sent_base, k, cap, rk, rows, plan.chunks, plan.per, bad, keys);
        else
            hipLaunchKernelGGL((vfr::sentences_scan_kernel<false>), grid, block, lds, st, S, Ns, V, clip_offsets, Nv, D, eps, probes, Nm,
                               vid_base, sent_base, k, cap, rk, rows, plan.chunks, plan.per, bad, keys);
        VFR_CHECK_LAUNCH("sentences_scan_kernel");
    }
    if (k > 0)
        return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Nm, k, out_dist, out_idx, nullptr, stream);
    return VFR_OK;
}

size_t vfr_score_video_sentences_workspace_bytes(int64_t Np, int64_t Ns, int k)
{
    if (Np < 0 || Ns < 0 || k < 0 || k > vfr::SCAN_MAX_K || Np * (int64_t)(k > 0 ? k : 1) > 0x7FFFFFFF) return 0;
    const vfr::ScanPlan p = vfr::scan_plan(Np, Ns, vfr::VSENT_TARGET_WAVES);
    return vfr::align_up((size_t)p.bound * (size_t)Np * (size_t)k * 8 + 256, 256);
}

int vfr_score_video_sentences_f32(const float *S, int64_t Ns, const float *V, const int32_t *clip_offsets, int Nv, int total_clips,
                                  int max_clips, int D, float eps, const int32_t *videos, int64_t Np, int64_t vid_base,
                                  int64_t sent_base, int k, float *out_dist, int64_t *out_idx, int num_rank, const float *rank_dist,
                                  const int64_t *rank_idx, int64_t *count_lt, int *bad, void *workspace, size_t workspace_bytes,
                                  vfr_stream_t stream)
{
    VFR_REQUIRE(Ns >= 0 && Np >= 0 && Nv >= 0 && total_clips >= 0 && D > 0 && k >= 0 && k <= vfr::SCAN_MAX_K && max_clips >= 0 &&
                max_clips <= vfr::SEN_MAX_CLIPS && vid_base >= 0 && sent_base >= 0, VFR_EINVAL,
                "vfr_score_video_sentences_f32: bad shape (k <= 448, max_clips <= 64, sizes, vid_base, sent_base >= 0)");
    VFR_REQUIRE(sent_base + Ns < (int64_t(1) << 32), VFR_EINVAL, "vfr_score_video_sentences_f32: sent_base + Ns must stay below 2^32");
    VFR_REQUIRE(Np * (int64_t)(k > 0 ? k : 1) <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_video_sentences_f32: Np * k must stay below 2^31");
    VFR_REQUIRE(num_rank >= 0 && num_rank <= vfr::SCAN_MAX_RANK, VFR_EINVAL, "vfr_score_video_sentences_f32: num_rank %d (0 .. 4)",
                num_rank);
    VFR_REQUIRE(num_rank == 0 || (rank_dist && rank_idx && count_lt), VFR_EINVAL,
                "vfr_score_video_sentences_f32: num_rank > 0 needs rank_dist, rank_idx and count_lt");
    VFR_REQUIRE(k == 0 || Np == 0 || (out_dist && out_idx), VFR_EINVAL, "vfr_score_video_sentences_f32: k > 0 needs out_dist / out_idx");
    VFR_REQUIRE(Np == 0 || videos, VFR_EINVAL, "vfr_score_video_sentences_f32: videos is null");
    VFR_REQUIRE(Ns == 0 || S, VFR_EINVAL, "vfr_score_video_sentences_f32: S is null");
    VFR_REQUIRE(Nv == 0 || (clip_offsets && (V || total_clips == 0)), VFR_EINVAL, "vfr_score_video_sentences_f32: null clip bank");
    const vfr::ScanPlan plan = vfr::scan_plan(Np, Ns, vfr::VSENT_TARGET_WAVES);
    VFR_REQUIRE(Np * plan.chunks <= 0x7FFFFFFF, VFR_EINVAL, "vfr_score_video_sentences_f32: too many probes");
    const size_t need = vfr_score_video_sentences_workspace_bytes(Np, Ns, k);
    VFR_REQUIRE(workspace && workspace_bytes >= need, VFR_EWORKSPACE, "vfr_score_video_sentences_f32: workspace %zu < %zu bytes",
                workspace_bytes, need);
    if (Np == 0 || (k == 0 && num_rank == 0 && !bad)) return VFR_OK;
    hipStream_t st = vfr::as_stream(stream);
    const int rows = max_clips < 1 ? 1 : max_clips;
    const int cap = vfr::scan_cap(k);
    const size_t lds = (size_t)rows * 64 * 4 + (size_t)cap * 8;                          // <= 16 KB + 4 KB
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    {
        vfr::ProfScope prof(vfr::SITE_SCORE_PAIRS, st);
        vfr::ScanRank rk{num_rank, rank_dist, rank_idx, count_lt};
        const dim3 grid((unsigned)(Np * plan.chunks)), block(64);
        if (vfr::rows_fast(S, V, D))
            hipLaunchKernelGGL((vfr::vsent_scan_kernel<true>), grid, block, lds, st, S, Ns, V, clip_offsets, Nv, total_clips, D, eps,
                               videos, Np, vid_base, sent_base, k, cap, rk, rows, plan.chunks, plan.per, bad, keys);
        else
            hipLaunchKernelGGL((vfr::vsent_scan_kernel<false>), grid, block, lds, st, S, Ns, V, clip_offsets, Nv, total_clips, D, eps,
                               videos, Np, vid_base, sent_base, k, cap, rk, rows, plan.chunks, plan.per, bad, keys);
        VFR_CHECK_LAUNCH("vsent_scan_kernel");
    }
    if (k > 0)
        return vfr_topk_merge_keys(reinterpret_cast<const int64_t *>(keys), plan.chunks, Np, k, out_dist, out_idx, nullptr, stream);
    return VFR_OK;
}

}  // extern "C"
