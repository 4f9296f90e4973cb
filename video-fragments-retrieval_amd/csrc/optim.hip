// f2, the training driver around the encoders' backward (model/main.py:43-80 with model/data.py:204-246,318-356): the pieces
// of a training step that are neither the model nor the loss.
//   vfr_triplet_gather_f32   one batch of CustomBatchSampler triplets -> custom_collate's posit / intra / inter [rows, 2F+2],
//                            maskp / maskn and the gathered query tokens, in ONE launch from the resident feature bank
//                            (rows [seg[off[v] + t] | ctx[v] | t/n | (t+1)/n], make_visual_features, data.py:204-213)
//   vfr_adam_step_f32        torch.optim.Adam (L2 weight decay, amsgrad off) over up to VFR_ADAM_MAX_TENSORS tensors in ONE
//                            launch, which also writes the sum of squares of every raw gradient (utils.grad_norm's input)
//   vfr_grad_sumsq_f32       the same per-tensor sums of squares without the update
// The plan of the gather and the tensor table of the optimizer travel BY VALUE in the kernel arguments: nothing is staged in
// host memory that a later call could overwrite before the copy has run, and nothing is cached between calls.
#include "vfr_common.h"

namespace vfr {

// ------------------------------------------------------------------------------------------------ triplet gather
constexpr int GATHER_MAX = 128;                  // samples per launch: 128 x 24 bytes of plan + the pointers < 4 KB of kernargs

struct GatherArgs {
    const float *seg, *ctx;                      // bank: seg [sum n, F], ctx [Nv, F]
    const int *clip_off;                         // [Nv + 1]
    const int64_t *tokens;                       // [A, Tq]
    float *posit, *intra, *inter;                // [P | Nn | P, 2F + 2]
    int64_t *maskp, *maskn, *lang;               // [P], [Nn], [S, Tq]
    int F, Tq, s0;                               // s0: global index of plan entry 0 (this launch's first sample)
    // per sample: video_pos, video_neg, (st | et << 8 | stn << 16 | etn << 24), token row, posit/inter row, intra row
    int plan[GATHER_MAX][6];
};

// grid (max rows of a sample, samples, 3): z = 0 posit (+ tokens), 1 intra, 2 inter.  A block writes one [2F+2] row as
// float2 pairs (rows are only 8-byte aligned: 2F+2 is even but not a multiple of 4); F even reads the bank as float2 too.
__global__ __launch_bounds__(256) void triplet_gather_kernel(const GatherArgs a)
{
    const int s = blockIdx.y, kind = blockIdx.z, r = blockIdx.x;
    const int *pl = a.plan[s];
    const unsigned tt = (unsigned)pl[2];
    const int st = kind == 1 ? (int)((tt >> 16) & 255u) : (int)(tt & 255u);
    const int et = kind == 1 ? (int)(tt >> 24) : (int)((tt >> 8) & 255u);
    if (r > et - st) return;
    const int v = kind == 2 ? pl[1] : pl[0];
    const int c0 = a.clip_off[v], n = a.clip_off[v + 1] - c0;
    const int t = st + r;
    const int64_t row = (int64_t)(kind == 1 ? pl[5] : pl[4]) + r;
    const int W = 2 * a.F + 2;
    float *out = (kind == 0 ? a.posit : kind == 1 ? a.intra : a.inter) + row * W;
    if (threadIdx.x == 0) {
        if (kind == 0) a.maskp[row] = a.s0 + s;
        if (kind == 1) a.maskn[row] = a.s0 + s;
    }
    if (kind == 0 && r == 0)
        for (int j = threadIdx.x; j < a.Tq; j += 256) a.lang[(int64_t)(a.s0 + s) * a.Tq + j] = a.tokens[(int64_t)pl[3] * a.Tq + j];
    float2 *o2 = reinterpret_cast<float2 *>(out);
    if (t >= n) {                                // outside the video (the host checks this; never read past the bank)
        for (int j = threadIdx.x; j < W / 2; j += 256) o2[j] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        return;
    }
    const float *sg = a.seg + (int64_t)(c0 + t) * a.F, *cx = a.ctx + (int64_t)v * a.F;
    const float tn = (float)t / (float)n, tn1 = (float)(t + 1) / (float)n;     // IEEE division of exact integers
    if ((a.F & 1) == 0) {
        const int h = a.F / 2;
        const float2 *sg2 = reinterpret_cast<const float2 *>(sg), *cx2 = reinterpret_cast<const float2 *>(cx);
        for (int j = threadIdx.x; j < h; j += 256) o2[j] = sg2[j];
        for (int j = threadIdx.x; j < h; j += 256) o2[h + j] = cx2[j];
        if (threadIdx.x == 0) o2[a.F] = make_float2(tn, tn1);
        return;
    }
    for (int j = threadIdx.x; j < W / 2; j += 256) {
        float e[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = 2 * j + k;
            e[k] = i < a.F ? sg[i] : i < 2 * a.F ? cx[i - a.F] : i == 2 * a.F ? tn : tn1;
        }
        o2[j] = make_float2(e[0], e[1]);
    }
}

// ------------------------------------------------------------------------------------------------ Adam + sums of squares
constexpr int ADAM_MAX = VFR_ADAM_MAX_TENSORS;
constexpr int ADAM_THREADS = 256, ADAM_PER_THREAD = 16, ADAM_CHUNK = ADAM_THREADS * ADAM_PER_THREAD;

struct AdamArgs {
    float *p[ADAM_MAX];
    const float *g[ADAM_MAX];
    float *m[ADAM_MAX], *v[ADAM_MAX];
    int64_t numel[ADAM_MAX];
    int chunk0[ADAM_MAX + 1];                    // first chunk of each tensor (prefix sums of ceil(numel / ADAM_CHUNK))
    float coef[ADAM_MAX][7];                     // wd, 1-beta1, beta2, 1-beta2, eps, -step_size, 1/bias_correction2_sqrt
    int vec[ADAM_MAX];                           // all four pointers 16-byte aligned
    int n;
    float *sumsq;                                // [n] sum of squares of the raw gradients
    float *partials;                             // [chunks] workspace
    unsigned *counter;                           // workspace word: zero on entry, left zero
};

// one element of torch.optim.Adam's single-tensor step (torch/optim/adam.py _single_tensor_adam, amsgrad off), each op
// rounded to fp32 as ATen's elementwise kernels do:
//   g' = g + wd p                  grad.add(param, alpha=wd)         (skipped for wd == 0, as torch does)
//   m  = lerp(m, g', 1 - beta1)    exp_avg.lerp_ (ATen's two-sided formula)
//   v  = v beta2;  v = v + (1 - beta2) (g' g')                       exp_avg_sq.mul_(beta2).addcmul_(g', g', 1 - beta2)
//   d  = sqrt(v) * (1 / bc2_sqrt) + eps                              (sqrt / CPU scalar is a multiply by its fp32 reciprocal)
//   p  = p + (-step_size) (m / d)                                    param.addcdiv_(m, d, value=-step_size)
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const float *c)
{
    const float wd = c[0], w1 = c[1], b2 = c[2], c2 = c[3], eps = c[4], nss = c[5], ibc2 = c[6];
    if (wd != 0.0f) g = g + wd * p;
    const float d = g - m;
    m = w1 < 0.5f ? m + w1 * d : g - d * (1.0f - w1);
    v = v * b2;
    v = v + c2 * (g * g);
    const float den = __builtin_sqrtf(v) * ibc2 + eps;
    p = p + nss * (m / den);
}

template <bool UPDATE>
__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(const AdamArgs a)
{
    __shared__ float red[ADAM_THREADS + 1];            // the tree, then [ADAM_THREADS] = "this block is the last one"
    const int chunk = blockIdx.x, tid = threadIdx.x;
    int ti = 0;
    while (ti + 1 < a.n && a.chunk0[ti + 1] <= chunk) ++ti;
    const int64_t n = a.numel[ti], base = (int64_t)(chunk - a.chunk0[ti]) * ADAM_CHUNK;
    const float *g = a.g[ti];
    float ss = 0.0f;
    if (a.vec[ti]) {
#pragma unroll
        for (int it = 0; it < ADAM_PER_THREAD / 4; ++it) {
            const int64_t i = base + ((int64_t)it * ADAM_THREADS + tid) * 4;
            if (i + 4 <= n) {
                const float4 g4 = *reinterpret_cast<const float4 *>(g + i);
                ss = ss + g4.x * g4.x; ss = ss + g4.y * g4.y; ss = ss + g4.z * g4.z; ss = ss + g4.w * g4.w;
                if constexpr (UPDATE) {
                    float4 p4 = *reinterpret_cast<const float4 *>(a.p[ti] + i);
                    float4 m4 = *reinterpret_cast<const float4 *>(a.m[ti] + i);
                    float4 v4 = *reinterpret_cast<const float4 *>(a.v[ti] + i);
                    adam_elem(p4.x, g4.x, m4.x, v4.x, a.coef[ti]);
                    adam_elem(p4.y, g4.y, m4.y, v4.y, a.coef[ti]);
                    adam_elem(p4.z, g4.z, m4.z, v4.z, a.coef[ti]);
                    adam_elem(p4.w, g4.w, m4.w, v4.w, a.coef[ti]);
                    *reinterpret_cast<float4 *>(a.p[ti] + i) = p4;
                    *reinterpret_cast<float4 *>(a.m[ti] + i) = m4;
                    *reinterpret_cast<float4 *>(a.v[ti] + i) = v4;
                }
            } else {
                for (int64_t k = i; k < n; ++k) {          // the tail: at most 3 elements, in one thread
                    const float gk = g[k];
                    ss = ss + gk * gk;
                    if constexpr (UPDATE) adam_elem(a.p[ti][k], gk, a.m[ti][k], a.v[ti][k], a.coef[ti]);
                }
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < ADAM_PER_THREAD; ++it) {
            const int64_t i = base + (int64_t)it * ADAM_THREADS + tid;
            if (i < n) {
                const float gk = g[i];
                ss = ss + gk * gk;
                if constexpr (UPDATE) adam_elem(a.p[ti][i], gk, a.m[ti][i], a.v[ti][i], a.coef[ti]);
            }
        }
    }
    // fixed-order partial of this chunk (no float atomics): a tree over the block's threads
    red[tid] = ss;
    __syncthreads();
    for (int w = ADAM_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    // hand-off to the last block: plain store, drain, agent-scope release, then the ticket
    if (tid == 0) {
        a.partials[chunk] = red[0];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned done = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = done == gridDim.x - 1;
        red[ADAM_THREADS] = last ? 1.0f : 0.0f;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (red[ADAM_THREADS] == 0.0f) return;
    // final reduce in a fixed order: per tensor, thread k adds chunks k, k + 256, ... in order, then the same tree
    for (int t = 0; t < a.n; ++t) {
        float acc = 0.0f;
        for (int c = a.chunk0[t] + tid; c < a.chunk0[t + 1]; c += ADAM_THREADS) acc = acc + a.partials[c];
        __syncthreads();
        red[tid] = acc;
        __syncthreads();
        for (int w = ADAM_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] = red[tid] + red[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.sumsq[t] = red[0];
    }
    if (tid == 0) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int64_t adam_chunks(const int64_t *numel, int n)
{
    int64_t c = 0;
    for (int i = 0; i < n; ++i) c += cdiv(numel[i], ADAM_CHUNK);
    return c;
}

static int adam_launch(bool update, int n, float *const *p, const float *const *g, float *const *m, float *const *v,
                       const int64_t *numel, const float *coef, float *sumsq, void *ws, size_t ws_bytes, hipStream_t st,
                       const char *who)
{
    VFR_REQUIRE(n >= 0 && n <= ADAM_MAX && g && numel && (n == 0 || sumsq), VFR_EINVAL, "%s: bad argument (n = %d, at most %d)", who,
                n, ADAM_MAX);
    if (n == 0) return VFR_OK;
    AdamArgs a{};
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        VFR_REQUIRE(numel[i] > 0 && g[i], VFR_EINVAL, "%s: tensor %d: empty or null gradient", who, i);
        a.g[i] = g[i];
        a.numel[i] = numel[i];
        a.chunk0[i] = (int)chunks;
        chunks += cdiv(numel[i], ADAM_CHUNK);
        uintptr_t orv = (uintptr_t)g[i];
        if (update) {
            VFR_REQUIRE(p && m && v && coef && p[i] && m[i] && v[i], VFR_EINVAL, "%s: tensor %d: null pointer", who, i);
            a.p[i] = p[i]; a.m[i] = m[i]; a.v[i] = v[i];
            for (int k = 0; k < 7; ++k) a.coef[i][k] = coef[7 * i + k];
            orv |= (uintptr_t)p[i] | (uintptr_t)m[i] | (uintptr_t)v[i];
        }
        VFR_REQUIRE((orv & 3u) == 0, VFR_EINVAL, "%s: tensor %d: not 4-byte aligned", who, i);
        a.vec[i] = (orv & 15u) == 0;
    }
    VFR_REQUIRE(chunks < (1 << 30), VFR_EUNSUPPORTED, "%s: %lld elements", who, (long long)chunks * ADAM_CHUNK);
    a.chunk0[n] = (int)chunks;
    const size_t need = vfr_adam_workspace_bytes(numel, n);
    VFR_REQUIRE(ws && ws_bytes >= need, VFR_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    a.n = n;
    a.sumsq = sumsq;
    a.counter = (unsigned *)ws;
    a.partials = (float *)((char *)ws + 256);
    if (update)
        hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)chunks), dim3(ADAM_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)chunks), dim3(ADAM_THREADS), 0, st, a);
    VFR_CHECK_LAUNCH("adam_kernel");
    return VFR_OK;
}

}  // namespace vfr

extern "C" {

int vfr_triplet_gather_f32(const float *seg, const float *ctx, const int *clip_off, int num_videos, int F, const int64_t *tokens,
                           int num_tokens_rows, int Tq, const int *plan_host, int S, int64_t P, int64_t Nn, float *posit,
                           float *intra, float *inter, int64_t *maskp, int64_t *maskn, int64_t *lang, vfr_stream_t stream)
{
    VFR_REQUIRE(F > 0 && Tq > 0 && S >= 0 && num_videos > 0 && num_tokens_rows > 0 && seg && ctx && clip_off && tokens &&
                    (S == 0 || plan_host), VFR_EINVAL, "vfr_triplet_gather_f32: bad argument");
    // host-side validation of the whole plan (it is host memory): every row written stays inside the outputs
    int64_t pr = 0, nr = 0;
    for (int s = 0; s < S; ++s) {
        const int *q = plan_host + 7 * s;
        VFR_REQUIRE(q[0] >= 0 && q[0] < num_videos && q[1] >= 0 && q[1] < num_videos && q[6] >= 0 && q[6] < num_tokens_rows,
                    VFR_EINVAL, "vfr_triplet_gather_f32: sample %d: video or token row out of range", s);
        VFR_REQUIRE(q[2] >= 0 && q[2] <= q[3] && q[3] < 256 && q[4] >= 0 && q[4] <= q[5] && q[5] < 256, VFR_EINVAL,
                    "vfr_triplet_gather_f32: sample %d: bad clip span (%d, %d) / (%d, %d)", s, q[2], q[3], q[4], q[5]);
        pr += q[3] - q[2] + 1;
        nr += q[5] - q[4] + 1;
    }
    VFR_REQUIRE(pr == P && nr == Nn, VFR_EINVAL, "vfr_triplet_gather_f32: plan has %lld / %lld rows, outputs %lld / %lld",
                (long long)pr, (long long)nr, (long long)P, (long long)Nn);
    if (S == 0) return VFR_OK;
    VFR_REQUIRE(posit && intra && inter && maskp && maskn && lang, VFR_EINVAL, "vfr_triplet_gather_f32: null output");
    VFR_REQUIRE(((uintptr_t)posit | (uintptr_t)intra | (uintptr_t)inter) % 8 == 0 && ((F & 1) || ((uintptr_t)seg | (uintptr_t)ctx) % 8 == 0),
                VFR_EINVAL, "vfr_triplet_gather_f32: outputs (and, F even, the bank) must be 8-byte aligned");
    hipStream_t st = vfr::as_stream(stream);
    int64_t prow = 0, nrow = 0;
    for (int s0 = 0; s0 < S; s0 += vfr::GATHER_MAX) {
        vfr::GatherArgs a{};
        a.seg = seg; a.ctx = ctx; a.clip_off = clip_off; a.tokens = tokens;
        a.posit = posit; a.intra = intra; a.inter = inter; a.maskp = maskp; a.maskn = maskn; a.lang = lang;
        a.F = F; a.Tq = Tq; a.s0 = s0;
        const int ns = S - s0 < vfr::GATHER_MAX ? S - s0 : vfr::GATHER_MAX;
        int maxlen = 1;
        for (int s = 0; s < ns; ++s) {
            const int *q = plan_host + 7 * (s0 + s);
            a.plan[s][0] = q[0]; a.plan[s][1] = q[1];
            a.plan[s][2] = (int)((unsigned)q[2] | (unsigned)q[3] << 8 | (unsigned)q[4] << 16 | (unsigned)q[5] << 24);
            a.plan[s][3] = q[6];
            a.plan[s][4] = (int)prow; a.plan[s][5] = (int)nrow;
            prow += q[3] - q[2] + 1;
            nrow += q[5] - q[4] + 1;
            maxlen = q[3] - q[2] + 1 > maxlen ? q[3] - q[2] + 1 : maxlen;
            maxlen = q[5] - q[4] + 1 > maxlen ? q[5] - q[4] + 1 : maxlen;
        }
        hipLaunchKernelGGL(vfr::triplet_gather_kernel, dim3((unsigned)maxlen, (unsigned)ns, 3), dim3(256), 0, st, a);
        VFR_CHECK_LAUNCH("triplet_gather_kernel");
    }
    return VFR_OK;
}

size_t vfr_adam_workspace_bytes(const int64_t *numel_host, int n)
{
    if (!numel_host || n <= 0) return 256;
    return 256 + (size_t)vfr::adam_chunks(numel_host, n) * sizeof(float);
}

int vfr_adam_step_f32(int n, float *const *param_host, const float *const *grad_host, float *const *exp_avg_host,
                      float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_host, float *grad_sumsq,
                      void *workspace, size_t workspace_bytes, vfr_stream_t stream)
{
    return vfr::adam_launch(true, n, param_host, grad_host, exp_avg_host, exp_avg_sq_host, numel_host, coef_host, grad_sumsq,
                            workspace, workspace_bytes, vfr::as_stream(stream), "vfr_adam_step_f32");
}

int vfr_grad_sumsq_f32(int n, const float *const *grad_host, const int64_t *numel_host, float *grad_sumsq, void *workspace,
                       size_t workspace_bytes, vfr_stream_t stream)
{
    return vfr::adam_launch(false, n, nullptr, grad_host, nullptr, nullptr, numel_host, nullptr, grad_sumsq, workspace,
                            workspace_bytes, vfr::as_stream(stream), "vfr_grad_sumsq_f32");
}

}  // extern "C"
