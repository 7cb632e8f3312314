// The classifier head (gfx950): global average pool -> dropout -> Linear -> mean over the frames of a clip in one kernel, its backward, the
// column sum behind the bias gradients, and the stand-alone global average pool; their launchers.  Belongs here: what runs after the
// last conv of a backbone.
#include "rowwalk.h"

namespace {

// models/resnet.py:212-221 / models/sound_mobilenet_v2.py:155-158: AdaptiveAvgPool2d(1) -> Dropout -> Linear -> mean over the
// remaining frames of a clip, one workgroup per clip.  feat (the pooled, dropout-masked features) is kept for the backward.
__global__ __launch_bounds__(NT) void head_fwd_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act,
                                                      const uint8_t* keep, float inv_keep, const float* W, const float* bias, float* feat,
                                                      float* logits, int clips_per_group, int T, int HW, int C, int K) {
    const int n = blockIdx.x, g = n / clips_per_group;
    if (scale) { scale += (size_t)g * gs; shift += (size_t)g * gs; }
    const int cpr = C >> 3;
    const float inv = 1.f / (float)HW;
    for (int e = threadIdx.x; e < T * cpr; e += NT) {
        const int t = e / cpr, ch = e - t * cpr;
        const size_t row = (size_t)n * T + t;
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int p = 0; p < HW; ++p)
            acc += transform8(*reinterpret_cast<const bf16x8*>(x + (row * HW + p) * C + ch * 8), scale, shift, ch * 8, act);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = acc[i] * inv;
            if (keep) v = keep[row * C + ch * 8 + i] ? v * inv_keep : 0.f;
            feat[row * C + ch * 8 + i] = v;
        }
    }
    __syncthreads();                                     // this workgroup's feat rows are visible to all its waves
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* f = feat + (size_t)n * T * C;
    for (int k = wave; k < K; k += NT / 64) {
        float a = 0.f;
        for (int e = lane; e < T * C; e += 64) a = fmaf(f[e], W[(size_t)k * C + (e % C)], a);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) logits[(size_t)n * K + k] = a / (float)T + (bias ? bias[k] : 0.f);
    }
}

// backward of the head w.r.t. the activated input of the pool: gx[n,t,hw,c] = keep * (1/(T*HW)) * sum_k g[n,k] W[k,c];
// side output gy[n*T+t, k] = g[n,k] / T (the rows of the weight-gradient GEMM gy^T feat)
__global__ __launch_bounds__(NT) void head_bwd_kernel(const float* g, const uint8_t* keep, float inv_keep, const float* W, bf16_t* gx,
                                                      float* gy, int T, int HW, int C, int K) {
    const size_t row = blockIdx.x;                        // (clip, frame)
    const size_t n = row / T;
    const int cpr = C >> 3;
    const float sc = 1.f / ((float)T * (float)HW);
    if (gy)
        for (int k = threadIdx.x; k < K; k += NT) gy[row * K + k] = g[n * K + k] / (float)T;      // (any class count: K = 400 / 1000 heads)
    for (int ch = threadIdx.x; ch < cpr; ch += NT) {
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float gk = g[n * K + k];
            const f32x8 w = load_f32x8(W + (size_t)k * C + ch * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(gk, w[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = acc[i] * sc;
            if (keep) v = keep[row * C + ch * 8 + i] ? v * inv_keep : 0.f;
            acc[i] = v;
        }
        const bf16x8 o = f32_to_bf8(acc);
        for (int p = 0; p < HW; ++p) *reinterpret_cast<bf16x8*>(gx + (row * HW + p) * C + ch * 8) = o;
    }
}

// out[c] (+)= sum_r a[r, c]: one workgroup, rows added in order (deterministic); bias gradients of the heads
__global__ void colsum_f32_kernel(const float* a, float* out, int rows, int cols, int accumulate) {
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += a[(size_t)r * cols + c];
        out[c] = accumulate ? out[c] + s : s;
    }
}

__global__ void gap_fwd_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act, float* out, int N, int HW,
                               int C) {
    x += (size_t)blockIdx.y * N * HW * C;
    out += (size_t)blockIdx.y * N * C;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const int cpr = C >> 3;
    const int total = N * cpr;
    for (int e = blockIdx.x * NT + threadIdx.x; e < total; e += gridDim.x * NT) {
        const int ch = e % cpr, n = e / cpr;
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int p = 0; p < HW; ++p)
            acc += transform8(*reinterpret_cast<const bf16x8*>(x + ((size_t)n * HW + p) * C + ch * 8), scale, shift, ch * 8, act);
        const float inv = 1.f / (float)HW;
#pragma unroll
        for (int i = 0; i < 8; ++i) out[(size_t)n * C + ch * 8 + i] = acc[i] * inv;
    }
}

__global__ void gap_bwd_kernel(const float* g, bf16_t* gx, int N, int HW, int C) {
    const int cpr = C >> 3;
    const size_t total = (size_t)N * HW * cpr;
    const float inv = 1.f / (float)HW;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const int ch = (int)(e % cpr);
        const int n = (int)(e / ((size_t)HW * cpr));
        f32x8 v = load_f32x8(g + (size_t)n * C + ch * 8);
        v *= inv;
        *reinterpret_cast<bf16x8*>(gx + e * 8) = f32_to_bf8(v);
    }
}

}  // namespace

extern "C" int adamml_head_fwd(const void* x, const float* scale, const float* shift, int gstride, int act, const uint8_t* keep_mask,
                               float inv_keep, const float* weight, const float* bias, float* feat, float* logits, int clips, int T, int HW,
                               int C, int K, int groups, hipStream_t stream) {
    CHECK_C(C, "head_fwd");
    if (!x || !weight || !feat || !logits) return adamml_set_error(ADAMML_EINVAL, "head_fwd: null argument");
    if (groups < 1) groups = 1;
    if (clips % groups || T < 1 || HW < 1 || K < 1) return adamml_set_error(ADAMML_EINVAL, "head_fwd: clips=%d groups=%d T=%d HW=%d K=%d", clips, groups, T, HW, K);
    if (!clips) return ADAMML_OK;
    hipLaunchKernelGGL(head_fwd_kernel, dim3(clips), dim3(NT), 0, stream, (const bf16_t*)x, scale, shift, gstride, act, keep_mask, inv_keep, weight,
                       bias, feat, logits, clips / groups, T, HW, C, K);
    return adamml_check_launch("head_fwd");
}

extern "C" int adamml_head_bwd(const float* g, const uint8_t* keep_mask, float inv_keep, const float* weight, void* g_x, float* g_rows, int clips,
                               int T, int HW, int C, int K, hipStream_t stream) {
    CHECK_C(C, "head_bwd");
    if (!g || !weight || !g_x) return adamml_set_error(ADAMML_EINVAL, "head_bwd: null argument");
    if (K < 1 || T < 1 || HW < 1) return adamml_set_error(ADAMML_EINVAL, "head_bwd: T=%d HW=%d K=%d", T, HW, K);
    if (!clips) return ADAMML_OK;
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)clips * T), dim3(NT), 0, stream, g, keep_mask, inv_keep, weight, (bf16_t*)g_x, g_rows, T, HW, C, K);
    return adamml_check_launch("head_bwd");
}

extern "C" int adamml_colsum_f32(const float* a, float* out, int rows, int cols, int accumulate, hipStream_t stream) {
    if (!a || !out || rows < 0 || cols < 1) return adamml_set_error(ADAMML_EINVAL, "colsum_f32: bad arguments");
    hipLaunchKernelGGL(colsum_f32_kernel, dim3(1), dim3(256), 0, stream, a, out, rows, cols, accumulate);
    return adamml_check_launch("colsum_f32");
}

extern "C" int adamml_gap_fwd(const void* x, const float* scale, const float* shift, int gstride, int act, float* out, int N, int HW,
                              int C, int groups, hipStream_t stream) {
    CHECK_C(C, "gap_fwd");
    const size_t n = (size_t)N * (C / 8);
    if (!n) return ADAMML_OK;
    if (groups < 1) groups = 1;
    hipLaunchKernelGGL(gap_fwd_kernel, dim3(grid_for(n, 64), groups), dim3(NT), 0, stream, (const bf16_t*)x, scale, shift, gstride, act, out,
                       N, HW, C);
    return adamml_check_launch("gap_fwd");
}

extern "C" int adamml_gap_bwd(const float* g, void* g_x, int N, int HW, int C, hipStream_t stream) {
    CHECK_C(C, "gap_bwd");
    const size_t n = (size_t)N * HW * (C / 8);
    if (!n) return ADAMML_OK;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, g, (bf16_t*)g_x, N, HW, C);
    return adamml_check_launch("gap_bwd");
}
