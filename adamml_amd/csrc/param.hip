// Kernels over the parameters (gfx950): packing conv weights into the layouts the conv kernels read, and the SGD / Adam steps; their
// launchers.  Belongs here: a kernel whose operands are weights, gradients of weights or optimizer state.
#include "rowwalk.h"

namespace {

// ------------------------------------------------------------------------------------------------ weights
__device__ __forceinline__ void pack_one(const float* w, void* out, int cout, int cin_true, int cin_pad, int taps, int mode, size_t e) {
    if (mode == 0) {            // [co][tap][ci]
        const int ci = (int)(e % cin_pad);
        const int tap = (int)((e / cin_pad) % taps);
        const int co = (int)(e / ((size_t)cin_pad * taps));
        float v = ci < cin_true ? w[((size_t)co * cin_true + ci) * taps + tap] : 0.f;
        reinterpret_cast<__bf16*>(out)[e] = (__bf16)v;
    } else if (mode == 1) {     // [ci][tap flipped][co]
        const int co = (int)(e % cout);
        const int tap = (int)((e / cout) % taps);
        const int ci = (int)(e / ((size_t)cout * taps));
        float v = ci < cin_true ? w[((size_t)co * cin_true + ci) * taps + (taps - 1 - tap)] : 0.f;
        reinterpret_cast<__bf16*>(out)[e] = (__bf16)v;
    } else {                    // depthwise [tap][c] fp32
        const int c = (int)(e % cout);
        const int tap = (int)(e / cout);
        reinterpret_cast<float*>(out)[e] = w[(size_t)c * taps + tap];
    }
}

// All weight packs of a backbone in ONE launch (they were ~190 launches of ~5 us at the head of every training step, on the
// critical path of each stream).  table: n rows of 6 x int64 {w, out, cout | cin_true << 32, cin_pad | kh << 32,
// kw | mode << 32, first block}; a block of PACK_EPB elements finds its row by binary search over the first-block column.
constexpr int PACK_EPB = 2048;
__global__ __launch_bounds__(NT) void pack_conv_weights_batched_kernel(const long long* table, int n) {
    int lo = 0, hi = n - 1;
    const long long b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * 6 + 5] <= b) lo = mid; else hi = mid - 1;
    }
    const long long* row = table + (size_t)lo * 6;
    const float* w = reinterpret_cast<const float*>(row[0]);
    void* out = reinterpret_cast<void*>(row[1]);
    const int cout = (int)(row[2] & 0xffffffff), cin_true = (int)(row[2] >> 32), cin_pad = (int)(row[3] & 0xffffffff), kh = (int)(row[3] >> 32),
              kw = (int)(row[4] & 0xffffffff), mode = (int)(row[4] >> 32);
    const int taps = kh * kw;
    const size_t total = mode == 2 ? (size_t)taps * cout : (size_t)cout * taps * cin_pad;
    const size_t e0 = (size_t)(b - row[5]) * PACK_EPB;
    for (size_t e = e0 + threadIdx.x; e < e0 + PACK_EPB && e < total; e += NT) pack_one(w, out, cout, cin_true, cin_pad, taps, mode, e);
}

__global__ void pack_conv_weight_kernel(const float* w, void* out, int cout, int cin_true, int cin_pad, int kh, int kw, int mode) {
    const int taps = kh * kw;
    const size_t total = mode == 2 ? (size_t)taps * cout : (size_t)cout * taps * cin_pad;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        pack_one(w, out, cout, cin_true, cin_pad, taps, mode, e);
    }
}

// ------------------------------------------------------------------------------------------------ optimizers
__global__ void sgd_step_kernel(float* p, const float* g, float* mom, size_t n, float lr, float momentum, float wd,
                                int nesterov, int first) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        float d = g[i] + wd * p[i];
        if (momentum != 0.f) {
            float b = first ? d : momentum * mom[i] + d;
            mom[i] = b;
            d = nesterov ? d + momentum * b : b;
        }
        p[i] -= lr * d;
    }
}

__global__ void adam_step_kernel(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                                 float eps, float wd, float bc1, float bc2) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        float d = g[i] + wd * p[i];
        float mi = b1 * m[i] + (1.f - b1) * d;
        float vi = b2 * v[i] + (1.f - b2) * d * d;
        m[i] = mi;
        v[i] = vi;
        float denom = sqrtf(vi) / sqrtf(bc2) + eps;
        p[i] -= (lr / bc1) * mi / denom;
    }
}

}  // namespace

extern "C" int adamml_pack_conv_weight(const float* w, void* out, int cout, int cin_true, int cin_pad, int kh, int kw, int mode,
                                       hipStream_t stream) {
    if (mode < 0 || mode > 2) return adamml_set_error(ADAMML_EINVAL, "pack_conv_weight: mode %d", mode);
    const size_t n = mode == 2 ? (size_t)kh * kw * cout : (size_t)cout * kh * kw * cin_pad;
    if (!n) return ADAMML_OK;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, w, out, cout, cin_true, cin_pad, kh, kw, mode);
    return adamml_check_launch("pack_conv_weight");
}

extern "C" int adamml_pack_conv_weights_batched(const int64_t* table, int n, int64_t total_blocks, hipStream_t stream) {
    if (!table || n < 1 || total_blocks < 1) return adamml_set_error(ADAMML_EINVAL, "pack_conv_weights_batched: bad arguments");
    hipLaunchKernelGGL(pack_conv_weights_batched_kernel, dim3((unsigned)total_blocks), dim3(NT), 0, stream, (const long long*)table, n);
    return adamml_check_launch("pack_conv_weights_batched");
}

extern "C" int adamml_pack_block_elems(void) { return PACK_EPB; }

extern "C" int adamml_sgd_step(float* p, const float* g, float* mom, size_t n, float lr, float momentum, float weight_decay,
                               int nesterov, int first_step, hipStream_t stream) {
    if (!n) return ADAMML_OK;
    hipLaunchKernelGGL(sgd_step_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, p, g, mom, n, lr, momentum, weight_decay, nesterov,
                       first_step);
    return adamml_check_launch("sgd_step");
}

extern "C" int adamml_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, hipStream_t stream) {
    if (!n) return ADAMML_OK;
    // bias corrections in double: 1 - powf(beta2, step) in fp32 cancels (beta2 = 0.999, step 2: half an ulp of the power near 1 is
    // 1.5e-5 of bc2); the kernel receives them rounded once to fp32, as before
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step)), bc2 = (float)(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                       bc1, bc2);
    return adamml_check_launch("adam_step");
}
