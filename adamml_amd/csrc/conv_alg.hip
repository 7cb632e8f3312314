// Small kernels of the algebraic BatchNorm backward through a 1x1 conv z = W a (neither z nor dz is read or written) and the
// train-mode statistics of z from the Gram matrix of a (adamml_gram_stats).  The GEMMs they frame are the CAT instance of conv_gemm_kernel
// (adamml_conv_bwd_data_alg, conv_gemm.hip) or the streaming kernel of conv1x1_stream.hip, and adamml_conv_bwd_weight_grouped
// (conv_wgrad.hip) / gram.hip for the products.
#include "common.h"
#include "../../include/adamml_hip.h"

// Per-channel sum / sum of squares of z = W a over the pixels of each group WITHOUT z: sum z[co] = W[co,:] . s and
// sum z[co]^2 = W[co,:] G W[co,:]^T with the Gram matrix G = a^T a [Cin, Cin] and the column sums s [Cin] of the conv input
// (both over the pixels, fp32 from adamml_conv_bwd_weight_grouped / adamml_lazy_colsum).  W = the bf16 forward pack the conv
// multiplies with.  sums: [groups][2*Cout] plain doubles (nslots = 1 for adamml_bn_finalize).  One wave per (group, cout).
__global__ void gram_stats_kernel(const bf16_t* w, const float* G, const float* s, double* sums, int Cout, int Cin) {
    const int co = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    const bf16_t* wr = w + (size_t)co * Cin;
    const float* Gg = G + (size_t)g * Cin * Cin;
    const float* sg = s + (size_t)g * Cin;
    double a1 = 0.0, a2 = 0.0;
    for (int ci = lane; ci < Cin; ci += 64) {
        const double wi = (double)__builtin_bit_cast(float, (unsigned)wr[ci] << 16);
        // t = (G w)[ci] read down COLUMN ci of the symmetric G: the 64 lanes of a load touch two contiguous lines (row-wise every lane walked
        // its own 256-byte row: 64 lines per load instruction, 67 us per launch on the forward critical path of every fused conv3), four
        // independent partial sums so that the loads of four steps are in flight together
        const float* col = Gg + ci;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int cj = 0; cj < Cin; cj += 4) {                        // (Cin % 4 == 0: 64 / 128 / 256)
            t0 += (double)col[(size_t)cj * Cin] * (double)__builtin_bit_cast(float, (unsigned)wr[cj] << 16);
            t1 += (double)col[(size_t)(cj + 1) * Cin] * (double)__builtin_bit_cast(float, (unsigned)wr[cj + 1] << 16);
            t2 += (double)col[(size_t)(cj + 2) * Cin] * (double)__builtin_bit_cast(float, (unsigned)wr[cj + 2] << 16);
            t3 += (double)col[(size_t)(cj + 3) * Cin] * (double)__builtin_bit_cast(float, (unsigned)wr[cj + 3] << 16);
        }
        a1 += wi * (double)sg[ci];
        a2 += wi * ((t0 + t1) + (t2 + t3));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { a1 += __shfl_xor(a1, off, 64); a2 += __shfl_xor(a2, off, 64); }
    if (lane == 0) {
        sums[(size_t)g * 2 * Cout + co] = a1;
        sums[(size_t)g * 2 * Cout + Cout + co] = a2;
    }
}

extern "C" int adamml_gram_stats(const void* w_packed, const float* G, const float* s, double* sums, int Cout, int Cin, int groups,
                                 hipStream_t stream) {
    if (!w_packed || !G || !s || !sums || Cout < 1 || Cin < 4 || (Cin & 3) || groups < 1) return adamml_set_error(ADAMML_EINVAL, "gram_stats: bad arguments (Cin must be a multiple of 4)");
    hipLaunchKernelGGL(gram_stats_kernel, dim3(Cout, groups), dim3(64), 0, stream, (const bf16_t*)w_packed, G, s, sums, Cout, Cin);
    return adamml_check_launch("gram_stats");
}

// ---- algebraic BatchNorm backward through a 1x1 conv z = W a followed by a linear BatchNorm (dz = A g' + B z + C per channel):
//   dx = (W^T diag(A)) g' + (W^T diag(B) W) a + W^T C,   dW = A (.) (g'^T a) + B (.) (W G) + C (x) s,  G = a^T a, s = sum_p a
// -- neither z nor dz is read or written.  Per BatchNorm group g the data gradient is ONE GEMM over the concatenated input
// [g' | a] with the weight pack [Cin][Cout + Cin] built here, plus a constant per output channel.
__global__ void alg_pack_kernel(const float* w, const float* aff, const float* m_pre, bf16_t* wp, float* cadd, int Cout, int Cin, int groups) {
    // one thread per (group, ci, k): k < Cout -> W[k][ci] * A[k]; else M[ci][k - Cout] = sum_co W[co][ci] B[co] W[co][k - Cout]
    const int K = Cout + Cin;
    const size_t total = (size_t)groups * Cin * K;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e % K);
        const int ci = (int)((e / K) % Cin);
        const int g = (int)(e / ((size_t)K * Cin));
        const float* A = aff + (size_t)g * 3 * Cout;
        const float* B = A + Cout;
        float v;
        if (k < Cout) v = w[(size_t)k * Cin + ci] * A[k];
        else {
            const int cj = k - Cout;
            if (m_pre) v = m_pre[((size_t)g * Cin + ci) * Cin + cj];      // M_g computed by a GEMM (large Cin)
            else {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;                // (Cout % 32 == 0; split accumulators: see alg_wgrad_combine)
#pragma unroll 4
                for (int co = 0; co < Cout; co += 4) {
                    a0 = fmaf(w[(size_t)co * Cin + ci] * B[co], w[(size_t)co * Cin + cj], a0);
                    a1 = fmaf(w[(size_t)(co + 1) * Cin + ci] * B[co + 1], w[(size_t)(co + 1) * Cin + cj], a1);
                    a2 = fmaf(w[(size_t)(co + 2) * Cin + ci] * B[co + 2], w[(size_t)(co + 2) * Cin + cj], a2);
                    a3 = fmaf(w[(size_t)(co + 3) * Cin + ci] * B[co + 3], w[(size_t)(co + 3) * Cin + cj], a3);
                }
                v = (a0 + a1) + (a2 + a3);
            }
        }
        wp[e] = __builtin_bit_cast(bf16_t, (__bf16)v);
        if (k == 0) {
            const float* Cc = A + 2 * Cout;
            float acc = 0.f;
            for (int co = 0; co < Cout; ++co) acc = fmaf(w[(size_t)co * Cin + ci], Cc[co], acc);
            cadd[(size_t)g * Cin + ci] = acc;
        }
    }
}

// dW[co][ci] += sum_g  A_g[co] P_g[co][ci] + B_g[co] sum_cj W[co][cj] G_g[cj][ci] + C_g[co] s_g[ci]
__global__ void alg_wgrad_combine_kernel(const float* w, const float* aff, const float* P, const float* G, const float* wg_pre, const float* s,
                                         float* dw, int Cout, int Cin, int groups) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * Cin) return;
    const int co = e / Cin, ci = e - co * Cin;
    float acc = 0.f;
    for (int g = 0; g < groups; ++g) {
        const float* A = aff + (size_t)g * 3 * Cout;
        const float* Gg = G + (size_t)g * Cin * Cin;
        float wg = 0.f;
        if (wg_pre) wg = wg_pre[(size_t)co * groups * Cin + (size_t)g * Cin + ci];        // (W G_g) computed by a GEMM (large Cin)
        else {
            // (unrolled with split accumulators: one dependent L2 round trip per cj made this 0.2 ms per layer-2 block)
            float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
            const float* wr = w + (size_t)co * Cin;
#pragma unroll 4
            for (int cj = 0; cj < Cin; cj += 4) {
                w0 = fmaf(wr[cj], Gg[(size_t)cj * Cin + ci], w0);
                w1 = fmaf(wr[cj + 1], Gg[(size_t)(cj + 1) * Cin + ci], w1);
                w2 = fmaf(wr[cj + 2], Gg[(size_t)(cj + 2) * Cin + ci], w2);
                w3 = fmaf(wr[cj + 3], Gg[(size_t)(cj + 3) * Cin + ci], w3);
            }
            wg = (w0 + w1) + (w2 + w3);
        }
        acc += A[co] * P[((size_t)g * Cout + co) * Cin + ci] + A[Cout + co] * wg + A[2 * Cout + co] * s[(size_t)g * Cin + ci];
    }
    dw[e] += acc;
}

// Second BatchNorm-backward moment from the algebraic identity  sum_p g'[p,co] z[p,co] = sum_cj W[co,cj] (g'^T a)[co,cj]  (z = W a):
// sums [groups][SLOTS][2C] holds sum(g') in its first halves (epilogues run with z == NULL leave the second halves zero);
// writes sum(g' zhat) = invstd (sum_j W (.) P - mean * sum g') into slot 0 of the second half.
__global__ void alg_sumfix_kernel(const float* w, const float* P, const float* vec, double* sums, int Cout, int Cin, int groups) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * groups) return;
    const int g = e / Cout, co = e - g * Cout;
    double* sg = sums + (size_t)g * ADAMML_STAT_SLOTS * 2 * Cout;
    double s1 = 0.0;
    s1 = det_decode(sg + co, 2 * (size_t)Cout);
    const float* Pg = P + ((size_t)g * Cout + co) * Cin;
    double dot = 0.0;
    for (int cj = 0; cj < Cin; ++cj) dot += (double)w[(size_t)co * Cin + cj] * (double)Pg[cj];
    const float* v = vec + (size_t)g * 4 * Cout;
    const double r = (double)v[3 * Cout + co] * (dot - (double)v[2 * Cout + co] * s1);
    det_encode(sg + Cout + co, 2 * (size_t)Cout, r);
}

extern "C" int adamml_alg_sumfix(const float* w, const float* P, const float* vec, double* sums, int Cout, int Cin, int groups,
                                 hipStream_t stream) {
    if (!w || !P || !vec || !sums) return adamml_set_error(ADAMML_EINVAL, "alg_sumfix: null argument");
    hipLaunchKernelGGL(alg_sumfix_kernel, dim3(ceil_div(Cout * groups, 128)), dim3(128), 0, stream, w, P, vec, sums, Cout, Cin, groups);
    return adamml_check_launch("alg_sumfix");
}

extern "C" int adamml_alg_pack(const float* w, const float* aff, const float* m_pre, void* w_alg, float* epi_add, int Cout, int Cin,
                               int groups, hipStream_t stream) {
    if (!w || !aff || !w_alg || !epi_add || Cout < 1 || Cin < 1 || groups < 1) return adamml_set_error(ADAMML_EINVAL, "alg_pack: bad arguments");
    if (Cout % 4) return adamml_set_error(ADAMML_EUNSUPPORTED, "alg_pack: Cout must be a multiple of 4");
    const size_t total = (size_t)groups * Cin * (Cout + Cin);
    hipLaunchKernelGGL(alg_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, aff, m_pre, (bf16_t*)w_alg, epi_add, Cout, Cin, groups);
    return adamml_check_launch("alg_pack");
}

extern "C" int adamml_alg_wgrad_combine(const float* w, const float* aff, const float* P, const float* G, const float* wg_pre, const float* s,
                                        float* dw, int Cout, int Cin, int groups, hipStream_t stream) {
    if (!w || !aff || !P || (!G && !wg_pre) || !s || !dw) return adamml_set_error(ADAMML_EINVAL, "alg_wgrad_combine: null argument");
    if (Cin % 4 || Cout % 4) return adamml_set_error(ADAMML_EUNSUPPORTED, "alg_wgrad_combine: Cin and Cout must be multiples of 4");
    hipLaunchKernelGGL(alg_wgrad_combine_kernel, dim3(ceil_div(Cout * Cin, 256)), dim3(256), 0, stream, w, aff, P, G, wg_pre, s, dw, Cout, Cin, groups);
    return adamml_check_launch("alg_wgrad_combine");
}
