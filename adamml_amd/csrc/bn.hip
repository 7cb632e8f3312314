// BatchNorm finalize / apply / backward and the residual-add backward (gfx950): HBM-bound row walkers -- 16 B per lane (8 bf16 channels of
// one NHWC pixel), per-channel reductions staged through LDS and published exactly (rowwalk.h) -- and the small per-channel kernels
// between them, each with its launcher.  Belongs here: a kernel whose whole job is a BatchNorm statistic, vector or gradient.
#include "rowwalk.h"

namespace {

// Every BatchNorm-related kernel below is batched over `groups` (blockIdx.y or an in-kernel loop): tensors are
// [groups][P][C], statistic accumulators [groups][nslots][2C], BatchNorm vectors vec = [groups][4][C]
// (scale, shift, mean, invstd), backward coefficients coef = [groups][3][C].
__global__ void stats_collapse_kernel(const double* stats, double* out, int C, int groups) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * C * groups) return;
    const int g = i / (2 * C), j = i - g * 2 * C;
    // the 32 slot (or deterministic-bin) values are folded in the order of the xor-butterfly of slot_sums_groups (16, 8, 4, 2, 1):
    // a collapsed vector fed to the finalize kernels with nslots = 1 then yields bit for bit what they compute from the 32 slots
    // themselves -- a SyncBatchNorm step over ONE rank equals the plain step exactly (tests/test_rccl_gpu.py)
    double v[ADAMML_STAT_SLOTS];
    const double* st = stats + (size_t)g * ADAMML_STAT_SLOTS * 2 * C + j;
#pragma unroll
    for (int k = 0; k < ADAMML_STAT_SLOTS; ++k) v[k] = det_bin_value(st, 2 * (size_t)C, k);
#pragma unroll
    for (int off = ADAMML_STAT_SLOTS / 2; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < off; ++k) v[k] += v[k + off];
    out[i] = v[0];
}

// one 32-lane group per channel: lane k reads slot k, the group folds with xor-shuffles (slot-parallel loads).
// Slot sums of up to 32 groups at once: the loads of all groups are in flight together (eight groups per batch: the S = 5 segments of the
// benchmark are ONE batch -- with four per batch the second, one-group batch was a second dependent round trip in each of the step's 314
// finalize launches), every lane of the 32-lane channel group ends up holding the sums of group g0 + k in (m1, m2): the per-group
// arithmetic that follows (fp64 divisions, square root) then runs one group per lane instead of one after the other on the lead lane.
__device__ __forceinline__ void slot_sums_groups(const double* stats, int nslots, int C, int c, int k, int g0, int groups, double& m1, double& m2) {
    m1 = 0.0; m2 = 0.0;
    const int ge = groups - g0 < 32 ? groups : g0 + 32;
    constexpr int GB = 8;
    for (int g = g0; g < ge; g += GB) {
        double a1[GB], a2[GB];
        const int nb = ge - g < GB ? ge - g : GB;           // (uniform)
#pragma unroll
        for (int j = 0; j < GB; ++j) {
            a1[j] = 0.0; a2[j] = 0.0;
            if (j < nb && c < C && k < nslots) {
                const double* st = stats + (size_t)(g + j) * nslots * 2 * C;
                if (nslots == ADAMML_STAT_SLOTS) {              // integer bins; nslots == 1: plain doubles (collapsed / all-reduced sums)
                    a1[j] = det_bin_value(st + c, 2 * (size_t)C, k);
                    a2[j] = det_bin_value(st + C + c, 2 * (size_t)C, k);
                } else {
                    a1[j] = st[(size_t)k * 2 * C + c];
                    a2[j] = st[(size_t)k * 2 * C + C + c];
                }
            }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
#pragma unroll
            for (int j = 0; j < GB; ++j) {
                if (j < nb) {
                    a1[j] += __shfl_xor(a1[j], off, 64);
                    a2[j] += __shfl_xor(a2[j], off, 64);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < GB; ++j)
            if (j < nb && k == g + j - g0) { m1 = a1[j]; m2 = a2[j]; }
    }
}

// The running statistics see the groups IN ORDER (the reference updates them once per segment call): lane g of a channel's
// 32-lane group finalises group g, the lead lane then folds the groups' (mean, unbiased variance) in order.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* stats, int nslots, int groups, double count, const float* gamma, const float* beta,
                                   float* rm, float* rv, float momentum, float eps, float* vec, int C) {
    const int c = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5), k = threadIdx.x & 31;
    float rmean = 0.f, rvar = 0.f;
    const bool lead = c < C && k == 0;
    if (lead && rm) { rmean = rm[c]; rvar = rv[c]; }
    float ga = 0.f, be = 0.f;
    if (c < C) { ga = gamma[c]; be = beta[c]; }
    for (int g0 = 0; g0 < groups; g0 += 32) {
        double s1, s2;
        slot_sums_groups(stats, nslots, C, c, k, g0, groups, s1, s2);
        const int g = g0 + k;
        double mu = s1 / count;
        double var = s2 / count - mu * mu;
        if (var < 0.0) var = 0.0;
        float is = (float)(1.0 / sqrt(var + (double)eps));
        float sc = ga * is;
        if (c < C && g < groups) {
            float* v = vec + (size_t)g * 4 * C;
            v[c] = sc;
            v[C + c] = be - (float)mu * sc;
            v[2 * C + c] = (float)mu;
            v[3 * C + c] = is;
        }
        double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        const float muf = (float)mu, unf = (float)unbiased;
        const int ng = groups - g0 < 32 ? groups - g0 : 32, base = threadIdx.x & 32;
        for (int j = 0; j < ng; ++j) {
            rmean = (1.f - momentum) * rmean + momentum * __shfl(muf, base + j, 64);
            rvar = (1.f - momentum) * rvar + momentum * __shfl(unf, base + j, 64);
        }
    }
    if (lead && rm) { rm[c] = rmean; rv[c] = rvar; }
}

__global__ void bn_eval_affine_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                      float* scale, float* shift, int C) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
}

// Row-walking elementwise kernels: a thread keeps ONE 8-channel chunk for all its pixels (ChanMap), so the per-channel
// BatchNorm vectors are loaded into registers once per thread instead of once per 16 B of activation traffic (the
// per-element form issued 14 cached vector loads per 2 streaming loads and ran at ~3.5 TB/s; this form streams at ~6).
template <bool STREAM>
__global__ __launch_bounds__(NT) void bn_act_add_kernel(const bf16_t* z, const float* scale, const float* shift, int z_gs, int act,
                                                        const bf16_t* idn, const float* id_scale, const float* id_shift, int id_gs,
                                                        bf16_t* out, uint8_t* mask_out, size_t P, int C, size_t ppb) {
    const size_t goff = (size_t)blockIdx.y * P * C;
    z += goff; out += goff;
    if (idn) idn += goff;
    if (mask_out) mask_out += goff >> 3;
    ChanMap m(C, threadIdx.x);
    if (!m.active) return;
    const int c = m.chunk * 8;
    f32x8 sc, sh, isc, ish;
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = 1.f; sh[i] = 0.f; isc[i] = 1.f; ish[i] = 0.f; }
    if (scale) { sc = load_f32x8(scale + (size_t)blockIdx.y * z_gs + c); sh = load_f32x8(shift + (size_t)blockIdx.y * z_gs + c); }
    if (idn && id_scale) { isc = load_f32x8(id_scale + (size_t)blockIdx.y * id_gs + c); ish = load_f32x8(id_shift + (size_t)blockIdx.y * id_gs + c); }
    const float lo = act_lo(act), hi = act_hi(act);
    const size_t pb = (size_t)blockIdx.x * ppb;
    const size_t pe = pb + ppb < P ? pb + ppb : P;
    auto row = [&](size_t p, bf16x8 zraw, bf16x8 iraw) {
        f32x8 v = bf8_to_f32(zraw);
        if (idn) {
            const f32x8 w = bf8_to_f32(iraw);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = clamp_act(fmaf(v[i], sc[i], sh[i]) + fmaf(w[i], isc[i], ish[i]), lo, hi);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = clamp_act(fmaf(v[i], sc[i], sh[i]), lo, hi);
        }
        if (STREAM) __builtin_nontemporal_store(f32_to_bf8(v), reinterpret_cast<bf16x8*>(out + p * C + c));
        else *reinterpret_cast<bf16x8*>(out + p * C + c) = f32_to_bf8(v);
        if (mask_out) {
            // act'(out) of the STORED value, one bit per element: the residual backward (adamml_conv_bwd_data_res) reads
            // 1/16 of the bytes it would read from `out`
            const f32x8 r = bf8_to_f32(f32_to_bf8(v));
            unsigned bits = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) bits |= (r[i] > lo && r[i] < hi) ? (1u << i) : 0u;
            mask_out[(p * C + c) >> 3] = (uint8_t)bits;
        }
    };
    auto ld = [&](const bf16_t* base, size_t p) {
        return STREAM ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(base + p * C + c)) : *reinterpret_cast<const bf16x8*>(base + p * C + c);
    };
    constexpr int U = 4;                                  // rows in flight per thread (one-shot workgroups: see one_shot_grid)
    const size_t step = m.rows_per_pass;
    size_t p = pb + m.rslot;
    for (; p + (U - 1) * step < pe; p += U * step) {
        bf16x8 zr[U], ir[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            zr[u] = ld(z, p + u * step);
            ir[u] = idn ? ld(idn, p + u * step) : zr[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(p + u * step, zr[u], ir[u]);
    }
    for (; p < pe; p += step) row(p, ld(z, p), idn ? ld(idn, p) : bf16x8{});
}

__global__ void act_bwd_from_output_kernel(const bf16_t* g_out, const bf16_t* out, int act, bf16_t* g, size_t nchunks) {
    const float lo = act_lo(act), hi = act_hi(act);
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < nchunks; e += (size_t)gridDim.x * NT) {
        f32x8 gv = bf8_to_f32(*reinterpret_cast<const bf16x8*>(g_out + e * 8));
        f32x8 ov = bf8_to_f32(*reinterpret_cast<const bf16x8*>(out + e * 8));
#pragma unroll
        for (int i = 0; i < 8; ++i) gv[i] *= mask_act(ov[i], lo, hi);
        *reinterpret_cast<bf16x8*>(g + e * 8) = f32_to_bf8(gv);
    }
}

__global__ __launch_bounds__(NT) void bn_bwd_reduce_kernel(const bf16_t* g, const bf16_t* z, const float* vec, int act, double* sums,
                                                           size_t P, int C, size_t ppb) {
    __shared__ float smem[2 * MAXC];
    g += (size_t)blockIdx.y * P * C;
    z += (size_t)blockIdx.y * P * C;
    vec += (size_t)blockIdx.y * 4 * C;
    sums += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C;
    ChanMap m(C, threadIdx.x);
    float s[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = q[i] = 0.f;
    const size_t pb = (size_t)blockIdx.x * ppb;
    const size_t pe = pb + ppb < P ? pb + ppb : P;
    if (m.active) {
        const int c = m.chunk * 8;
        f32x8 sc = load_f32x8(vec + c), sh = load_f32x8(vec + C + c), mu = load_f32x8(vec + 2 * C + c), is = load_f32x8(vec + 3 * C + c);
        const float lo = act_lo(act), hi = act_hi(act);
        for (size_t p = pb + m.rslot; p < pe; p += m.rows_per_pass) {
            f32x8 gv = bf8_to_f32(*reinterpret_cast<const bf16x8*>(g + p * C + c));
            f32x8 zv = bf8_to_f32(*reinterpret_cast<const bf16x8*>(z + p * C + c));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float gp = gv[i] * mask_act(fmaf(zv[i], sc[i], sh[i]), lo, hi);
                s[i] += gp;
                q[i] += gp * (zv[i] - mu[i]) * is[i];
            }
        }
    }
    block_channel_publish(s, q, m, smem, C, sums);
}

// Residual-add backward (models/resnet.py:110-111 / sound_mobilenet_v2.py:67): g2 = g_out * act'(out), plus the
// BatchNorm-backward sums of the one or two lazily normalised operands of the add (bn3 and, in the first block of a
// stage, the downsample BN) in the same pass over g_out / out.
template <bool STREAM>
__global__ __launch_bounds__(NT) void residual_bwd_kernel(const bf16_t* g_out, const bf16_t* out, int act, bf16_t* g2,
                                                          const bf16_t* za, const float* veca, double* sumsa,
                                                          const bf16_t* zb, const float* vecb, double* sumsb,
                                                          size_t P, int C, size_t ppb) {
    __shared__ float smem[2 * MAXC];
    {
        const size_t goff = (size_t)blockIdx.y * P * C;
        g_out += goff; out += goff; g2 += goff;
        if (za) { za += goff; veca += (size_t)blockIdx.y * 4 * C; sumsa += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C; }
        if (zb) { zb += goff; vecb += (size_t)blockIdx.y * 4 * C; sumsb += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C; }
    }
    ChanMap m(C, threadIdx.x);
    float sa[8], qa[8], sb[8], qb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = qa[i] = sb[i] = qb[i] = 0.f;
    const size_t pb = (size_t)blockIdx.x * ppb;
    const size_t pe = pb + ppb < P ? pb + ppb : P;
    if (m.active) {
        const int c = m.chunk * 8;
        f32x8 mua, isa, mub, isb;
        if (za) { mua = load_f32x8(veca + 2 * C + c); isa = load_f32x8(veca + 3 * C + c); }
        if (zb) { mub = load_f32x8(vecb + 2 * C + c); isb = load_f32x8(vecb + 3 * C + c); }
        const float lo = act_lo(act), hi = act_hi(act);
        for (size_t p = pb + m.rslot; p < pe; p += m.rows_per_pass) {
            auto ld = [](const bf16_t* q) {
                return STREAM ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(q)) : *reinterpret_cast<const bf16x8*>(q);
            };
            f32x8 gv = bf8_to_f32(ld(g_out + p * C + c));
            const f32x8 ov = bf8_to_f32(ld(out + p * C + c));
#pragma unroll
            for (int i = 0; i < 8; ++i) gv[i] *= mask_act(ov[i], lo, hi);
            const bf16x8 gb = f32_to_bf8(gv);
            if (g2 != g_out || act != ACT_NONE) {
                if (STREAM) __builtin_nontemporal_store(gb, reinterpret_cast<bf16x8*>(g2 + p * C + c));
                else *reinterpret_cast<bf16x8*>(g2 + p * C + c) = gb;
            }
            gv = bf8_to_f32(gb);
            if (za) {
                const f32x8 zv = bf8_to_f32(ld(za + p * C + c));
#pragma unroll
                for (int i = 0; i < 8; ++i) { sa[i] += gv[i]; qa[i] += gv[i] * (zv[i] - mua[i]) * isa[i]; }
            }
            if (zb) {
                const f32x8 zv = bf8_to_f32(ld(zb + p * C + c));
#pragma unroll
                for (int i = 0; i < 8; ++i) { sb[i] += gv[i]; qb[i] += gv[i] * (zv[i] - mub[i]) * isb[i]; }
            }
        }
    }
    if (za) block_channel_publish(sa, qa, m, smem, C, sumsa);
    if (zb) {
        __syncthreads();
        block_channel_publish(sb, qb, m, smem, C, sumsb);
    }
}

__global__ void bn_bwd_finalize_kernel(const double* sums, int nslots, int groups, double count, const float* gamma, const float* vec,
                                       float* dgamma, float* dbeta, float* coef, float* aff, int C, float grad_scale) {
    const int c = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5), k = threadIdx.x & 31;
    const bool lead = c < C && k == 0;
    float dg = 0.f, db = 0.f;
    for (int g0 = 0; g0 < groups; g0 += 32) {           // lane g: coefficients of group g; lead lane: dgamma / dbeta over the groups in order
        double sg, sgz;
        slot_sums_groups(sums, nslots, C, c, k, g0, groups, sg, sgz);
        const int g = g0 + k;
        if (c < C && g < groups) {
            float* cf = coef + (size_t)g * 3 * C;
            const float* v = vec + (size_t)g * 4 * C;
            const float k0 = gamma[c] * v[3 * C + c], k1 = (float)(sg / count), k2 = (float)(sgz / count);
            cf[c] = k0;
            cf[C + c] = k1;
            cf[2 * C + c] = k2;
            if (aff) {               // dz = A g' + B z + C of bn_bwd_affine_kernel in the same launch (same expressions on the same fp32 values)
                const float mu = v[2 * C + c], is = v[3 * C + c];
                float* a = aff + (size_t)g * 3 * C;
                a[c] = k0;
                a[C + c] = -k0 * k2 * is;
                a[2 * C + c] = k0 * (k2 * mu * is - k1);
            }
        }
        const float sgf = (float)sg, sgzf = (float)sgz;
        const int ng = groups - g0 < 32 ? groups - g0 : 32, base = threadIdx.x & 32;
        for (int j = 0; j < ng; ++j) {
            dg += __shfl(sgzf, base + j, 64);
            db += __shfl(sgf, base + j, 64);
        }
    }
    if (lead) {
        if (dgamma) dgamma[c] += dg * grad_scale;
        if (dbeta) dbeta[c] += db * grad_scale;
    }
}

// dz = k0 (g' - k1 - zhat k2), zhat = (z - mu) invstd  ==  A g' + B z + C  per channel: the form the dual-source loader of
// the 1x1 data gradient applies (adamml_conv_bwd_data_dual).  coef [G][3][C], vec [G][4][C] -> aff [G][3][C].
__global__ void bn_bwd_affine_kernel(const float* coef, const float* vec, float* aff, int C, int groups) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * groups) return;
    const int g = i / C, c = i - g * C;
    const float* cf = coef + (size_t)g * 3 * C;
    const float* v = vec + (size_t)g * 4 * C;
    const float k0 = cf[c], k1 = cf[C + c], k2 = cf[2 * C + c], mu = v[2 * C + c], is = v[3 * C + c];
    float* a = aff + (size_t)g * 3 * C;
    a[c] = k0;
    a[C + c] = -k0 * k2 * is;
    a[2 * C + c] = k0 * (k2 * mu * is - k1);
}

// s[g][c] = sum over the pixels of group g of act(scale x + shift)  (column sums of a lazily normalised activation: the
// C (x) s term of the algebraic BatchNorm backward).  Row walker; fp32 atomics of per-workgroup partials (s zeroed here).
__global__ __launch_bounds__(NT) void lazy_colsum_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act, float* s,
                                                         size_t P, int C, size_t ppb) {
    __shared__ float smem[MAXC];
    x += (size_t)blockIdx.y * P * C;
    s += (size_t)blockIdx.y * C;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    ChanMap m(C, threadIdx.x);
    for (int i = threadIdx.x; i < C; i += NT) smem[i] = 0.f;
    __syncthreads();
    float accd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m.active) {
        const int c = m.chunk * 8;
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        const size_t pb = (size_t)blockIdx.x * ppb;
        const size_t pe = pb + ppb < P ? pb + ppb : P;
        // (rounded to bf16 like the operand the conv kernels stage: s is then the exact column sum of what the MFMAs multiply)
        for (size_t p = pb + m.rslot; p < pe; p += m.rows_per_pass)
            acc += bf8_to_f32(f32_to_bf8(transform8(*reinterpret_cast<const bf16x8*>(x + p * C + c), scale, shift, c, act)));
#pragma unroll
        for (int i = 0; i < 8; ++i) accd[i] = acc[i];
    }
    {
        // one workgroup per group (see the launcher); the row slots add in turn, in a fixed order
        for (int r = 0; r < m.rows_per_pass; ++r) {
            if (m.active && m.rslot == r) {
#pragma unroll
                for (int i = 0; i < 8; ++i) smem[m.chunk * 8 + i] += accd[i];
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += NT) atomicAdd(&s[i], smem[i]);
}

// STREAM: the tensors are larger than the 256 MB Infinity Cache -> non-temporal accesses (nothing is re-used from cache);
// smaller tensors keep default caching so that the consumers of dz (data / weight gradient) still find it in L2 / MALL.
template <bool STREAM, int U>
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(const bf16_t* g, const bf16_t* z, const float* vec, int act, const float* coef,
                                                          bf16_t* dz, size_t P, int C, size_t ppb) {
    {
        const size_t goff = (size_t)blockIdx.y * P * C;
        g += goff; z += goff; dz += goff;
        vec += (size_t)blockIdx.y * 4 * C;
        coef += (size_t)blockIdx.y * 3 * C;
    }
    ChanMap m(C, threadIdx.x);
    if (!m.active) return;
    const int c = m.chunk * 8;
    const f32x8 sc = load_f32x8(vec + c), sh = load_f32x8(vec + C + c), mu = load_f32x8(vec + 2 * C + c), is = load_f32x8(vec + 3 * C + c);
    const f32x8 k0 = load_f32x8(coef + c), k1 = load_f32x8(coef + C + c), k2 = load_f32x8(coef + 2 * C + c);
    const float lo = act_lo(act), hi = act_hi(act);
    const size_t pb = (size_t)blockIdx.x * ppb;
    const size_t pe = pb + ppb < P ? pb + ppb : P;
    auto one = [&](bf16x8 graw, bf16x8 zraw) {
        const f32x8 gv = bf8_to_f32(graw), zv = bf8_to_f32(zraw);
        f32x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float gp = gv[i] * mask_act(fmaf(zv[i], sc[i], sh[i]), lo, hi);
            float zh = (zv[i] - mu[i]) * is[i];
            o[i] = k0[i] * (gp - k1[i] - zh * k2[i]);
        }
        return f32_to_bf8(o);
    };
    const size_t step = m.rows_per_pass;
    size_t p = pb + m.rslot;
    for (; p + (U - 1) * step < pe; p += U * step) {            // U rows (2 U loads) in flight per thread
        bf16x8 gr[U], zr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bf16x8* gp = reinterpret_cast<const bf16x8*>(g + (p + u * step) * C + c);
            const bf16x8* zp = reinterpret_cast<const bf16x8*>(z + (p + u * step) * C + c);
            if (STREAM) { gr[u] = __builtin_nontemporal_load(gp); zr[u] = __builtin_nontemporal_load(zp); }
            else { gr[u] = *gp; zr[u] = *zp; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bf16x8* op = reinterpret_cast<bf16x8*>(dz + (p + u * step) * C + c);
            if (STREAM) __builtin_nontemporal_store(one(gr[u], zr[u]), op);
            else *op = one(gr[u], zr[u]);
        }
    }
    for (; p < pe; p += step) *reinterpret_cast<bf16x8*>(dz + p * C + c) = one(*reinterpret_cast<const bf16x8*>(g + p * C + c),
                                                                                 *reinterpret_cast<const bf16x8*>(z + p * C + c));
}

}  // namespace

extern "C" int adamml_stats_collapse(const double* stats, double* out, int C, int groups, hipStream_t stream) {
    if (!stats || !out) return adamml_set_error(ADAMML_EINVAL, "stats_collapse: null argument");
    hipLaunchKernelGGL(stats_collapse_kernel, dim3(ceil_div(2 * C * groups, 128)), dim3(128), 0, stream, stats, out, C, groups);
    return adamml_check_launch("stats_collapse");
}

extern "C" int adamml_bn_finalize(const double* stats, int nslots, int groups, double count, const float* gamma, const float* beta,
                                  float* rm, float* rv, float momentum, float eps, float* vec, int C, hipStream_t stream) {
    if (!stats || !gamma || !beta || !vec) return adamml_set_error(ADAMML_EINVAL, "bn_finalize: null argument");
    if (nslots < 1 || nslots > ADAMML_STAT_SLOTS || groups < 1) return adamml_set_error(ADAMML_EINVAL, "bn_finalize: nslots=%d groups=%d", nslots, groups);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 8)), dim3(256), 0, stream, stats, nslots, groups, count, gamma, beta, rm, rv,
                       momentum, eps, vec, C);
    return adamml_check_launch("bn_finalize");
}

extern "C" int adamml_bn_eval_affine(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                     float* scale, float* shift, int C, hipStream_t stream) {
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(ceil_div(C, 128)), dim3(128), 0, stream, gamma, beta, rm, rv, eps, scale, shift, C);
    return adamml_check_launch("bn_eval_affine");
}

// One-shot workgroups (bn_act_add, bn_bwd_apply): every thread loads U = 4 rows of (g, z), stores them and (for tensors beyond 512 MB)
// retires -- 6.2-6.4 TB/s against 5.3-5.5 for the long row walk (>= 16 rows per thread, <= 8192 workgroups) and 6.05 for torch's add on
// the same tensors: with nothing to amortise (the 7 per-channel vectors are 28 cached loads per thread) the short-lived form keeps more
// requests in flight across workgroup turnover.  Measured (tools/bench_elementwise.py): U / rows per thread 2/2 5.0, 4/4 6.2, 4/8 5.9-6.4,
// 8/8 5.8-6.3, 8/16 5.1-5.7 TB/s; default caching instead of non-temporal accesses: -4 %.
static RowGrid one_shot_grid(size_t P, int C, int groups, bool retire_beyond_512mb = true) {
    const size_t ppb = (size_t)rows_per_pass(C) * (retire_beyond_512mb && tensor_bytes(P, C, groups) > ((size_t)512 << 20) ? 4 : 8);
    return {ppb, (P + ppb - 1) / ppb};
}

extern "C" int adamml_bn_act_add_mask(const void* z, const float* scale, const float* shift, int z_gstride, int act, const void* idn,
                                      const float* id_scale, const float* id_shift, int id_gstride, void* out, uint8_t* mask_out,
                                      size_t P, int C, int groups, hipStream_t stream) {
    CHECK_C(C, "bn_act_add");
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = one_shot_grid(P, C, groups, idn != nullptr);      // (two-pass form: 8 rows)
    dispatch_bool(exceeds_infinity_cache(P, C, groups), [&](auto nt) {
        hipLaunchKernelGGL(bn_act_add_kernel<decltype(nt)::value>, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)z, scale, shift,
                           z_gstride, act, (const bf16_t*)idn, id_scale, id_shift, id_gstride, (bf16_t*)out, mask_out, P, C, rg.ppb);
    });
    return adamml_check_launch("bn_act_add");
}

extern "C" int adamml_bn_act_add(const void* z, const float* scale, const float* shift, int z_gstride, int act, const void* idn,
                                 const float* id_scale, const float* id_shift, int id_gstride, void* out, size_t P, int C, int groups,
                                 hipStream_t stream) {
    return adamml_bn_act_add_mask(z, scale, shift, z_gstride, act, idn, id_scale, id_shift, id_gstride, out, nullptr, P, C, groups, stream);
}

extern "C" int adamml_act_bwd_from_output(const void* g_out, const void* out, int act, void* g, size_t n, hipStream_t stream) {
    if (n % 8) return adamml_set_error(ADAMML_EINVAL, "act_bwd_from_output: n must be a multiple of 8");
    if (!n) return ADAMML_OK;
    hipLaunchKernelGGL(act_bwd_from_output_kernel, dim3(grid_for(n / 8)), dim3(NT), 0, stream, (const bf16_t*)g_out,
                       (const bf16_t*)out, act, (bf16_t*)g, n / 8);
    return adamml_check_launch("act_bwd_from_output");
}

extern "C" int adamml_bn_bwd_reduce(const void* g, const void* z, const float* vec, int act, double* sums, size_t P, int C, int groups,
                                    hipStream_t stream) {
    CHECK_C(C, "bn_bwd_reduce");
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = reduce_grid(P, C, groups);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)g, (const bf16_t*)z, vec, act,
                       sums, P, C, rg.ppb);
    return adamml_check_launch("bn_bwd_reduce");
}

extern "C" int adamml_residual_bwd(const void* g_out, const void* out, int act, void* g2, const void* za, const float* veca,
                                   double* sumsa, const void* zb, const float* vecb, double* sumsb, size_t P, int C, int groups,
                                   hipStream_t stream) {
    CHECK_C(C, "residual_bwd");
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    if ((za && (!veca || !sumsa)) || (zb && (!vecb || !sumsb))) return adamml_set_error(ADAMML_EINVAL, "residual_bwd: null BN operands");
    const RowGrid rg = reduce_grid(P, C, groups);
    dispatch_bool(exceeds_infinity_cache(P, C, groups), [&](auto nt) {
        hipLaunchKernelGGL(residual_bwd_kernel<decltype(nt)::value>, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)g_out,
                           (const bf16_t*)out, act, (bf16_t*)g2, (const bf16_t*)za, veca, sumsa, (const bf16_t*)zb, vecb, sumsb, P, C, rg.ppb);
    });
    return adamml_check_launch("residual_bwd");
}

extern "C" int adamml_bn_bwd_finalize(const double* sums, int nslots, int groups, double count, const float* gamma, const float* vec,
                                      float* dgamma, float* dbeta, float* coef, int C, float grad_scale, hipStream_t stream) {
    if (nslots < 1 || nslots > ADAMML_STAT_SLOTS || groups < 1) return adamml_set_error(ADAMML_EINVAL, "bn_bwd_finalize: nslots=%d groups=%d", nslots, groups);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 8)), dim3(256), 0, stream, sums, nslots, groups, count, gamma, vec, dgamma,
                       dbeta, coef, (float*)nullptr, C, grad_scale);
    return adamml_check_launch("bn_bwd_finalize");
}

extern "C" int adamml_bn_bwd_finalize_affine(const double* sums, int nslots, int groups, double count, const float* gamma, const float* vec,
                                             float* dgamma, float* dbeta, float* coef, float* aff, int C, float grad_scale, hipStream_t stream) {
    if (nslots < 1 || nslots > ADAMML_STAT_SLOTS || groups < 1) return adamml_set_error(ADAMML_EINVAL, "bn_bwd_finalize_affine: nslots=%d groups=%d", nslots, groups);
    if (!coef || !aff) return adamml_set_error(ADAMML_EINVAL, "bn_bwd_finalize_affine: null argument");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 8)), dim3(256), 0, stream, sums, nslots, groups, count, gamma, vec, dgamma,
                       dbeta, coef, aff, C, grad_scale);
    return adamml_check_launch("bn_bwd_finalize_affine");
}

extern "C" int adamml_lazy_colsum(const void* x, const float* scale, const float* shift, int gstride, int act, float* s, size_t P, int C,
                                  int groups, hipStream_t stream) {
    CHECK_C(C, "lazy_colsum");
    if (!x || !s) return adamml_set_error(ADAMML_EINVAL, "lazy_colsum: null argument");
    if (groups < 1) groups = 1;
    (void)hipMemsetAsync(s, 0, (size_t)groups * C * sizeof(float), stream);
    if (!P) return ADAMML_OK;
    // one workgroup per group (all P rows): its fp32 adds run in a fixed order (fallback path only: adamml_gram_colsum serves the channel
    // counts of the model)
    hipLaunchKernelGGL(lazy_colsum_kernel, dim3(1, groups), dim3(NT), 0, stream, (const bf16_t*)x, scale, shift, gstride, act, s, P, C, P);
    return adamml_check_launch("lazy_colsum");
}

extern "C" int adamml_bn_bwd_affine(const float* coef, const float* vec, float* aff, int C, int groups, hipStream_t stream) {
    if (!coef || !vec || !aff || C < 1 || groups < 1) return adamml_set_error(ADAMML_EINVAL, "bn_bwd_affine: bad arguments");
    hipLaunchKernelGGL(bn_bwd_affine_kernel, dim3(ceil_div(C * groups, 256)), dim3(256), 0, stream, coef, vec, aff, C, groups);
    return adamml_check_launch("bn_bwd_affine");
}

extern "C" int adamml_bn_bwd_apply(const void* g, const void* z, const float* vec, int act, const float* coef, void* dz, size_t P, int C,
                                   int groups, hipStream_t stream) {
    CHECK_C(C, "bn_bwd_apply");
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = one_shot_grid(P, C, groups);
    dispatch_bool(exceeds_infinity_cache(P, C, groups), [&](auto nt) {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<decltype(nt)::value, 4>), dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)g,
                           (const bf16_t*)z, vec, act, coef, (bf16_t*)dz, P, C, rg.ppb);
    });
    return adamml_check_launch("bn_bwd_apply");
}
