// Pooling (gfx950).  First MaxPool2d(3, 2, 1) of the ResNet stem: forward (per output and as a column walk), backward, and the backward fused
// with the BatchNorm backward of the tensor the pool reads.  Then the temporal pools over the frames of a clip (kernel 3, stride 2, padding 1,
// max or average: models/common.py): forward, backward, and the backward fused with the residual-add backward of the producing block.  Each
// family's launchers follow its kernels.  (The global average pool lives with the classifier head: head.hip.)
#include "rowwalk.h"

namespace {

// ZSEL: also store the RAW input value at the arg-max tap (z_sel, same shape as y).  The BatchNorm backward of the pool's input
// then takes its two sums from (g_y, z_sel) -- a quarter of the pixels -- with the plain bn_bwd_reduce kernel: every pooled
// gradient lands on exactly one input pixel, so sum(g') and sum(g' zhat) over the input equal the same sums over the windows.
template <bool ZSEL>
__global__ void maxpool_fwd_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act, bf16_t* y,
                                   uint8_t* idx, bf16_t* zsel, int N, int H, int W, int C, int OH, int OW) {
    x += (size_t)blockIdx.y * N * H * W * C;
    y += (size_t)blockIdx.y * N * OH * OW * C;
    idx += (size_t)blockIdx.y * N * OH * OW * C;
    if (ZSEL) zsel += (size_t)blockIdx.y * N * OH * OW * C;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const int cpr = C >> 3;
    const size_t total = (size_t)N * OH * OW * cpr;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const int ch = (int)(e % cpr);
        size_t pix = e / cpr;
        const int ow = (int)(pix % OW);
        pix /= OW;
        const int oh = (int)(pix % OH);
        const int n = (int)(pix / OH);
        f32x8 best;
        int bi[8];
        bf16x8 zs;
#pragma unroll
        for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bi[i] = 0; zs[i] = 0; }
        // all nine taps are loaded UNCONDITIONALLY from clamped coordinates and the padding taps are turned into -inf afterwards: a
        // branch around each load makes the compiler wait for one tap before the next is requested (nine dependent L2 / HBM round
        // trips per output chunk: 2.6 ms at the stem shape against 1.2 ms of traffic)
        bf16x8 raw[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ih = min(max(oh * 2 - 1 + kh, 0), H - 1), iw = min(max(ow * 2 - 1 + kw, 0), W - 1);
                raw[kh * 3 + kw] = *reinterpret_cast<const bf16x8*>(x + (((size_t)n * H + ih) * W + iw) * C + ch * 8);
            }
        f32x8 tsc, tsh;
#pragma unroll
        for (int i = 0; i < 8; ++i) { tsc[i] = 1.f; tsh[i] = 0.f; }
        if (scale) { tsc = load_f32x8(scale + ch * 8); tsh = load_f32x8(shift + ch * 8); }
        const float tlo = scale ? act_lo(act) : -INFINITY, thi = scale ? act_hi(act) : INFINITY;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ih = oh * 2 - 1 + kh, iw = ow * 2 - 1 + kw;
                const bool ok = ih >= 0 && iw >= 0 && ih < H && iw < W;
                f32x8 v = bf8_to_f32(raw[kh * 3 + kw]);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float t = ok ? clamp_act(fmaf(v[i], tsc[i], tsh[i]), tlo, thi) : -INFINITY;
                    if (t > best[i] || __builtin_isnan(t)) {       // (a NaN tap wins, as in torch)
                        best[i] = t; bi[i] = kh * 3 + kw;
                        if (ZSEL) zs[i] = raw[kh * 3 + kw][i];
                    }
                }
            }
        *reinterpret_cast<bf16x8*>(y + e * 8) = f32_to_bf8(best);
        if (ZSEL) *reinterpret_cast<bf16x8*>(zsel + e * 8) = zs;
        uint64_t packed = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) packed |= (uint64_t)bi[i] << (8 * i);
        *reinterpret_cast<uint64_t*>(idx + e * 8) = packed;
    }
}

// Column walker of the same pool: a thread owns one 8-channel chunk of one output COLUMN and walks down `rows` output rows.  Input row
// 2oh+1 is both the bottom row of window oh and the top row of window oh+1, so its three transformed taps are carried over: six new
// loads per output instead of nine (the per-output form is bound by its nine L1 requests per 16 bytes of output, not by HBM), and the
// two rows of the next window are in flight while the current one is reduced.  Same scan order (kh, kw ascending, strict >, a NaN tap
// always taken): same arg-max taps.
template <bool ZSEL>
__global__ __launch_bounds__(NT) void maxpool_fwd_walk_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act, bf16_t* y,
                                                              uint8_t* idx, bf16_t* zsel, int N, int H, int W, int C, int OH, int OW, int rows,
                                                              int nrb) {
    x += (size_t)blockIdx.y * N * H * W * C;
    y += (size_t)blockIdx.y * N * OH * OW * C;
    idx += (size_t)blockIdx.y * N * OH * OW * C;
    if (ZSEL) zsel += (size_t)blockIdx.y * N * OH * OW * C;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const int cpr = C >> 3;
    const size_t total = (size_t)N * nrb * OW * cpr;
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int ch = (int)(e % cpr);
    size_t r = e / cpr;
    const int ow = (int)(r % OW);
    r /= OW;
    const int rb = (int)(r % nrb);
    const int n = (int)(r / nrb);
    f32x8 tsc, tsh;
#pragma unroll
    for (int i = 0; i < 8; ++i) { tsc[i] = 1.f; tsh[i] = 0.f; }
    if (scale) { tsc = load_f32x8(scale + ch * 8); tsh = load_f32x8(shift + ch * 8); }
    const float tlo = scale ? act_lo(act) : -INFINITY, thi = scale ? act_hi(act) : INFINITY;
    const bf16_t* img = x + (size_t)n * H * W * C + ch * 8;
    int iwc[3];
    bool cok[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
        const int iw = ow * 2 - 1 + kw;
        cok[kw] = (unsigned)iw < (unsigned)W;
        iwc[kw] = min(max(iw, 0), W - 1);
    }
    struct Row { bf16x8 v[3]; };
    auto load_row = [&](int ih, Row& rw) {                   // unconditional, clamped
        const bf16_t* rp = img + (size_t)min(max(ih, 0), H - 1) * W * C;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) rw.v[kw] = *reinterpret_cast<const bf16x8*>(rp + (size_t)iwc[kw] * C);
    };
    auto xform = [&](const Row& rw, int ih, f32x8 (&t)[3]) {
        const bool rok = (unsigned)ih < (unsigned)H;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const f32x8 v = bf8_to_f32(rw.v[kw]);
            const bool ok = rok && cok[kw];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[kw][i] = ok ? clamp_act(fmaf(v[i], tsc[i], tsh[i]), tlo, thi) : -INFINITY;
        }
    };
    const int oh_b = rb * rows, oh_e = min(OH, oh_b + rows);
    Row top, mid, bot, nmid, nbot;
    f32x8 ttop[3], tmid[3], tbot[3];
    load_row(oh_b * 2 - 1, top);
    load_row(oh_b * 2, nmid);
    load_row(oh_b * 2 + 1, nbot);
    xform(top, oh_b * 2 - 1, ttop);
    for (int oh = oh_b; oh < oh_e; ++oh) {
        mid = nmid; bot = nbot;
        load_row(oh * 2 + 2, nmid);                          // (unconditional: load_row clamps; under `oh + 1 < oh_e` every wait of the walk
        load_row(oh * 2 + 3, nbot);                          //  behind the request was a conservative one -- appendix A-18)
        xform(mid, oh * 2, tmid);
        xform(bot, oh * 2 + 1, tbot);
        f32x8 best;
        int bi[8];
        bf16x8 zs;
#pragma unroll
        for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bi[i] = 0; zs[i] = 0; }
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (ttop[kw][i] > best[i] || __builtin_isnan(ttop[kw][i])) { best[i] = ttop[kw][i]; bi[i] = kw; if (ZSEL) zs[i] = top.v[kw][i]; }
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (tmid[kw][i] > best[i] || __builtin_isnan(tmid[kw][i])) { best[i] = tmid[kw][i]; bi[i] = 3 + kw; if (ZSEL) zs[i] = mid.v[kw][i]; }
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (tbot[kw][i] > best[i] || __builtin_isnan(tbot[kw][i])) { best[i] = tbot[kw][i]; bi[i] = 6 + kw; if (ZSEL) zs[i] = bot.v[kw][i]; }
        const size_t o = ((((size_t)n * OH + oh) * OW + ow) * cpr + ch) * 8;
        *reinterpret_cast<bf16x8*>(y + o) = f32_to_bf8(best);
        if (ZSEL) *reinterpret_cast<bf16x8*>(zsel + o) = zs;
        uint64_t packed = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) packed |= (uint64_t)bi[i] << (8 * i);
        *reinterpret_cast<uint64_t*>(idx + o) = packed;
        top = bot;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) ttop[kw] = tbot[kw];
    }
}

__global__ void maxpool_bwd_kernel(const bf16_t* gy, const uint8_t* idx, bf16_t* gx, int N, int H, int W, int C, int OH,
                                   int OW, int accumulate) {
    const int cpr = C >> 3;
    const size_t total = (size_t)N * H * W * cpr;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const int ch = (int)(e % cpr);
        size_t pix = e / cpr;
        const int iw = (int)(pix % W);
        pix /= W;
        const int ih = (int)(pix % H);
        const int n = (int)(pix / H);
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        if (accumulate) acc = bf8_to_f32(*reinterpret_cast<const bf16x8*>(gx + e * 8));
        const int oh_lo = ih >> 1, oh_hi = (ih + 1) >> 1;   // windows with oh*2-1 <= ih <= oh*2+1
        const int ow_lo = iw >> 1, ow_hi = (iw + 1) >> 1;
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            if (oh >= OH) continue;
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                if (ow >= OW) continue;
                const int tap = (ih - (oh * 2 - 1)) * 3 + (iw - (ow * 2 - 1));
                const size_t o = ((((size_t)n * OH + oh) * OW + ow) * cpr + ch) * 8;
                const uint64_t packed = *reinterpret_cast<const uint64_t*>(idx + o);
                f32x8 g = bf8_to_f32(*reinterpret_cast<const bf16x8*>(gy + o));
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if ((int)((packed >> (8 * i)) & 0xff) == tap) acc[i] += g[i];
            }
        }
        *reinterpret_cast<bf16x8*>(gx + e * 8) = f32_to_bf8(acc);
    }
}

// MaxPool2d(3, 2, 1) backward fused with the BatchNorm backward of the tensor the pool reads (the ResNet stem:
// models/resnet.py:199-202 conv1 -> bn1 -> relu -> maxpool, the pool being the stem output's only consumer).  The routed
// gradient g[n,ih,iw,c] = sum over the <= 4 windows whose recorded arg-max is this pixel is cheap to recompute from the
// pooled gradient and the 1-byte indices (1/4 of the pixels), so it is never written: pass 1 (APPLY = false) accumulates
// sum(g') and sum(g' zhat), pass 2 (APPLY = true) writes dz = k0 (g' - k1 - zhat k2) -- instead of maxpool_bwd (write g),
// bn_bwd_reduce (read g, z) and bn_bwd_apply (read g, z, write dz): 29 -> 17 GB at the benchmark shape.
// A thread owns one 8-channel chunk of a 2x2 input quad (rows 2k, 2k+1; columns 2j, 2j+1): the quad is covered by exactly
// the four windows (k+a, j+b), a, b in {0, 1}, and pixel (dy, dx) belongs to window (a, b) iff a <= dy and b <= dx, at tap
// (dy - 2a + 1) * 3 + (dx - 2b + 1) -- four (index, gradient) loads per four pixels instead of 2.25 per pixel.
// EVEN: H and W even (the launcher's choice) -- every pixel of a quad exists, the four stores of a quad are unconditional code (appendix A-18)
template <bool APPLY, bool EVEN = false>
__global__ __launch_bounds__(NT) void maxpool_bwd_bn_kernel(const bf16_t* gy, const uint8_t* idx, const bf16_t* z, const float* vec, int act,
                                                            double* sums, const float* coef, bf16_t* dz, int N, int H, int W, int C,
                                                            int OH, int OW, size_t qpb) {
    __shared__ float smem[APPLY ? 1 : 2 * MAXC];
    const size_t P = (size_t)N * H * W;
    const int QH = (H + 1) >> 1, QW = (W + 1) >> 1;
    const size_t Q = (size_t)N * QH * QW;
    {
        const size_t po = (size_t)blockIdx.y * N * OH * OW * C;
        gy += po; idx += po;
        z += (size_t)blockIdx.y * P * C;
        vec += (size_t)blockIdx.y * 4 * C;
        if (APPLY) { dz += (size_t)blockIdx.y * P * C; coef += (size_t)blockIdx.y * 3 * C; }
        else sums += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C;
    }
    ChanMap m(C, threadIdx.x);
    float s[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = q[i] = 0.f;
    const size_t qb = (size_t)blockIdx.x * qpb;
    const size_t qe = qb + qpb < Q ? qb + qpb : Q;
    if (m.active) {
        const int c = m.chunk * 8;
        const f32x8 sc = load_f32x8(vec + c), sh = load_f32x8(vec + C + c), mu = load_f32x8(vec + 2 * C + c), is = load_f32x8(vec + 3 * C + c);
        f32x8 k0, k1, k2;
        if (APPLY) { k0 = load_f32x8(coef + c); k1 = load_f32x8(coef + C + c); k2 = load_f32x8(coef + 2 * C + c); }
        const float lo = act_lo(act), hi = act_hi(act);
        for (size_t qi = qb + m.rslot; qi < qe; qi += m.rows_per_pass) {
            const int n = (int)(qi / ((size_t)QH * QW));
            const int rem = (int)(qi - (size_t)n * QH * QW);
            const int k = rem / QW, j = rem - k * QW;
            // the four windows of the quad
            uint64_t wi[2][2];
            bf16x8 wg[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const bool ok = k + a < OH && j + b < OW;
                    const size_t o = (((size_t)n * OH + (ok ? k + a : 0)) * OW + (ok ? j + b : 0)) * C + c;
                    const uint64_t iv = *reinterpret_cast<const uint64_t*>(idx + o);              // (unconditional: clamped address)
                    wi[a][b] = ok ? iv : ~0ull;                                                   // 0xff never equals a tap
                    wg[a][b] = *reinterpret_cast<const bf16x8*>(gy + o);
                }
            bf16x8 zr[2][2];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const bool ok = 2 * k + dy < H && 2 * j + dx < W;
                    const size_t pp = ((size_t)n * H + (ok ? 2 * k + dy : 0)) * W + (ok ? 2 * j + dx : 0);
                    zr[dy][dx] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(z + pp * C + c));
                }
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const bool ok = 2 * k + dy < H && 2 * j + dx < W;
                    f32x8 acc;
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
                    for (int a = 0; a <= dy; ++a)
#pragma unroll
                        for (int b = 0; b <= dx; ++b) {
                            const unsigned tap = (unsigned)((dy - 2 * a + 1) * 3 + (dx - 2 * b + 1));
                            const f32x8 g = bf8_to_f32(wg[a][b]);
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                if ((unsigned)((wi[a][b] >> (8 * i)) & 0xff) == tap) acc[i] += g[i];
                        }
                    const f32x8 gv = bf8_to_f32(f32_to_bf8(acc));      // the unfused path stores the routed gradient in bf16
                    const f32x8 zv = bf8_to_f32(zr[dy][dx]);
                    if (APPLY) {
                        f32x8 o;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const float gp = gv[i] * mask_act(fmaf(zv[i], sc[i], sh[i]), lo, hi);
                            const float zh = (zv[i] - mu[i]) * is[i];
                            o[i] = k0[i] * (gp - k1[i] - zh * k2[i]);
                        }
                        if (EVEN || ok) {
                            const size_t pp = ((size_t)n * H + 2 * k + dy) * W + 2 * j + dx;
                            __builtin_nontemporal_store(f32_to_bf8(o), reinterpret_cast<bf16x8*>(dz + pp * C + c));
                        }
                    } else {
                        const float keep = ok ? 1.f : 0.f;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const float gp = keep * gv[i] * mask_act(fmaf(zv[i], sc[i], sh[i]), lo, hi);
                            s[i] += gp;
                            q[i] += gp * (zv[i] - mu[i]) * is[i];
                        }
                    }
                }
        }
    }
    if (!APPLY) block_channel_publish(s, q, m, smem, C, sums);
}

}  // namespace

extern "C" int adamml_maxpool2d_fwd(const void* x, const float* scale, const float* shift, int gstride, int act, void* y, uint8_t* idx,
                                    void* z_sel, int N, int H, int W, int C, int OH, int OW, int groups, hipStream_t stream) {
    CHECK_C(C, "maxpool2d_fwd");
    const size_t n = (size_t)N * OH * OW * (C / 8);
    if (!n) return ADAMML_OK;
    if (groups < 1) groups = 1;
    constexpr int walk = 8;          // output rows per thread
    dispatch_bool(z_sel != nullptr, [&](auto zsel) {
        if (OH >= 2 * walk) {
            const int nrb = (OH + walk - 1) / walk;
            const size_t nth = (size_t)N * nrb * OW * (C / 8);
            hipLaunchKernelGGL(maxpool_fwd_walk_kernel<decltype(zsel)::value>, dim3((unsigned)((nth + NT - 1) / NT), groups), dim3(NT), 0, stream,
                               (const bf16_t*)x, scale, shift, gstride, act, (bf16_t*)y, idx, (bf16_t*)z_sel, N, H, W, C, OH, OW, walk, nrb);
        } else {
            hipLaunchKernelGGL(maxpool_fwd_kernel<decltype(zsel)::value>, dim3(grid_for(n, NT, 4096 / groups + 1), groups), dim3(NT), 0, stream,
                               (const bf16_t*)x, scale, shift, gstride, act, (bf16_t*)y, idx, (bf16_t*)z_sel, N, H, W, C, OH, OW);
        }
    });
    return adamml_check_launch("maxpool2d_fwd");
}

extern "C" int adamml_maxpool2d_bwd(const void* g_y, const uint8_t* idx, void* g_x, int N, int H, int W, int C, int OH, int OW,
                                    int accumulate, hipStream_t stream) {
    CHECK_C(C, "maxpool2d_bwd");
    const size_t n = (size_t)N * H * W * (C / 8);
    if (!n) return ADAMML_OK;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, (const bf16_t*)g_y, idx, (bf16_t*)g_x, N, H, W, C,
                       OH, OW, accumulate);
    return adamml_check_launch("maxpool2d_bwd");
}

extern "C" int adamml_maxpool2d_bwd_bn_reduce(const void* g_y, const uint8_t* idx, const void* z, const float* vec, int act, double* sums,
                                              int N, int H, int W, int C, int OH, int OW, int groups, hipStream_t stream) {
    CHECK_C(C, "maxpool2d_bwd_bn_reduce");
    if (!g_y || !idx || !z || !vec || !sums) return adamml_set_error(ADAMML_EINVAL, "maxpool2d_bwd_bn_reduce: null argument");
    const size_t P = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2);          // 2x2 input quads
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = reduce_grid(P, C, groups);
    hipLaunchKernelGGL(maxpool_bwd_bn_kernel<false>, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)g_y, idx,
                       (const bf16_t*)z, vec, act, sums, (const float*)nullptr, (bf16_t*)nullptr, N, H, W, C, OH, OW, rg.ppb);
    return adamml_check_launch("maxpool2d_bwd_bn_reduce");
}

extern "C" int adamml_maxpool2d_bwd_bn_apply(const void* g_y, const uint8_t* idx, const void* z, const float* vec, int act, const float* coef,
                                             void* dz, int N, int H, int W, int C, int OH, int OW, int groups, hipStream_t stream) {
    CHECK_C(C, "maxpool2d_bwd_bn_apply");
    if (!g_y || !idx || !z || !vec || !coef || !dz) return adamml_set_error(ADAMML_EINVAL, "maxpool2d_bwd_bn_apply: null argument");
    const size_t P = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2);          // 2x2 input quads
    if (!P) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = rowwalk_grid(P, C, groups, 8192);
    dispatch_bool(H % 2 == 0 && W % 2 == 0, [&](auto even) {
        hipLaunchKernelGGL((maxpool_bwd_bn_kernel<true, decltype(even)::value>), dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream, (const bf16_t*)g_y,
                           idx, (const bf16_t*)z, vec, act, (double*)nullptr, coef, (bf16_t*)dz, N, H, W, C, OH, OW, rg.ppb);
    });
    return adamml_check_launch("maxpool2d_bwd_bn_apply");
}

namespace {

// ------------------------------------------------------------------------------------------------ temporal pools
// x: [NB, T, HWC] -> y: [NB, To, HWC], To = (T-1)/2+1
__global__ void temporal_pool_fwd_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act, bf16_t* y,
                                         int NB, int T, int To, size_t hwc8, int C, int mode) {
    x += (size_t)blockIdx.y * NB * T * hwc8 * 8;
    y += (size_t)blockIdx.y * NB * To * hwc8 * 8;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const size_t total = (size_t)NB * To * hwc8;
    const int cpr = C >> 3;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const size_t in = e % hwc8;
        size_t r = e / hwc8;
        const int to = (int)(r % To);
        const int nb = (int)(r / To);
        const int c = (int)(in % cpr) * 8;
        f32x8 accv;
#pragma unroll
        for (int i = 0; i < 8; ++i) accv[i] = mode == 0 ? -INFINITY : 0.f;
        // the three frames are loaded unconditionally (clamped frame index) and the padding frames neutralised afterwards: a branch
        // around each load serialises the three round trips
        bf16x8 raw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = min(max(2 * to + k - 1, 0), T - 1);
            raw[k] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(x + (((size_t)nb * T + t) * hwc8 + in) * 8));
        }
        f32x8 tsc, tsh;
#pragma unroll
        for (int i = 0; i < 8; ++i) { tsc[i] = 1.f; tsh[i] = 0.f; }
        if (scale) { tsc = load_f32x8(scale + c); tsh = load_f32x8(shift + c); }
        const float tlo = scale ? act_lo(act) : -INFINITY, thi = scale ? act_hi(act) : INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = 2 * to + k - 1;
            const bool ok = t >= 0 && t < T;
            const f32x8 v = bf8_to_f32(raw[k]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float tv = clamp_act(fmaf(v[i], tsc[i], tsh[i]), tlo, thi);
                accv[i] = mode == 0 ? __builtin_elementwise_maximum(accv[i], ok ? tv : -INFINITY) : accv[i] + (ok ? tv : 0.f);
            }
        }
        if (mode == 1) accv *= (1.f / 3.f);
        *reinterpret_cast<bf16x8*>(y + e * 8) = f32_to_bf8(accv);
    }
}

// The same pool as a column walk for the frame counts of the hot path (T = 8, 4, 2: models/resnet.py:207-210 halves the frames after
// layers 1-3): a thread owns one 8-channel chunk of one pixel for ALL T frames, requests the T rows up front, transforms each once
// and emits the To = T/2 outputs -- every input row is read once (the per-output form reads the shared odd frames twice, 1.5x the
// loads) and the frame loop is compile-time (no branches around the loads).
template <int T>
__global__ __launch_bounds__(NT) void temporal_pool_fwd_walk_kernel(const bf16_t* x, const float* scale, const float* shift, int gs, int act,
                                                                   bf16_t* y, int NB, size_t hwc8, int C, int mode) {
    constexpr int To = (T - 1) / 2 + 1;
    x += (size_t)blockIdx.y * NB * T * hwc8 * 8;
    y += (size_t)blockIdx.y * NB * To * hwc8 * 8;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const size_t total = (size_t)NB * hwc8;
    const int cpr = C >> 3;
    const float lo = scale ? act_lo(act) : -INFINITY, hi = scale ? act_hi(act) : INFINITY;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const size_t in = e % hwc8, nb = e / hwc8;
        const int c = (int)(in % cpr) * 8;
        bf16x8 raw[T];
#pragma unroll
        for (int t = 0; t < T; ++t) raw[t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(x + ((nb * T + t) * hwc8 + in) * 8));
        f32x8 sc, sh;
#pragma unroll
        for (int i = 0; i < 8; ++i) { sc[i] = 1.f; sh[i] = 0.f; }
        if (scale) { sc = load_f32x8(scale + c); sh = load_f32x8(shift + c); }
        f32x8 v[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            v[t] = bf8_to_f32(raw[t]);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[t][i] = clamp_act(fmaf(v[t][i], sc[i], sh[i]), lo, hi);
        }
#pragma unroll
        for (int to = 0; to < To; ++to) {
            f32x8 acc;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = mode == 0 ? -INFINITY : 0.f;
#pragma unroll
            for (int k = -1; k <= 1; ++k) {
                const int t = 2 * to + k;
                if (t < 0 || t >= T) continue;                   // (compile-time)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = mode == 0 ? __builtin_elementwise_maximum(acc[i], v[t][i]) : acc[i] + v[t][i];
            }
            if (mode == 1) acc *= (1.f / 3.f);
            __builtin_nontemporal_store(f32_to_bf8(acc), reinterpret_cast<bf16x8*>(y + ((nb * To + to) * hwc8 + in) * 8));
        }
    }
}

// gradient w.r.t. the ACTIVATED input value (the lazy transform's own backward is the producer's business)
__global__ void temporal_pool_bwd_kernel(const bf16_t* gy, const bf16_t* x, const float* scale, const float* shift, int gs, int act,
                                         bf16_t* gx, int NB, int T, int To, size_t hwc8, int C, int mode) {
    gy += (size_t)blockIdx.y * NB * To * hwc8 * 8;
    x += (size_t)blockIdx.y * NB * T * hwc8 * 8;
    gx += (size_t)blockIdx.y * NB * T * hwc8 * 8;
    if (scale) { scale += (size_t)blockIdx.y * gs; shift += (size_t)blockIdx.y * gs; }
    const size_t total = (size_t)NB * T * hwc8;
    const int cpr = C >> 3;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const size_t in = e % hwc8;
        size_t r = e / hwc8;
        const int t = (int)(r % T);
        const int nb = (int)(r / T);
        const int c = (int)(in % cpr) * 8;
        f32x8 acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        const int to_lo = t >> 1, to_hi = (t + 1) >> 1;
        for (int to = to_lo; to <= to_hi; ++to) {
            if (to >= To) continue;
            f32x8 g = bf8_to_f32(*reinterpret_cast<const bf16x8*>(gy + (((size_t)nb * To + to) * hwc8 + in) * 8));
            if (mode == 1) {
                acc += g * (1.f / 3.f);
                continue;
            }
            // recompute the window's first arg-max (scan order 2to-1, 2to, 2to+1, strict >)
            f32x8 best;
            int bt[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bt[i] = -1; }
#pragma unroll
            for (int k = -1; k <= 1; ++k) {
                const int tt = 2 * to + k;
                if (tt < 0 || tt >= T) continue;
                f32x8 v = transform8(*reinterpret_cast<const bf16x8*>(x + (((size_t)nb * T + tt) * hwc8 + in) * 8), scale, shift, c, act);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (v[i] > best[i]) { best[i] = v[i]; bt[i] = tt; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (bt[i] == t) acc[i] += g[i];
        }
        *reinterpret_cast<bf16x8*>(gx + e * 8) = f32_to_bf8(acc);
    }
}

// Temporal max-pool backward fused with the residual-add backward of the block that produced the pool's input
// (models/common.py:28-33 after models/resnet.py:110-111): the pool is the only consumer of the block output `out`, so
// its input gradient IS the block-output gradient.  One thread walks the T frames of one (clip, pixel, 8-channel chunk)
// column: window arg-maxes from `out` (first maximum in scan order 2to-1, 2to, 2to+1, as the forward kernel), routed
// gradient, activation mask act'(out), store g', and the BatchNorm-backward sums of the add's BatchNorm'd operand z.
// Replaces temporal_pool_bwd (write gx) + residual_bwd (re-read gx, out): 6.5 -> 3.5 tensor passes.
template <int T>
__global__ __launch_bounds__(NT) void temporal_pool_residual_bwd_kernel(const bf16_t* gy, const bf16_t* out, int act, bf16_t* g2,
                                                                        const bf16_t* za, const float* veca, double* sumsa,
                                                                        size_t NBHW, int HW, int C, size_t cpb) {
    constexpr int To = (T - 1) / 2 + 1;
    __shared__ float smem[2 * MAXC];
    const int NB = (int)(NBHW / HW);
    {
        const size_t goff = (size_t)blockIdx.y * NB * T * HW * C;
        gy += (size_t)blockIdx.y * NB * To * HW * C;
        out += goff; g2 += goff;
        if (za) { za += goff; veca += (size_t)blockIdx.y * 4 * C; }        // za == nullptr: sum(g') only (algebraic BatchNorm backward)
        sumsa += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C;
    }
    ChanMap m(C, threadIdx.x);
    float sa[8], qa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = qa[i] = 0.f;
    const size_t cb = (size_t)blockIdx.x * cpb;
    const size_t ce = cb + cpb < NBHW ? cb + cpb : NBHW;
    if (m.active) {
        const int c = m.chunk * 8;
        f32x8 mua, isa;
#pragma unroll
        for (int i = 0; i < 8; ++i) { mua[i] = 0.f; isa[i] = 0.f; }
        if (za) { mua = load_f32x8(veca + 2 * C + c); isa = load_f32x8(veca + 3 * C + c); }
        const float lo = act_lo(act), hi = act_hi(act);
        const size_t fstride = (size_t)HW * C;                    // elements between consecutive frames of a clip
        for (size_t col = cb + m.rslot; col < ce; col += m.rows_per_pass) {
            const size_t nb = col / HW, hw = col - nb * HW;
            const size_t base = (nb * T * HW + hw) * C + c, gbase = (nb * To * HW + hw) * C + c;
            bf16x8 ov[T], zv[T], gv[To];
#pragma unroll
            for (int t = 0; t < T; ++t) ov[t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(out + base + t * fstride));
#pragma unroll
            for (int t = 0; t < To; ++t) gv[t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(gy + gbase + t * fstride));
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (za) zv[t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(za + base + t * fstride));
                else zv[t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};          // isa == 0: the second moment stays 0
            }
            int bt[To][8];
#pragma unroll
            for (int to = 0; to < To; ++to) {
                f32x8 best;
#pragma unroll
                for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bt[to][i] = -1; }
#pragma unroll
                for (int k = -1; k <= 1; ++k) {
                    const int tt = 2 * to + k;
                    if (tt < 0 || tt >= T) continue;
                    const f32x8 v = bf8_to_f32(ov[tt]);
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (v[i] > best[i]) { best[i] = v[i]; bt[to][i] = tt; }
                }
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const f32x8 o = bf8_to_f32(ov[t]);
                f32x8 acc;
                const f32x8 g0 = bf8_to_f32(gv[t >> 1]);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = bt[t >> 1][i] == t ? g0[i] : 0.f;
                if ((t & 1) && ((t + 1) >> 1) < To) {
                    const f32x8 g1 = bf8_to_f32(gv[((t + 1) >> 1) < To ? ((t + 1) >> 1) : 0]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] += bt[((t + 1) >> 1) < To ? ((t + 1) >> 1) : 0][i] == t ? g1[i] : 0.f;
                }
                // (the unfused path rounds the routed gradient to bf16 before masking: same here)
                acc = bf8_to_f32(f32_to_bf8(acc));
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] *= mask_act(o[i], lo, hi);
                const bf16x8 gb = f32_to_bf8(acc);
                __builtin_nontemporal_store(gb, reinterpret_cast<bf16x8*>(g2 + base + t * fstride));
                const f32x8 gq = bf8_to_f32(gb), z = bf8_to_f32(zv[t]);
#pragma unroll
                for (int i = 0; i < 8; ++i) { sa[i] += gq[i]; qa[i] += gq[i] * (z[i] - mua[i]) * isa[i]; }
            }
        }
    }
    block_channel_publish(sa, qa, m, smem, C, sumsa);
}

// The same backward when the forward fused the pool into the producing conv (adamml_conv_fwd_bn_add_tpool): the block output was never
// stored; 2 bits per pooled element say which window tap held the first maximum (3: the maximum did not pass the ReLU).  One thread
// owns the T frames of one (clip, pixel, 8-channel chunk) column: To gradient rows + To code words in, T gradient rows out.
template <int T>
__global__ __launch_bounds__(NT) void temporal_pool_code_bwd_kernel(const bf16_t* gy, const uint16_t* code, bf16_t* g2, double* sumsa,
                                                                    size_t NBHW, int HW, int C, size_t cpb) {
    constexpr int To = T / 2;
    __shared__ float smem[2 * MAXC];
    const int NB = (int)(NBHW / HW);
    {
        const size_t poff = (size_t)blockIdx.y * NB * To * HW * C;
        gy += poff;
        code += poff >> 3;
        g2 += (size_t)blockIdx.y * NB * T * HW * C;
        sumsa += (size_t)blockIdx.y * ADAMML_STAT_SLOTS * 2 * C;
    }
    ChanMap m(C, threadIdx.x);
    float sa[8], qa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = qa[i] = 0.f;
    const size_t cb = (size_t)blockIdx.x * cpb;
    const size_t ce = cb + cpb < NBHW ? cb + cpb : NBHW;
    if (m.active) {
        const int c = m.chunk * 8;
        const size_t fstride = (size_t)HW * C;
        for (size_t col = cb + m.rslot; col < ce; col += m.rows_per_pass) {
            const size_t nb = col / HW, hw = col - nb * HW;
            const size_t base = (nb * T * HW + hw) * C + c, gbase = (nb * To * HW + hw) * C + c;
            bf16x8 gv[To];
            unsigned cw[To];
#pragma unroll
            for (int t = 0; t < To; ++t) {
                gv[t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(gy + gbase + t * fstride));
                cw[t] = code[(gbase + t * fstride) >> 3];
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                // frame t is tap (t - (2 to - 1)) of window to: tap 1 of window t / 2 for even t; for odd t, tap 2 of window (t - 1) / 2 and tap 0 of
                // window (t + 1) / 2 (when that window exists)
                f32x8 acc;
                const int w0 = t >> 1, k0 = t - (2 * w0 - 1);
                const f32x8 g0 = bf8_to_f32(gv[w0]);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = ((cw[w0] >> (2 * i)) & 3u) == (unsigned)k0 ? g0[i] : 0.f;
                if ((t & 1) && ((t + 1) >> 1) < To) {
                    const int w1 = (t + 1) >> 1;
                    const f32x8 g1 = bf8_to_f32(gv[w1 < To ? w1 : 0]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] += ((cw[w1 < To ? w1 : 0] >> (2 * i)) & 3u) == 0u ? g1[i] : 0.f;
                }
                const bf16x8 gb = f32_to_bf8(acc);
                __builtin_nontemporal_store(gb, reinterpret_cast<bf16x8*>(g2 + base + t * fstride));
                const f32x8 gq = bf8_to_f32(gb);
#pragma unroll
                for (int i = 0; i < 8; ++i) sa[i] += gq[i];
            }
        }
    }
    block_channel_publish(sa, qa, m, smem, C, sumsa);
}

}  // namespace

extern "C" int adamml_temporal_pool_fwd(const void* x, const float* scale, const float* shift, int gstride, int act, void* y, int NB,
                                        int T, size_t HWC, int C, int mode, int groups, hipStream_t stream) {
    CHECK_C(C, "temporal_pool_fwd");
    if (mode == 1 && T < 3)   // models/common.py:20 nn.AvgPool3d raises for T < kernel (torch: "input image smaller than kernel size")
        return adamml_set_error(ADAMML_EINVAL, "temporal_pool_fwd: avg pooling needs T >= 3 (got %d), as in the reference", T);
    const int To = (T - 1) / 2 + 1;
    const size_t n = (size_t)NB * To * (HWC / 8);
    if (!n) return ADAMML_OK;
    if (groups < 1) groups = 1;
    if (T == 8 || T == 4 || T == 2) {
        const dim3 grid(grid_for((size_t)NB * (HWC / 8), NT, 8192 / groups + 1), groups);
        dispatch_frames_8_4_2(T, [&](auto frames) {
            hipLaunchKernelGGL(temporal_pool_fwd_walk_kernel<decltype(frames)::value>, grid, dim3(NT), 0, stream, (const bf16_t*)x, scale, shift, gstride,
                               act, (bf16_t*)y, NB, HWC / 8, C, mode);
        });
    } else {
        hipLaunchKernelGGL(temporal_pool_fwd_kernel, dim3(grid_for(n, NT, 4096 / groups + 1), groups), dim3(NT), 0, stream, (const bf16_t*)x,
                           scale, shift, gstride, act, (bf16_t*)y, NB, T, To, HWC / 8, C, mode);
    }
    return adamml_check_launch("temporal_pool_fwd");
}

extern "C" int adamml_temporal_pool_bwd(const void* g_y, const void* x, const float* scale, const float* shift, int gstride, int act,
                                        void* g_x, int NB, int T, size_t HWC, int C, int mode, int groups, hipStream_t stream) {
    CHECK_C(C, "temporal_pool_bwd");
    const int To = (T - 1) / 2 + 1;
    const size_t n = (size_t)NB * T * (HWC / 8);
    if (!n) return ADAMML_OK;
    if (groups < 1) groups = 1;
    hipLaunchKernelGGL(temporal_pool_bwd_kernel, dim3(grid_for(n, NT, 4096 / groups + 1), groups), dim3(NT), 0, stream, (const bf16_t*)g_y,
                       (const bf16_t*)x, scale, shift, gstride, act, (bf16_t*)g_x, NB, T, To, HWC / 8, C, mode);
    return adamml_check_launch("temporal_pool_bwd");
}

extern "C" int adamml_temporal_pool_bwd_res_supported(int T, int C, int mode) {
    return (T == 2 || T == 4 || T == 8) && mode == 0 && C % 8 == 0 && C <= MAXC ? 1 : 0;
}

extern "C" int adamml_temporal_pool_bwd_res(const void* g_y, const void* out, int act, void* g2, const void* z_a, const float* vec_a,
                                            double* sums_a, int NB, int T, int HW, int C, int groups, hipStream_t stream) {
    CHECK_C(C, "temporal_pool_bwd_res");
    if (!adamml_temporal_pool_bwd_res_supported(T, C, 0)) return adamml_set_error(ADAMML_EUNSUPPORTED, "temporal_pool_bwd_res: T=%d C=%d", T, C);
    if (!g_y || !out || !g2 || !sums_a || (z_a && !vec_a)) return adamml_set_error(ADAMML_EINVAL, "temporal_pool_bwd_res: null argument");
    const size_t cols = (size_t)NB * HW;
    if (!cols) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = reduce_grid(cols, C, groups);
    dispatch_frames_8_4_2(T, [&](auto frames) {
        hipLaunchKernelGGL(temporal_pool_residual_bwd_kernel<decltype(frames)::value>, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream,
                           (const bf16_t*)g_y, (const bf16_t*)out, act, (bf16_t*)g2, (const bf16_t*)z_a, vec_a, sums_a, cols, HW, C, rg.ppb);
    });
    return adamml_check_launch("temporal_pool_bwd_res");
}

extern "C" int adamml_temporal_pool_bwd_code(const void* g_y, const uint16_t* code, void* g2, double* sums_a, int NB, int T, int HW, int C,
                                             int groups, hipStream_t stream) {
    CHECK_C(C, "temporal_pool_bwd_code");
    if (!adamml_temporal_pool_bwd_res_supported(T, C, 0)) return adamml_set_error(ADAMML_EUNSUPPORTED, "temporal_pool_bwd_code: T=%d C=%d", T, C);
    if (!g_y || !code || !g2 || !sums_a) return adamml_set_error(ADAMML_EINVAL, "temporal_pool_bwd_code: null argument");
    const size_t cols = (size_t)NB * HW;
    if (!cols) return ADAMML_OK;
    if (groups < 1) groups = 1;
    const RowGrid rg = reduce_grid(cols, C, groups);
    dispatch_frames_8_4_2(T, [&](auto frames) {
        hipLaunchKernelGGL(temporal_pool_code_bwd_kernel<decltype(frames)::value>, dim3((unsigned)rg.nblk, groups), dim3(NT), 0, stream,
                           (const bf16_t*)g_y, code, (bf16_t*)g2, sums_a, cols, HW, C, rg.ppb);
    });
    return adamml_check_launch("temporal_pool_bwd_code");
}
