// Input re-layout (gfx950): a clip batch -- fp32 planes, decoded uint8 frames, or uint8 frames turned into RGB differences -- to the
// segment-major NHWC bf16 tensors the stems read, with frame sub-sampling, bilinear resize and normalisation; their launchers.  Belongs
// here: a kernel that reads the data loader's layout.
#include "rowwalk.h"

namespace {

// x [B, S*F*C, H, W] fp32 -> y [S][B*Fk][OH][OW][c_pad] bf16; frames f = fk*frame_step; bilinear when OH != H.
__global__ void clip_to_nhwc_kernel(const float* x, bf16_t* y, int B, int S, int F, int C, int H, int W, int OH, int OW,
                                    int frame_step, int Fk, int c_pad) {
    const size_t total = (size_t)S * B * Fk * OH * OW;
    const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
    const bool resize = (OH != H) || (OW != W);
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        size_t r = e;
        const int ow = (int)(r % OW); r /= OW;
        const int oh = (int)(r % OH); r /= OH;
        const int fk = (int)(r % Fk); r /= Fk;
        const int b = (int)(r % B);
        const int s = (int)(r / B);
        const int f = fk * frame_step;
        const float* src = x + (((size_t)b * S + s) * F + f) * C * (size_t)H * W;
        int h0 = oh, h1 = oh, w0 = ow, w1 = ow;
        float lh1 = 0.f, lw1 = 0.f;
        if (resize) {
            float fh = fmaxf(sh * (oh + 0.5f) - 0.5f, 0.f), fw = fmaxf(sw * (ow + 0.5f) - 0.5f, 0.f);
            h0 = (int)fh; w0 = (int)fw;
            h1 = h0 + (h0 < H - 1 ? 1 : 0); w1 = w0 + (w0 < W - 1 ? 1 : 0);
            lh1 = fh - h0; lw1 = fw - w0;
        }
        const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
        bf16_t* dst = y + e * c_pad;
        if (c_pad == 4) {
            // 4-channel pixels (8 bytes): the layout the 7x7 stem kernels read for <= 4 input channels -- half the bytes of the 8-channel
            // padding in this kernel's store and in the stem's forward / weight-gradient loads
            f32x4 v4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float val = 0.f;
                if (i < C) {
                    const float* pl = src + (size_t)i * H * W;
                    if (resize)
                        val = lh0 * (lw0 * pl[(size_t)h0 * W + w0] + lw1 * pl[(size_t)h0 * W + w1]) +
                              lh1 * (lw0 * pl[(size_t)h1 * W + w0] + lw1 * pl[(size_t)h1 * W + w1]);
                    else
                        val = pl[(size_t)oh * W + ow];
                }
                v4[i] = val;
            }
            *reinterpret_cast<bf16x4*>(dst) = f32_to_bf4(v4);
            continue;
        }
        for (int c8 = 0; c8 < c_pad; c8 += 8) {
            f32x8 v;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = c8 + i;
                float val = 0.f;
                if (c < C) {
                    const float* pl = src + (size_t)c * H * W;
                    if (resize)
                        val = lh0 * (lw0 * pl[(size_t)h0 * W + w0] + lw1 * pl[(size_t)h0 * W + w1]) +
                              lh1 * (lw0 * pl[(size_t)h1 * W + w0] + lw1 * pl[(size_t)h1 * W + w1]);
                    else
                        val = pl[(size_t)oh * W + ow];
                }
                v[i] = val;
            }
            *reinterpret_cast<bf16x8*>(dst + c8) = f32_to_bf8(v);
        }
    }
}

// The main-net RGB path of the benchmark (no resize, <= 4 channels -> 8-byte pixels, W % 4 == 0): a thread owns FOUR consecutive pixels
// of a row -- one 16-byte load per channel plane, 32 contiguous output bytes -- where the generic kernel above moves 4 bytes per lane and
// load (round 5: it ran at 3.2 TB/s for 2.9 GB).  Same values: a re-layout with one fp32 -> bf16 rounding per element.
__global__ void clip_to_nhwc4_kernel(const float* x, bf16_t* y, int B, int S, int F, int C, int H, int W, int frame_step, int Fk) {
    const int W4 = W >> 2;
    const size_t total = (size_t)S * B * Fk * H * W4;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        size_t r = e;
        const int w4 = (int)(r % W4); r /= W4;
        const int oh = (int)(r % H); r /= H;
        const int fk = (int)(r % Fk); r /= Fk;
        const int b = (int)(r % B);
        const int s = (int)(r / B);
        const float* src = x + (((size_t)b * S + s) * F + fk * frame_step) * C * (size_t)H * W + (size_t)oh * W + 4 * w4;
        f32x4 pl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pl[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < C) pl[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (size_t)i * H * W));
        }
        union { bf16x4 q[4]; bf16x8 h[2]; } o;
#pragma unroll
        for (int px = 0; px < 4; ++px) o.q[px] = f32_to_bf4(f32x4{pl[0][px], pl[1][px], pl[2][px], pl[3][px]});
        bf16x8* dst = reinterpret_cast<bf16x8*>(y + ((((size_t)s * B + b) * Fk + fk) * H + oh) * (size_t)W * 4 + 16 * (size_t)w4);
        dst[0] = o.h[0];
        dst[1] = o.h[1];
    }
}

// Decoded-frame input path (utils/video_transforms.py:302-343 Stack -> ToTorchFormatTensor -> GroupNormalize, then
// models/adamml.py:42-67): x [B][H][W][S*F*C] uint8 -- the HW(FC) array `Stack` produces, one byte per value instead of the
// four of the normalised fp32 tensor -- to y [S][B*Fk][OH][OW][c_pad] bf16 with value ((u8 / 255) - mean[c % nm]) / std[c % nm]
// with the normalisation in fp32 exactly as the reference evaluates it, bilinear (align_corners = False) when OH != H: the four taps are
// combined by bilerp4() below -- three explicit fmaf, the same in both uint8 kernels, not the unfused sum torch evaluates (they agree to the
// roundings tests/abi_ref.py counts).  The source coordinate `sh * (oh + 0.5f) - 0.5f` may still be contracted per kernel; an index
// only depends on that where the coordinate lands within an ulp of an integer.  A thread owns one output
// pixel for every (segment, frame): it reads the 1..4 source pixels' contiguous S*F*C bytes and writes S*Fk chunks.
struct NormVec { float mean[4], std[4]; int n; };
// The four-tap bilinear expression of the two uint8 kernels below, with its roundings pinned: under the default -ffp-contract=fast the
// compiler chose WHICH products of `lh0 * (lw0 * a + lw1 * b) + lh1 * (..)` to fuse per kernel, and the table-driven RGB kernel and the
// generic kernel then differed in the last bf16 bit of a few elements (tests/test_abi_conformance_gpu.py, the clip_u8_to_nhwc[rgb-*] rows).
__device__ __forceinline__ float bilerp4(float lh0, float lh1, float lw0, float lw1, float p00, float p01, float p10, float p11) {
#pragma clang fp contract(off)
    const float top = fmaf(lw1, p01, lw0 * p00), bot = fmaf(lw1, p11, lw0 * p10);
    return fmaf(lh1, bot, lh0 * top);
}
// DIFF: the source holds C/3 + 1 consecutive RGB frames per frame group and the C output channels are the C/3 RGB differences
// of neighbours, quantised exactly as utils/video_dataset.py:32-38 does (uint8((next - cur + 255) * 0.5), truncation).
template <bool DIFF>
__global__ void clip_u8_to_nhwc_kernel(const uint8_t* x, bf16_t* y, int B, int S, int F, int C, int H, int W, int OH, int OW,
                                       int frame_step, int Fk, int c_pad, NormVec nv, int div255) {
    const size_t total = (size_t)B * OH * OW;
    const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
    const bool resize = (OH != H) || (OW != W);
    const int CS = DIFF ? C + 3 : C;                     // source channels per frame group
    const int SFC = S * F * CS;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        size_t r = e;
        const int ow = (int)(r % OW); r /= OW;
        const int oh = (int)(r % OH);
        const int b = (int)(r / OH);
        int h0 = oh, h1 = oh, w0 = ow, w1 = ow;
        float lh1 = 0.f, lw1 = 0.f;
        if (resize) {
            float fh = fmaxf(sh * (oh + 0.5f) - 0.5f, 0.f), fw = fmaxf(sw * (ow + 0.5f) - 0.5f, 0.f);
            h0 = (int)fh; w0 = (int)fw;
            h1 = h0 + (h0 < H - 1 ? 1 : 0); w1 = w0 + (w0 < W - 1 ? 1 : 0);
            lh1 = fh - h0; lw1 = fw - w0;
        }
        const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
        const uint8_t* p00 = x + (((size_t)b * H + h0) * W + w0) * SFC;
        const uint8_t* p01 = x + (((size_t)b * H + h0) * W + w1) * SFC;
        const uint8_t* p10 = x + (((size_t)b * H + h1) * W + w0) * SFC;
        const uint8_t* p11 = x + (((size_t)b * H + h1) * W + w1) * SFC;
        for (int s = 0; s < S; ++s)
            for (int fk = 0; fk < Fk; ++fk) {
                const int off = (s * F + fk * frame_step) * CS;
                bf16_t* dst = y + (((((size_t)s * B + b) * Fk + fk) * OH + oh) * OW + ow) * c_pad;
                const int cw = c_pad == 4 ? 4 : 8;               // 4-channel pixels: see clip_to_nhwc_kernel
                for (int c8 = 0; c8 < c_pad; c8 += 8) {
                    f32x8 v;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int c = c8 + i;
                        float val = 0.f;
                        if (c < C && i < cw) {
                            const float m = nv.mean[c % nv.n], sd = nv.std[c % nv.n];
                            auto nrm = [&](const uint8_t* q) {
                                float t = (float)q[off + c];
                                if (DIFF) t = floorf(((float)q[off + c + 3] - t + 255.f) * 0.5f);
                                if (div255) t = t / 255.f;
                                return (t - m) / sd;
                            };
                            val = resize ? bilerp4(lh0, lh1, lw0, lw1, nrm(p00), nrm(p01), nrm(p10), nrm(p11)) : nrm(p00);
                        }
                        v[i] = val;
                    }
                    if (cw == 4) *reinterpret_cast<bf16x4*>(dst) = f32_to_bf4(f32x4{v[0], v[1], v[2], v[3]});
                    else *reinterpret_cast<bf16x8*>(dst + c8) = f32_to_bf8(v);
                }
            }
    }
}

// The RGB case of the kernel above (C = 3 source channels, 8 frames per segment: every visual input of the reference recipes that is not
// RGB-diff) at streaming speed.  Round 5 priced the generic kernel with `bench.py --u8-input`: 11 ms per step more than the fp32 path -- it
// issues one BYTE load per value (120 per pixel, each touching 64 lines of a wave's 7.5 KB) and two fp32 divisions per value.  Here a
// thread reads its pixel's S * 24 bytes with 8-byte loads into registers (the frames' bytes are then at compile-time positions: S and
// the frame step are template parameters), and the normalisation ((u8 / 255) - mean) / std is a 3 x 256-entry fp32 table in LDS filled
// with exactly that expression -- bit-identical to the generic kernel by construction, no division per value.  Stores as there: 8 or 16
// bytes per lane, consecutive lanes = consecutive pixels of one frame plane.
template <int S, int STEP, bool RESIZE>
__global__ __launch_bounds__(NT) void clip_u8_rgb_kernel(const uint8_t* x, bf16_t* y, int B, int H, int W, int OH, int OW, int c_pad, NormVec nv,
                                                         int div255) {
    constexpr int F = 8, FK = F / STEP, NW = 3 * S;           // S * F * 3 bytes = NW 8-byte words per source pixel
    __shared__ float lut[3][256];
    for (int i = threadIdx.x; i < 3 * 256; i += NT) {
        const int c = i >> 8;
        float t = (float)(i & 255);
        if (div255) t = t / 255.f;
        lut[c][i & 255] = (t - nv.mean[c % nv.n]) / nv.std[c % nv.n];
    }
    __syncthreads();
    const size_t total = (size_t)B * OH * OW;
    const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        size_t r = e;
        const int ow = (int)(r % OW); r /= OW;
        const int oh = (int)(r % OH);
        const int b = (int)(r / OH);
        int h0 = oh, h1 = oh, w0 = ow, w1 = ow;
        float lh1 = 0.f, lw1 = 0.f;
        if (RESIZE) {
            float fh = fmaxf(sh * (oh + 0.5f) - 0.5f, 0.f), fw = fmaxf(sw * (ow + 0.5f) - 0.5f, 0.f);
            h0 = (int)fh; w0 = (int)fw;
            h1 = h0 + (h0 < H - 1 ? 1 : 0); w1 = w0 + (w0 < W - 1 ? 1 : 0);
            lh1 = fh - h0; lw1 = fw - w0;
        }
        const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
        constexpr int NSRC = RESIZE ? 4 : 1;
        uint64_t wd[NSRC][NW];
        const uint64_t* src[4] = {reinterpret_cast<const uint64_t*>(x + (((size_t)b * H + h0) * W + w0) * (NW * 8)),
                                  reinterpret_cast<const uint64_t*>(x + (((size_t)b * H + h0) * W + w1) * (NW * 8)),
                                  reinterpret_cast<const uint64_t*>(x + (((size_t)b * H + h1) * W + w0) * (NW * 8)),
                                  reinterpret_cast<const uint64_t*>(x + (((size_t)b * H + h1) * W + w1) * (NW * 8))};
#pragma unroll
        for (int q = 0; q < NSRC; ++q)
#pragma unroll
            for (int i = 0; i < NW; ++i) wd[q][i] = src[q][i];
        auto byte_of = [&](int q, int pos) { return (unsigned)(wd[q][pos >> 3] >> (8 * (pos & 7))) & 255u; };      // pos: compile-time after unrolling
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int fk = 0; fk < FK; ++fk) {
                const int off = (s * F + fk * STEP) * 3;
                float v[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (RESIZE)
                        v[c] = bilerp4(lh0, lh1, lw0, lw1, lut[c][byte_of(0, off + c)], lut[c][byte_of(1, off + c)], lut[c][byte_of(2, off + c)],
                                       lut[c][byte_of(3, off + c)]);
                    else
                        v[c] = lut[c][byte_of(0, off + c)];
                }
                bf16_t* dst = y + (((((size_t)s * B + b) * FK + fk) * OH + oh) * OW + ow) * c_pad;
                if (c_pad == 4) *reinterpret_cast<bf16x4*>(dst) = f32_to_bf4(f32x4{v[0], v[1], v[2], 0.f});
                else {
                    f32x8 o8 = {v[0], v[1], v[2], 0.f, 0.f, 0.f, 0.f, 0.f};
                    *reinterpret_cast<bf16x8*>(dst) = f32_to_bf8(o8);
                    for (int c8 = 8; c8 < c_pad; c8 += 8) *reinterpret_cast<bf16x8*>(dst + c8) = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
            }
    }
}

template <int S>
static bool launch_u8_rgb(const uint8_t* x, bf16_t* y, int B, int H, int W, int OH, int OW, int frame_step, int c_pad, const NormVec& nv, int div255,
                          size_t n, hipStream_t stream) {
    const bool resize = OH != H || OW != W;
    const dim3 grid(grid_for(n)), block(NT);
    if (frame_step == 1 && !resize) hipLaunchKernelGGL((clip_u8_rgb_kernel<S, 1, false>), grid, block, 0, stream, x, y, B, H, W, OH, OW, c_pad, nv, div255);
    else if (frame_step == 1) hipLaunchKernelGGL((clip_u8_rgb_kernel<S, 1, true>), grid, block, 0, stream, x, y, B, H, W, OH, OW, c_pad, nv, div255);
    else if (frame_step == 2 && !resize) hipLaunchKernelGGL((clip_u8_rgb_kernel<S, 2, false>), grid, block, 0, stream, x, y, B, H, W, OH, OW, c_pad, nv, div255);
    else if (frame_step == 2) hipLaunchKernelGGL((clip_u8_rgb_kernel<S, 2, true>), grid, block, 0, stream, x, y, B, H, W, OH, OW, c_pad, nv, div255);
    else return false;
    return true;
}

}  // namespace

extern "C" int adamml_clip_to_nhwc_four_pixel(const float* x, const void* y, int H, int W, int OH, int OW, int c_pad) {
    return c_pad == 4 && OH == H && OW == W && (W & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 ? 1 : 0;
}

extern "C" int adamml_clip_to_nhwc(const float* x, void* y, int B, int S, int F, int C, int H, int W, int OH, int OW,
                                   int frame_step, int c_pad, hipStream_t stream) {
    if ((c_pad % 8 && c_pad != 4) || c_pad < C || frame_step < 1) return adamml_set_error(ADAMML_EINVAL, "clip_to_nhwc: bad c_pad/frame_step");
    const int Fk = (F + frame_step - 1) / frame_step;
    const size_t n = (size_t)S * B * Fk * OH * OW;
    if (!n) return ADAMML_OK;
    if (adamml_clip_to_nhwc_four_pixel(x, y, H, W, OH, OW, c_pad)) {
        hipLaunchKernelGGL(clip_to_nhwc4_kernel, dim3(grid_for(n / 4)), dim3(NT), 0, stream, x, (bf16_t*)y, B, S, F, C, H, W, frame_step, Fk);
        return adamml_check_launch("clip_to_nhwc (4-pixel)");
    }
    hipLaunchKernelGGL(clip_to_nhwc_kernel, dim3(grid_for(n)), dim3(NT), 0, stream, x, (bf16_t*)y, B, S, F, C, H, W, OH, OW,
                       frame_step, Fk, c_pad);
    return adamml_check_launch("clip_to_nhwc");
}

extern "C" int adamml_clip_u8_to_nhwc(const uint8_t* x, void* y, int B, int S, int F, int C, int H, int W, int OH, int OW, int frame_step,
                                      int c_pad, const float* mean, const float* std, int n_mean, int div255, hipStream_t stream) {
    if (!x || !y || !mean || !std) return adamml_set_error(ADAMML_EINVAL, "clip_u8_to_nhwc: null argument");
    if ((c_pad % 8 && c_pad != 4) || c_pad < C || frame_step < 1) return adamml_set_error(ADAMML_EINVAL, "clip_u8_to_nhwc: bad c_pad/frame_step");
    if (n_mean < 1 || n_mean > 4 || C % n_mean) return adamml_set_error(ADAMML_EINVAL, "clip_u8_to_nhwc: %d mean/std values for %d channels", n_mean, C);
    const int Fk = (F + frame_step - 1) / frame_step;
    const size_t n = (size_t)B * OH * OW;
    if (!n || !S || !Fk) return ADAMML_OK;
    NormVec nv;
    nv.n = n_mean;
    for (int i = 0; i < 4; ++i) { nv.mean[i] = i < n_mean ? mean[i] : 0.f; nv.std[i] = i < n_mean ? std[i] : 1.f; }
    if (C == 3 && F == 8 && n_mean == 3 && S >= 1 && S <= 5 && ((uintptr_t)x & 7) == 0) {
        decltype(&launch_u8_rgb<1>) const by_segments[5] = {launch_u8_rgb<1>, launch_u8_rgb<2>, launch_u8_rgb<3>, launch_u8_rgb<4>, launch_u8_rgb<5>};
        if (by_segments[S - 1](x, (bf16_t*)y, B, H, W, OH, OW, frame_step, c_pad, nv, div255, n, stream)) return adamml_check_launch("clip_u8_to_nhwc (rgb)");
    }
    hipLaunchKernelGGL(clip_u8_to_nhwc_kernel<false>, dim3(grid_for(n)), dim3(NT), 0, stream, x, (bf16_t*)y, B, S, F, C, H, W, OH, OW, frame_step,
                       Fk, c_pad, nv, div255);
    return adamml_check_launch("clip_u8_to_nhwc");
}

extern "C" int adamml_clip_u8_rgbdiff_to_nhwc(const uint8_t* x, void* y, int B, int S, int F, int D, int H, int W, int OH, int OW,
                                              int frame_step, int c_pad, const float* mean, const float* std, int n_mean,
                                              hipStream_t stream) {
    const int C = 3 * D;
    if (!x || !y || !mean || !std) return adamml_set_error(ADAMML_EINVAL, "clip_u8_rgbdiff_to_nhwc: null argument");
    if (D < 1 || c_pad % 8 || c_pad < C || frame_step < 1) return adamml_set_error(ADAMML_EINVAL, "clip_u8_rgbdiff_to_nhwc: bad D/c_pad/frame_step");
    if (n_mean < 1 || n_mean > 4 || C % n_mean) return adamml_set_error(ADAMML_EINVAL, "clip_u8_rgbdiff_to_nhwc: %d mean/std values for %d channels", n_mean, C);
    const int Fk = (F + frame_step - 1) / frame_step;
    const size_t n = (size_t)B * OH * OW;
    if (!n || !S || !Fk) return ADAMML_OK;
    NormVec nv;
    nv.n = n_mean;
    for (int i = 0; i < 4; ++i) { nv.mean[i] = i < n_mean ? mean[i] : 0.f; nv.std[i] = i < n_mean ? std[i] : 1.f; }
    hipLaunchKernelGGL(clip_u8_to_nhwc_kernel<true>, dim3(grid_for(n)), dim3(NT), 0, stream, x, (bf16_t*)y, B, S, F, C, H, W, OH, OW, frame_step,
                       Fk, c_pad, nv, 1);
    return adamml_check_launch("clip_u8_rgbdiff_to_nhwc");
}
