// Crop / scale / flip of decoded video frames, byte-exact to Pillow's 8-bit BILINEAR resample (the visual half of
// utils/utils.py:110-150 get_augmentor before Stack; adamml_amd/video.py builds the tables and packs the frames).
//
// src: N decoded videos in one flat uint8 buffer, each [H, W, K_in] channels-last at its own byte offset and row stride (the
// frames of a video concatenated along the channel axis, as Stack does).  y: [N, OH, OW, K_out] uint8, exactly Stack's array.
// Per output pixel: for each of the ny taps of its row entry, one horizontal pass over the nx taps of its column entry,
// clamp((2^21 + sum k * src) >> 22, 0, 255) stored as a byte (Pillow clips between the passes), then the same formula over
// those bytes with the row coefficients.  The host tables carry the geometry: crop-then-resize (GroupMultiScaleCrop) and
// resize-then-crop (GroupScale / GroupRandomScale + crop) are both "first source index + taps + int32 coefficients" per output
// row / column; an axis that keeps its size has one tap of 2^22; a horizontal flip is the reversed column table.
//
// The horizontal-pass bytes of a source row are recomputed for every output row that reads it instead of being staged in LDS:
// at the augmentor's scales (short side 256 -> 224 ... 320) an output reads 2-4 rows of 2-4 taps, all from L1 / L2, and the
// kernel stays a single pass with no barrier.  A lane owns VEC consecutive channels of one output pixel (VEC-byte loads and
// stores: consecutive lanes cover a pixel's channels contiguously).
//
// Safety: every source row / column index is clamped into its video's [0, H) x [0, W), every table read into [0, meta_len),
// every tap count into [0, min(stride - 2, VR_KMAX)], and every source byte address into [0, src_bytes): no table or descriptor
// content can make the kernel read outside its buffers.  Products: coefficient <= 2^22 (checked on the host), pixel <= 255, so
// 24-bit multiplies are exact and the sums stay below 2^31.
#include "common.h"
#include "../../include/adamml_hip.h"

namespace {

constexpr int VR_DESC = 10;        // ints per video descriptor (include/adamml_hip.h)
constexpr int VR_KMAX = 32;        // taps per table entry (adamml_amd/video.py KMAX)
constexpr int VR_THREADS = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int VEC>
__device__ __forceinline__ void load_bytes(const uint8_t* p, int (&v)[VEC]) {
    if constexpr (VEC == 16) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = (w[e >> 2] >> (8 * (e & 3))) & 255;
    } else if constexpr (VEC == 8) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (w[e >> 2] >> (8 * (e & 3))) & 255;
    } else if constexpr (VEC == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (w >> (8 * e)) & 255;
    } else {
        v[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store_bytes(uint8_t* p, const int (&v)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = (uint8_t)v[0];
    } else {
        uint32_t w[VEC / 4];
#pragma unroll
        for (int j = 0; j < VEC / 4; ++j)
            w[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
        if constexpr (VEC == 16) {
            *reinterpret_cast<u32x4*>(p) = u32x4{w[0], w[1], w[2], w[3]};
        } else if constexpr (VEC == 8) {
            *reinterpret_cast<u32x2*>(p) = u32x2{w[0], w[1]};
        } else {
            *reinterpret_cast<uint32_t*>(p) = w[0];
        }
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> 22, 0, 255); }

// Table entry `o` of the table at meta[tab] with `stride` ints per entry: first source index, tap count (clamped), coefficients.
__device__ __forceinline__ const int* table_entry(const int* __restrict__ meta, int meta_len, int tab, int stride, int o, int& first, int& taps) {
    int64_t e = (int64_t)tab + (int64_t)o * stride;
    e = e < 0 ? 0 : (e > meta_len - 2 ? meta_len - 2 : e);
    first = meta[e];
    const int lim = min(min(stride - 2, VR_KMAX), (int)(meta_len - e - 2));
    taps = clampi(meta[e + 1], 0, lim);
    return meta + e + 2;
}

// DIFF: the source sample of output channel c is (next - cur + 255) >> 1 of the frame group's consecutive native frames
// (utils/video_dataset.py:32-38 compute_img_diff), formed before the horizontal pass: channel c of group g = c / (3 D) reads
// input channels g * 3 (D + 1) + c % (3 D) (cur) and that + 3 (next).
template <int VEC, bool DIFF>
__global__ void __launch_bounds__(VR_THREADS)
video_resample_u8_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ meta, int meta_len, uint8_t* __restrict__ y,
                         int OH, int OW, int K_in, int K_out, int diffs) {
    const int n = blockIdx.y;
    const int kv = K_out / VEC;
    const int64_t per = (int64_t)OH * OW * kv;
    const int64_t i = (int64_t)blockIdx.x * VR_THREADS + threadIdx.x;
    if (i >= per) return;
    const int* d = meta + (size_t)n * VR_DESC;
    const int64_t off = (int64_t)(uint32_t)d[0] | ((int64_t)d[1] << 32);
    const int H = d[2], W = d[3], rs = d[4], flags = d[9];
    const int c = (int)(i % kv) * VEC;
    const int64_t pix = i / kv;
    const int ox = (int)(pix % OW), oy = (int)(pix / OW);

    int x0, nx, y0, ny;
    const int* kx = table_entry(meta, meta_len, d[5], d[6], ox, x0, nx);
    const int* ky = table_entry(meta, meta_len, d[7], d[8], oy, y0, ny);

    int cin[VEC];                                            // DIFF: input channel of `cur` per output channel
    if constexpr (DIFF) {
        const int g3 = 3 * diffs;
#pragma unroll
        for (int e = 0; e < VEC; ++e) cin[e] = ((c + e) / g3) * (g3 + 3) + (c + e) % g3;
    }
    const int64_t qmax = DIFF ? src_bytes - 1 : ((src_bytes - VEC) & ~(int64_t)(VEC - 1));

    int acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 1 << 21;
    for (int ty = 0; ty < ny; ++ty) {
        const int sy = clampi(y0 + ty, 0, H - 1);
        const int64_t row = off + (int64_t)sy * rs;
        int h[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) h[e] = 1 << 21;
        for (int tx = 0; tx < nx; ++tx) {
            const int sx = clampi(x0 + tx, 0, W - 1);
            const int k = kx[tx];
            const int64_t q = row + (int64_t)sx * K_in;
            int p[VEC];
            if constexpr (DIFF) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    int64_t qa = q + cin[e], qb = qa + 3;
                    qa = qa < 0 ? 0 : (qa > qmax ? qmax : qa);
                    qb = qb < 0 ? 0 : (qb > qmax ? qmax : qb);
                    p[e] = ((int)src[qb] - (int)src[qa] + 255) >> 1;
                }
            } else {
                int64_t qa = (q + c) & ~(int64_t)(VEC - 1);          // (a no-op for the host's aligned descriptors)
                qa = qa < 0 ? 0 : (qa > qmax ? qmax : qa);
                load_bytes<VEC>(src + qa, p);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) h[e] += __mul24(k, p[e]);
        }
        const int k = ky[ty];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += __mul24(k, clip8(h[e]));
    }
    int out[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int v = clip8(acc[e]);
        out[e] = ((flags & 1) && !((c + e) & 1)) ? 255 - v : v;     // flipped flow: ImageOps.invert of the x images
    }
    store_bytes<VEC>(y + (((int64_t)n * OH + oy) * OW + ox) * K_out + c, out);
}

template <bool DIFF>
void launch(int vec, dim3 grid, hipStream_t stream, const uint8_t* src, int64_t src_bytes, const int* meta, int meta_len, uint8_t* y, int OH,
            int OW, int K_in, int K_out, int diffs) {
    switch (vec) {
        case 16:
            hipLaunchKernelGGL((video_resample_u8_kernel<16, DIFF>), grid, dim3(VR_THREADS), 0, stream, src, src_bytes, meta, meta_len, y, OH, OW,
                               K_in, K_out, diffs);
            break;
        case 8:
            hipLaunchKernelGGL((video_resample_u8_kernel<8, DIFF>), grid, dim3(VR_THREADS), 0, stream, src, src_bytes, meta, meta_len, y, OH, OW,
                               K_in, K_out, diffs);
            break;
        case 4:
            hipLaunchKernelGGL((video_resample_u8_kernel<4, DIFF>), grid, dim3(VR_THREADS), 0, stream, src, src_bytes, meta, meta_len, y, OH, OW,
                               K_in, K_out, diffs);
            break;
        default:
            hipLaunchKernelGGL((video_resample_u8_kernel<1, DIFF>), grid, dim3(VR_THREADS), 0, stream, src, src_bytes, meta, meta_len, y, OH, OW,
                               K_in, K_out, diffs);
    }
}

}  // namespace

extern "C" int adamml_video_resample_u8(const uint8_t* src, int64_t src_bytes, const int32_t* meta, int meta_len, uint8_t* y, int N, int OH,
                                        int OW, int K_in, int K_out, int diffs, hipStream_t stream) {
    if (N < 0 || N > 65535) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: N = %d outside [0, 65535]", N);
    if (OH < 1 || OW < 1) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: bad output size OH = %d / OW = %d", OH, OW);
    if (K_in < 1 || K_out < 1) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: bad channels K_in = %d / K_out = %d", K_in, K_out);
    if (diffs < 0) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: diffs = %d < 0", diffs);
    if (diffs == 0 && K_out != K_in)
        return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: K_out = %d != K_in = %d without differences", K_out, K_in);
    if (diffs > 0 && (K_in % (3 * (diffs + 1)) != 0 || K_out != K_in / (diffs + 1) * diffs))
        return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: rgbdiff needs K_in = G*3*(D+1) and K_out = G*3*D, got K_in = %d, K_out = %d, D = %d",
                                K_in, K_out, diffs);
    if (N == 0) return ADAMML_OK;
    if (meta_len < N * VR_DESC)
        return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: meta_len = %d < N * %d descriptor ints", meta_len, VR_DESC);
    if (src_bytes < 1) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: src_bytes = %lld < 1", (long long)src_bytes);
    if (!src || !meta || !y) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: null argument");
    int vec = 1;
    for (int v = 16; v >= 4; v /= 2) {
        const bool in_ok = diffs > 0 || (K_in % v == 0 && src_bytes % v == 0 && ((uintptr_t)src & (v - 1)) == 0);
        if (K_out % v == 0 && in_ok && ((uintptr_t)y & (v - 1)) == 0) {
            vec = v;
            break;
        }
    }
    const int64_t per = (int64_t)OH * OW * (K_out / vec);
    const int64_t blocks = (per + VR_THREADS - 1) / VR_THREADS;
    if (blocks > 0x7fffffff) return adamml_set_error(ADAMML_EINVAL, "video_resample_u8: output of %lld bytes per video too large", (long long)per * vec);
    const dim3 grid((unsigned)blocks, (unsigned)N);
    if (diffs > 0)
        launch<true>(vec, grid, stream, src, src_bytes, meta, meta_len, y, OH, OW, K_in, K_out, diffs);
    else
        launch<false>(vec, grid, stream, src, src_bytes, meta, meta_len, y, OH, OW, K_in, K_out, diffs);
    return adamml_check_launch("video_resample_u8");
}
