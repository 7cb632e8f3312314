// Baseline JPEG frames decoded on the GPU, byte-exact to libjpeg(-turbo) as Pillow uses it (utils/video_dataset.py:51-66 opens every
// frame with PIL.Image.open; adamml_amd/jpeg.py parses the headers and packs the batch).  Three kernels on one stream:
//
//   1. jpeg_entropy_kernel   Huffman decode.  Segments (the scan split at its restart markers) are independent and sequential: one
//      lane decodes one segment, JE_LANES segments per wave, one image per workgroup.  What the decoding lane touches lives in LDS:
//      the image's Huffman tables, built here from BITS / HUFFVAL (an 8-bit first-level table + the canonical max-code walk for the
//      longer codes), the zigzag order, and a 16-byte window of the lane's bitstream that is refilled with 16-byte loads issued one
//      window ahead (the load of window w + 1 is in flight while window w is consumed).  Output: int16 coefficients in natural
//      order, only the non-zero ones (the workspace is cleared first).
//   2. jpeg_idct_kernel      dequantise + libjpeg's jidctint ("islow": CONST_BITS 13, PASS1_BITS 2) per 8 x 8 block, one lane per
//      block, into uint8 component planes.  64-bit arithmetic throughout, as libjpeg's `long`.
//   3. jpeg_colour_kernel    "fancy" h2v2 chroma upsampling (4:2:0), fixed-point YCbCr -> RGB, store at the image's strides.
//
// Safety (these kernels terminate and stay inside their buffers on ANY input): every loop bound is structural or a clamped
// descriptor value -- the MCU loop runs the segment's stated count (clamped to the image's), a block runs at most 63 AC steps each
// advancing the index, the refill loop at most 8 bytes, the long-code walk 8 lengths; the bit reader feeds zero bits from the
// segment's end or a marker on.  H and W are clamped to [1, 65535] and H * W to JPEG_MAX_PIXELS, every table index into
// [0, meta_len - table size], every bitstream address into [0, src_bytes), every workspace block into [0, blocks) and every output
// address into [0, y_bytes).  A bad segment sets status bits (1 ran past its end, 2 no code matches / DC category > 11,
// 4 coefficient index > 63) and its remaining blocks stay zero; 8 marks a descriptor that had to be clamped, 16 a segment with a byte or
// more left over after its last MCU.  Nothing traps or spins.
#include "common.h"
#include "../../include/adamml_hip.h"

namespace {

constexpr int JD = 22;                 // ints per image descriptor (include/adamml_hip.h)
constexpr int JSEG = 4;                // ints per segment record
constexpr int JHUFF = 80;              // ints per Huffman table in meta: BITS[16], HUFFVAL[256] as 64 words
constexpr int JE_THREADS = 64;         // one wave per workgroup
constexpr int JE_LANES = 16;           // decoding lanes (segments) per wave
constexpr int JE_GRID = 4;             // workgroups per image: 64 segments in flight, more in a strided loop
constexpr int JI_THREADS = 256, JI_GRID = 8;
constexpr int JC_THREADS = 256, JC_GRID = 32;
constexpr int64_t JPEG_MAX_PIXELS = (int64_t)1 << 26;
constexpr int ST_OVERRUN = 1, ST_BAD_CODE = 2, ST_BAD_INDEX = 4, ST_BAD_DESC = 8, ST_LEFTOVER = 16;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__constant__ uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The clamped geometry of image `img`; `flag` collects ST_BAD_DESC when a word had to be clamped.
struct Image {
    int H, W, ncomp, hs, mw, mh;
    int64_t blk0, nblk;       // first workspace block, block count
    int nb0, bw0, bw1;        // blocks of component 0; blocks per row of component 0 / of the chroma components
};

__device__ __forceinline__ Image load_image(const int* __restrict__ d, int64_t total_blocks, int& flag) {
    Image im;
    im.H = clampi(d[0], 1, 65535);
    im.W = clampi(d[1], 1, 65535);
    if ((int64_t)im.H * im.W > JPEG_MAX_PIXELS) {
        im.H = 1;
        im.W = 1;
        flag |= ST_BAD_DESC;
    }
    im.ncomp = d[2] == 3 ? 3 : 1;
    im.hs = (im.ncomp == 3 && d[3] == 2) ? 2 : 1;
    if (im.H != d[0] || im.W != d[1] || (d[2] != 1 && d[2] != 3) || (d[3] != 1 && d[3] != 2)) flag |= ST_BAD_DESC;
    im.mw = (im.W + 8 * im.hs - 1) / (8 * im.hs);
    im.mh = (im.H + 8 * im.hs - 1) / (8 * im.hs);
    im.bw0 = im.mw * im.hs;
    im.bw1 = im.mw;
    im.nb0 = im.mw * im.mh * im.hs * im.hs;
    im.nblk = im.ncomp == 3 ? (int64_t)im.nb0 + 2 * im.mw * im.mh : im.nb0;
    im.blk0 = (int64_t)((uint64_t)(uint32_t)d[20] | ((uint64_t)(uint32_t)d[21] << 32));
    if (im.blk0 < 0 || im.blk0 > total_blocks - im.nblk) {
        im.blk0 = clampl(im.blk0, 0, total_blocks);
        flag |= ST_BAD_DESC;
    }
    return im;
}

__device__ __forceinline__ int64_t ws_block(const Image& im, int64_t local, int64_t total_blocks) {
    return clampl(im.blk0 + local, 0, total_blocks - 1);
}

// (meta_len >= JHUFF is checked on the host, so the range is never empty)
__device__ __forceinline__ int table_at(int64_t idx, int size, int meta_len) { return (int)clampl(idx, 0, meta_len - size); }

// ---- 1. entropy decode -------------------------------------------------------------------------------------------------------------

struct HuffLds {
    uint16_t look[256];       // 8-bit prefix -> length << 8 | symbol; 0 = a longer code
    uint8_t val[256];
    int maxcode[17];          // largest code of each length, -1 = none
    int valoff[17];           // index of the first symbol of a length minus its first code
};

struct Reader {
    const uint8_t* src;
    u32x4* win;               // this lane's 16-byte window in LDS
    int64_t last_chunk;       // src_bytes / 16 - 1
    u32x4 pend;               // the next window, its load in flight
    uint64_t acc;
    uint32_t cw;              // the word of the window that holds byte p
    int p, end, n, fake;      // byte position, segment end, valid bits in acc, zero bits fed at the tail of acc
    bool done;

    __device__ __forceinline__ u32x4 chunk(int64_t c) const {
        c = c < 0 ? 0 : (c > last_chunk ? last_chunk : c);
        return *reinterpret_cast<const u32x4*>(src + c * 16);
    }
    __device__ __forceinline__ void start(int p0, int e) {
        p = p0, end = e, acc = 0, n = 0, fake = 0, done = false;
        *win = chunk(p >> 4);
        pend = chunk((p >> 4) + 1);
        cw = reinterpret_cast<const uint32_t*>(win)[(p >> 2) & 3];
    }
    __device__ __forceinline__ int cur() const { return (cw >> (8 * (p & 3))) & 255; }
    __device__ __forceinline__ void advance() {
        ++p;
        if ((p & 3) == 0) {
            if ((p & 15) == 0) {
                *win = pend;
                pend = chunk((p >> 4) + 1);
            }
            cw = reinterpret_cast<const uint32_t*>(win)[(p >> 2) & 3];
        }
    }
    // At least 57 valid bits afterwards.  A stuffed FF 00 is the data byte FF; any other FF xx, or the segment's end, ends the data:
    // zero bits follow (counted in `fake`, which stays the number of made-up bits at the tail of acc while it is <= n).
    __device__ __forceinline__ void fill() {
#pragma unroll 1
        for (int i = 0; i < 8 && n <= 56; ++i) {
            int v = 0;
            if (!done && p < end) {
                v = cur();
                advance();
                if (v == 0xFF) {
                    if (p < end && cur() == 0) {
                        advance();
                    } else {
                        done = true;
                        v = 0;
                    }
                }
            } else {
                done = true;
            }
            if (done) fake = min(fake + 8, 128);
            acc = (acc << 8) | (uint64_t)v;
            n += 8;
        }
    }
    __device__ __forceinline__ int bits(int k) {      // 0 <= k <= 16 <= n
        const int v = (int)((acc >> (n - k)) & ((1u << k) - 1));
        n -= k;
        return v;
    }
};

// One Huffman symbol, or -1 when no code matches.  Leaves at least 41 valid bits for the value that follows.
__device__ __forceinline__ int symbol(Reader& r, const HuffLds& h) {
    r.fill();
    const int look = (int)((r.acc >> (r.n - 16)) & 0xFFFF);
    const int e = h.look[look >> 8];
    if (e) {
        r.n -= e >> 8;
        return e & 255;
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = look >> (16 - l);
        if (code <= h.maxcode[l]) {
            r.n -= l;
            return h.val[clampi(h.valoff[l] + code, 0, 255)];
        }
    }
    return -1;
}

__device__ __forceinline__ int extend(int v, int s) { return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1; }

__global__ void __launch_bounds__(JE_THREADS)
jpeg_entropy_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ meta, int meta_len, int16_t* __restrict__ coef,
                    int64_t total_blocks, int* __restrict__ status) {
    __shared__ HuffLds huff[6];                      // DC of components 0..2, AC of components 0..2
    __shared__ u32x4 window[JE_LANES];
    __shared__ uint8_t zigzag[64];
    const int img = blockIdx.y, lane = threadIdx.x;
    const int* d = meta + (size_t)img * JD;
    int flag = 0;
    const Image im = load_image(d, total_blocks, flag);
    const int nseg = clampi(d[5], 0, im.mw * im.mh);
    if (blockIdx.x == 0 && lane == 0 && (flag || nseg != d[5])) atomicOr(status + img, ST_BAD_DESC);
    if ((int)blockIdx.x * JE_LANES >= nseg) return;

    zigzag[lane] = JPEG_ZIGZAG[lane];
    for (int t = 0; t < 2 * im.ncomp; ++t) {
        HuffLds& h = huff[t < im.ncomp ? t : 3 + t - im.ncomp];
        const int* tab = meta + table_at(d[(t < im.ncomp ? 9 : 12 - im.ncomp) + t], JHUFF, meta_len);
        int maxcode[17], valoff[17];
        int code = 0, k = 0;
#pragma unroll
        for (int l = 1; l <= 16; ++l) {
            const int b = clampi(tab[l - 1], 0, 256);
            valoff[l] = k - code;
            k += b;
            code += b;
            maxcode[l] = b ? code - 1 : -1;
            code <<= 1;
        }
        const uint32_t w = (uint32_t)tab[16 + lane];
        reinterpret_cast<uint32_t*>(h.val)[lane] = w;
        if (lane < 17) {
            int mc = -1, vo = 0;
#pragma unroll
            for (int l = 1; l <= 16; ++l)
                if (l == lane) mc = maxcode[l], vo = valoff[l];
            h.maxcode[lane] = mc;
            h.valoff[lane] = vo;
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) {
            const int pre = lane + 64 * j;
            int e = 0;
#pragma unroll
            for (int l = 8; l >= 1; --l) {
                const int c = pre >> (8 - l);
                if (c <= maxcode[l]) e = (l << 8) | h.val[clampi(valoff[l] + c, 0, 255)];
            }
            h.look[pre] = (uint16_t)e;
        }
    }
    __syncthreads();

    const int nmcu = im.mw * im.mh;
    const int seg_at = d[4];
    for (int s0 = blockIdx.x * JE_LANES; s0 < nseg; s0 += JE_GRID * JE_LANES) {
        const int s = s0 + lane;
        if (lane >= JE_LANES || s >= nseg) continue;
        const int* sg = meta + table_at((int64_t)seg_at + (int64_t)s * JSEG, JSEG, meta_len);
        const int64_t off = clampl(sg[0], 0, src_bytes);
        const int64_t len = clampl(sg[1], 0, src_bytes - off);
        const int first = clampi(sg[2], 0, nmcu);
        const int count = clampi(sg[3], 0, nmcu - first);
        Reader r;
        r.src = src;
        r.win = window + lane;
        r.last_chunk = src_bytes / 16 - 1;
        r.start((int)off, (int)(off + len));
        int pred[3] = {0, 0, 0};
        int err = 0;
        for (int m = 0; m < count && !err; ++m) {
            const int my = (first + m) / im.mw, mx = (first + m) % im.mw;
            for (int c = 0; c < im.ncomp && !err; ++c) {
                const int hv = c == 0 ? im.hs : 1;
                const int bw = c == 0 ? im.bw0 : im.bw1;
                const int64_t base = c == 0 ? 0 : (int64_t)im.nb0 + (int64_t)(c - 1) * im.mw * im.mh;
                for (int b = 0; b < hv * hv && !err; ++b) {
                    const int by = my * hv + b / hv, bx = mx * hv + b % hv;
                    int16_t* blk = coef + ws_block(im, base + (int64_t)by * bw + bx, total_blocks) * 64;
                    const int t = symbol(r, huff[c]);
                    if (t < 0 || t > 11) {
                        err |= ST_BAD_CODE;
                        break;
                    }
                    const int p = clampi(pred[c] + extend(r.bits(t), t), -32768, 32767);
                    pred[c] = p;
                    blk[0] = (int16_t)p;
                    int k = 1;
                    for (int it = 0; it < 63 && k <= 63; ++it) {
                        const int rs = symbol(r, huff[3 + c]);
                        if (rs < 0) {
                            err |= ST_BAD_CODE;
                            break;
                        }
                        const int run = rs >> 4, size = rs & 15;
                        if (size == 0) {
                            if (run != 15) break;
                            k += 16;
                            continue;
                        }
                        k += run;
                        if (k > 63) {
                            err |= ST_BAD_INDEX;
                            break;
                        }
                        blk[zigzag[k]] = (int16_t)extend(r.bits(size), size);
                        ++k;
                    }
                    if (!err && r.n < r.fake) err |= ST_OVERRUN;
                }
            }
        }
        if (!err) {                                      // a whole byte or more of the segment left undecoded
            r.fill();
            if (r.n - r.fake >= 8) err = ST_LEFTOVER;
        }
        if (err) atomicOr(status + img, err);
    }
}

// ---- 2. dequantise + IDCT ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void idct_1d(const int64_t (&x)[8], int64_t (&o)[8], int shift) {
    int64_t z1 = (x[2] + x[6]) * 4433;
    const int64_t t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
    const int64_t t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int64_t a = x[7], b = x[5], c = x[3], d = x[1];
    z1 = a + d;
    int64_t z2 = b + c, z3 = a + c, z4 = b + d;
    const int64_t z5 = (z3 + z4) * 9633;
    a *= 2446, b *= 16819, c *= 25172, d *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
    const int64_t r = (int64_t)1 << (shift - 1);
    o[0] = (t10 + d + r) >> shift, o[7] = (t10 - d + r) >> shift;
    o[1] = (t11 + c + r) >> shift, o[6] = (t11 - c + r) >> shift;
    o[2] = (t12 + b + r) >> shift, o[5] = (t12 - b + r) >> shift;
    o[3] = (t13 + a + r) >> shift, o[4] = (t13 - a + r) >> shift;
}

__global__ void __launch_bounds__(JI_THREADS)
jpeg_idct_kernel(const int* __restrict__ meta, int meta_len, const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, int64_t total_blocks) {
    const int img = blockIdx.y;
    const int* d = meta + (size_t)img * JD;
    int flag = 0;
    const Image im = load_image(d, total_blocks, flag);
    for (int64_t g = (int64_t)blockIdx.x * JI_THREADS + threadIdx.x; g < im.nblk; g += (int64_t)JI_GRID * JI_THREADS) {
        const int c = g < im.nb0 ? 0 : (g - im.nb0 < (int64_t)im.mw * im.mh ? 1 : 2);
        const int64_t cbase = c == 0 ? 0 : (int64_t)im.nb0 + (int64_t)(c - 1) * im.mw * im.mh;
        const int bw = c == 0 ? im.bw0 : im.bw1;
        const int by = (int)((g - cbase) / bw), bx = (int)((g - cbase) % bw);
        const int* q = meta + table_at(d[6 + c], 64, meta_len);
        const int16_t* blk = coef + ws_block(im, g, total_blocks) * 64;
        int64_t ws[64];
#pragma unroll
        for (int col = 0; col < 8; ++col) {               // pass 1: columns of the dequantised block
            int64_t x[8], o[8];
#pragma unroll
            for (int row = 0; row < 8; ++row) x[row] = (int64_t)blk[row * 8 + col] * (int64_t)q[row * 8 + col];
            idct_1d(x, o, 11);
#pragma unroll
            for (int row = 0; row < 8; ++row) ws[row * 8 + col] = o[row];
        }
        // the block's rows go to the component plane of bw * 8 bytes per row, the component's blocks in raster order
        const int64_t pbase = clampl(im.blk0 + cbase, 0, total_blocks - 1) * 64;
#pragma unroll
        for (int row = 0; row < 8; ++row) {               // pass 2: rows
            int64_t x[8], o[8];
#pragma unroll
            for (int col = 0; col < 8; ++col) x[col] = ws[row * 8 + col];
            idct_1d(x, o, 18);
            uint32_t w[2] = {0, 0};
#pragma unroll
            for (int col = 0; col < 8; ++col) {
                const int64_t v = o[col] + 128;
                w[col >> 2] |= (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * (col & 3));
            }
            const int64_t at = clampl(pbase + ((int64_t)by * 8 + row) * bw * 8 + bx * 8, 0, total_blocks * 64 - 8);
            *reinterpret_cast<u32x2*>(planes + at) = u32x2{w[0], w[1]};
        }
    }
}

// ---- 3. upsample + colour + store ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(JC_THREADS)
jpeg_colour_kernel(const int* __restrict__ meta, const uint8_t* __restrict__ planes, int64_t total_blocks, uint8_t* __restrict__ y, int64_t y_bytes) {
    const int img = blockIdx.y;
    const int* d = meta + (size_t)img * JD;
    int flag = 0;
    const Image im = load_image(d, total_blocks, flag);
    const int64_t off = clampl((int64_t)((uint64_t)(uint32_t)d[15] | ((uint64_t)(uint32_t)d[16] << 32)), -y_bytes, y_bytes) + d[19];
    const int64_t rs = d[17], ps = d[18];
    const int64_t pmax = total_blocks * 64 - 1;
    const uint8_t* p0 = planes;
    const int64_t b0 = clampl(im.blk0, 0, total_blocks - 1) * 64;
    const int64_t b1 = clampl(im.blk0 + im.nb0, 0, total_blocks - 1) * 64;
    const int64_t b2 = clampl(im.blk0 + im.nb0 + (int64_t)im.mw * im.mh, 0, total_blocks - 1) * 64;
    const int pw0 = im.bw0 * 8, pw1 = im.bw1 * 8;
    const int ch = (im.H + 1) >> 1, cw = (im.W + 1) >> 1;
    const int64_t npix = (int64_t)im.H * im.W;
    for (int64_t i = (int64_t)blockIdx.x * JC_THREADS + threadIdx.x; i < npix; i += (int64_t)JC_GRID * JC_THREADS) {
        const int py = (int)(i / im.W), px = (int)(i % im.W);
        const int Y = p0[min(b0 + (int64_t)py * pw0 + px, pmax)];
        const int64_t o = off + py * rs + px * ps;
        if (im.ncomp == 1) {
            y[clampl(o, 0, y_bytes - 1)] = (uint8_t)Y;
            continue;
        }
        int cb, cr;
        if (im.hs == 1) {
            cb = p0[min(b1 + (int64_t)py * pw1 + px, pmax)];
            cr = p0[min(b2 + (int64_t)py * pw1 + px, pmax)];
        } else {
            const int r = py >> 1, c = px >> 1;
            const int nb = (py & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
            const int cn = (px & 1) ? min(c + 1, cw - 1) : max(c - 1, 0);
            const bool edge = cn == c;
            const int64_t a = (int64_t)r * pw1, b = (int64_t)nb * pw1;
            const int bias = (px & 1) ? 7 : 8;
            int s = 3 * p0[min(b1 + a + c, pmax)] + p0[min(b1 + b + c, pmax)];
            int sn = 3 * p0[min(b1 + a + cn, pmax)] + p0[min(b1 + b + cn, pmax)];
            cb = ((edge ? 4 * s : 3 * s + sn) + bias) >> 4;
            s = 3 * p0[min(b2 + a + c, pmax)] + p0[min(b2 + b + c, pmax)];
            sn = 3 * p0[min(b2 + a + cn, pmax)] + p0[min(b2 + b + cn, pmax)];
            cr = ((edge ? 4 * s : 3 * s + sn) + bias) >> 4;
        }
        cb -= 128, cr -= 128;
        const int R = Y + ((91881 * cr + 32768) >> 16);
        const int B = Y + ((116130 * cb + 32768) >> 16);
        const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        y[clampl(o, 0, y_bytes - 1)] = (uint8_t)clampi(R, 0, 255);
        y[clampl(o + 1, 0, y_bytes - 1)] = (uint8_t)clampi(G, 0, 255);
        y[clampl(o + 2, 0, y_bytes - 1)] = (uint8_t)clampi(B, 0, 255);
    }
}

}  // namespace

extern "C" size_t adamml_jpeg_decode_workspace(int64_t total_blocks) {
    return total_blocks < 1 ? 0 : (size_t)total_blocks * 192;      // int16 coefficients + uint8 planes, 64 of each per block
}

extern "C" int adamml_jpeg_decode_u8(const uint8_t* src, int64_t src_bytes, const int32_t* meta, int meta_len, uint8_t* y, int64_t y_bytes,
                                     int32_t* status, void* workspace, int64_t workspace_bytes, int N, hipStream_t stream) {
    if (N < 0 || N > 65535) return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: N = %d outside [0, 65535]", N);
    if (N == 0) return ADAMML_OK;
    if ((int64_t)meta_len < (int64_t)N * JD + JHUFF)
        return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: meta_len = %d < N * %d descriptor ints + %d (one table)", meta_len, JD, JHUFF);
    if (src_bytes < 16 || src_bytes % 16 != 0 || src_bytes > 0x7ffffff0)
        return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: src_bytes = %lld must be a multiple of 16 in [16, 2^31 - 16]", (long long)src_bytes);
    if (y_bytes < 1) return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: y_bytes = %lld < 1", (long long)y_bytes);
    if (workspace_bytes < 192)
        return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: workspace_bytes = %lld < 192 (one block)", (long long)workspace_bytes);
    if (!src || !meta || !y || !status || !workspace) return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: null argument");
    if (((uintptr_t)src & 15) || ((uintptr_t)workspace & 15))
        return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: src and workspace must be 16-byte aligned");
    const int64_t total_blocks = workspace_bytes / 192;
    int16_t* coef = static_cast<int16_t*>(workspace);
    uint8_t* planes = static_cast<uint8_t*>(workspace) + total_blocks * 128;
    if (hipMemsetAsync(coef, 0, (size_t)total_blocks * 128, stream) != hipSuccess || hipMemsetAsync(status, 0, (size_t)N * 4, stream) != hipSuccess)
        return adamml_set_error(ADAMML_EINVAL, "jpeg_decode_u8: clearing the workspace failed");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(JE_GRID, N), dim3(JE_THREADS), 0, stream, src, src_bytes, meta, meta_len, coef, total_blocks, status);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(JI_GRID, N), dim3(JI_THREADS), 0, stream, meta, meta_len, coef, planes, total_blocks);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(JC_GRID, N), dim3(JC_THREADS), 0, stream, meta, planes, total_blocks, y, y_bytes);
    return adamml_check_launch("jpeg_decode_u8");
}
