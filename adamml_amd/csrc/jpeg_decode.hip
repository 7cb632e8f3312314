// Baseline JPEG frames decoded on the GPU, byte-exact to libjpeg(-turbo) as Pillow uses it (utils/video_dataset.py:51-66 opens every
// frame with PIL.Image.open; adamml_amd/jpeg.py parses the headers and packs the batch).  Four kernels on one stream:
//
//   0. jpeg_parallel_kernel  Huffman decode of the images whose scan is ONE segment (no restart markers): self-synchronising
//      subsequences, one lane each, one workgroup per image (section 1b below).  It returns at once for every other image, and an
//      image it cannot vouch for (anything but a clean stream) it hands to kernel 1 through a word in the image's plane region.
//   1. jpeg_entropy_kernel   Huffman decode of every other image, and of those kernel 0 gave up (their coefficients cleared
//      first); it returns at once for the images kernel 0 finished.  Segments (the scan split at its restart markers) are independent and sequential: one
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
// more left over after its last MCU.  Nothing traps or spins.  Kernel 0 keeps to the same rules: its rounds number at most the
// (clamped) subsequence count, a subsequence's decode at most its bits, its records live in LDS at indices below that count, its
// bytes come from inside the segment the record names (checked against src_bytes before anything is read), and it waits on nothing
// but its own workgroup's barriers.  Status is kernel 1's alone: what kernel 0 keeps is an image on which both agree, bit for bit.
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

// The image's Huffman tables and the zigzag order into LDS: the work of 64 lanes (`active`: lane < 64); every thread of the workgroup
// calls it (it holds barriers).
__device__ __forceinline__ void build_tables(HuffLds* huff, uint8_t* zigzag, const int* __restrict__ d, const Image& im,
                                             const int* __restrict__ meta, int meta_len, int lane, bool active) {
    if (active) zigzag[lane] = JPEG_ZIGZAG[lane];
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
        if (active) {
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
        }
        __syncthreads();
        for (int j = 0; j < 4 && active; ++j) {
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
}

// ---- 1b. entropy decode of a marker-less scan: self-synchronising subsequences ------------------------------------------------------
//
// A scan without restart markers is ONE segment; jpeg_entropy_kernel would walk it with one lane.  jpeg_parallel_kernel cuts it into
// subsequences of JP_SUBSEQ raw bytes (byte stuffing in place), one lane each, one workgroup per image:
//   1. every lane decodes its subsequence from a GUESSED state (bit position = its first byte, block 0 of an MCU, DC next) up to the
//      subsequence's end and records its exit state and the blocks it completed;
//   2. rounds of "decode my subsequence again from my predecessor's exit state" (only the lanes whose input changed) until a round
//      changes nothing: subsequence 0 starts from the true state, so after round i subsequence i does too -- at most as many rounds
//      as subsequences, far fewer on real content because a Huffman decoder started at a wrong bit falls into step within a few
//      dozen symbols.  A guessed state that meets a code no table entry matches just records "unknown", which its successor
//      ignores (from a true state it is the stream that is bad: step 3 meets the same code again and gives the image up);
//   3. a prefix sum of the block counts gives every subsequence its first block; one more decode from the now TRUE states stores the
//      coefficients, the DC coefficient as the DIFFERENCE the stream holds;
//   4. per component a prefix sum of the DC differences in scan order.
// A state is one word: raw bit position << 9 | block in MCU << 6 | next zigzag index (0 = DC next).  The position always names a
// data byte, never the 00 of a stuffed FF 00: whoever consumes the last bit of an FF steps over the 00 with it.  A subsequence owns
// the symbols (code + magnitude bits) that BEGIN in its bytes, so one that begins inside a code or inside magnitude bits starts
// where its predecessor stopped, a few bits in.
// JP_SUBSEQ = 128: synchronisation costs about as many symbols whatever the size, so the rounds fall with the size (18 at 128 B, 12
// at 256 B on a full frame) while the lanes per frame -- the point of the exercise -- fall too; at 128 B a 44 KB frame has 340
// lanes, its 18 rounds decode every subsequence 2.3 times on average, and JP_MAXSUB = 2048 records (24 KB of LDS) cover files up to
// 256 KB.  Measured on a step's 2 880 frames of 50 KB (profiles/jpeg_decode.json): 64 B 23.7 ms, 128 B 23.1 ms, 256 B 21.9 ms for the
// whole decode -- the IDCT and colour stages dominate, and 256 B is the next thing to try.
// The stage takes no decision about a damaged stream: whenever what it sees could differ from the sequential walk in status or in a
// single coefficient (an unknown state after the rounds, a bad code / index / DC category from a true state, a marker, a block count
// that is not the image's, a stream that overruns or has a byte or more left over, a DC prefix outside int16 where the sequential
// walk saturates per step) it sets the image's "gave up" word -- the first word of the image's own plane region, idle until the
// IDCT -- and jpeg_entropy_kernel, launched after it over all images, clears the image's coefficients and decodes it as ever.

constexpr int JP_SUBSEQ = ADAMML_JPEG_SUBSEQ_BYTES;
constexpr int JP_MAXSUB = 2048;
constexpr int JP_THREADS = 256;
constexpr int JP_PER = JP_MAXSUB / JP_THREADS;     // subsequences per thread at the cap
constexpr uint32_t JP_UNKNOWN = 0xFFFFFFFFu;

// Whether image `d` takes the parallel stage -- structural, the same answer in both entropy kernels: one segment that is the whole
// scan, nothing clamped, at most JP_MAXSUB subsequences.  off / len: the segment's bytes.
__device__ __forceinline__ bool parallel_eligible(const int* __restrict__ d, const int* __restrict__ meta, int meta_len, int64_t src_bytes,
                                                  const Image& im, int flag, int& off, int& len) {
    off = 0, len = 0;
    if (flag || d[5] != 1 || d[4] < 0 || d[4] > meta_len - JSEG) return false;
    const int* sg = meta + d[4];
    if (sg[0] < 0 || sg[1] < 1 || sg[1] > JP_MAXSUB * JP_SUBSEQ || (int64_t)sg[0] + sg[1] > src_bytes) return false;
    if (sg[2] != 0 || sg[3] != im.mw * im.mh) return false;
    off = sg[0], len = sg[1];
    return true;
}

__device__ __forceinline__ int* gave_up_word(uint8_t* planes, const Image& im, int64_t total_blocks) {
    return reinterpret_cast<int*>(planes + clampl(im.blk0, 0, total_blocks - 1) * 64);
}

// Bit reader that knows where it is: `pos` is the raw bit position (relative to the segment) of the next unconsumed bit.  `stf` runs
// beside `acc` with a 1 at the last bit of every FF data byte, whose consumption carries `pos` over the stuffed 00 as well.  Bytes
// come from the segment through an aligned 8-byte word; from the segment's end on they are zero.
struct PReader {
    const uint8_t* src;       // the whole buffer: 16-byte aligned, a multiple of 16 bytes
    int off, len;             // the segment: off + len <= src_bytes
    uint64_t acc, stf, cw;
    int64_t cwi;
    int n, p, pos;
    bool marker;              // an FF that no 00 follows was loaded

    __device__ __forceinline__ int byte(int i) {
        if (i < 0 || i >= len) return 0;
        const int64_t a = (int64_t)off + i;
        if ((a >> 3) != cwi) {
            cwi = a >> 3;
            cw = *reinterpret_cast<const uint64_t*>(src + cwi * 8);
        }
        return (int)((cw >> (8 * (a & 7))) & 255);
    }
    __device__ __forceinline__ void fill() {
#pragma unroll 1
        for (int i = 0; i < 8 && n <= 56; ++i) {
            const int v = byte(p);
            ++p;
            const bool ff = v == 0xFF;
            if (ff) {
                if (byte(p) == 0 && p < len)
                    ++p;
                else
                    marker = true;
            }
            acc = (acc << 8) | (uint64_t)v;
            stf = (stf << 8) | (uint64_t)(ff ? 1 : 0);
            n += 8;
        }
    }
    __device__ __forceinline__ void start(int pos0) {
        pos = pos0, p = pos0 >> 3, acc = 0, stf = 0, n = 0, cwi = -1, cw = 0, marker = false;
        fill();
        n -= pos0 & 7;
    }
    __device__ __forceinline__ void consume(int k) {                // 0 <= k <= 16 <= n
        const uint64_t m = (stf >> (n - k)) & ((1u << k) - 1);
        pos += k + 8 * __popcll(m);
        n -= k;
    }
    __device__ __forceinline__ int bits(int k) {
        const int v = (int)((acc >> (n - k)) & ((1u << k) - 1));
        consume(k);
        return v;
    }
};

__device__ __forceinline__ int psymbol(PReader& r, const HuffLds& h) {
    r.fill();
    const int look = (int)((r.acc >> (r.n - 16)) & 0xFFFF);
    const int e = h.look[look >> 8];
    if (e) {
        r.consume(e >> 8);
        return e & 255;
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = look >> (16 - l);
        if (code <= h.maxcode[l]) {
            r.consume(l);
            return h.val[clampi(h.valoff[l] + code, 0, 255)];
        }
    }
    return -1;
}

// Block `g` of the image in scan order (block `rr` of its MCU) -> its 64 coefficients in the workspace.
__device__ __forceinline__ int16_t* scan_block(int16_t* __restrict__ coef, const Image& im, int64_t total_blocks, int64_t g, int rr, int bpm) {
    const int m = (int)(g / bpm);
    const int hs2 = im.hs * im.hs;
    const int c = im.ncomp == 1 ? 0 : (rr < hs2 ? 0 : rr - hs2 + 1);
    const int hv = c == 0 ? im.hs : 1, b = c == 0 ? rr : 0;
    const int bw = c == 0 ? im.bw0 : im.bw1;
    const int64_t base = c == 0 ? 0 : (int64_t)im.nb0 + (int64_t)(c - 1) * im.mw * im.mh;
    const int by = (m / im.mw) * hv + b / hv, bx = (m % im.mw) * hv + b % hv;
    return coef + ws_block(im, base + (int64_t)by * bw + bx, total_blocks) * 64;
}

// Decode the symbols that begin in [state's position, end) from state `st`; returns the exit state, or JP_UNKNOWN when a code, an
// index or a DC category is bad.  count: blocks completed.  STORE: block `g` (scan order) is the one in progress at `st`; stops at
// the image's last block; coefficients are stored, the DC as its difference; fail: set when the image must take the sequential walk.
template <bool STORE>
__device__ __forceinline__ uint32_t decode_subsequence(PReader& r, uint32_t st, int end, const Image& im, int bpm, const HuffLds* huff,
                                                       const uint8_t* zigzag, int& count, int16_t* __restrict__ coef, int64_t total_blocks,
                                                       int64_t g, bool last, bool& fail) {
    count = 0;
    if (st == JP_UNKNOWN) {
        fail = true;
        return JP_UNKNOWN;
    }
    int rr = min((int)((st >> 6) & 7), bpm - 1), k = (int)(st & 63);
    const int hs2 = im.hs * im.hs;
    r.start((int)(st >> 9));
    int16_t* blk = nullptr;
    if (STORE) {
        if (g % bpm != rr) fail = true;
        blk = scan_block(coef, im, total_blocks, g, rr, bpm);
    }
    bool bad = false;
#pragma unroll 1
    for (int it = 0; it < JP_SUBSEQ * 8 + 64 && r.pos < end; ++it) {      // every symbol is at least one bit
        if (STORE && g >= im.nblk) break;
        const int c = im.ncomp == 1 ? 0 : (rr < hs2 ? 0 : rr - hs2 + 1);
        if (k == 0) {
            const int t = psymbol(r, huff[c]);
            if (t < 0 || t > 11) {
                bad = true;
                break;
            }
            const int v = extend(r.bits(t), t);
            if (STORE) blk[0] = (int16_t)v;
            k = 1;
        } else {
            const int rs = psymbol(r, huff[3 + c]);
            if (rs < 0) {
                bad = true;
                break;
            }
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                k = run == 15 ? k + 16 : 64;
            } else {
                k += run;
                if (k > 63) {
                    bad = true;
                    break;
                }
                const int v = extend(r.bits(size), size);
                if (STORE) blk[zigzag[k]] = (int16_t)v;
                ++k;
            }
        }
        if (k >= 64) {
            k = 0;
            rr = rr + 1 == bpm ? 0 : rr + 1;
            ++count;
            if (STORE) {
                ++g;
                blk = scan_block(coef, im, total_blocks, g, rr, bpm);
            }
        }
    }
    if (STORE) {
        const int stream_end = r.len * 8;
        if (bad || r.marker || r.pos > stream_end) fail = true;           // bad stream, a marker, or bits from past the end
        if (r.pos < end) {                                                // stopped at the image's last block: what is left over?
            const int at = r.pos >> 3;
            const int whole = (r.pos & 7) == 0 ? at : (r.byte(at) == 0xFF ? at + 2 : at + 1);      // the first untouched data byte
            if (g < im.nblk || whole < r.len) fail = true;
        }
        if (last && g != im.nblk) fail = true;                            // the stream ended before the image did
    }
    if (bad) return JP_UNKNOWN;
    return ((uint32_t)min(r.pos, (1 << 22) - 1) << 9) | ((uint32_t)rr << 6) | (uint32_t)k;
}

__global__ void __launch_bounds__(JP_THREADS)
jpeg_parallel_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ meta, int meta_len, int16_t* __restrict__ coef,
                     uint8_t* __restrict__ planes, int64_t total_blocks) {
    __shared__ HuffLds huff[6];
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t s_in[JP_MAXSUB], s_out[JP_MAXSUB];      // entry and exit state per subsequence; s_out later: its first block
    __shared__ int s_cnt[JP_MAXSUB];                            // blocks it completed
    __shared__ int64_t s_scan[JP_THREADS];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int* d = meta + (size_t)img * JD;
    int flag = 0, off, len;
    const Image im = load_image(d, total_blocks, flag);
    if (!parallel_eligible(d, meta, meta_len, src_bytes, im, flag, off, len)) return;
    build_tables(huff, zigzag, d, im, meta, meta_len, tid, tid < 64);

    const int nsub = clampi((len + JP_SUBSEQ - 1) / JP_SUBSEQ, 1, JP_MAXSUB);
    const int bpm = im.ncomp == 3 ? im.hs * im.hs + 2 : 1;
    PReader r;
    r.src = src, r.off = off, r.len = len;
    r.start(0);

    // 1. guessed starts (subsequence 0: the true one); a subsequence that begins on the 00 of a stuffed FF 00 begins one byte later
    unsigned need = 0;
    for (int j = 0; j < JP_PER; ++j) {
        const int i = tid + j * JP_THREADS;
        if (i >= nsub) break;
        int at = i * JP_SUBSEQ;
        if (i > 0 && r.byte(at) == 0 && r.byte(at - 1) == 0xFF) ++at;
        s_in[i] = (uint32_t)(at * 8) << 9;
        need |= 1u << j;
    }
    // 2. rounds: decode where the entry state changed, then take the predecessor's exit state
    bool fail = false, settled = false;
#pragma unroll 1
    for (int round = 0; round < nsub; ++round) {
        for (int j = 0; j < JP_PER; ++j) {
            const int i = tid + j * JP_THREADS;
            if (i >= nsub || !((need >> j) & 1)) continue;
            int count = 0;
            bool ignored = false;
            s_out[i] = decode_subsequence<false>(r, s_in[i], min((i + 1) * JP_SUBSEQ, len) * 8, im, bpm, huff, zigzag, count, coef, total_blocks,
                                                 0, false, ignored);
            s_cnt[i] = count;
        }
        __syncthreads();
        need = 0;
        for (int j = 0; j < JP_PER; ++j) {
            const int i = tid + j * JP_THREADS;
            if (i >= nsub || i == 0) continue;
            const uint32_t from = s_out[i - 1];
            if (from != JP_UNKNOWN && from != s_in[i]) {             // an unknown exit tells its successor nothing
                s_in[i] = from;
                need |= 1u << j;
            }
        }
        if (!__syncthreads_or(need != 0)) {              // the workgroup's "nothing changed"
            settled = true;
            break;
        }
    }
    fail = !settled;
    // 3. first block of every subsequence: thread t sums the JP_PER consecutive counts from t * JP_PER, the threads scan
    int64_t sum = 0;
    for (int j = 0; j < JP_PER; ++j) {
        const int i = tid * JP_PER + j;
        if (i < nsub) {
            sum += s_cnt[i];
            if (s_in[i] == JP_UNKNOWN) fail = true;
        }
    }
    s_scan[tid] = sum;
    __syncthreads();
    for (int step = 1; step < JP_THREADS; step <<= 1) {
        const int64_t add = tid >= step ? s_scan[tid - step] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    int64_t first = s_scan[tid] - sum;
    for (int j = 0; j < JP_PER; ++j) {
        const int i = tid * JP_PER + j;
        if (i < nsub) {
            s_out[i] = (uint32_t)clampl(first, 0, 0x7fffffff);
            first += s_cnt[i];
        }
    }
    if (!__syncthreads_or(fail)) {
        for (int j = 0; j < JP_PER; ++j) {
            const int i = tid + j * JP_THREADS;
            if (i >= nsub) break;
            int count = 0;
            decode_subsequence<true>(r, s_in[i], min((i + 1) * JP_SUBSEQ, len) * 8, im, bpm, huff, zigzag, count, coef, total_blocks,
                                     (int64_t)s_out[i], i == nsub - 1, fail);
        }
    }
    // 4. DC: per component the prefix sum of the differences in scan order, thread t a run of consecutive blocks
    if (!__syncthreads_or(fail)) {
        for (int c = 0; c < im.ncomp; ++c) {
            const int rr0 = c == 0 ? 0 : im.hs * im.hs + c - 1;
            const int per_mcu = c == 0 ? im.hs * im.hs : 1;
            const int64_t nb = c == 0 ? im.nb0 : (int64_t)im.mw * im.mh;
            const int64_t chunk = (nb + JP_THREADS - 1) / JP_THREADS;
            const int64_t lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
            sum = 0;
            for (int64_t b = lo; b < hi; ++b) sum += *scan_block(coef, im, total_blocks, b / per_mcu * bpm, rr0 + (int)(b % per_mcu), bpm);
            __syncthreads();
            s_scan[tid] = sum;
            __syncthreads();
            for (int step = 1; step < JP_THREADS; step <<= 1) {
                const int64_t add = tid >= step ? s_scan[tid - step] : 0;
                __syncthreads();
                s_scan[tid] += add;
                __syncthreads();
            }
            int64_t pred = s_scan[tid] - sum;
            for (int64_t b = lo; b < hi; ++b) {
                int16_t* dc = scan_block(coef, im, total_blocks, b / per_mcu * bpm, rr0 + (int)(b % per_mcu), bpm);
                pred += *dc;
                if (pred < -32768 || pred > 32767) fail = true;         // the sequential walk saturates here: leave it to it
                *dc = (int16_t)clampl(pred, -32768, 32767);
            }
        }
    }
    const int gave_up = __syncthreads_or(fail);
    if (tid == 0) *gave_up_word(planes, im, total_blocks) = gave_up ? 1 : 0;
}

__global__ void __launch_bounds__(JE_THREADS)
jpeg_entropy_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ meta, int meta_len, int16_t* __restrict__ coef,
                    uint8_t* __restrict__ planes, int64_t total_blocks, int* __restrict__ status) {
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
    int par_off, par_len;
    if (parallel_eligible(d, meta, meta_len, src_bytes, im, flag, par_off, par_len)) {      // jpeg_parallel_kernel had this image:
        if (*gave_up_word(planes, im, total_blocks) == 0) return;                           // done, or it gave up -- then from scratch
        u32x4* mine = reinterpret_cast<u32x4*>(coef + im.blk0 * 64);
        for (int64_t j = lane; j < im.nblk * 8; j += JE_THREADS) mine[j] = u32x4{0, 0, 0, 0};
    }

    build_tables(huff, zigzag, d, im, meta, meta_len, lane, true);

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

extern "C" int adamml_jpeg_decode_parallel_supported(int H, int W, int components, int sampling, int segments, int64_t coded_bytes) {
    if (H < 1 || H > 65535 || W < 1 || W > 65535 || (int64_t)H * W > JPEG_MAX_PIXELS) return 0;
    if ((components != 1 && components != 3) || (sampling != 1 && sampling != 2)) return 0;
    return segments == 1 && coded_bytes >= 1 && coded_bytes <= (int64_t)JP_MAXSUB * JP_SUBSEQ ? 1 : 0;
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
    hipLaunchKernelGGL(jpeg_parallel_kernel, dim3(N), dim3(JP_THREADS), 0, stream, src, src_bytes, meta, meta_len, coef, planes, total_blocks);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(JE_GRID, N), dim3(JE_THREADS), 0, stream, src, src_bytes, meta, meta_len, coef, planes, total_blocks,
                       status);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(JI_GRID, N), dim3(JI_THREADS), 0, stream, meta, meta_len, coef, planes, total_blocks);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(JC_GRID, N), dim3(JC_THREADS), 0, stream, meta, planes, total_blocks, y, y_bytes);
    return adamml_check_launch("jpeg_decode_u8");
}
