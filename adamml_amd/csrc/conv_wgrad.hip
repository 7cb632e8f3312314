// Weight gradient of the dense convs for gfx950: bf16 MFMA over pixel-major (NHWC) operands fetched from LDS with the hardware
// transpose read (ds_read_b64_tr_b16), split over pixels; three kernels (register-staged, LDS-DMA staged, 3x3 LDS patch), the split
// plan shared by the workspace query and the launcher, and the split reduce every one-partial-per-workgroup kernel of the library ends
// with.  Tile primitives: tile.h.
//
// Replaces the weight gradients torch autograd computes for the nn.Conv2d of models/resnet.py:83-113,138,199-210,
// models/sound_mobilenet_v2.py:33-69 and models/policy_net.py:38-95.
#include "common.h"
#include "tile.h"
#include "conv_internal.h"
#include "../../include/adamml_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Weight gradient:  dW[co][ci][kh][kw] += sum_p dz[p][co] * a[p@(kh,kw)][ci]   (fp32 atomics, split over pixels)
// Both operands are pixel-major in HBM (NHWC), i.e. K-major for this GEMM, so MFMA fragments are fetched
// from LDS with the hardware transpose read ds_read_b64_tr_b16.
struct WgradP {
    const bf16_t* dz;      // [N,OH,OW,Cout]
    const bf16_t* x;       // [N,H,W,Cin]
    const float* in_scale;
    const float* in_shift;
    float* dw;             // OIHW fp32, Cin_true input channels
    float* ws;             // optional [nsplit][numel(dw)] partial buffer (plain stores) instead of atomics
    size_t dw_numel;
    int nsplit;
    int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, act, cin_true;
    int P, pix_per_block, n_cotiles, n_tiles, cin_shift, NK;   // NK = KH*KW*Cin: flattened (tap, ci) GEMM-N extent
    size_t gdz, gx;        // element strides between BatchNorm groups (blockIdx.y = group)
    int in_gstride;
    // LZ kernels: lazy transform of the dz operand as well (Gram matrix a^T a of a lazily normalised activation)
    const float* dz_scale;
    const float* dz_shift;
    int dz_act, dz_gstride;
};


template <int BM, int BN, int WPD = 1, bool LZ = false>
__global__ __launch_bounds__(NTHREADS) void conv_wgrad_kernel(WgradP p) {
    constexpr int AROW = BM * 2;            // bytes per LDS row (one pixel)
    constexpr int BROW = BN * 2;
    constexpr int TILE_BYTES = 32 * (AROW + BROW);
    constexpr int MT = BM / 32, NT = BN / 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * TILE_BYTES];

    // block -> (group, pixel split, tile), tile fastest, through the XCD-contiguous bijection: each XCD works through a
    // contiguous run of this list, so the tiles of one pixel range (which all re-read the same dz / activation rows)
    // meet in one L2, and every XCD gets an equal share however few splits there are
    const int lb = (int)xcd_contiguous(blockIdx.x, gridDim.x);
    const int tile = lb % p.n_tiles;
    const int unit = lb / p.n_tiles;
    const int split = unit % p.nsplit, grp = unit / p.nsplit;
    p.dz += (size_t)grp * p.gdz;
    p.x += (size_t)grp * p.gx;
    if (p.in_scale) { p.in_scale += (size_t)grp * p.in_gstride; p.in_shift += (size_t)grp * p.in_gstride; }
    if (LZ && p.dz_scale) { p.dz_scale += (size_t)grp * p.dz_gstride; p.dz_shift += (size_t)grp * p.dz_gstride; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int co0 = (tile % p.n_cotiles) * BM;
    const int n0 = (tile / p.n_cotiles) * BN;           // offset in the flattened (tap, ci) axis
    const int ps = split * p.pix_per_block;
    const int pe = min(p.P, ps + p.pix_per_block);

    constexpr int ACH = BM / 8, BCH = BN / 8;                 // 16-byte chunks per row
    constexpr int AL = (32 * ACH) / NTHREADS, BL = (32 * BCH) / NTHREADS;
    // register prefetch ring: global loads run WPD K steps (of 32 pixels) ahead of the MFMAs.  One K step is ~0.1 us of
    // matrix work but an HBM round trip is 1-2 us: with a one-step look-ahead the layer2-4 problems (3-4 workgroups per CU)
    // sat at 250-450 TFLOP/s and ~2.4 TB/s -- neither roof.  WPD = 4 costs 40 VGPRs (5 -> 3 waves per SIMD), which loses
    // on the HBM-bound layer-1 shapes and on grids with > 4 workgroups per CU, so the launcher picks per problem.
    bf16x8 ra[WPD][AL], rb[WPD][BL];
    bool rbv[WPD][BL];
    bool rav_a[LZ ? WPD : 1][AL];
    int b_kh[BL], b_kw[BL], b_ci[BL], b_n[BL], b_oh[BL], b_ow[BL];
    bool b_ok[BL];
#pragma unroll
    for (int l = 0; l < BL; ++l) {
        int e = tid + l * NTHREADS;
        int row = e / BCH, ch = e - row * BCH;
        int n = n0 + ch * 8;
        b_ok[l] = n < p.NK;
        int tap = n >> p.cin_shift;
        b_ci[l] = n - (tap << p.cin_shift);
        b_kh[l] = tap / p.KW - p.pad;
        b_kw[l] = tap - (tap / p.KW) * p.KW - p.pad;
        int pp = ps + row;                                   // pixel of this chunk at K step 0; advanced by 32 per step
        b_n[l] = pp / (p.OH * p.OW);
        int rem = pp - b_n[l] * (p.OH * p.OW);
        b_oh[l] = rem / p.OW;
        b_ow[l] = rem - b_oh[l] * p.OW;
    }

    auto issue_loads = [&](auto slot_c, int pbase) {
        constexpr int SL = decltype(slot_c)::value;
#pragma unroll
        for (int l = 0; l < AL; ++l) {
            int e = tid + l * NTHREADS;
            int row = e / ACH, ch = e - row * ACH;
            int pp = pbase + row, co = co0 + ch * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (pp < pe && co < p.Cout) v = *reinterpret_cast<const bf16x8*>(p.dz + (size_t)pp * p.Cout + co);
            ra[SL][l] = v;
            if (LZ) rav_a[LZ ? SL : 0][l] = pp < pe && co < p.Cout;
        }
#pragma unroll
        for (int l = 0; l < BL; ++l) {
            int e = tid + l * NTHREADS;
            int row = e / BCH;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            int ih = b_oh[l] * p.stride + b_kh[l], iw = b_ow[l] * p.stride + b_kw[l];
            bool ok = (pbase + row < pe) && b_ok[l] && ih >= 0 && iw >= 0 && ih < p.H && iw < p.W;
            if (ok) v = *reinterpret_cast<const bf16x8*>(p.x + ((size_t)(b_n[l] * p.H + ih) * p.W + iw) * p.Cin + b_ci[l]);
            rbv[SL][l] = ok;
            rb[SL][l] = v;
            // advance this chunk's pixel by one K step (32 output pixels)
            b_ow[l] += 32;
            while (b_ow[l] >= p.OW) { b_ow[l] -= p.OW; ++b_oh[l]; }
            while (b_oh[l] >= p.OH) { b_oh[l] -= p.OH; ++b_n[l]; }
        }
    };
    auto store_tile = [&](auto slot_c, int buf) {
        constexpr int SL = decltype(slot_c)::value;
        char* base = smem + buf * TILE_BYTES;
#pragma unroll
        for (int l = 0; l < AL; ++l) {
            int e = tid + l * NTHREADS;
            int row = e / ACH, ch = e - row * ACH;
            bf16x8 va = ra[SL][l];
            if (LZ && p.dz_scale && rav_a[LZ ? SL : 0][l]) va = f32_to_bf8(transform8(va, p.dz_scale, p.dz_shift, co0 + ch * 8, p.dz_act));
            *reinterpret_cast<bf16x8*>(base + row * AROW + ((ch ^ (tr_swz<BM>(row) >> 1)) << 4)) = va;
        }
#pragma unroll
        for (int l = 0; l < BL; ++l) {
            int e = tid + l * NTHREADS;
            int row = e / BCH, ch = e - row * BCH;
            bf16x8 v = rb[SL][l];
            if (p.in_scale && rbv[SL][l]) v = f32_to_bf8(transform8(v, p.in_scale, p.in_shift, b_ci[l], p.act));
            *reinterpret_cast<bf16x8*>(base + 32 * AROW + row * BROW + ((ch ^ (tr_swz<BN>(row) >> 1)) << 4)) = v;
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int jn = 0; jn < NT; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = pe > ps ? (pe - ps + 31) / 32 : 0;
    const int li = lane & 15, lg = lane >> 4;
    // transpose-read addressing: lane li of a 16-lane group supplies the 8-byte unit
    // [pixel row 8*lg + (li>>2) (+4)][channels 4*(li&3) ..+3]; it receives channel li of rows 0..3.
    const int trow = 8 * lg + (li >> 2), tq = li & 3;
    const int a_lo = trow * AROW, a_hi = (trow + 4) * AROW, b_lo = trow * BROW, b_hi = (trow + 4) * BROW;
    const int ax_lo = tr_swz<BM>(trow), ax_hi = tr_swz<BM>(trow + 4), bx_lo = tr_swz<BN>(trow), bx_hi = tr_swz<BN>(trow + 4);
    auto compute = [&](int buf) {                        // (tr_swz_frag in its own text: with the helper the <64, 64, 1, true> instance gets other instructions)
        const char* base = smem + buf * TILE_BYTES;
        bf16x8 fa[MT], fb[NT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int u = (wm * (BM / 2) + t * 16) / 4 + tq;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + a_lo + ((u ^ ax_lo) << 3)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + a_hi + ((u ^ ax_hi) << 3)));
            union { struct { s16x4 a, b; } s; bf16x8 v; } cvt;
            cvt.s.a = lo; cvt.s.b = hi;
            fa[t] = cvt.v;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int u = (wn * (BN / 2) + t * 16) / 4 + tq;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 32 * AROW + b_lo + ((u ^ bx_lo) << 3)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 32 * AROW + b_hi + ((u ^ bx_hi) << 3)));
            union { struct { s16x4 a, b; } s; bf16x8 v; } cvt;
            cvt.s.a = lo; cvt.s.b = hi;
            fb[t] = cvt.v;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
    };
    static_for<WPD>([&](auto sc) {
        if ((int)decltype(sc)::value < nk) issue_loads(sc, ps + (int)decltype(sc)::value * 32);
    });
    for (int kt0 = 0; kt0 < nk; kt0 += WPD) {
        static_for<WPD>([&](auto sc) {
            const int kt = kt0 + (int)decltype(sc)::value;
            if (kt < nk) {                               // uniform
                store_tile(sc, kt & 1);                  // waits (counted vmcnt) only for this slot's loads
                if (kt + WPD < nk) issue_loads(sc, ps + (kt + WPD) * 32);
                __syncthreads();                         // tile kt visible; everyone is past compute(kt-1)
                compute(kt & 1);
            }
        });
    }
    const int taps = p.KH * p.KW;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int nn = n0 + wn * (BN / 2) + nt * 16 + li;
            const int tap = nn >> p.cin_shift;
            const int ci = nn - (tap << p.cin_shift);
            if (nn >= p.NK || ci >= p.cin_true) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm * (BM / 2) + mt * 16 + lg * 4 + r;
                if (co >= p.Cout) continue;
                // workspace partials are tap-major [co][tap][ci] (lanes = consecutive ci -> 64 B runs instead of 4 B
                // stores 36 B apart); the split reduction permutes to OIHW
                if (p.ws) p.ws[((size_t)grp * p.nsplit + split) * p.dw_numel + ((size_t)co * taps + tap) * p.cin_true + ci] = acc[mt][nt][r];
                else atomicAdd(p.dw + ((size_t)co * p.cin_true + ci) * taps + tap, acc[mt][nt][r]);
            }
        }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient with LDS-DMA staging (global_load_lds_dwordx4) for operands that are PLAIN in memory (no lazy transform):
// the same tiles, LDS image and MFMA schedule as conv_wgrad_kernel, but the operand tiles go global -> LDS directly --
// no VGPR ring, no ds_write pass -- through a ring of ST LDS stages with counted vmcnt across raw barriers, so that ST-2
// K steps of loads stay in flight while one is being multiplied.  (Ablation of the register-staged kernel, layer-2 3x3: 418
// TFLOP/s as is, 481 without its LDS stores, 717 without its global loads, 956 without both, 447 without its MFMAs: it is
// bound by its staging, not by the matrix cores.)  The LDS destination of an LDS-DMA is wave-uniform base + lane * 16, so the
// image is lane-linear and the bank swizzle of the transposed reads is applied to the SOURCE chunk index instead (an
// involution within a pixel row: the same cache lines are fetched).  Out-of-range chunks (padding taps, tails) read a zero page.
// LZB (1x1 convs): a lazily normalised x operand is staged RAW and its BatchNorm + activation transform is applied to the B fragment
// after the transpose read.  That fragment holds 8 pixels of ONE channel per lane, so the transform needs one scale / shift pair per
// lane and fragment (registers, loaded once) and ~28 VALU instructions beside 4-8 MFMAs -- unlike the forward kernels' fragments
// (8 channels of one pixel per lane).  Rows past the pixel range hold zeros in the dz operand, so whatever act(shift) the transform
// makes of the x operand's zero rows is multiplied by 0; K x K convs keep the staging-side transform (their padding taps must BE zero).
template <int BM, int BN, int ST, bool LZB = false>
__global__ __launch_bounds__(NTHREADS) void conv_wgrad_glds_kernel(WgradP p) {
    const bf16_t* zeros = reinterpret_cast<const bf16_t*>(g_zero_page);
    constexpr int AROW = BM * 2, BROW = BN * 2;
    constexpr int TILE_BYTES = 32 * (AROW + BROW);
    constexpr int MT = BM / 32, NT = BN / 32;
    __shared__ __attribute__((aligned(1024))) char smem[ST * TILE_BYTES];
    const int lb = (int)xcd_contiguous(blockIdx.x, gridDim.x);
    const int tile = lb % p.n_tiles;
    const int unit = lb / p.n_tiles;
    const int split = unit % p.nsplit, grp = unit / p.nsplit;
    p.dz += (size_t)grp * p.gdz;
    p.x += (size_t)grp * p.gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int co0 = (tile % p.n_cotiles) * BM;
    const int n0 = (tile / p.n_cotiles) * BN;
    const int ps = split * p.pix_per_block;
    const int pe = min(p.P, ps + p.pix_per_block);
    constexpr int ACH = BM / 8, BCH = BN / 8;
    constexpr int AL = (32 * ACH) / NTHREADS, BL = (32 * BCH) / NTHREADS;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

    // staging slots of this thread: LDS chunk e = l * 256 + tid of a tile region, i.e. row e / CH at position e % CH, which holds
    // SOURCE chunk position ^ swizzle(row)
    int a_row[AL], a_co[AL];
    bool a_cok[AL];
#pragma unroll
    for (int l = 0; l < AL; ++l) {
        const int e = tid + l * NTHREADS;
        a_row[l] = e / ACH;
        const int ch = (e - a_row[l] * ACH) ^ (tr_swz<BM>(a_row[l]) >> 1);
        a_co[l] = co0 + ch * 8;
        a_cok[l] = a_co[l] < p.Cout;
    }
    int b_row[BL], b_kh[BL], b_kw[BL], b_ci[BL], b_n[BL], b_oh[BL], b_ow[BL];
    bool b_ok[BL];
#pragma unroll
    for (int l = 0; l < BL; ++l) {
        const int e = tid + l * NTHREADS;
        b_row[l] = e / BCH;
        const int ch = (e - b_row[l] * BCH) ^ (tr_swz<BN>(b_row[l]) >> 1);
        const int n = n0 + ch * 8;
        b_ok[l] = n < p.NK;
        const int tap = n >> p.cin_shift;
        b_ci[l] = n - (tap << p.cin_shift);
        b_kh[l] = tap / p.KW - p.pad;
        b_kw[l] = tap - (tap / p.KW) * p.KW - p.pad;
        const int pp = ps + b_row[l];
        b_n[l] = pp / (p.OH * p.OW);
        const int rem = pp - b_n[l] * (p.OH * p.OW);
        b_oh[l] = rem / p.OW;
        b_ow[l] = rem - b_oh[l] * p.OW;
    }
    auto stage = [&](int pbase, int st) {                       // 4 LDS-DMAs per thread (128 x 128 tile)
        const unsigned sbase = lds0 + st * TILE_BYTES + wave * 1024;
#pragma unroll
        for (int l = 0; l < AL; ++l) {
            const int pp = pbase + a_row[l];
            const bf16_t* src = (pp < pe && a_cok[l]) ? p.dz + (size_t)pp * p.Cout + a_co[l] : zeros;
            glds16(src, __builtin_amdgcn_readfirstlane(sbase + l * NTHREADS * 16));
        }
#pragma unroll
        for (int l = 0; l < BL; ++l) {
            const int ih = b_oh[l] * p.stride + b_kh[l], iw = b_ow[l] * p.stride + b_kw[l];
            const bool ok = (pbase + b_row[l] < pe) && b_ok[l] && ih >= 0 && iw >= 0 && ih < p.H && iw < p.W;
            const bf16_t* src = ok ? p.x + ((size_t)(b_n[l] * p.H + ih) * p.W + iw) * p.Cin + b_ci[l] : zeros;
            glds16(src, __builtin_amdgcn_readfirstlane(sbase + 32 * AROW + l * NTHREADS * 16));
            b_ow[l] += 32;
            while (b_ow[l] >= p.OW) { b_ow[l] -= p.OW; ++b_oh[l]; }
            while (b_oh[l] >= p.OH) { b_oh[l] -= p.OH; ++b_n[l]; }
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int jn = 0; jn < NT; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = pe > ps ? (pe - ps + 31) / 32 : 0;
    const int li = lane & 15, lg = lane >> 4;
    const int trow = 8 * lg + (li >> 2), tq = li & 3;
    const int a_lo = trow * AROW, a_hi = (trow + 4) * AROW, b_lo = trow * BROW, b_hi = (trow + 4) * BROW;
    const int ax_lo = tr_swz<BM>(trow), ax_hi = tr_swz<BM>(trow + 4), bx_lo = tr_swz<BN>(trow), bx_hi = tr_swz<BN>(trow + 4);
    float bsc[LZB ? NT : 1], bsh[LZB ? NT : 1];
    if constexpr (LZB) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nn = min(n0 + wn * (BN / 2) + t * 16 + li, p.NK - 1);        // (1x1: the flattened index IS the input channel)
            bsc[t] = p.in_scale[(size_t)grp * p.in_gstride + nn];
            bsh[t] = p.in_shift[(size_t)grp * p.in_gstride + nn];
        }
    }
    const float blo = act_lo(p.act), bhi = act_hi(p.act);
    auto compute = [&](int st) {
        const char* base = smem + st * TILE_BYTES;
        bf16x8 fa[MT], fb[NT];
#pragma unroll
        for (int t = 0; t < MT; ++t) fa[t] = tr_swz_frag(base, a_lo, ax_lo, a_hi, ax_hi, (wm * (BM / 2) + t * 16) / 4 + tq);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            fb[t] = tr_swz_frag(base + 32 * AROW, b_lo, bx_lo, b_hi, bx_hi, (wn * (BN / 2) + t * 16) / 4 + tq);
            if constexpr (LZB) {
                f32x8 f = bf8_to_f32(fb[t]);
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], bsc[t], bsh[t]), blo, bhi);
                fb[t] = f32_to_bf8(f);
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
    };
    // ring of ST stages: steps kt+1 .. kt+ST-2 stay in flight (vmcnt counts this thread's LDS-DMAs, AL + BL per step) while step kt
    // is multiplied; ONE raw barrier per step orders "step kt landed for every wave" and "everyone is done reading stage (kt-1) % ST"
    constexpr int PER = AL + BL;
#pragma unroll
    for (int s0 = 0; s0 < ST - 1; ++s0)
        if (s0 < nk) stage(ps + s0 * 32, s0);
    int st = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + ST - 2 <= nk - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((ST - 2) * PER) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + ST - 1 < nk) stage(ps + (kt + ST - 1) * 32, st == 0 ? ST - 1 : st - 1);
        compute(st);
        st = st + 1 == ST ? 0 : st + 1;
    }
    const int taps = p.KH * p.KW;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int nn = n0 + wn * (BN / 2) + nt * 16 + li;
            const int tap = nn >> p.cin_shift;
            const int ci = nn - (tap << p.cin_shift);
            if (nn >= p.NK || ci >= p.cin_true) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm * (BM / 2) + mt * 16 + lg * 4 + r;
                if (co >= p.Cout) continue;
                p.ws[((size_t)grp * p.nsplit + split) * p.dw_numel + ((size_t)co * taps + tap) * p.cin_true + ci] = acc[mt][nt][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------
// 3x3 weight gradient, all nine taps per workgroup.  One K step = up to 32 output pixels of one image (a row
// segment, or floor(32/OW) whole rows); the matching input patch (with its 1-pixel halo) is staged ONCE in LDS and
// the nine shifted B operands are fetched from it with per-lane transpose reads, so dz and the activations are
// read once per (co-tile, ci-tile) instead of once per tap.  Tile: 64 co x (9 taps x 64 ci); wave w owns the 16-ci
// slice w for all taps and all 64 co (36 accumulator tiles = 144 VGPRs).
struct W3P {
    const bf16_t* dz;
    const bf16_t* x;
    const float* in_scale;
    const float* in_shift;
    float* dw;
    float* ws;
    size_t dw_numel;
    int nsplit;
    int N, H, W, Cin, OH, OW, Cout, pad, act, cin_true;
    int cw, rows, PR, PC, units_per_img, units_per_row, total_units, units_per_block, n_cotiles, n_tiles;
    size_t gdz, gx;
    int in_gstride;
};

template <int S, int MAXSLOT>
__global__ __launch_bounds__(NTHREADS, 2) void conv3x3_wgrad_kernel(W3P p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lb = (int)xcd_contiguous(blockIdx.x, gridDim.x);   // (group, split, tile) list, tile fastest (see conv_wgrad_kernel)
    const int tile = lb % p.n_tiles;
    const int split = (lb / p.n_tiles) % p.nsplit, grp = (lb / p.n_tiles) / p.nsplit;
    p.dz += (size_t)grp * p.gdz;
    p.x += (size_t)grp * p.gx;
    if (p.in_scale) { p.in_scale += (size_t)grp * p.in_gstride; p.in_shift += (size_t)grp * p.in_gstride; }
    const int patch_bytes = p.PR * p.PC * 128;
    const int buf_bytes = 32 * 128 + patch_bytes;               // dz tile [32][64] + patch [PR*PC][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int co0 = (tile % p.n_cotiles) * 64;
    const int ci0 = (tile / p.n_cotiles) * 64;
    const int u0 = split * p.units_per_block;
    const int u1 = min(p.total_units, u0 + p.units_per_block);

    // ---- fixed per-thread staging slots ---------------------------------------------------------------------
    // dz tile: 32 rows x 8 chunks = 256 chunks -> one per thread
    const int a_j = tid >> 3, a_ch = tid & 7;
    const int a_r = a_j / p.cw, a_c = a_j - a_r * p.cw;
    // patch: PR*PC pixels x 8 chunks, up to MAXSLOT slots per thread
    const int n_chunks = p.PR * p.PC * 8;
    int s_pr[MAXSLOT], s_pc[MAXSLOT];
#pragma unroll
    for (int l = 0; l < MAXSLOT; ++l) {
        const int e = tid + l * NTHREADS;
        const int pix = e >> 3;
        s_pr[l] = pix / p.PC;
        s_pc[l] = pix - s_pr[l] * p.PC;
    }
    const int b_ch = tid & 7;                                   // chunk within the 64-ci row (same for all slots)
    bf16x8 ra, rb[MAXSLOT];
    bool rbv[MAXSLOT];

    auto decode = [&](int u, int& n, int& oh0, int& ow0) {
        n = u / p.units_per_img;
        int rem = u - n * p.units_per_img;
        int ug = rem / p.units_per_row;                         // row group
        int seg = rem - ug * p.units_per_row;
        oh0 = ug * p.rows;
        ow0 = seg * p.cw;
    };
    auto issue_loads = [&](int u) {
        int n, oh0, ow0;
        decode(u, n, oh0, ow0);
        {
            const int oh = oh0 + a_r, ow = ow0 + a_c;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (a_r < p.rows && oh < p.OH && ow < p.OW)
                v = *reinterpret_cast<const bf16x8*>(p.dz + ((size_t)(n * p.OH + oh) * p.OW + ow) * p.Cout + co0 + a_ch * 8);
            ra = v;
        }
        const int ih0 = oh0 * S - p.pad, iw0 = ow0 * S - p.pad;
#pragma unroll
        for (int l = 0; l < MAXSLOT; ++l) {
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            const int ih = ih0 + s_pr[l], iw = iw0 + s_pc[l];
            const bool ok = (tid + l * NTHREADS) < n_chunks && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            if (ok) v = *reinterpret_cast<const bf16x8*>(p.x + ((size_t)(n * p.H + ih) * p.W + iw) * p.Cin + ci0 + b_ch * 8);
            rbv[l] = ok;
            rb[l] = v;
        }
    };
    auto store_tile = [&](int buf) {
        char* base = smem + buf * buf_bytes;
        *reinterpret_cast<bf16x8*>(base + a_j * 128 + ((a_ch ^ (tr_swz<64>(a_j) >> 1)) << 4)) = ra;
        char* pb = base + 32 * 128;
#pragma unroll
        for (int l = 0; l < MAXSLOT; ++l) {
            if (tid + l * NTHREADS < n_chunks) {
                bf16x8 v = rb[l];
                if (p.in_scale && rbv[l]) v = f32_to_bf8(transform8(v, p.in_scale, p.in_shift, ci0 + b_ch * 8, p.act));
                const int pix = s_pr[l] * p.PC + s_pc[l];
                // 16-byte chunk swizzle by patch column: neighbouring columns that share a bank half get distinct slots
                *reinterpret_cast<bf16x8*>(pb + pix * 128 + ((b_ch ^ (((s_pc[l] >> 1) & 3) << 1)) << 4)) = v;
            }
        }
    };

    f32x4 acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- fixed per-lane fragment addressing -----------------------------------------------------------------
    const int trow = 8 * lg + (li >> 2), tq = li & 3;
    const int a_lo = trow * 128, a_hi = (trow + 4) * 128;
    const int ax_lo = tr_swz<64>(trow), ax_hi = tr_swz<64>(trow + 4);
    int b_base[2], b_col[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = trow + 4 * h;
        int r = j / p.cw, c = j - r * p.cw;
        if (r >= p.rows) { r = 0; c = 0; }                       // padding k-rows (dz row is zero): read any FINITE patch pixel
        b_col[h] = c * S;                                        // patch column of tap (.,0) for k-row j
        b_base[h] = r * S * p.PC + c * S;                        // patch pixel index of tap (0,0)
    }
    const int b_unit = wave * 4 + tq;                            // 8-byte unit of this lane's 4 ci inside the 64-ci row

    if (u0 < u1) {
        issue_loads(u0);
        store_tile(0);
    }
    __syncthreads();
    for (int u = u0; u < u1; ++u) {
        const int buf = (u - u0) & 1;
        if (u + 1 < u1) issue_loads(u + 1);
        const char* base = smem + buf * buf_bytes;
        const char* pb = base + 32 * 128;
        bf16x8 fa[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) fa[t] = tr_swz_frag(base, a_lo, ax_lo, a_hi, ax_hi, t * 4 + tq);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                s16x4 half[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int pix = b_base[h] + kh * p.PC + kw;
                    const int un = b_unit ^ ((((b_col[h] + kw) >> 1) & 3) << 2);
                    half[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(pb + pix * 128 + (un << 3)));
                }
                union { struct { s16x4 a, b; } s; bf16x8 v; } cvt;
                cvt.s.a = half[0]; cvt.s.b = half[1];
                const bf16x8 fb = cvt.v;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[mt][kh * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb, acc[mt][kh * 3 + kw], 0, 0, 0);
            }
        if (u + 1 < u1) store_tile(buf ^ 1);
        __syncthreads();
    }
    const int ci = ci0 + wave * 16 + li;
    if (ci < p.cin_true) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + mt * 16 + lg * 4 + r;
                    if (p.ws) p.ws[((size_t)grp * p.nsplit + split) * p.dw_numel + ((size_t)co * 9 + t) * p.cin_true + ci] = acc[mt][t][r];
                    else atomicAdd(p.dw + ((size_t)co * p.cin_true + ci) * 9 + t, acc[mt][t][r]);
                }
    }
}

// dw[perm(i)] += sum_s ws[s][i]: 16 indices x 16 split lanes per workgroup (the split loop is the long axis).
// taps > 1: ws is tap-major [co][tap][cin], dw is OIHW [co][cin][tap].
// blockIdx.y = output group (per-group products of the algebraic BatchNorm backward: ws [group][split][n] -> dw [group][n], stored)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, float* dw, size_t n, int nsplit, int taps, int cin, int store) {
    ws += (size_t)blockIdx.y * nsplit * n;
    dw += (size_t)blockIdx.y * n;
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const size_t i = (size_t)blockIdx.x * 16 + tx;
    float a = 0.f;
    if (i < n) {
        // four independent partial sums (fixed order): with one accumulator every load waits for the previous add -- hundreds of
        // dependent round trips when a small problem was split over ~2000 workgroups
        float a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int s = ty;
        for (; s + 48 < nsplit; s += 64) {
            a += ws[(size_t)s * n + i];
            a1 += ws[(size_t)(s + 16) * n + i];
            a2 += ws[(size_t)(s + 32) * n + i];
            a3 += ws[(size_t)(s + 48) * n + i];
        }
        for (; s < nsplit; s += 16) a += ws[(size_t)s * n + i];
        a = (a + a1) + (a2 + a3);
    }
    red[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][tx];
        size_t o = i;
        if (taps > 1) {
            const size_t per_co = (size_t)taps * cin;
            const size_t co = i / per_co;
            const int rem = (int)(i - co * per_co), tap = rem / cin, ci = rem - tap * cin;
            o = (co * cin + ci) * taps + tap;
        }
        if (store) dw[o] = t; else dw[o] += t;
    }
}

// The same reduction, four consecutive indices per thread (n % 4 == 0): 16-byte loads, 256 contiguous bytes per split row of a workgroup
// instead of 64 -- the one-index form moved 1 TB/s and was, at 104 launches x 17 us, the largest of the step's small kernels
// (1.8 ms per step; 2.2 of 34 ms of kernel time at the per-GPU share of the reference recipe).  Same fixed summation order per index.
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float* ws, float* dw, size_t n, int nsplit, int taps, int cin, int store) {
    ws += (size_t)blockIdx.y * nsplit * n;
    dw += (size_t)blockIdx.y * n;
    __shared__ f32x4 red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const size_t i = ((size_t)blockIdx.x * 16 + tx) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
        f32x4 a1 = a, a2 = a, a3 = a;
        int s = ty;
        for (; s + 48 < nsplit; s += 64) {
            a += *reinterpret_cast<const f32x4*>(ws + (size_t)s * n + i);
            a1 += *reinterpret_cast<const f32x4*>(ws + (size_t)(s + 16) * n + i);
            a2 += *reinterpret_cast<const f32x4*>(ws + (size_t)(s + 32) * n + i);
            a3 += *reinterpret_cast<const f32x4*>(ws + (size_t)(s + 48) * n + i);
        }
        for (; s < nsplit; s += 16) a += *reinterpret_cast<const f32x4*>(ws + (size_t)s * n + i);
        a = (a + a1) + (a2 + a3);
    }
    red[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && i < n) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][tx];
        if (taps > 1) {
            const size_t per_co = (size_t)taps * cin;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t ii = i + q;
                const size_t co = ii / per_co;
                const int rem = (int)(ii - co * per_co), tap = rem / cin, ci = rem - tap * cin;
                const size_t o = (co * cin + ci) * taps + tap;
                if (store) dw[o] = t[q]; else dw[o] += t[q];
            }
        } else if ((reinterpret_cast<uintptr_t>(dw + i) & 15) == 0) {
            f32x4* o = reinterpret_cast<f32x4*>(dw + i);
            if (store) *o = t; else *o += t;
        } else {                                  // (gradient views of the flat buffer are only 4-byte aligned behind an odd-sized parameter)
#pragma unroll
            for (int q = 0; q < 4; ++q) { if (store) dw[i + q] = t[q]; else dw[i + q] += t[q]; }
        }
    }
}

}  // namespace

// picks the 16-byte form whenever the index count allows it
void launch_wgrad_reduce(const float* ws, float* dw, size_t n, int nsplit, int taps, int cin, int store, int groups, hipStream_t stream) {
    if (n % 4 == 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0)
        hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((unsigned)((n / 4 + 15) / 16), groups), dim3(256), 0, stream, ws, dw, n, nsplit, taps, cin, store);
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 15) / 16), groups), dim3(256), 0, stream, ws, dw, n, nsplit, taps, cin, store);
}

constexpr int W3_SLOTS = 4;      // 16-byte patch chunks a thread of conv3x3_wgrad_kernel stages per unit (3 x 34 pixels x 8 chunks = 816 <= 4 x 256)

// split plan shared by the workspace query and the launcher
struct WgradPlan { bool use3x3; int nsplit, per_block, n_cotiles, n_tiles, BM, BN, NK, cin_shift; int cw, rows, PR, PC, upi, upr, total_units, buf_bytes; };

static int wgrad_plan(const adamml_conv_desc_t* d, int cin_true, WgradPlan* pl) {
    const int taps = d->KH * d->KW;
    pl->use3x3 = false;
    // the LDS-patch kernel only pays on wide feature maps (measured on MI355X: 56x56 1.87 ms vs 1.97 ms generic; at
    // 28x28 and below the generic implicit-GEMM gather is 5-40 % faster)
    // (stride 1 only: a 32-column strip of a stride-2 conv needs a 3 x 65 patch, more than the staging slots of a workgroup hold)
    if (d->OW > 32 && d->KH == 3 && d->KW == 3 && d->pad == 1 && d->stride == 1 && d->Cin % 64 == 0 && d->Cout % 64 == 0 &&
        cin_true == d->Cin) {
        if (d->OW > 32) { pl->cw = 32; pl->rows = 1; pl->upr = ceil_div(d->OW, 32); }
        else { pl->cw = d->OW; pl->rows = 32 / d->OW; pl->upr = 1; }
        pl->PR = (pl->rows - 1) * d->stride + 3;
        pl->PC = (pl->cw - 1) * d->stride + 3;
        pl->upi = ceil_div(d->OH, pl->rows) * pl->upr;
        pl->total_units = d->N * pl->upi;
        pl->buf_bytes = 32 * 128 + pl->PR * pl->PC * 128;
        if (pl->PR * pl->PC * 8 <= W3_SLOTS * NTHREADS && 2 * pl->buf_bytes <= 64 * 1024 && pl->total_units > 0) {
            pl->use3x3 = true;
            pl->n_cotiles = d->Cout / 64;
            pl->n_tiles = pl->n_cotiles * (d->Cin / 64);
            int nsplit = ceil_div(512, pl->n_tiles * (d->groups < 1 ? 1 : d->groups));
            int upb = ceil_div(pl->total_units, nsplit);
            if (upb < 4) upb = 4;
            pl->nsplit = ceil_div(pl->total_units, upb);
            pl->per_block = upb;
            return 0;
        }
    }
    pl->NK = taps * d->Cin;
    pl->cin_shift = 30;                     // 1x1: tap = n >> 30 = 0
    if (taps > 1) {
        pl->cin_shift = ilog2_exact(d->Cin);
        if (pl->cin_shift < 0) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_weight: KxK conv needs power-of-two Cin (got %d)", d->Cin);
    }
    pl->BM = d->Cout <= 64 ? 64 : 128;
    pl->BN = pl->NK <= 64 ? 64 : 128;
    pl->n_cotiles = ceil_div(d->Cout, pl->BM);
    pl->n_tiles = pl->n_cotiles * ceil_div(pl->NK, pl->BN);
    const int P = d->N * d->OH * d->OW;
    int nsplit = ceil_div(768, pl->n_tiles * (d->groups < 1 ? 1 : d->groups));
    int ppb = ceil_div(ceil_div(P, nsplit), 32) * 32;
    if (ppb < 256) ppb = 256;
    pl->nsplit = ceil_div(P, ppb);
    pl->per_block = ppb;
    return 0;
}

int adamml_launch_split_reduce(const float* ws, float* dw, size_t n, int nsplit, hipStream_t stream, int taps, int cin) {
    launch_wgrad_reduce(ws, dw, n, nsplit, taps, cin, 0, 1, stream);
    return adamml_check_launch("split_reduce");
}

// per-group form: ws [groups][nsplit][n] -> out [groups][n], OVERWRITTEN (the products of the algebraic BatchNorm backward)
int adamml_launch_split_reduce_grouped(const float* ws, float* out, size_t n, int nsplit, int groups, int cin, hipStream_t stream) {
    launch_wgrad_reduce(ws, out, n, nsplit, 1, cin, 1, groups, stream);
    return adamml_check_launch("split_reduce");
}

extern "C" size_t adamml_conv_bwd_weight_workspace(const adamml_conv_desc_t* d, int cin_true) {
    WgradPlan pl;
    if (!d || wgrad_plan(d, cin_true, &pl)) return 0;
    const int groups = d->groups < 1 ? 1 : d->groups;
    size_t need = (size_t)groups * pl.nsplit * d->Cout * cin_true * d->KH * d->KW * sizeof(float);
    if (adamml_conv3x3_c64_wgrad_supported(d, cin_true)) {
        const size_t n3 = (size_t)adamml_conv3x3_c64_wgrad_blocks(d, nullptr) * d->Cout * cin_true * 9 * sizeof(float);
        if (n3 > need) need = n3;
    }
    return need;
}

// register-staged kernel: the positional template list is written here once
template <int BM, int BN, int WPD = 1, bool LZ = false>
static void launch_wgrad(dim3 grid, hipStream_t stream, const WgradP& p) {
    hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, WPD, LZ>), grid, dim3(NTHREADS), 0, stream, p);
}

// LDS-DMA staged kernel (both operands plain in memory, or LZB: a lazily normalised x of a 1x1 conv transformed at the B fragment), 128-wide
// tile plan pl: the tile choice is the same for both.
// 256-wide tiles halve the operand bytes fetched per MAC (this kernel is bound by the L1 load path: 16 KB per 128 x 128 x 32
// step = 256 cycles of 64 B/clk against 256 cycles of MFMA).  Measured (tools/bench_conv.py, B = 72, TFLOP/s 128^2 -> wide):
// 256 x 128 for Cout % 256 == 0: layer 3 conv1 366 -> 476, conv2 458 -> 616, downsample 329 -> 451, layer-2 downsample
// 407 -> 512; it loses where the pixel axis is short and the tile list long (layer 4 conv2 / downsample: 376 -> 367, 366 -> 339);
// 128 x 256 for a single cout tile: layer-2 conv1 374 -> 453.
template <bool LZB>
static void launch_wgrad_glds(const adamml_conv_desc_t* d, const WgradPlan& pl, int groups, hipStream_t stream, WgradP& p) {
    const dim3 block(NTHREADS);
    if (d->Cout % 256 == 0 && pl.n_tiles <= 64) {
        p.n_cotiles = d->Cout / 256; p.n_tiles = p.n_cotiles * ceil_div(pl.NK, 128);
        hipLaunchKernelGGL((conv_wgrad_glds_kernel<256, 128, 2, LZB>), dim3(pl.nsplit * p.n_tiles * groups), block, 0, stream, p);
    } else if (d->Cout == 128 && (pl.NK % 256 == 0 || (!LZB && pl.NK > 512))) {
        // (NK % 256 != 0: the last tile is half empty -- 3x3 / 128 -> 128: 5 tiles of 256 instead of 9 of 128; measured +4 %;
        // the LZB form only ever took this tile with whole tiles)
        p.n_tiles = p.n_cotiles * ceil_div(pl.NK, 256);
        hipLaunchKernelGGL((conv_wgrad_glds_kernel<128, 256, 2, LZB>), dim3(pl.nsplit * p.n_tiles * groups), block, 0, stream, p);
    } else
        hipLaunchKernelGGL((conv_wgrad_glds_kernel<128, 128, 3, LZB>), dim3(pl.nsplit * pl.n_tiles * groups), block, 0, stream, p);
}

struct WgradExtra { const float* dz_scale; const float* dz_shift; int dz_act, dz_gstride; bool per_group; };

static int wgrad_launch(const adamml_conv_desc_t* d, const void* dz, const void* x, const float* in_scale, const float* in_shift, float* dw,
                        int cin_true, void* workspace, size_t workspace_bytes, hipStream_t stream, const WgradExtra* ex) {
    if (!d || !dz || !x || !dw) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_weight: null argument");
    if (d->Cin % 8 || d->Cout % 8) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_weight: channels must be multiples of 8");
    if ((long)d->N * d->OH * d->OW <= 0) return ADAMML_OK;
    WgradPlan pl;
    int rc = wgrad_plan(d, cin_true, &pl);
    if (rc) return rc;
    const size_t dw_numel = (size_t)d->Cout * cin_true * d->KH * d->KW;
    const int groups = d->groups < 1 ? 1 : d->groups;
    if (ex && ex->per_group && !(workspace && workspace_bytes >= (size_t)groups * pl.nsplit * dw_numel * sizeof(float)))
        return adamml_set_error(ADAMML_EINVAL, "conv_bwd_weight_grouped: workspace too small");
    // a workspace below the query's answer is ignored as a whole (atomic accumulation).  The query answers the largest of the plans'
    // sizes; each plan below compares with its own, so a buffer between two of them used to be taken by one plan and not by another
    if (!ex && workspace && workspace_bytes < adamml_conv_bwd_weight_workspace(d, cin_true)) workspace = nullptr;
    if (!ex && workspace && adamml_conv3x3_c64_wgrad_supported(d, cin_true)) {
        // 3x3 / 64 -> 64: LDS-patch kernel with one partial per workgroup (conv3x3_c64.hip)
        const int nblk = adamml_conv3x3_c64_wgrad_blocks(d, nullptr);
        if (workspace_bytes >= (size_t)nblk * dw_numel * sizeof(float)) {
            rc = adamml_conv3x3_c64_wgrad_launch(d, dz, x, in_scale, in_shift, (float*)workspace, stream);
            if (rc) return rc;
            return adamml_launch_split_reduce((const float*)workspace, dw, dw_numel, nblk, stream, 9, cin_true);
        }
    }
    if (!ex && workspace && adamml_conv1x1_narrow_wgrad_supported(d, cin_true) && workspace_bytes >= (size_t)groups * pl.nsplit * dw_numel * sizeof(float)) {
        // narrow 1x1 convs of the MobileNetV2s: barrier-free streaming kernel, one partial per workgroup (conv1x1_narrow.hip)
        int nblk = 0;
        rc = adamml_conv1x1_narrow_wgrad_launch(d, dz, x, in_scale, in_shift, (float*)workspace, pl.nsplit, &nblk, stream);
        if (rc) return rc;
        return adamml_launch_split_reduce((const float*)workspace, dw, dw_numel, groups * nblk, stream, 1, cin_true);
    }
    float* ws = nullptr;
    if (workspace && workspace_bytes >= (size_t)groups * pl.nsplit * dw_numel * sizeof(float)) ws = (float*)workspace;
    dim3 grid(pl.nsplit * pl.n_tiles * groups), block(NTHREADS);
    const size_t gdz = (size_t)d->N * d->OH * d->OW * d->Cout, gx = (size_t)d->N * d->H * d->W * d->Cin;
    if (pl.use3x3) {
        W3P q;
        q.dz = (const bf16_t*)dz; q.x = (const bf16_t*)x; q.in_scale = in_scale; q.in_shift = in_shift; q.dw = dw;
        q.ws = ws; q.dw_numel = dw_numel; q.nsplit = pl.nsplit;
        q.gdz = gdz; q.gx = gx; q.in_gstride = d->in_gstride;
        q.N = d->N; q.H = d->H; q.W = d->W; q.Cin = d->Cin; q.OH = d->OH; q.OW = d->OW; q.Cout = d->Cout; q.pad = d->pad;
        q.act = d->act; q.cin_true = cin_true;
        q.cw = pl.cw; q.rows = pl.rows; q.PR = pl.PR; q.PC = pl.PC; q.units_per_img = pl.upi; q.units_per_row = pl.upr;
        q.total_units = pl.total_units; q.units_per_block = pl.per_block; q.n_cotiles = pl.n_cotiles; q.n_tiles = pl.n_tiles;
        hipLaunchKernelGGL((conv3x3_wgrad_kernel<1, W3_SLOTS>), grid, block, 2 * pl.buf_bytes, stream, q);
    } else {
        WgradP p;
        p.dz = (const bf16_t*)dz; p.x = (const bf16_t*)x; p.in_scale = in_scale; p.in_shift = in_shift; p.dw = dw;
        p.ws = ws; p.dw_numel = dw_numel; p.nsplit = pl.nsplit;
        p.gdz = gdz; p.gx = gx; p.in_gstride = d->in_gstride;
        p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
        p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad; p.act = d->act; p.cin_true = cin_true;
        p.P = d->N * d->OH * d->OW; p.NK = pl.NK; p.cin_shift = pl.cin_shift; p.n_cotiles = pl.n_cotiles; p.n_tiles = pl.n_tiles;
        p.pix_per_block = pl.per_block;
        p.dz_scale = ex ? ex->dz_scale : nullptr; p.dz_shift = ex ? ex->dz_shift : nullptr;
        p.dz_act = ex ? ex->dz_act : 0; p.dz_gstride = ex ? ex->dz_gstride : 0;
        const bool lazy_dz = ex && ex->dz_scale;
        const bool glds = ws && !lazy_dz && pl.BM == 128 && pl.BN == 128;       // LDS-DMA staging of the operands as they are in memory
        if (glds && in_scale && d->KH * d->KW == 1 && d->pad == 0)
            launch_wgrad_glds<true>(d, pl, groups, stream, p);   // 1x1 conv with a lazily normalised input: raw tensor staged, transform at the B fragment
        else if (glds && !in_scale)
            launch_wgrad_glds<false>(d, pl, groups, stream, p);  // both operands plain in memory
        else if (lazy_dz) {
            if (pl.BM == 64 && pl.BN == 64) launch_wgrad<64, 64, 1, true>(grid, stream, p);
            else if (pl.BM == 128 && pl.BN == 128) launch_wgrad<128, 128, 1, true>(grid, stream, p);
            else return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_weight_grouped: lazy dz needs Cout == Cin in {64, >= 128}");
        }
        else if (pl.BM == 64 && pl.BN == 64) launch_wgrad<64, 64>(grid, stream, p);
        else if (pl.BM == 64) launch_wgrad<64, 128>(grid, stream, p);
        else if (pl.BN == 64) launch_wgrad<128, 64>(grid, stream, p);
        else if ((long)grid.x * grid.y <= 1100) launch_wgrad<128, 128, 6>(grid, stream, p);
        else launch_wgrad<128, 128>(grid, stream, p);
    }
    rc = adamml_check_launch("conv_bwd_weight");
    if (rc || !ws) return rc;
    if (ex && ex->per_group) {
        launch_wgrad_reduce(ws, dw, dw_numel, pl.nsplit, 1, cin_true, 1, groups, stream);
        return adamml_check_launch("split_reduce");
    }
    return adamml_launch_split_reduce(ws, dw, dw_numel, groups * pl.nsplit, stream, d->KH * d->KW, cin_true);
}

extern "C" int adamml_conv_bwd_weight(const adamml_conv_desc_t* d, const void* dz, const void* x, const float* in_scale,
                                      const float* in_shift, float* dw, int cin_true, void* workspace, size_t workspace_bytes,
                                      hipStream_t stream) {
    return wgrad_launch(d, dz, x, in_scale, in_shift, dw, cin_true, workspace, workspace_bytes, stream, nullptr);
}

// Per-group products for the algebraic BatchNorm backward: out[g] = dz_g^T x_g ([groups][Cout][cin_true], OVERWRITTEN), with an
// optional lazy transform of the dz operand too (Gram matrix a^T a: dz = x = the raw tensor, both transformed).  1x1 convs.
extern "C" int adamml_conv_bwd_weight_grouped(const adamml_conv_desc_t* d, const void* dz, const float* dz_scale, const float* dz_shift,
                                              int dz_act, int dz_gstride, const void* x, const float* in_scale, const float* in_shift,
                                              float* out, int cin_true, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!d || d->KH * d->KW != 1) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_weight_grouped: 1x1 convs only");
    if (!workspace) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_weight_grouped: needs the split workspace");
    WgradExtra ex{dz_scale, dz_shift, dz_act, dz_gstride, true};
    return wgrad_launch(d, dz, x, in_scale, in_shift, out, cin_true, workspace, workspace_bytes, stream, &ex);
}
