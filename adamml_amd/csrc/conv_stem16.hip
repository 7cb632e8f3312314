// 7x7 stride-2 pad-3 stem of a 16-channel image to 64 channels: the first conv of the flow (10 channels) and RGB-diff (15 channels) ResNets
// (models/resnet.py:138), stored as 16 bf16 channels per pixel (NHWC, 32 B per pixel), gfx950.
//
// The generic implicit-GEMM kernel gathers every (tap, 16-channel) fragment of the 49 taps through L1/L2 (see conv_stem.hip).  Here, as in
// conv_stem_kernel, a workgroup stages the INPUT PATCH of a strip of output rows in LDS once and builds the MFMA operands from it:
//   one patch pixel = 32 contiguous bytes = one tap x 16 channels, so a 32-deep MFMA step is two taps: lane group lg reads the 16 bytes of
//   tap 2j + (lg >> 1), channel half lg & 1.  Taps are paired in flat order (kh, kw) -> 7 kh + kw: 25 steps, K = 800 with the last
//   half step zero in the weights (its patch address is tap 48's) -- the K grouping of the generic kernel's [co][tap][ci] pack, which IS the
//   weight operand here (adamml_pack_conv_weight mode 0 with cin_pad = 16: no pack of its own);
//   the 16 pixels of an MFMA tile are 64 B apart, so the 16-byte slots of the patch are XOR-swizzled (pslot) to spread them over the banks;
//   the weights [64][800] bf16 (101 KB) stay resident in LDS for all strips of the workgroup: at W = 224 that leaves room for a one-row
//   strip only (7 x 230 x 32 B = 51.5 KB patch; 103 424 + 512 + 51 520 = 155 456 B of the 160 KB), one workgroup of 4 waves per CU; each
//   wave owns two pixel tiles x all four cout tiles (6 ds_read_b128 per 8 MFMA).  The next strip's patch is prefetched into registers
//   while the current one is in the matrix cores.
// Not built: the rolling patch (consecutive strips of an image share 5 of their 7 input rows; they are re-read from L2 here) and the
// register-resident weight slices (98 VGPRs per 16-cout slice and lane; it would free the 101 KB for taller strips at the price of every
// wave reading every patch fragment): the LDS-resident form was built first because it is conv_stem_kernel's proven scheme, and the
// register-resident one was not built or timed, so there are no numbers of a loser to give.
// Compiler's resource report (tools/kernel_resources.py), gfx950:
//   conv_stem16_kernel        vgpr 221 agpr 32 sgpr 106 occ 2 scratch 0 vspill 0, dynamic LDS <= 160 KB (155 456 B at W = 224)
//   conv_stem16_wgrad_kernel  vgpr 227 agpr  0 sgpr 106 occ 2 scratch 0 vspill 0, dynamic LDS = patch + 17 408 B (68 928 B at W = 224)
// Measured (tools/bench_stem16.py, profiles/stem16.json; 224 x 224, against the tile kernels on the same tensors): forward 757 vs 862 us at
// N = 360 and 108 vs 110 us at N = 45 (a tie within the spread; 512 workgroups instead of 256 lost there: 116 us); weight gradient 643 vs
// 1275 us and 102 vs 167 us.
//
// Both kernels are reached through adamml_conv_fwd / adamml_conv_bwd_weight (conv_plain / wgrad_launch dispatch on
// adamml_conv_stem16_supported, as they do for the 3x3 / 64 -> 64 kernels): plain input only, no data gradient (network input).
#include "common.h"
#include "conv_internal.h"

namespace {

constexpr int NT = 256;
constexpr int TAPS = 49;
constexpr int KSTEPS = 25;             // two taps each, flat tap order
constexpr int KTOT = KSTEPS * 32;      // 800: the reduction length the kernel sums (784 real)
constexpr int KREAL = TAPS * 16;       // 784: row length of the [co][tap][ci] pack
constexpr int WROW = KTOT * 2 + 16;    // LDS bytes per weight row (+16 B skew: 101 sixteen-byte slots, odd)
constexpr int MAXPX = 128;             // output pixels per strip (8 MFMA pixel tiles, 2 per wave)
constexpr int SROW = 128 + 8;          // staging row: 64 bf16 + 8 B skew
constexpr int MAXSLOT = 15;            // 16-byte patch slots per thread (W = 256: 7 x 262 x 2 = 3668 <= 3840)
constexpr int LDS_BUDGET = 160 * 1024;
constexpr int FWD_BLOCKS = 256;        // workgroup cap of the forward

// byte offset of half h (8 channels) of patch pixel q: the two low bits of the 16-byte slot index are XORed with pixel bits 3-4, so that the
// 16 pixels of an MFMA tile (2 apart, every fourth one 256 B = all 64 banks further) land in 16 distinct slots of a 256-byte bank row
__device__ __forceinline__ int pslot(int q, int h) { return ((2 * q + h) ^ ((q >> 3) & 3)) << 4; }

struct Stem16P {
    const bf16_t* x;     // [G*N, H, W, 16] bf16
    const bf16_t* w;     // [64][49][16] bf16 (adamml_pack_conv_weight mode 0)
    bf16_t* y;           // [G*N, OH, OW, 64]
    double* stats;       // [G][SLOTS][128] or null
    int N, H, W, OH, OW;
    int R;               // output rows per strip
    int tiles_per_img, total_tiles, tpb;
    int PW, PR;          // patch width (pixels, even) / rows
    size_t gx, gy;
};

__global__ __launch_bounds__(NT, 1) void conv_stem16_kernel(Stem16P p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* s_w = smem;                                                // [64][WROW]
    float* cs = reinterpret_cast<float*>(smem + 64 * WROW);          // [128] channel sums / second moments
    char* s_patch = smem + 64 * WROW + 512;                          // patch [PR][PW] x 32 B (swizzled), later the staging tile [MAXPX][SROW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int half = lg & 1, hi = lg >> 1;
    const int g = blockIdx.y;
    p.x += (size_t)g * p.gx;
    p.y += (size_t)g * p.gy;

    if (tid < 128) cs[tid] = 0.f;

    // ---- input patch of a strip: rows 2*oh0-3 .. +PR-1, columns -3 .. PW-4; out-of-image = 0; one half pixel (16 B) per slot.
    // The slot -> (row, column) map is strip-invariant.  All loads of a patch are issued back to back into registers and the NEXT strip's
    // loads are in flight while the current strip is computed (conv_stem_kernel's scheme).
    const int nslots = p.PR * p.PW * 2;
    int s_dst[MAXSLOT], s_ih[MAXSLOT], s_iw[MAXSLOT];
#pragma unroll
    for (int l = 0; l < MAXSLOT; ++l) {
        const int e = tid + l * NT, q = e >> 1;
        const int pr = q / p.PW, pc = q - pr * p.PW;
        s_ih[l] = e < nslots ? pr : -(1 << 20);                // dead slots fail the row test
        s_iw[l] = pc - 3;
        s_dst[l] = pslot(q, e & 1);
    }
    bf16x8 rp[MAXSLOT];
    unsigned vmask = 0;                  // 1 validity bit per slot of the prefetched patch
    auto load_patch = [&](int tile) {
        const int n = tile / p.tiles_per_img, tr = tile - n * p.tiles_per_img;
        const int ih0 = 2 * tr * p.R - 3;
        vmask = 0;
        const bf16_t* img = p.x + (size_t)n * p.H * p.W * 16 + (tid & 1) * 8;
#pragma unroll
        for (int l = 0; l < MAXSLOT; ++l) {
            // unconditional loads from clamped addresses; validity is applied where the registers are consumed
            const int ih = ih0 + s_ih[l], iw = s_iw[l];
            rp[l] = *reinterpret_cast<const bf16x8*>(img + ((size_t)min(max(ih, 0), p.H - 1) * p.W + min(max(iw, 0), p.W - 1)) * 16);
            vmask |= (((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) ? 1u : 0u) << l;
        }
    };
    const int tile0 = blockIdx.x * p.tpb;
    if (tile0 < p.total_tiles) load_patch(tile0);           // (in flight while the weights are staged)
    // weights -> LDS (once per workgroup): 64 rows x 100 sixteen-byte slots, the last two of a row (K = 784..799) zero
    {
        constexpr int RS = KTOT / 8, CH = 5;                         // 25 slots per thread, 5 loads in flight at a time
        static_assert(64 * RS == 5 * CH * NT, "weight slots must divide evenly");
        for (int c = 0; c < 5; ++c) {
            bf16x8 wv[CH];
#pragma unroll
            for (int l = 0; l < CH; ++l) {
                const int e = tid + (c * CH + l) * NT;
                const int co = e / RS, ch = e - co * RS;
                wv[l] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if (ch < KREAL / 8) wv[l] = *reinterpret_cast<const bf16x8*>(p.w + (size_t)co * KREAL + ch * 8);
            }
#pragma unroll
            for (int l = 0; l < CH; ++l) {
                const int e = tid + (c * CH + l) * NT;
                const int co = e / RS, ch = e - co * RS;
                *reinterpret_cast<bf16x8*>(s_w + co * WROW + ch * 16) = wv[l];
            }
        }
    }
    // patch pixel of the window origin of each of this lane's output pixels: strip-invariant; pixels past a short last strip still
    // address valid patch rows and are zeroed at staging
    int pixq[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        int q = (wave * 2 + pt) * 16 + li;
        if (q >= p.R * p.OW) q = 0;
        const int r = q / p.OW, c = q - r * p.OW;
        pixq[pt] = 2 * r * p.PW + 2 * c;
    }

    for (int it = 0; it < p.tpb; ++it) {
        const int tile = tile0 + it;
        if (tile >= p.total_tiles) break;
        const int n = tile / p.tiles_per_img, tr = tile - n * p.tiles_per_img;
        const int oh0 = tr * p.R;
        const int rows = min(p.R, p.OH - oh0);
        const int npx = rows * p.OW;
#pragma unroll
        for (int l = 0; l < MAXSLOT; ++l) {
            if (tid + l * NT < nslots)
                *reinterpret_cast<bf16x8*>(s_patch + s_dst[l]) = (vmask >> l) & 1u ? rp[l] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        __syncthreads();
        if (it + 1 < p.tpb && tile + 1 < p.total_tiles) load_patch(tile + 1);

        // ---- MFMA: wave w owns pixel tiles 2w, 2w+1 (16 consecutive output pixels each, row-major over the strip) x all 64 couts ----
        f32x4 acc[4][2];                                     // [cout tile][pixel tile]
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KSTEPS; ++j) {
            // taps 2j (lane groups 0-1) and 2j+1 (lane groups 2-3); the 50th tap has zero weights and reads tap 48's pixel
            const int tA = 2 * j, tB = 2 * j + 1 < TAPS ? 2 * j + 1 : TAPS - 1;
            const int tq = hi ? (tB / 7) * p.PW + tB % 7 : (tA / 7) * p.PW + tA % 7;
            bf16x8 fw[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) fw[ct] = *reinterpret_cast<const bf16x8*>(s_w + (ct * 16 + li) * WROW + j * 64 + lg * 16);
            bf16x8 fa[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) fa[pt] = *reinterpret_cast<const bf16x8*>(s_patch + pslot(pixq[pt] + tq, half));
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ct], fa[pt], acc[ct][pt], 0, 0, 0);
        }
        __syncthreads();                                     // patch consumed: its LDS becomes the staging tile

        // ---- stage [MAXPX][64] bf16 (rows >= npx zero), store the strip (contiguous in HBM) 16 B per lane ---------------
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int q = (wave * 2 + pt) * 16 + li;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                bf16x4 v = f32_to_bf4(acc[ct][pt]);
                if (q >= npx) v = bf16x4{0, 0, 0, 0};
                *reinterpret_cast<bf16x4*>(s_patch + q * SROW + (ct * 16 + lg * 4) * 2) = v;
            }
        }
        __syncthreads();
        bf16_t* ybase = p.y + ((size_t)n * p.OH + oh0) * p.OW * 64;
        for (int e = tid; e < npx * 8; e += NT) {
            const int q = e >> 3, ch = e & 7;
            const s16x4 lo = *reinterpret_cast<const s16x4*>(s_patch + q * SROW + ch * 16);
            const s16x4 hi4 = *reinterpret_cast<const s16x4*>(s_patch + q * SROW + ch * 16 + 8);
            union { struct { s16x4 a, b; } s; bf16x8 v; } u;
            u.s.a = lo; u.s.b = hi4;
            *reinterpret_cast<bf16x8*>(ybase + (size_t)q * 64 + ch * 8) = u.v;
        }
        if (p.stats) {
            // wave w: channels 16w..16w+15; F = [32 pixels][16 channels] by transpose reads; ones*F and diag(F^T F)
            const bf16x8 ones = bf16x8_ones();
            const int trow = 8 * lg + (li >> 2);
            f32x4 dsum = {0.f, 0.f, 0.f, 0.f}, dsq = {0.f, 0.f, 0.f, 0.f};
            const int nps = (npx + 31) >> 5;
            for (int ps = 0; ps < nps; ++ps) {
                const bf16x8 f = tr_rows(s_patch + (ps * 32 + trow) * SROW + (wave * 16 + 4 * (li & 3)) * 2, SROW);
                dsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, f, dsum, 0, 0, 0);
                dsq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, f, dsq, 0, 0, 0);
            }
            if (lg == 0) cs[wave * 16 + li] += dsum[0];
            if ((li >> 2) == lg) cs[64 + wave * 16 + li] += mfma_diag(dsq, li);
        }
        __syncthreads();                                     // staging consumed before the next patch lands
    }
    if (p.stats) {
        __syncthreads();
        // (every cs entry was accumulated by one wave in strip order; one exact integer-bin add per channel and workgroup: common.h)
        if (tid < 128) det_add(p.stats + (size_t)g * ADAMML_STAT_SLOTS * 128 + tid, 128, cs[tid]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: dW[co][c][kh][kw] = sum_p dz[p][co] * x[2p + (kh,kw) - 3][c] as an MFMA GEMM with the PIXELS as the reduction
// dimension, M = 64 cout, N = 49 tiles of 16 = one tap x 16 channels each.  The 16 columns of an N tile are the 32 contiguous bytes of one
// patch pixel, so the B fragments come from the patch by tr_pair with a wave-uniform tap offset (as in conv_stem_wgrad_kernel; the patch
// is linear here) and the A fragments from the staged dz tile by tr_rows.  8 waves: wave w owns taps w, w + 8, .. (7 for wave 0, 6 for
// the others) x all four cout tiles = 112 accumulator registers, kept over all strips of the workgroup; one partial [64][784] fp32 per
// workgroup goes to the workspace, and stem16_wgrad_reduce_kernel sums the partials in workgroup order into dw, dropping the padded channels.
constexpr int NTW = 512;
constexpr int DZROW = 128 + 8;       // LDS bytes per staged dz pixel
constexpr int WSLOT = 8;             // 16-byte patch slots per thread (3668 / 512)
constexpr int WDZ = MAXPX * 8 / NTW; // 16-byte dz slots per thread
constexpr int WTAPS = 7;             // taps per wave
constexpr int WG_BLOCKS = 256;       // workgroup cap: one [64][784] fp32 partial (200 KB) each -> <= 51 MB of workspace

struct Stem16WP {
    const bf16_t* x;     // [G*N, H, W, 16]
    const bf16_t* dz;    // [G*N, OH, OW, 64]
    float* ws;           // [nblocks][64][784] partials
    int N, H, W, OH, OW, R, tiles_per_img, total_tiles, tpb, PW, PR;
};

__global__ __launch_bounds__(NTW) void conv_stem16_wgrad_kernel(Stem16WP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* s_patch = smem;                                   // [PR][PW] x 32 B
    char* s_dz = smem + p.PR * p.PW * 32;                   // [MAXPX][DZROW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int nslots = p.PR * p.PW * 2;
    int s_rc[WSLOT];                     // patch row << 12 | patch column of the slot's pixel; -1: dead slot
#pragma unroll
    for (int l = 0; l < WSLOT; ++l) {
        const int e = tid + l * NTW, q = e >> 1;
        const int pr = q / p.PW, pc = q - pr * p.PW;
        s_rc[l] = e < nslots ? (pr << 12 | pc) : -1;
    }
    bf16x8 rp[WSLOT], rz[WDZ];
    unsigned vmask = 0;                  // 1 validity bit per patch slot, then 1 per dz slot (bit WSLOT + l)
    auto load_tile = [&](int tile) {
        const int n = tile / p.tiles_per_img, tr = tile - n * p.tiles_per_img;
        const int ih0 = 2 * tr * p.R - 3;
        vmask = 0;
        const bf16_t* img = p.x + (size_t)n * p.H * p.W * 16 + (tid & 1) * 8;
#pragma unroll
        for (int l = 0; l < WSLOT; ++l) {
            const int ih = s_rc[l] < 0 ? -1 : ih0 + (s_rc[l] >> 12), iw = (s_rc[l] & 4095) - 3;
            rp[l] = *reinterpret_cast<const bf16x8*>(img + ((size_t)min(max(ih, 0), p.H - 1) * p.W + min(max(iw, 0), p.W - 1)) * 16);
            vmask |= (((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) ? 1u : 0u) << l;
        }
        const int oh0 = tr * p.R;
        const int npx = min(p.R, p.OH - oh0) * p.OW;
        const bf16_t* zb = p.dz + ((size_t)n * p.OH + oh0) * p.OW * 64;
#pragma unroll
        for (int l = 0; l < WDZ; ++l) {
            const int e = tid + l * NTW;                       // (pixel e >> 3, chunk e & 7); pixels >= npx contribute zero
            rz[l] = *reinterpret_cast<const bf16x8*>(zb + (size_t)(e < npx * 8 ? e : 0) * 8);
            vmask |= (e < npx * 8 ? 1u : 0u) << (WSLOT + l);
        }
    };
    f32x4 acc[4][WTAPS];                                    // [cout tile][own tap j]: tap = wave + 8*j
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < WTAPS; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int toff[WTAPS];                                        // patch byte offset of each own tap (wave-uniform)
#pragma unroll
    for (int j = 0; j < WTAPS; ++j) {
        const int tap = min(wave + 8 * j, TAPS - 1);
        toff[j] = ((tap / 7) * p.PW + tap % 7) * 32;
    }
    const int tile0 = blockIdx.x * p.tpb;
    if (tile0 < p.total_tiles) load_tile(tile0);
    const int trow = 8 * lg + (li >> 2);                    // pixel of the K step this lane addresses (and +4)
    // patch offsets of this lane's two transposed-read rows for every K step: strip-invariant
    int poff0[MAXPX / 32], poff1[MAXPX / 32];
#pragma unroll
    for (int ks = 0; ks < MAXPX / 32; ++ks) {
        int q0 = ks * 32 + trow, q1 = q0 + 4;
        if (q0 >= p.R * p.OW) q0 = 0;                       // past-the-end pixels read pixel 0 (their dz rows are zero)
        if (q1 >= p.R * p.OW) q1 = 0;
        const int r0 = q0 / p.OW, c0 = q0 - r0 * p.OW, r1 = q1 / p.OW, c1 = q1 - r1 * p.OW;
        poff0[ks] = (2 * r0 * p.PW + 2 * c0) * 32 + (li & 3) * 8;
        poff1[ks] = (2 * r1 * p.PW + 2 * c1) * 32 + (li & 3) * 8;
    }

    for (int it = 0; it < p.tpb; ++it) {
        const int tile = tile0 + it;
        if (tile >= p.total_tiles) break;
#pragma unroll
        for (int l = 0; l < WSLOT; ++l) {
            const int e = tid + l * NTW;
            if (e < nslots) *reinterpret_cast<bf16x8*>(s_patch + e * 16) = (vmask >> l) & 1u ? rp[l] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int l = 0; l < WDZ; ++l) {
            const int e = tid + l * NTW;
            union { struct { s16x4 a, b; } s; bf16x8 v; } u;
            u.v = (vmask >> (WSLOT + l)) & 1u ? rz[l] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            char* dst = s_dz + (e >> 3) * DZROW + (e & 7) * 16;
            *reinterpret_cast<s16x4*>(dst) = u.s.a;
            *reinterpret_cast<s16x4*>(dst + 8) = u.s.b;
        }
        __syncthreads();
        if (it + 1 < p.tpb && tile + 1 < p.total_tiles) load_tile(tile + 1);
        const int tr = tile % p.tiles_per_img;
        const int npx = min(p.R, p.OH - tr * p.R) * p.OW;
        const int nks = (npx + 31) >> 5;
#pragma unroll
        for (int ks = 0; ks < MAXPX / 32; ++ks) {
            if (ks >= nks) break;
            const char* pb0 = s_patch + poff0[ks];
            const char* pb1 = s_patch + poff1[ks];
            const char* zb0 = s_dz + (ks * 32 + trow) * DZROW + 4 * (li & 3) * 2;
            bf16x8 fa[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) fa[mt] = tr_rows(zb0 + mt * 32, DZROW);
#pragma unroll
            for (int j = 0; j < WTAPS; ++j) {
                if (wave + 8 * j < TAPS) {                       // wave-uniform
                    const bf16x8 f = tr_pair(pb0 + toff[j], pb1 + toff[j]);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], f, acc[mt][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                         // strip consumed before the next one lands
    }
    // partial dW of this workgroup: D rows (cout) = mt*16 + lg*4 + r, column (tap, c) = tap*16 + li
    float* out = p.ws + (size_t)blockIdx.x * 64 * KREAL;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int j = 0; j < WTAPS; ++j) {
            const int tap = wave + 8 * j;
            if (tap < TAPS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(size_t)(mt * 16 + lg * 4 + r) * KREAL + tap * 16 + li] = acc[mt][j][r];
            }
        }
}

// dw[co][c][tap] += sum_b ws[b][co][tap][c16]: 16 elements x 16 partial-lanes per workgroup (the partial loop is the long axis)
__global__ __launch_bounds__(256) void stem16_wgrad_reduce_kernel(const float* ws, float* dw, int nblk, int cin_true) {
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + tx;                      // (64 * 784 is a multiple of 16)
    float a = 0.f;
    for (int b = ty; b < nblk; b += 16) a += ws[(size_t)b * 64 * KREAL + e];
    red[ty][tx] = a;
    __syncthreads();
    if (ty == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][tx];
        const int c = e & 15, tap = (e >> 4) % TAPS, co = e / KREAL;
        if (c < cin_true) dw[((size_t)co * cin_true + c) * TAPS + tap] += s;
    }
}

struct Stem16Geom { int R, PR, PW, tiles_per_img; size_t patch; };

Stem16Geom stem16_geom(const adamml_conv_desc_t* d) {
    Stem16Geom g;
    g.R = MAXPX / d->OW > d->OH ? d->OH : MAXPX / d->OW;
    g.PR = 2 * g.R + 5; g.PW = d->W + 6;
    g.tiles_per_img = ceil_div(d->OH, g.R);
    g.patch = (size_t)g.PR * g.PW * 32;
    return g;
}

size_t stem16_fwd_lds(const Stem16Geom& g) {
    const size_t stage = (size_t)MAXPX * SROW;
    return 64 * WROW + 512 + (g.patch > stage ? g.patch : stage);
}

int stem16_wgrad_nblk(const adamml_conv_desc_t* d, int* tpb_out) {
    const Stem16Geom g = stem16_geom(d);
    const long total = (long)(d->groups < 1 ? 1 : d->groups) * d->N * g.tiles_per_img;
    int tpb = (int)((total + WG_BLOCKS - 1) / WG_BLOCKS);
    if (tpb < 1) tpb = 1;
    if (tpb_out) *tpb_out = tpb;
    return (int)((total + tpb - 1) / tpb);
}

}  // namespace

extern "C" int adamml_conv_stem16_supported(const adamml_conv_desc_t* d) {
    if (!d) return 0;
    if (d->KH != 7 || d->KW != 7 || d->stride != 2 || d->pad != 3 || d->Cout != 64 || d->Cin != 16 || d->up > 1) return 0;
    if (d->N < 1 || d->H < 1 || d->W < 2 || d->W % 2 || d->OW != d->W / 2 || d->OH != (d->H + 6 - 7) / 2 + 1 || d->OW > MAXPX) return 0;
    if ((long)(d->groups < 1 ? 1 : d->groups) * d->N * d->OH >= (1L << 30)) return 0;      // (strip indices are ints)
    const Stem16Geom g = stem16_geom(d);
    if (g.PR * g.PW * 2 > MAXSLOT * NT || g.PR * g.PW * 2 > WSLOT * NTW) return 0;
    return stem16_fwd_lds(g) <= (size_t)LDS_BUDGET && g.patch + (size_t)MAXPX * DZROW <= (size_t)LDS_BUDGET;
}

int adamml_conv_stem16_fwd_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, void* y, double* stats, hipStream_t stream) {
    if (!adamml_conv_stem16_supported(d)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd (stem16): not a 16-channel stem shape");
    const Stem16Geom g = stem16_geom(d);
    Stem16P p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w_packed; p.y = (bf16_t*)y; p.stats = stats;
    p.N = d->N; p.H = d->H; p.W = d->W; p.OH = d->OH; p.OW = d->OW;
    p.R = g.R; p.PR = g.PR; p.PW = g.PW; p.tiles_per_img = g.tiles_per_img;
    p.total_tiles = d->N * g.tiles_per_img;
    const int groups = d->groups < 1 ? 1 : d->groups;
    p.gx = (size_t)d->N * d->H * d->W * 16;
    p.gy = (size_t)d->N * d->OH * d->OW * 64;
    // <= 256 workgroups (one per CU) over all groups: the resident weights (101 KB from L2) and the statistics publication are amortised
    // over the consecutive strips of a workgroup (512 workgroups measured 116 us against the tile kernel's 110 at N = 45)
    p.tpb = (int)(((long)p.total_tiles * groups + FWD_BLOCKS - 1) / FWD_BLOCKS);
    if (p.tpb < 1) p.tpb = 1;
    static AdamLdsOnce once;
    int rc = adamml_raise_lds_limit(once, reinterpret_cast<const void*>(conv_stem16_kernel), LDS_BUDGET, "conv_fwd (stem16)");
    if (rc) return rc;
    hipLaunchKernelGGL(conv_stem16_kernel, dim3(ceil_div(p.total_tiles, p.tpb), groups), dim3(NT), stem16_fwd_lds(g), stream, p);
    return adamml_check_launch("conv_fwd (stem16)");
}

size_t adamml_conv_stem16_wgrad_workspace(const adamml_conv_desc_t* d) {
    if (!adamml_conv_stem16_supported(d)) return 0;
    return (size_t)stem16_wgrad_nblk(d, nullptr) * 64 * KREAL * sizeof(float);
}

int adamml_conv_stem16_wgrad_launch(const adamml_conv_desc_t* d, const void* dz, const void* x, float* dw, int cin_true, float* ws,
                                    hipStream_t stream) {
    if (!adamml_conv_stem16_supported(d) || cin_true < 1 || cin_true > 16)
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_weight (stem16): not a 16-channel stem shape");
    const Stem16Geom g = stem16_geom(d);
    Stem16WP p;
    p.x = (const bf16_t*)x; p.dz = (const bf16_t*)dz; p.ws = ws;
    p.N = d->N * (d->groups < 1 ? 1 : d->groups);           // groups are plain batch here: the weight gradient sums over all of them
    p.H = d->H; p.W = d->W; p.OH = d->OH; p.OW = d->OW;
    p.R = g.R; p.PR = g.PR; p.PW = g.PW; p.tiles_per_img = g.tiles_per_img;
    p.total_tiles = p.N * g.tiles_per_img;
    const int nblk = stem16_wgrad_nblk(d, &p.tpb);
    static AdamLdsOnce once;
    int rc = adamml_raise_lds_limit(once, reinterpret_cast<const void*>(conv_stem16_wgrad_kernel), LDS_BUDGET, "conv_bwd_weight (stem16)");
    if (rc) return rc;
    hipLaunchKernelGGL(conv_stem16_wgrad_kernel, dim3(nblk), dim3(NTW), g.patch + (size_t)MAXPX * DZROW, stream, p);
    rc = adamml_check_launch("conv_bwd_weight (stem16)");
    if (rc) return rc;
    hipLaunchKernelGGL(stem16_wgrad_reduce_kernel, dim3(64 * KREAL / 16), dim3(256), 0, stream, (const float*)ws, dw, nblk, cin_true);
    return adamml_check_launch("conv_bwd_weight (stem16 reduce)");
}
