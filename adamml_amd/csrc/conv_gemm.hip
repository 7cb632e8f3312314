// Implicit-GEMM convolution for gfx950: bf16 MFMA (v_mfma_f32_16x16x32_bf16), NHWC activations,
// weights packed [Cout][KH*KW*Cin].  One kernel serves
//   * forward conv (any KxK / stride / pad) with the producer's BatchNorm+activation applied while the
//     input patch is staged into LDS, and per-channel sum / sum-of-squares of the (bf16-rounded) output
//     accumulated in the epilogue (train-mode BN statistics, SURVEY.md section 7 hard part 1);
//   * data-gradient (same kernel on the flipped/transposed weight pack, `up` = forward stride).
// This file: the tile kernel, conv_launch (which instance, or which streaming kernel of another file, serves a launch) and the
// forward / data-gradient entry points.  Weight gradients: conv_wgrad.hip.  Small kernels of the algebraic BatchNorm backward:
// conv_alg.hip.  Tile primitives: tile.h.  Launchers of the other files: conv_internal.h.
//
// Replaces the torch operators called at models/resnet.py:83-113,138,199-210,
// models/sound_mobilenet_v2.py:33-69 and models/policy_net.py:38-95 (nn.Conv2d + nn.BatchNorm2d + ReLU/ReLU6).
#include "common.h"
#include "tile.h"
#include "conv_internal.h"
#include "../../include/adamml_hip.h"
#include <stdlib.h>
#include <stdio.h>


namespace {

constexpr int BP = 128;      // pixels per block tile
constexpr int BK = 32;       // K step (one MFMA K)

struct ConvP {
    const bf16_t* x;
    const bf16_t* w;
    const float* in_scale;
    const float* in_shift;
    bf16_t* y;
    double* stats;
    int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, up, up_shift, act, accumulate;
    int P, K, cin_shift, n_ptiles, n_ctiles, tpb;
    // data-gradient epilogue fused with the BatchNorm backward reduction of the tensor the gradient flows into
    size_t gx, gy;               // element strides between BatchNorm groups of x / y (blockIdx.y = group)
    int in_gstride;
    const bf16_t* bn_z;          // raw conv output that produced the consumer's input (same shape as y), or null
    const float* bn_vec;         // [4][Cout']: scale, shift, mean, invstd of that BatchNorm
    int bn_act;
    // residual form of that epilogue (RES kernels; the gradient flows into the OUTPUT of a residual add,
    // out = act(bn(z) [+ bn2(z2)] + ..)): the activation mask comes from the stored block output, `accumulate` adds the
    // identity-path gradient already in y, and the sums of a second BatchNorm feeding the same add (downsample branch)
    // are accumulated alongside
    const bf16_t* res_out;       // block output [same shape as y]
    const uint8_t* res_mask;     // or: 1 bit per element, act'(block output) != 0 (adamml_bn_act_add_mask) -- 1/16 of the bytes
    int res_act;
    const bf16_t* bn_z2;         // raw output of the second BatchNorm'd operand of the add, or null
    const float* bn_vec2;
    double* stats2;
    // DUAL kernels (1x1 data gradient whose input dz is the BatchNorm backward of (g, z)): the loader reads g (= x) and z
    // (= x2) and forms dz = A[c] g + B[c] z + C[c] on the way into LDS (aff = [3][K] per group); `side` (optional) receives
    // dz for the weight-gradient kernel, written by the workgroups of cout tile 0 -- adamml_bn_bwd_apply never runs
    const bf16_t* x2;
    const float* aff;
    bf16_t* side;
    // K-concatenated second input (MODE 0): K steps k >= K1 read xb [pixels][C2] (with the lazy in_scale / in_shift transform,
    // which then applies to xb ONLY) instead of x [pixels][K1]; weights are per group (gw elements apart); epi_add [Cout] per
    // group is added to every output row before the epilogue's mask / store.  Used by the algebraic BatchNorm backward
    // (adamml_conv_bwd_data_alg): dx = (W^T diag(A)) g' + (W^T diag(B) W) a + W^T C without ever forming dz.
    const bf16_t* xb;
    int K1, C2;
    size_t gw;
    const float* epi_add;
    // FADD kernels (forward 1x1 conv whose BatchNorm vectors are known BEFORE the launch -- eval mode, or train mode with the
    // statistics derived from the Gram matrix of the input, adamml_gram_stats): the epilogue applies bn_vec (scale, shift of
    // THIS conv's BatchNorm), adds the identity operand res_out (optionally lazily normalised with id_scale / id_shift),
    // applies res_act and writes the block output + its 1-bit activation mask; the raw conv output never reaches HBM
    const float* id_scale;
    const float* id_shift;
    int id_gstride;
    uint8_t* mask_out;
    // PF (RES + EID kernels): the per-group product P[g][cout][c] = sum_p g'[p][cout] * a[p][c] of the gradient tile this kernel
    // has just formed with a second, lazily normalised tensor a [pixels][pf_C] (the input of the conv whose output gradient g'
    // is -- the g'^T a of the algebraic BatchNorm backward) is accumulated on the matrix cores from the staged tile: the separate
    // pass over g' and a (adamml_conv_bwd_weight_grouped) disappears.  One partial [BC][pf_C] per workgroup -> pf_ws.
    const bf16_t* pf_a;
    const float* pf_scale;
    const float* pf_shift;
    float* pf_ws;                // [group][cout tile][split = workgroup of that pair][BC][pf_C]
    int pf_act, pf_gs, pf_nsplit;
    // MODE 3 (one parity class of the data gradient of a stride-2 conv, see conv_dgrad_stride2)
    int wK;                      // weight row stride in elements (== K except in MODE 3, where K covers the class taps only)
    int cls_nt;                  // taps of this class (0..4)
    unsigned cls_code;           // per tap, 8 bits: dh | dw << 1 | weight-pack tap index << 2
    int oH, oW, o_ph, o_pw;      // output rows are scattered: pixel (i, j) of the class grid -> (2i + o_ph, 2j + o_pw) of [oH, oW]
    // TP (FADD kernels): the block output feeds ONLY a temporal max-pool (models/common.py:4-33 after the last block of a ResNet stage,
    // models/resnet.py:205-209).  A pixel tile then holds the TP frames of a clip for BP / TP pixels (row r = frame r / (BP / TP), pixel
    // r % (BP / TP) of block tp_blk), the epilogue pools over the frames and writes the POOLED tensor tp_y [clips * TP / 2][Q][Cout] and
    // 2 bits per pooled element (tp_code, one uint16 per 8-channel chunk: window tap 0..2 of the first maximum, 3 = maximum <= 0, i.e.
    // no gradient passes the ReLU) -- the full-rate block output, its activation mask and the pool's own pass never touch HBM
    int tp_nblk, tp_Q;           // pixel blocks per clip (ceil(Q / (BP / TP))), pixels per frame
    bf16_t* tp_y;
    uint16_t* tp_code;
};

__device__ __forceinline__ int lds_off(int row, int chunk) {
    // 64-byte rows, 16-byte chunks, chunk ^= 2*((row>>3)&1): conflict-free ds_read_b128 for the
    // 16-lane service groups of gfx950 (MI355X_MICROARCH.md LDS table)
    return row * 64 + ((chunk ^ (((row >> 3) & 1) << 1)) << 4);
}

// MODE 0: 1x1 conv; MODE 1: KxK conv, fast tap addressing (per-row validity mask + LDS tap-offset table);
// MODE 2: generic path with zero-upsampled input (data gradient of strided convs other than the stride-2 fast path);
// MODE 3: one parity class of a stride-2 data gradient: MODE 1 addressing over the class's tap subset (input and weight
//         tap tables), output rows scattered with stride 2 -- no MFMA or load is spent on the zeros of the up-sampling.
// PD = register prefetch depth (K steps of global loads in flight).  PD 1 keeps 3-4 workgroups per CU (latency hidden by
// occupancy: best for the big, short-K layers); PD 3 is for small grids with long K loops (layer3/4), where a CU holds a
// single workgroup and only explicit look-ahead hides the HBM round trip.
// RES: residual form of the BatchNorm-fused data-gradient epilogue (MODE 0, and MODE 1 for dense 3x3 / stride-1 data gradients).  Its epilogue keeps four 16-byte streams
// per row in flight and two sets of per-channel vectors, so it is compiled for 2 workgroups per CU (256 VGPRs) as its own
// instantiation -- inside the shared kernel it pushed every MODE 0 instance into scratch spills.
// DUAL: the BatchNorm-backward affine of two source tensors is applied by the MODE 0 loader (own instantiation as well:
// a second register ring for z, 2 workgroups per CU, deep prefetch).
// CAT: K-concatenated second input + per-group weights + epilogue constant (algebraic BatchNorm backward); own instantiation
// for the same reason.
// FADD: forward conv + BatchNorm + residual add + activation in the epilogue (see ConvP::id_scale); own instantiation.
// GLDS: operands that are plain in memory (no lazy transform) are staged global -> LDS by LDS-DMA through a ring of three tile
// buffers with counted vmcnt across raw barriers (as conv_wgrad_glds_kernel): no register ring, no ds_write pass.
// EID (FADD / RES): the epilogue's identity-side operands (identity tensor; identity-path gradient + activation mask bits) are
// requested at the START of a tile, behind the first operand loads, instead of in the epilogue: the whole tile then costs ONE HBM
// round trip instead of three (operands, 2 x 4 identity rows), and a workgroup keeps ~3x the bytes in flight.  PMC on the layer-1
// shapes: these kernels held ~350 reads outstanding at the fabric against ~700-900 of the elementwise kernels (TCC_EA0_RDREQ_LEVEL),
// at a LOWER latency per read -- they were bound by their own request rate, not by HBM.  Costs 32 VGPRs: 2 workgroups per CU.
// LZF (GLDS, MODE 0): the lazy BatchNorm + activation transform of the INPUT is applied to the MFMA fragment after its ds_read
// instead of on the way into LDS, so that lazily normalised inputs can be staged by LDS-DMA as well (raw tile global -> LDS, deep
// counted-vmcnt pipeline, no register ring / ds_write pass / exec-masked loads).  Same fma / clamp / round sequence on the same
// values: bit-identical to the staging-side transform.  The two waves that share a pixel half repeat the transform (VALU has the
// slack on these HBM-bound layers); K <= 512 (per-channel vectors in LDS).
// EPI: which epilogue of the plain (non-RES / non-FADD) kernels is compiled.  -1: all of them, selected at run time (the CAT / DUAL /
// deep-prefetch / MODE 2 instances); 0: forward (plain store + statistics on the matrix cores); 1: data gradient with the activation
// mask and the BatchNorm-backward sums (bn_z); 2: data gradient, optionally accumulating into y.  One kernel body for all three made
// every edit of a data-gradient epilogue move the register allocation of the forward instances (spills inside their K loops); apart,
// the forward instances carry no dead epilogue state and the data-gradient ones can request a batch of rows ahead of their stores.
// PF: see ConvP::pf_a (BC = 128, 64 channels of a; RES + GLDS + EID only).
// Workgroups per CU the register allocation is sized for.  The fused instances (RES / DUAL / CAT / EID) take 256 registers; the plain
// ones rely on occupancy (PD 1: 3-4 workgroups per CU) or on their register ring (PD 3).  The instances under "fewer" did not fit
// that budget (2-13 registers in scratch, tools/kernel_resources.py) and get one workgroup less: the data-gradient epilogues behind the
// KxK loaders at 64-wide tiles (EPI 1 -- compiled behind LDS-DMA only, as is MODE 3: a gradient operand is never lazy -- and EPI 2), the
// register-staged accumulating KxK epilogue at 128, the strided (MODE 2) loaders and the FADD epilogue without EID.
constexpr int conv_gemm_wg_per_cu(int BC, int MODE, int PD, bool RES, bool DUAL, bool CAT, bool FADD, bool GLDS, int EID, int EPI) {
    if (RES || DUAL || CAT || EID) return 2;
    const int n = PD == 1 ? (BC == 128 ? 3 : 4) : (BC == 128 ? 2 : 3);
    const bool fewer = (MODE == 2 && !(BC == 128 && PD == 3)) || FADD ||
                       (BC == 64 && PD == 1 && ((EPI == 1 && MODE != 0) || (EPI == 2 && MODE == 1))) ||
                       (BC == 128 && MODE == 1 && EPI == 2 && !GLDS);
    return fewer ? n - 1 : n;
}

template <int BC, int MODE, int PD, bool RES = false, bool DUAL = false, bool CAT = false, bool FADD = false, bool GLDS = false, int EID = 0,
          bool LZF = false, int EPI = -1, bool PF = false, int TP = 0>
__global__ __launch_bounds__(NTHREADS, conv_gemm_wg_per_cu(BC, MODE, PD, RES, DUAL, CAT, FADD, GLDS, EID, EPI)) void conv_gemm_kernel(ConvP p) {
    static_assert(TP == 0 || (FADD && EID && MODE == 0 && BC == 128 && (TP == 2 || TP == 4 || TP == 8)), "TP: FADD + EID, 128-wide cout tiles");
    constexpr int PPF = TP ? BP / TP : BP;  // TP: pixels of one frame in a tile
    constexpr int WCT = BC / 32;            // 16-wide cout tiles per wave
    constexpr int WROWS = BC / 64;          // weight rows staged per thread
    constexpr int TILE_BYTES = (BP + BC) * 64;
    constexpr int EPI_BYTES = BP * (BC * 2 + 16);
    constexpr int NBUF = GLDS ? 3 : 2;
    constexpr int STAGE_BYTES = (NBUF * TILE_BYTES) > EPI_BYTES ? (NBUF * TILE_BYTES) : EPI_BYTES;
    // per-channel sums of a workgroup: the forward statistics come out of the matrix cores with ONE owner wave per channel (one row of
    // 2 * BC floats); the data-gradient epilogues fold on the VALU, where all four waves hold partials of every channel -- each wave then
    // accumulates into its own row and the rows are summed in wave order at publication (common.h: reproducible reductions)
    constexpr int NSR = (FADD || EPI == 0) ? 1 : 4;
    constexpr int CS_BYTES = NSR * 2 * BC * 4;
    constexpr int CS2_OFF = STAGE_BYTES + CS_BYTES + (MODE == 0 ? 0 : 256) + (MODE == 3 ? BP * 4 + 16 : 0);     // second sum set (RES); 256: tap tables
    // MODE 0: the per-input-channel vectors of the loader transform (lazy BatchNorm scale / shift, or the three DUAL affine
    // vectors) are staged in LDS once per workgroup when K <= VEC_MAXK: read from global inside store_tile they were an
    // exposed L1/L2 round trip in every K step (the loads can only be issued when the tile registers are consumed)
    constexpr int VEC_MAXK = 1024;
    constexpr int VEC_OFF = CS2_OFF + (RES ? CS_BYTES : 0);
    constexpr int LZF_MAXK = 512;              // LZF keeps 3 workgroups per CU at BC = 128: 3 x (3 tiles + sums + 4 KB of vectors) <= 160 KB
    constexpr int PF_C = 64;                   // channels of the PF operand
    constexpr int PF_OFF = (VEC_OFF + (LZF ? 2 * LZF_MAXK * 4 : (MODE == 0 && !GLDS) ? (DUAL ? 3 : 2) * VEC_MAXK * 4 : 0) + 1023) / 1024 * 1024;
    constexpr int SMEM_BYTES = PF ? PF_OFF + BP * PF_C * 2 : VEC_OFF + (LZF ? 2 * LZF_MAXK * 4 : (MODE == 0 && !GLDS) ? (DUAL ? 3 : 2) * VEC_MAXK * 4 : 0);   // + per-channel sums + tap-offset table (+ MODE 3: output row table, weight tap table)
    __shared__ __attribute__((aligned(1024))) char smem[SMEM_BYTES];

    {   // BatchNorm group of this workgroup: one launch covers the S per-segment calls of the reference
        const int g = blockIdx.y;
        p.x += (size_t)g * p.gx;
        p.y += (size_t)g * p.gy;
        if (p.stats) p.stats += (size_t)g * ADAMML_STAT_SLOTS * 2 * p.Cout;
        if (p.in_scale) { p.in_scale += (size_t)g * p.in_gstride; p.in_shift += (size_t)g * p.in_gstride; }
        if (p.bn_z) { p.bn_z += (size_t)g * p.gy; p.bn_vec += (size_t)g * 4 * p.Cout; }
        if (CAT) {
            p.xb += (size_t)g * (p.gx / p.K1) * p.C2;
            p.w += (size_t)g * p.gw;
            p.epi_add += (size_t)g * p.Cout;
        }
        if (DUAL) {
            p.x2 += (size_t)g * p.gx;
            p.aff += (size_t)g * 3 * p.K;
            if (p.side) p.side += (size_t)g * p.gx;
        }
        if (FADD) {
            p.bn_vec += (size_t)g * 4 * p.Cout;
            if (p.res_out) p.res_out += (size_t)g * p.gy;
            if (p.mask_out) p.mask_out += ((size_t)g * p.gy) >> 3;
            if (p.id_scale) { p.id_scale += (size_t)g * p.id_gstride; p.id_shift += (size_t)g * p.id_gstride; }
            if (TP) { p.tp_y += (size_t)g * (p.gy >> 1); if (p.tp_code) p.tp_code += ((size_t)g * (p.gy >> 1)) >> 3; }
        }
        if (PF) {
            p.pf_a += (size_t)g * p.P * PF_C;
            if (p.pf_scale) { p.pf_scale += (size_t)g * p.pf_gs; p.pf_shift += (size_t)g * p.pf_gs; }
        }
        if (RES) {
            p.res_out += (size_t)g * p.gy;
            if (p.res_mask) p.res_mask += ((size_t)g * p.gy) >> 3;
            if (p.bn_z2) { p.bn_z2 += (size_t)g * p.gy; p.bn_vec2 += (size_t)g * 4 * p.Cout; p.stats2 += (size_t)g * ADAMML_STAT_SLOTS * 2 * p.Cout; }
        }
    }
    const int tid = threadIdx.x;
    float* s_vec = reinterpret_cast<float*>(smem + (MODE == 0 ? VEC_OFF : 0));
    const int nvec = CAT ? p.C2 : p.K;                            // entries of the loader's per-channel vectors
    const bool vec_lds = MODE == 0 && nvec <= VEC_MAXK && (DUAL || p.in_scale != nullptr);
    if (LZF) {
        // scale at [0, LZF_MAXK), shift at [LZF_MAXK, 2 LZF_MAXK); zero beyond K up to the K-step boundary (zero weights there, but
        // 0 * garbage must not make a NaN)
        const int kpad = (p.K + BK - 1) / BK * BK;
        for (int i = tid; i < kpad; i += NTHREADS) {
            s_vec[i] = i < p.K ? p.in_scale[i] : 0.f;
            s_vec[LZF_MAXK + i] = i < p.K ? p.in_shift[i] : 0.f;
        }
        __syncthreads();
    } else
    if (vec_lds) {
        if (DUAL) {
            for (int i = tid; i < 3 * p.K; i += NTHREADS) s_vec[i] = p.aff[i];
        } else {
            for (int i = tid; i < nvec; i += NTHREADS) { s_vec[i] = p.in_scale[i]; s_vec[nvec + i] = p.in_shift[i]; }
        }
        __syncthreads();
    }
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wp = wave & 1;                // pixel half
    const int wc = wave >> 1;               // cout half

    // XCD-aware tile order: blocks b, b+8, b+16.. share an XCD (and its L2); give them consecutive
    // tiles so the cout tiles of one pixel tile hit the same L2 (cdna_hip_programming.md T1, bijective form)
    // (common.h's xcd_contiguous in signed arithmetic, kept as text: through the unsigned helper every instance keeps its resources and
    // gets other instructions -- bid feeds the two signed divisions below)
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int ctile = bid % p.n_ctiles;
    const int pgrp = bid / p.n_ctiles;
    const int c0 = ctile * BC;

    const int chunk = tid & 3;
    const int row_a = tid >> 2;             // 0..63 (+64 for second row)
    int* s_tapoff = reinterpret_cast<int*>(smem + STAGE_BYTES + CS_BYTES);    // MODE 1/3: element offset of each tap
    int* s_wtap = s_tapoff + 64;                                              // MODE 3: weight offset of each class tap [4]
    int* s_orow = s_wtap + 4;                                                 // MODE 3: output row of each tile pixel [BP]
    if (MODE == 1) {
        if (tid < p.KH * p.KW) {
            const int kh = tid / p.KW, kw = tid - kh * p.KW;
            s_tapoff[tid] = (kh * p.W + kw) * p.Cin;
        }
    }
    if (MODE == 3) {
        if (tid < p.cls_nt) {
            const unsigned code = (p.cls_code >> (8 * tid)) & 0xffu;
            s_tapoff[tid] = ((int)(code & 1) * p.W + (int)((code >> 1) & 1)) * p.Cin;
            s_wtap[tid] = (int)(code >> 2) * p.Cin;
        }
    }
    const bf16_t* wrow[WROWS];
    bool w_ok[WROWS];
#pragma unroll
    for (int r = 0; r < WROWS; ++r) {
        int co = c0 + row_a + r * 64;
        w_ok[r] = co < p.Cout;
        wrow[r] = p.w + (size_t)(w_ok[r] ? co : 0) * p.wK;
    }
    const int li = lane & 15, lg = lane >> 4;
    // epilogue thread mapping (fixed across the tiles of this workgroup, so the per-channel sums live in registers)
    constexpr int CROW = BC * 2 + 16;                  // LDS row stride (bytes): +16 B skews the banks
    static_assert(BP * CROW <= STAGE_BYTES, "epilogue tile must fit the staging buffers");
    float* cs = reinterpret_cast<float*>(smem + STAGE_BYTES);          // [NSR][2*BC] channel sums, live across the tile loop
    float* cs2 = reinterpret_cast<float*>(smem + CS2_OFF);             // [NSR][2*BC] sums of the second BatchNorm (RES only)
    const bool second = RES && p.bn_z2 != nullptr;
    const bool epi_bnz = EPI < 0 ? p.bn_z != nullptr : EPI == 1;
    const bool epi_acc = EPI < 0 ? p.accumulate != 0 : (EPI == 2 && p.accumulate != 0);
    if (p.stats) {
        for (int i = tid; i < NSR * 2 * BC; i += NTHREADS) cs[i] = 0.f;
        if (second)
            for (int i = tid; i < NSR * 2 * BC; i += NTHREADS) cs2[i] = 0.f;
    }
    constexpr int CPR = BC / 8;                        // 16-byte chunks per tile row
    constexpr int RSTEP = NTHREADS / CPR;              // rows covered per pass
    const int ech = tid % CPR, erow0 = tid / CPR;
    const int eco = c0 + ech * 8;

    // PF: product accumulators of this wave (64 cout x 32 a-channels of the workgroup's [128][64] block), live across the tile loop,
    // and the per-lane scale / shift of the transposed a fragment (8 pixels of ONE channel per lane: conv_wgrad_glds_kernel LZB)
    f32x4 pacc[PF ? 4 : 1][PF ? 2 : 1];
    float pfs[PF ? 2 : 1], pfh[PF ? 2 : 1];
    if constexpr (PF) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) pacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ch = wc * 32 + t * 16 + li;
            pfs[t] = p.pf_scale ? p.pf_scale[ch] : 1.f;
            pfh[t] = p.pf_scale ? p.pf_shift[ch] : 0.f;
        }
    }
    // a workgroup walks `tpb` consecutive pixel tiles of its cout tile: statistics are published once per workgroup
    for (int it = 0; it < p.tpb; ++it) {
    const int ptile = pgrp * p.tpb + it;
    if (ptile >= p.n_ptiles) break;
    const int p0 = ptile * BP;
    // TP: tile = (clip, pixel block); tile row r -> pixel (clip * TP + r / PPF) * Q + blk * PPF + r % PPF, valid while the pixel exists
    const int tp_clip = TP ? ptile / p.tp_nblk : 0;
    const int tp_q0 = TP ? (ptile - tp_clip * p.tp_nblk) * PPF : 0;
    auto tp_row = [&](int r, bool& ok) -> int {
        const int q = tp_q0 + (r % PPF);
        ok = q < p.tp_Q;
        return (tp_clip * TP + r / PPF) * p.tp_Q + (ok ? q : 0);
    };

    // ---- per-thread staging coordinates -------------------------------------------------------
    int a_n[2], a_h0[2], a_w0[2], a_base[2];
    unsigned long long a_mask[2];
    bool a_ok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int pp = p0 + row_a + r * 64;
        a_ok[r] = pp < p.P;
        int ppc = a_ok[r] ? pp : 0;
        if constexpr (TP != 0) {
            bool ok;
            ppc = tp_row(row_a + r * 64, ok);
            a_ok[r] = ok;
        }
        if (MODE == 0 && p.stride == 1 && p.pad == 0) {
            // 1x1 / stride 1 (pad 0): the input pixel IS the output pixel -- none of the two integer divisions below (~80 VALU
            // instructions per row, executed per tile AHEAD of the tile's first load)
            a_n[r] = a_h0[r] = a_w0[r] = 0;
            a_base[r] = ppc * p.Cin;
            a_mask[r] = 0;
            continue;
        }
        int n = ppc / (p.OH * p.OW);
        int rem = ppc - n * (p.OH * p.OW);
        int oh = rem / p.OW;
        int ow = rem - oh * p.OW;
        a_n[r] = n;
        a_h0[r] = oh * p.stride - p.pad;
        a_w0[r] = ow * p.stride - p.pad;
        a_base[r] = ((n * p.H + a_h0[r]) * p.W + a_w0[r]) * p.Cin;      // may point before the row start for padded taps
        unsigned long long m = 0;
        if (MODE == 1 && a_ok[r]) {
            for (int kh = 0; kh < p.KH; ++kh) {
                const bool hok = (unsigned)(a_h0[r] + kh) < (unsigned)p.H;
                for (int kw = 0; kw < p.KW; ++kw)
                    if (hok && (unsigned)(a_w0[r] + kw) < (unsigned)p.W) m |= 1ull << (kh * p.KW + kw);
            }
        }
        if (MODE == 3 && a_ok[r]) {
            for (int t = 0; t < p.cls_nt; ++t) {
                const unsigned code = (p.cls_code >> (8 * t)) & 0xffu;
                if ((unsigned)(a_h0[r] + (int)(code & 1)) < (unsigned)p.H && (unsigned)(a_w0[r] + (int)((code >> 1) & 1)) < (unsigned)p.W)
                    m |= 1ull << t;
            }
        }
        a_mask[r] = m;
    }
    if (MODE == 3 && tid < BP) {
        // scattered output rows of this tile (read by the epilogue, after at least one barrier)
        const int pp = p0 + tid;
        int orow = 0;
        if (pp < p.P) {
            const int n = pp / (p.OH * p.OW), rem = pp - n * (p.OH * p.OW);
            const int i = rem / p.OW, j = rem - i * p.OW;
            orow = (n * p.oH + 2 * i + p.o_ph) * p.oW + 2 * j + p.o_pw;
        }
        s_orow[tid] = orow;
    }
    if ((MODE == 1 || MODE == 3) && it == 0) __syncthreads();          // tap-offset tables visible

    // EID: identity-side operands of this tile's epilogue (every lane loads -- clamped addresses -- so that the number of
    // outstanding VMEM operations is the same for every wave: the LDS-DMA loop below waits with counted vmcnt)
    constexpr int NRE = BP / RSTEP;
    bf16x8 eid[EID ? NRE : 1];
    unsigned embits[EID ? NRE : 1];
    auto issue_eid = [&]() {
        if constexpr (PF) {
            // a tile [128 pixels][64 channels] raw, as four [32][64] transpose-read images (source-side swizzle, conv_wgrad_glds_kernel):
            // LDS chunk e = l * 256 + tid -> row e / 8, position e % 8 holds source chunk position ^ swizzle(row % 32)
            const bf16_t* zeros = reinterpret_cast<const bf16_t*>(g_zero_page);
            const unsigned pbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + PF_OFF + wave * 1024;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const int e = tid + l * NTHREADS;
                const int row = e >> 3;
                const int ch = (e & 7) ^ (tr_swz<64>(row & 31) >> 1);
                const bf16_t* src = (p0 + row < p.P) ? p.pf_a + (size_t)(p0 + row) * PF_C + ch * 8 : zeros;
                glds16(src, __builtin_amdgcn_readfirstlane(pbase + l * NTHREADS * 16));
            }
        }
        if constexpr (EID != 0) {
            const int ecoc = eco < p.Cout ? eco : 0;
#pragma unroll
            for (int j = 0; j < NRE; ++j) {
                const int r = erow0 + j * RSTEP;
                size_t pre = (size_t)(p0 + r < p.P ? p0 + r : p0) * p.Cout + ecoc;
                if constexpr (TP != 0) {
                    bool ok;
                    pre = (size_t)tp_row(r, ok) * p.Cout + ecoc;
                }
                if (FADD) eid[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.res_out + pre));
                else {
                    eid[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.y + pre));
                    embits[j] = p.res_mask[pre >> 3];
                }
            }
        }
    };
    constexpr int NEID = (EID ? (FADD ? NRE : 2 * NRE) : 0) + (PF ? 4 : 0);       // VMEM loads issue_eid() puts in flight per thread

    // register prefetch ring of depth PD: global loads run PD K-steps ahead of the MFMAs.  One K step of compute is
    // ~0.15 us but an HBM round trip is 1-2 us, so a one-step look-ahead left the kernel latency-bound.
    // UNC (the deep rings): every ring load is issued UNCONDITIONALLY from a clamped (always valid) address and zeroed on its way into
    // LDS.  Behind `if (ok)` each load sat in its own exec-masked block; the compiler's wait-count bookkeeping must then assume that none
    // of the younger loads was issued and waits for a slot with vmcnt(0) -- at the top of every PD K steps the whole ring drained and the
    // most recent request was exposed as a full HBM round trip (the ring was one step deep in effect).  Unconditional loads make the
    // counts exact: the wait for a slot leaves the (PD - 1) younger slots in flight.
    // Only the CAT / DUAL instances: the plain deep-ring instances (layer 3-4 shapes, small grids) measured 5-7 % SLOWER with it.
    constexpr bool UNC = PD > 1 && (CAT || DUAL);
    bf16x8 ra[PD][2], rw[PD][WROWS];
    bf16x8 ra2[DUAL ? PD : 1][2];
    int rci[PD];
    bool rav[PD][2];
    bool rkok[UNC ? PD : 1];
#pragma unroll
    for (int i = 0; i < PD; ++i) rci[i] = 0;

    auto issue_loads = [&](auto slot_c, int kt) {
        constexpr int SL = decltype(slot_c)::value;
        const int k = kt * BK + chunk * 8;
        const bool kok = k < p.K;
        int kw_off = k;                                  // offset of this K chunk in a weight row
        if (MODE == 0) {
            const bool from_b = CAT && kt * BK >= p.K1;                 // wave-uniform: a K step lies in one source (K1 % BK == 0)
            rci[SL] = from_b ? k - p.K1 : (CAT ? -1 : k);               // < 0: no lazy transform for this step
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool ok = a_ok[r] && kok;
                rav[SL][r] = ok;
                if constexpr (UNC) {
                    const bf16_t* src = p.x + (size_t)(unsigned)(a_base[r] + k);
                    if (CAT && from_b) src = p.xb + (size_t)(unsigned)(a_base[r] / p.K1) * p.C2 + (k - p.K1);
                    ra[SL][r] = *reinterpret_cast<const bf16x8*>(ok ? src : p.x);
                    if (DUAL) ra2[DUAL ? SL : 0][r] = *reinterpret_cast<const bf16x8*>(ok ? p.x2 + (size_t)(unsigned)(a_base[r] + k) : p.x2);
                    continue;
                }
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (CAT && from_b) {
                    if (ok) v = *reinterpret_cast<const bf16x8*>(p.xb + (size_t)(unsigned)(a_base[r] / p.K1) * p.C2 + (k - p.K1));
                } else if (ok) v = *reinterpret_cast<const bf16x8*>(p.x + (size_t)(unsigned)(a_base[r] + k));
                ra[SL][r] = v;
                if (DUAL) {
                    bf16x8 v2 = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (ok) v2 = *reinterpret_cast<const bf16x8*>(p.x2 + (size_t)(unsigned)(a_base[r] + k));
                    ra2[DUAL ? SL : 0][r] = v2;
                }
            }
        } else if (MODE == 1 || MODE == 3) {
            const int tap = kok ? (k >> p.cin_shift) : 0;
            const int ci = k & (p.Cin - 1);
            const int toff = s_tapoff[tap] + ci;
            if (MODE == 3) kw_off = s_wtap[tap] + ci;
            rci[SL] = ci;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool ok = kok && ((a_mask[r] >> tap) & 1ull);
                rav[SL][r] = ok;
                if constexpr (UNC) {
                    ra[SL][r] = *reinterpret_cast<const bf16x8*>(ok ? p.x + (size_t)(unsigned)(a_base[r] + toff) : p.x);
                    continue;
                }
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) v = *reinterpret_cast<const bf16x8*>(p.x + (size_t)(unsigned)(a_base[r] + toff));
                ra[SL][r] = v;
            }
        } else {
            const int tap = k >> p.cin_shift;
            const int ci = k - (tap << p.cin_shift);
            const int kh = tap / p.KW, kw = tap - kh * p.KW;
            rci[SL] = ci;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int ih = a_h0[r] + kh, iw = a_w0[r] + kw;
                bool ok = a_ok[r] && kok && ih >= 0 && iw >= 0;
                ok = ok && ((ih | iw) & (p.up - 1)) == 0;
                ih >>= p.up_shift;
                iw >>= p.up_shift;
                ok = ok && ih < p.H && iw < p.W;
                rav[SL][r] = ok;
                if constexpr (UNC) {
                    ra[SL][r] = *reinterpret_cast<const bf16x8*>(ok ? p.x + ((size_t)(a_n[r] * p.H + ih) * p.W + iw) * p.Cin + ci : p.x);
                    continue;
                }
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) v = *reinterpret_cast<const bf16x8*>(p.x + ((size_t)(a_n[r] * p.H + ih) * p.W + iw) * p.Cin + ci);
                ra[SL][r] = v;
            }
        }
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            if constexpr (UNC) {
                rw[SL][r] = *reinterpret_cast<const bf16x8*>(wrow[r] + (kok ? kw_off : 0));       // (wrow is row 0 for rows past Cout)
                continue;
            }
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (w_ok[r] && kok) v = *reinterpret_cast<const bf16x8*>(wrow[r] + kw_off);
            rw[SL][r] = v;
        }
        if constexpr (UNC) rkok[SL] = kok;
    };
    auto store_tile = [&](auto slot_c, int buf) {
        constexpr int SL = decltype(slot_c)::value;
        char* base = smem + buf * TILE_BYTES;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            bf16x8 v = ra[SL][r];
            if (DUAL) {
                if (rav[SL][r]) {
                    const f32x8 gv = bf8_to_f32(v), zv = bf8_to_f32(ra2[DUAL ? SL : 0][r]);
                    f32x8 ca, cb, cc;
                    if (vec_lds) { ca = load_f32x8(s_vec + rci[SL]); cb = load_f32x8(s_vec + p.K + rci[SL]); cc = load_f32x8(s_vec + 2 * p.K + rci[SL]); }
                    else { ca = load_f32x8(p.aff + rci[SL]); cb = load_f32x8(p.aff + p.K + rci[SL]); cc = load_f32x8(p.aff + 2 * p.K + rci[SL]); }
                    f32x8 o;
#pragma unroll
                    for (int i = 0; i < 8; ++i) o[i] = fmaf(ca[i], gv[i], fmaf(cb[i], zv[i], cc[i]));
                    v = f32_to_bf8(o);
                    if (p.side && ctile == 0) *reinterpret_cast<bf16x8*>(p.side + (size_t)(unsigned)(a_base[r] + rci[SL])) = v;
                }
            } else if (p.in_scale && rav[SL][r] && (!CAT || rci[SL] >= 0)) {
                if (vec_lds) {
                    const f32x8 sc = load_f32x8(s_vec + rci[SL]), sh = load_f32x8(s_vec + nvec + rci[SL]);
                    const float lo = act_lo(p.act), hi = act_hi(p.act);
                    f32x8 f = bf8_to_f32(v);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], sc[i], sh[i]), lo, hi);
                    v = f32_to_bf8(f);
                } else v = f32_to_bf8(transform8(v, p.in_scale, p.in_shift, rci[SL], p.act));
            }
            if (UNC && !rav[SL][r]) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            *reinterpret_cast<bf16x8*>(base + lds_off(row_a + r * 64, chunk)) = v;
        }
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            bf16x8 v = rw[SL][r];
            if (UNC && !(w_ok[r] && rkok[UNC ? SL : 0])) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            *reinterpret_cast<bf16x8*>(base + BP * 64 + lds_off(row_a + r * 64, chunk)) = v;
        }
    };

    f32x4 acc[WCT][4];
#pragma unroll
    for (int i = 0; i < WCT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (p.K + BK - 1) / BK;
    const bool tail_rows = TP ? tp_q0 + PPF > p.tp_Q : p0 + BP > p.P;      // (uniform) this tile has rows without a pixel
    auto compute = [&](int buf, int kt = 0) {
        const char* base = smem + buf * TILE_BYTES;
        bf16x8 fa[4], fw[WCT];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            fa[t] = *reinterpret_cast<const bf16x8*>(base + lds_off(wp * 64 + t * 16 + li, lg));
        if constexpr (LZF) {
            // fragment lane (pixel li of tile t, K chunk lg) = 8 consecutive input channels kt*32 + lg*8 ..+7 of one pixel
            const f32x8 sc = load_f32x8(s_vec + kt * BK + lg * 8), sh = load_f32x8(s_vec + LZF_MAXK + kt * BK + lg * 8);
            const float lo = act_lo(p.act), hi = act_hi(p.act);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x8 f = bf8_to_f32(fa[t]);
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], sc[i], sh[i]), lo, hi);
                fa[t] = f32_to_bf8(f);
            }
            if (tail_rows) {                              // zero-filled rows must stay zero (statistics, never-stored outputs)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = wp * 64 + t * 16 + li;
                    if (TP ? tp_q0 + (r % PPF) >= p.tp_Q : p0 + r >= p.P) fa[t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
            }
        }
#pragma unroll
        for (int t = 0; t < WCT; ++t)
            fw[t] = *reinterpret_cast<const bf16x8*>(base + BP * 64 + lds_off(wc * (BC / 2) + t * 16 + li, lg));
#pragma unroll
        for (int ct = 0; ct < WCT; ++ct)
#pragma unroll
            for (int pt = 0; pt < 4; ++pt)
                acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ct], fa[pt], acc[ct][pt], 0, 0, 0);
    };
    if constexpr (GLDS) {
        // LDS-DMA staging: position `chunk` of an LDS row holds source chunk chunk ^ swizzle(row) (lds_off is an involution)
        const bf16_t* zeros = reinterpret_cast<const bf16_t*>(g_zero_page);
        const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + wave * 1024;
        const int kc8 = (chunk ^ (((row_a >> 3) & 1) << 1)) * 8;
        auto glds_stage = [&](int kt, int buf) {
            const int k = kt * BK + kc8;
            const bool kok = k < p.K;
            const unsigned base = lds0 + buf * TILE_BYTES;
            int kw_off = k;
            if (MODE == 0) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const bf16_t* src = (a_ok[r] && kok) ? p.x + (size_t)(unsigned)(a_base[r] + k) : zeros;
                    glds16(src, __builtin_amdgcn_readfirstlane(base + r * 4096));
                }
            } else {
                const int tap = kok ? (k >> p.cin_shift) : 0;
                const int ci = k & (p.Cin - 1);
                const int toff = s_tapoff[tap] + ci;
                if (MODE == 3) kw_off = s_wtap[tap] + ci;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const bool ok = kok && ((a_mask[r] >> tap) & 1ull);
                    const bf16_t* src = ok ? p.x + (size_t)(unsigned)(a_base[r] + toff) : zeros;
                    glds16(src, __builtin_amdgcn_readfirstlane(base + r * 4096));
                }
            }
#pragma unroll
            for (int r = 0; r < WROWS; ++r) {
                const bf16_t* src = (w_ok[r] && kok) ? wrow[r] + kw_off : zeros;
                glds16(src, __builtin_amdgcn_readfirstlane(base + BP * 64 + r * 4096));
            }
        };
        constexpr int PER = 2 + WROWS;                       // LDS-DMAs of this thread per K step
        glds_stage(0, 0);
        if (nk > 1) glds_stage(1, 1);
        issue_eid();                                         // in flight behind steps 0 and 1, ahead of steps 2..
        int buf = 0;
        for (int kt = 0; kt < nk; ++kt) {
            // step kt landed; step kt + 1 may fly -- and, while the steps waited for are OLDER than the EID loads (kt <= 1), so may they
            if (NEID && kt <= 1) {
                if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + NEID) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NEID) : "memory");
            } else
            if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");       // step kt landed, step kt + 1 may fly
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                    // ... for every wave; and everyone is past compute(kt - 1)
            if (kt + 2 < nk) glds_stage(kt + 2, buf == 0 ? 2 : buf - 1);
            compute(buf, kt);
            buf = buf == 2 ? 0 : buf + 1;
        }
    } else {
    int kt0 = 0;
    if (UNC && nk >= 2 * PD) {                           // (uniform)
        // steady state of a deep ring, with NO run-time condition around a load: prologue and every step issue, so the compiler's
        // wait counts are exact (a load issued under a condition -- even a uniform one -- forces every wait that follows the join to
        // assume it was not issued, i.e. vmcnt(0..3) for a slot instead of vmcnt((PD - 1) x loads per slot))
        static_for<PD>([&](auto sc) { issue_loads(sc, (int)decltype(sc)::value); });
        for (; kt0 + 2 * PD <= nk; kt0 += PD) {
            static_for<PD>([&](auto sc) {
                const int kt = kt0 + (int)decltype(sc)::value;
                store_tile(sc, kt & 1);
                issue_loads(sc, kt + PD);
                __syncthreads();
                compute(kt & 1);
            });
        }
    } else {
    // prologue: fill the ring
    static_for<PD>([&](auto sc) {
        if ((int)decltype(sc)::value < nk) issue_loads(sc, (int)decltype(sc)::value);
    });
    }
    issue_eid();
    for (; kt0 < nk; kt0 += PD) {
        static_for<PD>([&](auto sc) {
            const int kt = kt0 + (int)decltype(sc)::value;
            if (kt < nk) {                               // uniform
                store_tile(sc, kt & 1);                  // waits (counted vmcnt) only for this slot's loads
                if (kt + PD < nk) issue_loads(sc, kt + PD);
                __syncthreads();                         // tile kt visible; everyone is past compute(kt-1)
                compute(kt & 1);
            }
        });
    }
    }
    __syncthreads();                                     // operand tiles consumed: the epilogue reuses the LDS

    // ---- epilogue: stage the bf16 tile through LDS, store 16 B per lane fully coalesced, and accumulate the
    //      per-channel sum / sum-of-squares of the stored (rounded) values on the way out -------------------
    // (the last K step ended with __syncthreads(): every wave is done reading the operand tiles)
    f32x8 esum, esq, esq2;
#pragma unroll
    for (int i = 0; i < 8; ++i) esum[i] = esq[i] = esq2[i] = 0.f;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int ct = 0; ct < WCT; ++ct) {
            const int prow = wp * 64 + pt * 16 + li;
            const int ccol = wc * (BC / 2) + ct * 16 + lg * 4;
            *reinterpret_cast<bf16x4*>(smem + prow * CROW + ccol * 2) = f32_to_bf4(acc[ct][pt]);
        }
    __syncthreads();
    if (FADD) {
        // out = act(scale * z + shift + identity): z is the bf16-rounded tile staged above (the value the unfused path would
        // have stored and re-read), the identity operand streams in once, the block output and its activation mask stream
        // out once.  All identity loads of a batch of rows are issued before the first store (in-order vmcnt, see RES).
        if (eco < p.Cout) {
            const f32x8 sc = load_f32x8(p.bn_vec + eco), sh = load_f32x8(p.bn_vec + p.Cout + eco);
            f32x8 isc, ish;
#pragma unroll
            for (int i = 0; i < 8; ++i) { isc[i] = 1.f; ish[i] = 0.f; }
            if (p.id_scale) { isc = load_f32x8(p.id_scale + eco); ish = load_f32x8(p.id_shift + eco); }
            const float rlo = act_lo(p.res_act), rhi = act_hi(p.res_act);
            constexpr int NR = BP / RSTEP, EB = EID ? NR : (NR < 4 ? NR : 4);
            if constexpr (TP != 0) {
                // this thread's NR = 8 rows are rows erow0 + 16 j: NPX = PPF / 16 pixels x TP frames (frame t of pixel s at j = t * NPX + s)
                static_assert(RSTEP == 16 && NR == 8, "TP epilogue mapping");
                constexpr int NPX = PPF / 16, To = TP / 2;
                bf16x8 vb[NR];
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int r = erow0 + j * RSTEP;
                    f32x8 f = bf8_to_f32(*reinterpret_cast<const bf16x8*>(smem + r * CROW + ech * 16));
                    const f32x8 w = bf8_to_f32(eid[j]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], sc[i], sh[i]) + fmaf(w[i], isc[i], ish[i]), rlo, rhi);
                    vb[j] = f32_to_bf8(f);                                  // the value the unfused path stores and the pool re-reads
                }
#pragma unroll
                for (int s = 0; s < NPX; ++s) {
                    const int q = tp_q0 + erow0 + 16 * s;
                    if (q >= p.tp_Q) continue;
#pragma unroll
                    for (int to = 0; to < To; ++to) {
                        f32x8 best;
                        unsigned code = 0;
#pragma unroll
                        for (int i = 0; i < 8; ++i) best[i] = -INFINITY;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int tt = 2 * to - 1 + k;
                            if (tt < 0 || tt >= TP) continue;
                            const f32x8 v = bf8_to_f32(vb[tt * NPX + s]);
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                if (v[i] > best[i] || __builtin_isnan(v[i])) { best[i] = v[i]; code = (code & ~(3u << (2 * i))) | ((unsigned)k << (2 * i)); }   // first maximum in scan order
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (!(best[i] > rlo && best[i] < rhi)) code |= 3u << (2 * i);       // act'(maximum) == 0: no gradient through this window
                        const size_t po = ((size_t)(tp_clip * To + to) * p.tp_Q + q) * p.Cout + eco;
                        *reinterpret_cast<bf16x8*>(p.tp_y + po) = f32_to_bf8(best);
                        if (p.tp_code) p.tp_code[po >> 3] = (uint16_t)code;
                    }
                }
            } else
#pragma unroll
            for (int b0 = 0; b0 < NR; b0 += EB) {
                bf16x8 ir[EB];
                size_t pr[EB];
                bool ok[EB];
#pragma unroll
                for (int j = 0; j < EB; ++j) {
                    const int r = erow0 + (b0 + j) * RSTEP;
                    ok[j] = p0 + r < p.P;
                    pr[j] = (size_t)(ok[j] ? p0 + r : p0) * p.Cout + eco;
                    if constexpr (EID != 0) ir[j] = eid[b0 + j];                 // requested at the start of the tile
                    else if (p.res_out) ir[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.res_out + pr[j]));
                }
#pragma unroll
                for (int j = 0; j < EB; ++j) {
                    const int r = erow0 + (b0 + j) * RSTEP;
                    f32x8 f = bf8_to_f32(*reinterpret_cast<const bf16x8*>(smem + r * CROW + ech * 16));
                    if (p.res_out) {
                        const f32x8 w = bf8_to_f32(ir[j]);
#pragma unroll
                        for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], sc[i], sh[i]) + fmaf(w[i], isc[i], ish[i]), rlo, rhi);
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) f[i] = clamp_act(fmaf(f[i], sc[i], sh[i]), rlo, rhi);
                    }
                    const bf16x8 v = f32_to_bf8(f);
                    if (ok[j]) {
                        *reinterpret_cast<bf16x8*>(p.y + pr[j]) = v;
                        if (p.mask_out) {
                            const f32x8 q = bf8_to_f32(v);
                            unsigned bits = 0;
#pragma unroll
                            for (int i = 0; i < 8; ++i) bits |= (q[i] > rlo && q[i] < rhi) ? (1u << i) : 0u;
                            p.mask_out[pr[j] >> 3] = (uint8_t)bits;
                        }
                    }
                }
            }
        }
    } else if (RES) {
        // Residual form: y already holds the identity-path gradient (accumulate), the mask is act'(block output), and a
        // second BatchNorm operand of the add (downsample branch) gets its sum(g' * zhat2) in the same pass.  Rows are
        // processed in batches of EB: ALL global loads of a batch (z, identity-path gradient, block output, second z) are
        // issued before the first store.  Loads and stores retire in order through vmcnt on this ISA, so a row-at-a-time
        // loop (load, mask, store, next row) exposes one HBM round trip per row, and this epilogue is the whole kernel
        // (K = 64..512: a few MFMA steps per tile).
        if (eco < p.Cout) {
        // bn_z == nullptr: only sum(g') is accumulated (the algebraic BatchNorm backward derives sum(g' zhat) from g'^T a)
        f32x8 mu, is;
        if (p.bn_z) { mu = load_f32x8(p.bn_vec + 2 * p.Cout + eco); is = load_f32x8(p.bn_vec + 3 * p.Cout + eco); }
        f32x8 mu2, is2;
        if (second) { mu2 = load_f32x8(p.bn_vec2 + 2 * p.Cout + eco); is2 = load_f32x8(p.bn_vec2 + 3 * p.Cout + eco); }
        const float rlo = act_lo(p.res_act), rhi = act_hi(p.res_act);
        constexpr int NR = BP / RSTEP, EB = EID ? NR : (NR < 4 ? NR : 4);
#pragma unroll
        for (int b0 = 0; b0 < NR; b0 += EB) {
            bf16x8 zr[EID ? 1 : EB], dr[EB], orr[EID ? 1 : EB], z2r[EID ? 1 : EB];
            unsigned mbits[EB];
            size_t pr[EB];
            bool ok[EB];
#pragma unroll
            for (int j = 0; j < EB; ++j) {
                const int r = erow0 + (b0 + j) * RSTEP;
                ok[j] = p0 + r < p.P;
                pr[j] = (size_t)(ok[j] ? p0 + r : p0) * p.Cout + eco;       // clamped: out-of-range rows re-read row p0, never stored
                if constexpr (EID != 0) {
                    // (the launcher selects EID only for: accumulate, 1-bit mask, no z operands -- the algebraic backward's form)
                    dr[j] = eid[b0 + j];
                    mbits[j] = embits[b0 + j];
                } else {
                if (p.bn_z) zr[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.bn_z + pr[j]));
                if (p.accumulate) dr[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.y + pr[j]));
                if (p.res_mask) mbits[j] = p.res_mask[pr[j] >> 3];
                else orr[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.res_out + pr[j]));
                if (second) z2r[j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p.bn_z2 + pr[j]));
                }
            }
#pragma unroll
            for (int j = 0; j < EB; ++j) {
                const int r = erow0 + (b0 + j) * RSTEP;
                f32x8 f = bf8_to_f32(*reinterpret_cast<const bf16x8*>(smem + r * CROW + ech * 16));
                if (EID || p.accumulate) f += bf8_to_f32(dr[j]);
                if (EID || p.res_mask) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = (mbits[j] >> i) & 1u ? f[i] : 0.f;
                } else {
                    const f32x8 ov = bf8_to_f32(orr[EID ? 0 : j]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = (ov[i] > rlo && ov[i] < rhi) ? f[i] : 0.f;   // (selects, as the bit form above: a masked NaN / inf is 0, not NaN * 0)
                }
                const bf16x8 v = f32_to_bf8(f);
                if (ok[j]) *reinterpret_cast<bf16x8*>(p.y + pr[j]) = v;
                if constexpr (PF)          // g' replaces the raw GEMM tile in LDS (zero rows past the last pixel): A operand of the product
                    *reinterpret_cast<bf16x8*>(smem + r * CROW + ech * 16) = ok[j] ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                const float keep = ok[j] ? 1.f : 0.f;
                f = bf8_to_f32(v) * keep;
                esum += f;
                if constexpr (EID == 0) {
                if (p.bn_z) {
                    const f32x8 zv = bf8_to_f32(zr[j]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) esq[i] += f[i] * (zv[i] - mu[i]) * is[i];
                }
                if (second) {
                    const f32x8 z2 = bf8_to_f32(z2r[j]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) esq2[i] += f[i] * (z2[i] - mu2[i]) * is2[i];
                }
                }
            }
        }
        }
    } else if (eco < p.Cout && epi_bnz) {
        // data gradient w.r.t. a lazily normalised tensor: apply the activation mask here, store g' and accumulate
        // sum(g') and sum(g' * zhat) -- the BatchNorm-backward reduction pass never has to re-read g and z
        const f32x8 sc = load_f32x8(p.bn_vec + eco), sh = load_f32x8(p.bn_vec + p.Cout + eco);
        const f32x8 mu = load_f32x8(p.bn_vec + 2 * p.Cout + eco), is = load_f32x8(p.bn_vec + 3 * p.Cout + eco);
        f32x8 cadd;
#pragma unroll
        for (int i = 0; i < 8; ++i) cadd[i] = 0.f;
        if (CAT) cadd = load_f32x8(p.epi_add + eco);
        // EPI 1: the z rows of a batch of rows are requested before the batch's first store (clamped addresses).  The compiler cannot
        // move a z load above a store to y, and loads / stores retire in order through vmcnt: row at a time, every row exposes one
        // HBM round trip.
        constexpr int NRZ = BP / RSTEP, EBZ = (EPI == 1 || CAT || DUAL) ? (NRZ < 4 ? NRZ : 4) : 1;     // (CAT / DUAL: 2 workgroups per CU, registers to spare)
#pragma unroll 1
        for (int b0 = 0; b0 < NRZ; b0 += EBZ) {                    // (batches not unrolled: less address arithmetic hoisted into registers)
            bf16x8 zrow[EBZ];
#pragma unroll
            for (int j = 0; j < EBZ; ++j) {
                const int r = erow0 + (b0 + j) * RSTEP;
                const int rc = p0 + r < p.P ? r : 0;
                const size_t pp = MODE == 3 ? (size_t)s_orow[rc] : (size_t)(p0 + rc);
                zrow[j] = *reinterpret_cast<const bf16x8*>(p.bn_z + pp * p.Cout + eco);
            }
#pragma unroll
            for (int j = 0; j < EBZ; ++j) {
                const int r = erow0 + (b0 + j) * RSTEP;
                if (p0 + r < p.P) {
                    const size_t pp = MODE == 3 ? (size_t)s_orow[r] : (size_t)(p0 + r);
                    f32x8 f = bf8_to_f32(*reinterpret_cast<const bf16x8*>(smem + r * CROW + ech * 16)) + cadd;
                    const f32x8 zv = bf8_to_f32(zrow[j]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] *= act_mask(fmaf(zv[i], sc[i], sh[i]), p.bn_act);
                    const bf16x8 v = f32_to_bf8(f);
                    *reinterpret_cast<bf16x8*>(p.y + pp * p.Cout + eco) = v;
                    f = bf8_to_f32(v);
                    esum += f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) esq[i] += f[i] * (zv[i] - mu[i]) * is[i];
                }
            }
        }
    } else if (eco < p.Cout) {
        // (EPI 2: the rows of the tensor accumulated into are requested per batch of rows, as above)
        constexpr int NRA = BP / RSTEP, EBA = (EPI == 2 || CAT || DUAL) ? (NRA < 4 ? NRA : 4) : 1;
#pragma unroll 1
        for (int b0 = 0; b0 < NRA; b0 += EBA) {
            bf16x8 arow[EBA];
            if (epi_acc) {
#pragma unroll
                for (int j = 0; j < EBA; ++j) {
                    const int r = erow0 + (b0 + j) * RSTEP;
                    const int rc = p0 + r < p.P ? r : 0;
                    const size_t pp = MODE == 3 ? (size_t)s_orow[rc] : (size_t)(p0 + rc);
                    arow[j] = *reinterpret_cast<const bf16x8*>(p.y + pp * p.Cout + eco);
                }
            }
#pragma unroll
            for (int j = 0; j < EBA; ++j) {
                const int r = erow0 + (b0 + j) * RSTEP;
                if (p0 + r < p.P) {
                    const size_t pp = MODE == 3 ? (size_t)s_orow[r] : (size_t)(p0 + r);
                    bf16x8 v = *reinterpret_cast<const bf16x8*>(smem + r * CROW + ech * 16);
                    f32x8 f = bf8_to_f32(v);
                    if (CAT) {
                        f += load_f32x8(p.epi_add + eco);
                        v = f32_to_bf8(f);
                    }
                    if (epi_acc) {
                        f += bf8_to_f32(arow[j]);
                        v = f32_to_bf8(f);
                    }
                    *reinterpret_cast<bf16x8*>(p.y + pp * p.Cout + eco) = v;
                }
            }
        }
    }
    if (p.stats && !epi_bnz && !RES) {
        // Forward statistics on the (otherwise ~90 % idle) matrix cores instead of the VALU: with F = the staged bf16 tile
        // [32 pixels][16 channels] as an MFMA fragment (hardware transpose read), ones * F gives the per-channel sums and
        // F^T F the Gram matrix whose diagonal is the per-channel sum of squares -- exact products of the STORED values,
        // fp32 accumulation.  The VALU form (convert + add + fma per element) cost 30 % on the HBM-bound 1x1 layers.
        // Rows past P and channels past Cout hold zeros (their operands were zero-filled).
        constexpr int NCB = BC / 64;                       // 16-channel blocks per wave
        const bf16x8 ones = bf16x8_ones();
        const int trow = 8 * lg + (li >> 2);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int ch0 = (wave * NCB + cb) * 16;
            f32x4 dsum = {0.f, 0.f, 0.f, 0.f}, dsq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ps = 0; ps < BP / 32; ++ps) {
                const bf16x8 f = tr_rows(smem + (ps * 32 + trow) * CROW + (ch0 + 4 * (li & 3)) * 2, CROW);
                dsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, f, dsum, 0, 0, 0);
                dsq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, f, dsq, 0, 0, 0);
            }
            // row 0 of dsum is held by lanes 0..15; the diagonal of dsq by lanes with li>>2 == lg
            if (lg == 0) cs[ch0 + li] += dsum[0];
            if ((li >> 2) == lg) cs[BC + ch0 + li] += mfma_diag(dsq, li);
        }
    }
    if (p.stats && (epi_bnz || RES)) {
        // Lanes l, l+CPR, l+2*CPR.. of a wave hold partial sums of the same channel chunk.  They are folded on the VALU
        // with the gfx950 lane-swap instructions (v_permlane32_swap / v_permlane16_swap: "swap the upper half (odd rows)
        // of a with the lower half (even rows) of b", so a' + b' folds TWO values at once and halves the register count
        // per step) -- 24 VALU ops instead of 32-48 ds_bpermute, which had made this epilogue LDS-pipe-bound (-30 % on
        // the HBM-bound 1x1 layers).  16 values -> 4 registers per lane, then 4 LDS adds per lane, into this WAVE's row of the sums (one
        // owner lane per entry: the adds of an entry happen in tile order, whatever the timing of the other waves).
        // (the same sequence as conv3x3_c64.hip's fold16_to_cs, kept as text: behind one function the instances that hold it keep their
        // resources and get other instructions -- profiles/tile_idioms.md)
        auto fold = [&](const f32x8& s1, const f32x8& s2, float* dst) {
            dst += (NSR > 1 ? wave : 0) * 2 * BC;
            float v[16];
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[i] = s1[i]; v[8 + i] = s2[i]; }
            if (CPR == 8) {
#pragma unroll
                for (int i = 0; i < 16; ++i)              // lanes l and l+8 of a 16-lane row: DPP row_ror:8
                    v[i] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[i]), 0x128, 0xf, 0xf, false));
            }
            float u[8], wv[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // (inline asm: with this toolchain the __builtin_amdgcn_permlane32_swap result pair is mis-compiled when both
                // halves feed a float add -- verified on hardware, tools/scratch/fold.hip; s_nop covers the VALU->permlane hazard)
                float a = v[2 * i], b = v[2 * i + 1];
                asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
                u[i] = a + b;                                   // rows 0,1: v[2i]; rows 2,3: v[2i+1]
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = u[2 * j], b = u[2 * j + 1];
                asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
                wv[j] = a + b;                                  // row r holds value 4j + {0,2,1,3}[r]
            }
            const int lrow = lane >> 4;
            const int vsel = ((lrow & 1) << 1) | (lrow >> 1);
            if (eco < p.Cout && (CPR >= 16 || !(lane & 8))) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int id = 4 * j + vsel;              // 0..7: sum of channel id; 8..15: second moment of channel id-8
                    atomicAdd(&dst[(id >> 3) * BC + ech * 8 + (id & 7)], wv[j]);
                }
            }
        };
        static_assert(NSR == 4 || EPI == 0 || FADD, "VALU-folded sums need one row per wave");
        fold(esum, esq, cs);
        if (second) fold(esum, esq2, cs2);
    }
    if constexpr (PF) {
        // P[cout][c] += sum over the tile's 128 pixels of g'[p][cout] * a[p][c]: both operands pixel-major in LDS -> transpose reads.
        // g' tile: rows of CROW bytes (the padded epilogue image, as the MFMA statistics read it); a tile: four swizzled [32][64] images
        // staged raw by LDS-DMA at the start of the tile, BatchNorm + activation applied to the fragment (one channel per lane).
        __syncthreads();                               // every row of g' is back in LDS (and the a tile landed: vmcnt(0) of the last K step)
        const int trow = 8 * lg + (li >> 2), tq = li & 3;
        const int x_lo = tr_swz<64>(trow), x_hi = tr_swz<64>(trow + 4);
        const float plo = p.pf_scale ? act_lo(p.pf_act) : -INFINITY, phi = p.pf_scale ? act_hi(p.pf_act) : INFINITY;
#pragma unroll
        for (int ks = 0; ks < BP / 32; ++ks) {
            bf16x8 fa[4], fb[2];
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = tr_rows(smem + (ks * 32 + trow) * CROW + (wp * 64 + t * 16 + 4 * tq) * 2, CROW);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const char* base = smem + PF_OFF + ks * 32 * 128;
                const int u = (wc * 32 + t * 16) / 4 + tq;
                f32x8 q = bf8_to_f32(tr_swz_frag(base, trow * 128, x_lo, (trow + 4) * 128, x_hi, u));
#pragma unroll
                for (int i = 0; i < 8; ++i) q[i] = clamp_act(fmaf(q[i], pfs[t], pfh[t]), plo, phi);
                fb[t] = f32_to_bf8(q);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) pacc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb[nt], pacc[mt][nt], 0, 0, 0);
        }
    }
    __syncthreads();                                   // staging tile consumed before the next tile's operands land
    }   // tile loop
    if constexpr (PF) {
        // one partial [BC][64] per workgroup (plain stores; summed in a fixed order by wgrad_reduce_kernel): wave (wp, wc) holds rows
        // wp*64 + mt*16 + lg*4 + r (cout within the tile), column wc*32 + nt*16 + li
        float* out = p.pf_ws + (((size_t)blockIdx.y * p.n_ctiles + ctile) * p.pf_nsplit + pgrp) * (BC * PF_C);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(size_t)(wp * 64 + mt * 16 + lg * 4 + r) * PF_C + wc * 32 + nt * 16 + li] = pacc[mt][nt][r];
    }
    if (p.stats) {
        // one publication per workgroup and channel: the wave rows are folded in wave order, the workgroup partial goes to the exact
        // integer bins (common.h)
        __syncthreads();
        const unsigned slot = blockIdx.x & (ADAMML_STAT_SLOTS - 1);
        for (int i = tid; i < 2 * BC; i += NTHREADS) {
            const int c = i < BC ? i : i - BC;                 // i < BC: sum of channel c0 + i; else second moment of channel c0 + i - BC
            if (c0 + c < p.Cout) {
                const size_t e = (i < BC ? 0 : (size_t)p.Cout) + c0 + c;
                float v = cs[i];
#pragma unroll
                for (int w = 1; w < NSR; ++w) v += cs[w * 2 * BC + i];
                stat_publish(p.stats + e, 2 * (size_t)p.Cout, slot, v);
                if (second) {
                    float v2 = cs2[i];
#pragma unroll
                    for (int w = 1; w < NSR; ++w) v2 += cs2[w * 2 * BC + i];
                    stat_publish(p.stats2 + e, 2 * (size_t)p.Cout, slot, v2);
                }
            }
        }
    }
}

}  // namespace

// one parity class (ph, pw) of the data gradient of a stride-2 conv (see conv_dgrad_stride2)
struct DgradClass { int nt; unsigned code; int ph, pw, OHc, OWc; };
// residual form of the BatchNorm-fused data-gradient epilogue (ConvP::res_out ..)
struct ResEpi { const void* res_out; const uint8_t* res_mask; int res_act; const void* bn_z2; const float* bn_vec2; double* stats2; };
// dual-source input of a 1x1 data gradient (ConvP::x2 ..)
struct DualIn { const void* z; const float* aff; void* side; };
// K-concatenated second input, per-group weights, epilogue constant (ConvP::xb ..)
struct CatIn { const void* xb; int C2; size_t gw; const float* epi_add; };
// product with a second tensor accumulated from the gradient tile (ConvP::pf_a ..); ws: partial workspace, nsplit: out
struct PfIn { const void* a; const float* scale; const float* shift; int act, gs, C; float* out; void* ws; size_t ws_bytes; };
// forward BatchNorm + residual-add epilogue (ConvP::id_scale ..)
struct FaddEpi { const float* vec; const void* idn; const float* id_scale; const float* id_shift; int id_gstride; int act; uint8_t* mask_out;
                 int tp_frames; void* tp_y; uint16_t* tp_code; };      // tp_frames > 0: temporal max-pool in the epilogue (ConvP::tp_y ..)

// ---- the instances of conv_gemm_kernel, one launcher per family.  The kernel's positional template list
//   <BC, MODE, PD, RES, DUAL, CAT, FADD, GLDS, EID, LZF, EPI, PF, TP>
// is written out HERE and nowhere else; a launcher's own parameters are the ones that vary inside its family, under the kernel's names.
struct ConvGrid { dim3 grid; hipStream_t stream; };

template <int BC, int MODE, bool GLDS, int EPI>         // plain conv, one K step of look-ahead, the epilogue compiled in
static void launch_plain(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, MODE, 1, false, false, false, false, GLDS, 0, false, EPI>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC, int MODE, int PD>                     // plain conv, epilogue selected at run time: deep prefetch (PD 3) and the MODE 2 loaders
static void launch_rt_epi(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, MODE, PD>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC, bool GLDS, int EID, bool LZF>         // FADD: conv + BatchNorm + residual add + activation
static void launch_fadd(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, 0, 1, false, false, false, true, GLDS, EID, LZF>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <bool LZF, int TP>                             // FADD with the temporal max-pool of TP frames in the epilogue
static void launch_fadd_tp(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<128, 0, 1, false, false, false, true, true, 1, LZF, -1, false, TP>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC, int EID>                              // RES: residual form of the BatchNorm-fused data-gradient epilogue
static void launch_res(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, 0, 1, true, false, false, false, true, EID>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC>                                       // RES behind the KxK (MODE 1) LDS-DMA loaders: 3x3 / stride-1 data gradients
static void launch_res_kxk(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, 1, 1, true, false, false, false, true, 0>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
static void launch_res_prod(const ConvGrid& g, const ConvP& p) {      // RES + EID with the product of the gradient tile (PF)
    hipLaunchKernelGGL((conv_gemm_kernel<128, 0, 1, true, false, false, false, true, 1, false, -1, true>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC>                                       // CAT: K-concatenated second input (algebraic BatchNorm backward)
static void launch_cat(const ConvGrid& g, const ConvP& p) {
    hipLaunchKernelGGL((conv_gemm_kernel<BC, 0, 3, false, false, true>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}
template <int BC>                                       // DUAL: BatchNorm-backward affine of two tensors in the loader
static void launch_dual(const ConvGrid& g, const ConvP& p) {
    constexpr int PD = BC == 64 ? 3 : 2;                // (a third ring slot of g, z and weights does not fit 256 registers at 128-wide tiles)
    hipLaunchKernelGGL((conv_gemm_kernel<BC, 0, PD, false, true>), g.grid, dim3(NTHREADS), 0, g.stream, p);
}

// ---- run-time value -> template argument, each choice written once: f receives the value as a std::integral_constant
template <int V> using int_c = std::integral_constant<int, V>;
template <class F> static void with_bc(int BC, F f) { if (BC == 64) f(int_c<64>{}); else f(int_c<128>{}); }
template <class F> static void with_epi(int epi, F f) { if (epi == 0) f(int_c<0>{}); else if (epi == 1) f(int_c<1>{}); else f(int_c<2>{}); }
template <class F> static void with_tp(int tp, F f) { if (tp == 8) f(int_c<8>{}); else if (tp == 4) f(int_c<4>{}); else f(int_c<2>{}); }
template <class F> static void with_flag(bool b, F f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// the plain instances of one (BC, MODE): LDS-DMA staging or the register-staged loader with the epilogue compiled in, deep prefetch (MODE
// 0) or the strided loader (MODE 2) with the run-time epilogue.  `lazy` = the input has a lazy transform (register-staged loader); the
// caller has refused a lazy GRADIENT operand (cls or bn_z), so MODE 3 and the bn_z epilogue (EPI 1) exist behind LDS-DMA only, and `deep`
// is never set for MODE 1
template <int BC, int MODE>
static void launch_conv(bool lazy, bool deep, int epi, const ConvGrid& g, const ConvP& p) {
    if constexpr (MODE == 2) {
        if (deep) launch_rt_epi<BC, 2, 3>(g, p); else launch_rt_epi<BC, 2, 1>(g, p);
    } else if constexpr (MODE == 3) {
        with_epi(epi, [&](auto e) { launch_plain<BC, 3, true, e()>(g, p); });
    } else {
        if (!lazy) return with_epi(epi, [&](auto e) { launch_plain<BC, MODE, true, e()>(g, p); });
        if constexpr (MODE == 0)
            if (deep) return launch_rt_epi<BC, 0, 3>(g, p);
        if (epi == 0) launch_plain<BC, MODE, false, 0>(g, p); else launch_plain<BC, MODE, false, 2>(g, p);
    }
}

static int conv_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                       const float* in_shift, void* y, double* stats, const void* bn_z, const float* bn_vec, int bn_act,
                       hipStream_t stream, const DgradClass* cls = nullptr, const ResEpi* res = nullptr, const DualIn* dual = nullptr,
                       const CatIn* cat = nullptr, const FaddEpi* fadd = nullptr, const PfIn* pf = nullptr) {
    if (!d || !x || !w_packed || !y) return adamml_set_error(ADAMML_EINVAL, "conv_fwd: null argument");
    if (d->Cin % 8 || d->Cout % 8) return adamml_set_error(ADAMML_EINVAL, "conv_fwd: channels must be multiples of 8 (Cin=%d Cout=%d)", d->Cin, d->Cout);
    if (!cls && !fadd && !res && adamml_conv3x3_c64_supported(d))       // (the residual form of the 64-channel kernel: adamml_conv_bwd_data_res)
        return adamml_conv3x3_c64_launch(d, x, w_packed, in_scale, in_shift, y, stats, bn_z, bn_vec, bn_act, stream);
    // narrow 1x1 convs of the MobileNetV2s (plain forward / plain data gradient): the barrier-free streaming kernel (conv1x1_narrow.hip)
    if (!cls && !fadd && !res && !dual && !cat && !pf && !bn_z && adamml_conv1x1_narrow_fwd_supported(d))
        return adamml_conv1x1_narrow_fwd_launch(d, x, w_packed, in_scale, in_shift, y, stats, stream);
    // expanding 1x1 convs of ResNet layers 3-4 (K = 256 / 512 -> >= 2 K channels; plain forward, stride-2 downsample forward, plain or
    // accumulating data gradient): activation-stationary streaming kernel (conv1x1_wide.hip; it has no accumulating form of a lazy input:
    // that call stays with conv_gemm_kernel)
    if (!cls && !fadd && !res && !dual && !cat && !pf && !bn_z && !(d->accumulate && in_scale) && adamml_conv1x1_wide_expand_supported(d))
        return adamml_conv1x1_wide_expand_launch(d, x, w_packed, in_scale, in_shift, y, stats, stream);
    // ... their data gradients with the BatchNorm-fused epilogue (bn_z) or accumulating into the output
    if (!cls && !fadd && !res && !dual && !cat && !pf && !in_scale && (bn_z ? stats != nullptr && !d->accumulate : d->accumulate != 0) &&
        adamml_conv1x1_narrow_dgrad_epi_supported(d))
        return adamml_conv1x1_narrow_dgrad_epi_launch(d, x, w_packed, y, bn_z, bn_vec, bn_act, stats, stream);
    ConvP p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w_packed; p.in_scale = in_scale; p.in_shift = in_shift;
    p.y = (bf16_t*)y; p.stats = stats;
    p.bn_z = (const bf16_t*)bn_z; p.bn_vec = bn_vec; p.bn_act = bn_act;
    p.res_out = res ? (const bf16_t*)res->res_out : nullptr; p.res_act = res ? res->res_act : 0;
    p.res_mask = res ? res->res_mask : nullptr;
    p.bn_z2 = res ? (const bf16_t*)res->bn_z2 : nullptr; p.bn_vec2 = res ? res->bn_vec2 : nullptr; p.stats2 = res ? res->stats2 : nullptr;
    p.x2 = dual ? (const bf16_t*)dual->z : nullptr; p.aff = dual ? dual->aff : nullptr; p.side = dual ? (bf16_t*)dual->side : nullptr;
    p.xb = cat ? (const bf16_t*)cat->xb : nullptr; p.K1 = d->Cin; p.C2 = cat ? cat->C2 : 0; p.gw = cat ? cat->gw : 0;
    p.epi_add = cat ? cat->epi_add : nullptr;
    p.id_scale = fadd ? fadd->id_scale : nullptr; p.id_shift = fadd ? fadd->id_shift : nullptr; p.id_gstride = fadd ? fadd->id_gstride : 0;
    p.mask_out = fadd ? fadd->mask_out : nullptr;
    p.tp_nblk = p.tp_Q = 0; p.tp_y = nullptr; p.tp_code = nullptr;
    p.pf_a = nullptr; p.pf_scale = p.pf_shift = nullptr; p.pf_ws = nullptr; p.pf_act = p.pf_gs = p.pf_nsplit = 0;
    if (fadd) { p.bn_vec = fadd->vec; p.res_out = (const bf16_t*)fadd->idn; p.res_act = fadd->act; }
    const int groups = d->groups < 1 ? 1 : d->groups;
    p.gx = (size_t)d->N * d->H * d->W * d->Cin;
    p.gy = (size_t)d->N * d->OH * d->OW * d->Cout;
    p.in_gstride = d->in_gstride;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad; p.up = d->up < 1 ? 1 : d->up;
    p.up_shift = ilog2_exact(p.up);
    if (p.up_shift < 0) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd: up=%d is not a power of two", p.up);
    p.act = d->act; p.accumulate = d->accumulate;
    p.P = d->N * d->OH * d->OW; p.K = d->KH * d->KW * d->Cin;
    if (cat) {
        if (d->KH * d->KW != 1 || d->stride != 1 || (d->up > 1) || d->Cin % BK || cat->C2 % 8 || cls || res || dual)
            return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_alg: 1x1 / stride-1 convs with Cout %% 32 == 0 only");
        p.K = d->Cin + cat->C2;
    }
    p.wK = p.K;
    p.cls_nt = 0; p.cls_code = 0; p.oH = d->OH; p.oW = d->OW; p.o_ph = p.o_pw = 0;
    if (cls) {
        p.cls_nt = cls->nt; p.cls_code = cls->code; p.o_ph = cls->ph; p.o_pw = cls->pw;
        p.OH = cls->OHc; p.OW = cls->OWc;
        p.P = d->N * cls->OHc * cls->OWc;
        p.K = cls->nt * d->Cin;
    }
    const bool multitap = d->KH * d->KW > 1 || cls;
    p.cin_shift = 0;
    if (multitap) {
        p.cin_shift = ilog2_exact(d->Cin);
        if (p.cin_shift < 0) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd: KxK conv needs power-of-two Cin (got %d)", d->Cin);
    }
    if (p.P <= 0) return ADAMML_OK;
    bool narrow = d->Cout <= 64 || (d->Cout % 128 != 0 && d->Cout < 256);
    // small problems: halve the cout tile so that at least ~2 workgroups per CU exist
    if (!narrow && (long)ceil_div(p.P, BP) * ceil_div(d->Cout, 128) * groups < 512) narrow = true;
    const int tp = fadd ? fadd->tp_frames : 0;
    if (tp) narrow = false;
    const int BC = narrow ? 64 : 128;
    p.n_ptiles = ceil_div(p.P, BP);
    if (tp) {
        // tiles = (clip, block of BP / tp pixels); all frames of a clip's pixel block sit in one tile
        p.tp_Q = d->OH * d->OW;
        p.tp_nblk = ceil_div(p.tp_Q, BP / tp);
        p.n_ptiles = (d->N / tp) * p.tp_nblk;
        p.tp_y = (bf16_t*)fadd->tp_y; p.tp_code = fadd->tp_code;
    }
    p.n_ctiles = ceil_div(d->Cout, BC);
    // consecutive pixel tiles per workgroup (amortises the statistics publication), keeping >= ~2048 workgroups
    p.tpb = (int)((long)p.n_ptiles * p.n_ctiles * groups / 2048);
    if (p.tpb < 1) p.tpb = 1;
    if (p.tpb > 8) p.tpb = 8;
    if (pf) {
        // one [BC][64] partial per workgroup: few, long-lived workgroups (~6 per CU slot pair over all groups and cout tiles)
        const long target = 1536;
        long nsp = target / ((long)p.n_ctiles * groups);
        if (nsp < 1) nsp = 1;
        p.tpb = (int)ceil_div(p.n_ptiles, (int)nsp);
        if (p.tpb < 1) p.tpb = 1;
    }
    const dim3 grid(ceil_div(p.n_ptiles, p.tpb) * p.n_ctiles, groups);
    const ConvGrid cg{grid, stream};
    const int taps = d->KH * d->KW;
    // MODE 0 needs the whole row base in 32-bit element offsets (true for every layer of the hot path)
    if ((long)d->N * d->H * d->W * d->Cin >= (1L << 31)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd: input tensor exceeds 2^31 elements");
    const int mode = cls ? 3 : (p.up > 1 ? 2 : (multitap ? (taps <= 64 ? 1 : 2) : 0));
    if (mode == 2 && !multitap) { p.cin_shift = 30; }      // 1x1 strided dgrad: tap = k >> 30 = 0, ci = k
    const int nk = ceil_div(p.K, BK);
    // < 1 wave of workgroups per CU slot and a long K loop: explicit look-ahead instead of occupancy.  Measured (tools/bench_conv.py,
    // B = 72): it pays for the 1x1 layers of layer 4 (0.115 vs 0.137 ms) and costs on its 3x3 layers (0.189 vs 0.139 ms forward,
    // 0.197 vs 0.146 ms data gradient: the tap gathers of MODE 1 hit L2 and the deeper ring only lowers the occupancy)
    const bool deep = (long)grid.x * grid.y <= 768 && nk >= 8 && mode != 1;
    if (fadd) {
        if (mode != 0 || res || dual || cat || stats) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd_bn_add: only 1x1 / stride-1 convs");
        if (!in_scale || p.K <= 512) {
            // operands by LDS-DMA (a lazily normalised input is transformed at the fragment: LZF); with an identity operand, that one is
            // requested at the start of each tile (EID)
            const bool eid = p.res_out != nullptr;
            if (tp) {
                with_flag(in_scale != nullptr, [&](auto lzf) { with_tp(tp, [&](auto tv) { launch_fadd_tp<lzf(), tv()>(cg, p); }); });
                return adamml_check_launch("conv_fwd_bn_add_tpool");
            }
            with_bc(BC, [&](auto bc) {
                with_flag(in_scale != nullptr, [&](auto lzf) {
                    if (eid) launch_fadd<bc(), true, 1, lzf()>(cg, p); else launch_fadd<bc(), true, 0, lzf()>(cg, p);
                });
            });
        } else
        if (tp) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd_bn_add_tpool: needs the LDS-DMA kernel (K <= 512 for a lazy input)");
        else with_bc(BC, [&](auto bc) { launch_fadd<bc(), false, 0, false>(cg, p); });
        return adamml_check_launch("conv_fwd_bn_add");
    }
    if (res) {
        // MODE 1 (3x3 / pad 1 / stride 1, dense dz): the epilogue only needs tile row r to be output pixel p0 + r, as in MODE 0
        if (mode != 0 && !(mode == 1 && !pf && p.up == 1 && p.stride == 1))
            return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_res: only 1x1 / stride-1 and 3x3 / pad-1 / stride-1 convs");
        if (pf) {
            if (BC != 128 || d->Cout % 128 || pf->C != 64 || in_scale || !p.res_mask || !p.accumulate || p.bn_z || p.bn_z2 || !stats)
                return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_res_prod: needs Cout %% 128 == 0, a 64-channel product operand, "
                                                             "the accumulate + 1-bit-mask + sum(g')-only form");
            p.pf_nsplit = ceil_div(p.n_ptiles, p.tpb);
            const size_t need = (size_t)groups * p.n_ctiles * p.pf_nsplit * 128 * 64 * sizeof(float);
            if (!pf->ws || pf->ws_bytes < need) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_res_prod: workspace too small (need %zu bytes)", need);
            p.pf_a = (const bf16_t*)pf->a; p.pf_scale = pf->scale; p.pf_shift = pf->scale ? pf->shift : nullptr; p.pf_act = pf->act; p.pf_gs = pf->gs;
            p.pf_ws = (float*)pf->ws;
            launch_res_prod(cg, p);
            int rc = adamml_check_launch("conv_bwd_data_res_prod");
            if (rc) return rc;
            // P[g][ctile * 128 + r][c] = sum over the workgroups of (g, ctile), in workgroup order
            launch_wgrad_reduce((const float*)pf->ws, pf->out, (size_t)128 * 64, p.pf_nsplit, 1, 64, 1, groups * p.n_ctiles, stream);
            return adamml_check_launch("conv_bwd_data_res_prod (reduce)");
        }
        if (in_scale) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_res: the gradient operand is never lazy");
        if (mode == 1) {
            with_bc(BC, [&](auto bc) { launch_res_kxk<bc()>(cg, p); });
            return adamml_check_launch("conv_bwd_data_res (3x3)");
        }
        // the algebraic backward's form (identity gradient + 1-bit mask, sum(g') only): identity-side loads at the start of each tile (EID)
        const bool eid = p.res_mask && p.accumulate && !p.bn_z && !p.bn_z2;
        with_bc(BC, [&](auto bc) { if (eid) launch_res<bc(), 1>(cg, p); else launch_res<bc(), 0>(cg, p); });
        return adamml_check_launch("conv_bwd_data_res");
    }
    if (cat) {
        if (mode != 0) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_alg: only 1x1 / stride-1 convs");
        with_bc(BC, [&](auto bc) { launch_cat<bc()>(cg, p); });
        return adamml_check_launch("conv_bwd_data_alg");
    }
    if (dual) {
        if (mode != 0 || res) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_dual: only 1x1 / stride-1 convs");
        with_bc(BC, [&](auto bc) { launch_dual<bc()>(cg, p); });
        return adamml_check_launch("conv_bwd_data_dual");
    }
    // (the fragment-side lazy transform, LZF, is NOT used for the plain forward convs: measured 5-10 % slower than the register-staged
    // loader -- layer-1 conv3 1.77 vs 1.61 ms, layer 2 0.59 vs 0.54, layer 3 0.23 vs 0.21: each pixel half is transformed by two waves,
    // between the ds_read and the MFMA; it only pays together with the early identity loads of the FADD kernel)
    // operands without a lazy transform are staged by LDS-DMA (MODE 0 / 1 / 3)
    const bool lazy = in_scale != nullptr;
    // the epilogue is a template parameter (EPI) of the LDS-DMA and one-step instances; deep-prefetch and MODE 2 keep the run-time form
    const int epi = bn_z ? 1 : (p.accumulate ? 2 : 0);
    // a gradient operand (a parity class, or the input of the BatchNorm-fused epilogue) is plain in memory -- every caller passes it so -- and
    // the register-staged loaders are not compiled for MODE 3 or with EPI 1
    if (lazy && (mode == 3 || (mode != 2 && epi == 1)))
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data: the gradient operand is never lazy");
    with_bc(BC, [&](auto bc) {
        if (mode == 0) launch_conv<bc(), 0>(lazy, deep, epi, cg, p);
        else if (mode == 1) launch_conv<bc(), 1>(lazy, deep, epi, cg, p);
        else if (mode == 2) launch_conv<bc(), 2>(lazy, deep, epi, cg, p);
        else launch_conv<bc(), 3>(lazy, deep, epi, cg, p);
    });
    return adamml_check_launch("conv_fwd");
}

// The descriptor conv_launch dispatches on for the data gradient of the forward conv d: a stride-1 conv of dz (pixels and channels of d's
// output) into dx (those of d's input) with the flipped / transposed weight pack.  `upsampled`: dz is read zero-upsampled by d's stride and
// padded for the flipped taps (the generic form of any conv); otherwise dense -- 1x1 / stride-1 convs and the parity classes of
// conv_dgrad_stride2.  The gradient operand is never lazily normalised (act / in_gstride are cleared).
static adamml_conv_desc_t dgrad_desc(const adamml_conv_desc_t* d, int accumulate, bool upsampled = false) {
    adamml_conv_desc_t g = *d;
    g.H = d->OH; g.W = d->OW; g.Cin = d->Cout;
    g.OH = d->H; g.OW = d->W; g.Cout = d->Cin;
    g.stride = 1; g.up = upsampled ? d->stride : 1; g.pad = upsampled ? d->KH - 1 - d->pad : 0;
    g.act = ACT_NONE; g.accumulate = accumulate != 0; g.in_gstride = 0;
    return g;
}

extern "C" int adamml_conv1x1_narrow_supported(const adamml_conv_desc_t* d, int kind) {
    if (!d) return 0;
    if (kind == 0) return adamml_conv1x1_narrow_fwd_supported(d) ? 1 : 0;
    if (kind == 1) return adamml_conv1x1_narrow_wgrad_supported(d, d->Cin) ? 1 : 0;
    if (kind == 2) return adamml_conv1x1_narrow_dual_supported(d) ? 1 : 0;
    if (d->stride != 1 || d->pad != 0 || d->up > 1) return 0;    // (the streaming kernels take dense 1x1 launches only)
    const adamml_conv_desc_t g = dgrad_desc(d, 0);
    if (kind == 3) return adamml_conv1x1_narrow_fwd_supported(&g) ? 1 : 0;
    if (kind == 4) return adamml_conv1x1_narrow_dgrad_epi_supported(&g) ? 1 : 0;
    return 0;
}

extern "C" int adamml_conv1x1_wide_supported(const adamml_conv_desc_t* d, int kind) {
    if (!d) return 0;
    if (kind == 0) { adamml_conv_desc_t f = *d; f.accumulate = 0; return adamml_conv1x1_wide_expand_supported(&f) ? 1 : 0; }
    if (kind != 3 && kind != 4) return 0;
    if (d->stride != 1) return 0;                                // (strided data gradients run by parity class: conv_dgrad_stride2)
    const adamml_conv_desc_t g = dgrad_desc(d, kind == 4);
    return adamml_conv1x1_wide_expand_supported(&g) ? 1 : 0;
}

extern "C" int adamml_conv_fused_input_supported(const adamml_conv_desc_t* d) {
    return d && adamml_conv3x3_c64_supported(d) ? 1 : 0;
}

extern "C" int adamml_conv_fwd(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                               const float* in_shift, void* y, double* stats, hipStream_t stream) {
    return conv_launch(d, x, w_packed, in_scale, in_shift, y, stats, nullptr, nullptr, 0, stream);
}

extern "C" int adamml_conv_fwd_bn_add_supported(const adamml_conv_desc_t* d) {
    return d && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && (d->up <= 1) && d->Cin % 8 == 0 && d->Cout % 8 == 0 ? 1 : 0;
}

extern "C" int adamml_conv_fwd_bn_add_streams(const adamml_conv_desc_t* d) {
    return d && adamml_conv_fwd_bn_add_supported(d) && adamml_conv1x1_fadd_stream_supported(d) ? 1 : 0;
}

extern "C" int adamml_conv_fwd_bn_add(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                                      const float* in_shift, const float* bn_vec, const void* idn, const float* id_scale,
                                      const float* id_shift, int id_gstride, int act, void* out, uint8_t* mask_out, hipStream_t stream) {
    if (!adamml_conv_fwd_bn_add_supported(d)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd_bn_add: 1x1 / stride-1 convs only");
    if (!bn_vec) return adamml_set_error(ADAMML_EINVAL, "conv_fwd_bn_add: null BatchNorm vectors");
    if (idn && adamml_conv1x1_fadd_stream_supported(d))
        return adamml_conv1x1_fadd_stream_launch(d, x, w_packed, in_scale, in_shift, bn_vec, idn, id_scale, id_shift, id_gstride, act, out, mask_out, stream);
    FaddEpi f{bn_vec, idn, id_scale, id_shift, id_gstride, act, mask_out, 0, nullptr, nullptr};
    return conv_launch(d, x, w_packed, in_scale, in_shift, out, nullptr, nullptr, nullptr, 0, stream, nullptr, nullptr, nullptr, nullptr, &f);
}

extern "C" int adamml_conv_fwd_bn_add_next_supported(const adamml_conv_desc_t* d, int next_cout) {
    return d && next_cout > 0 && adamml_conv_fwd_bn_add_supported(d) && adamml_conv1x1_fadd_next_supported(d, next_cout) ? 1 : 0;
}

extern "C" int adamml_conv_fwd_bn_add_next(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                                           const float* in_shift, const float* bn_vec, const void* idn, const float* id_scale,
                                           const float* id_shift, int id_gstride, int act, void* out, uint8_t* mask_out, const void* w_next,
                                           void* y_next, double* stats_next, hipStream_t stream) {
    if (!d || !x || !w_packed || !bn_vec || !out || !w_next || !y_next) return adamml_set_error(ADAMML_EINVAL, "conv_fwd_bn_add_next: null argument");
    if (!adamml_conv_fwd_bn_add_next_supported(d, 64))
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd_bn_add_next: 1x1 / stride-1, 64 -> 256 channels, next conv 256 -> 64 only");
    return adamml_conv1x1_fadd_next_launch(d, x, w_packed, in_scale, in_shift, bn_vec, idn, id_scale, id_shift, id_gstride, act, out, mask_out,
                                           w_next, y_next, stats_next, stream);
}

extern "C" int adamml_conv_fwd_bn_add_tpool_supported(const adamml_conv_desc_t* d, int frames, int act, int lazy_input) {
    if (!adamml_conv_fwd_bn_add_supported(d)) return 0;
    if (!(frames == 2 || frames == 4 || frames == 8) || d->N % frames || d->Cout % 128 || act != ADAMML_ACT_RELU) return 0;
    if (lazy_input && d->Cin > 512) return 0;                         // (the fragment-side lazy transform keeps its vectors in LDS)
    return 1;
}

// which kernel serves adamml_conv_fwd_bn_add_tpool (a label for profilers): 0 = the tile kernel's TP instance, 1 = the round-5 streaming kernel
// (csrc/conv1x1_fadd_next.hip: a wave owns all 256 channels of 16 pixels), 2 = the wave-slice streaming kernel (csrc/conv1x1_fadd_stream.hip)
extern "C" int adamml_conv_fwd_bn_add_tpool_streams(const adamml_conv_desc_t* d, int frames) {
    if (!d) return 0;
    if (adamml_conv1x1_fadd_tpool_stream_supported(d, frames)) return 2;
    return adamml_conv1x1_fadd_tpool_supported(d, frames) ? 1 : 0;
}

extern "C" int adamml_conv_fwd_bn_add_tpool(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale,
                                            const float* in_shift, const float* bn_vec, const void* idn, const float* id_scale,
                                            const float* id_shift, int id_gstride, int act, int frames, void* pooled, uint16_t* code,
                                            hipStream_t stream) {
    if (!adamml_conv_fwd_bn_add_tpool_supported(d, frames, act, in_scale != nullptr))
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd_bn_add_tpool: 1x1 / stride-1 conv, Cout %% 128 == 0, ReLU, 2 / 4 / 8 frames per clip");
    if (!bn_vec || !idn || !pooled) return adamml_set_error(ADAMML_EINVAL, "conv_fwd_bn_add_tpool: null argument");
    if (adamml_conv1x1_fadd_tpool_stream_supported(d, frames))        // (csrc/conv1x1_fadd_stream.hip: the wave-slice streaming structure)
        return adamml_conv1x1_fadd_tpool_stream_launch(d, x, w_packed, in_scale, in_shift, bn_vec, idn, id_scale, id_shift, id_gstride, act, frames, pooled,
                                                       code, stream);
    if (adamml_conv1x1_fadd_tpool_supported(d, frames))
        return adamml_conv1x1_fadd_tpool_launch(d, x, w_packed, in_scale, in_shift, bn_vec, idn, id_scale, id_shift, id_gstride, act, frames, pooled, code,
                                                stream);
    FaddEpi f{bn_vec, idn, id_scale, id_shift, id_gstride, act, nullptr, frames, pooled, code};
    // (`pooled` doubles as the kernel's y pointer: the full-rate output is never written)
    return conv_launch(d, x, w_packed, in_scale, in_shift, pooled, nullptr, nullptr, nullptr, 0, stream, nullptr, nullptr, nullptr, nullptr, &f);
}

// Data gradient of a stride-2 conv (3x3 pad 1 / 1x1 pad 0: every strided conv of the hot path) WITHOUT the 4x wasted work
// of a zero-upsampled stride-1 conv: the dx pixels split into 4 parity classes (ih % 2, iw % 2); class (ph, pw) only
// receives the taps with kh == ph + pad (mod 2), kw likewise -- 1, 2, 2 and 4 of the 9 taps of a 3x3, 1/0/0/0 of a 1x1 --
// and is a dense stride-1 conv of dz with that tap subset whose output rows are scattered with stride 2.  A class
// without taps is zero-filled (or skipped when accumulating).
static int conv_dgrad_stride2(const adamml_conv_desc_t* d, const void* dz, const void* w, void* dx, int accumulate, double* sums,
                              const void* z_in, const float* bn_vec, int act, hipStream_t stream) {
    const adamml_conv_desc_t g = dgrad_desc(d, accumulate);
    const int taps = d->KH * d->KW;
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            DgradClass c;
            c.nt = 0; c.code = 0; c.ph = ph; c.pw = pw;
            c.OHc = (d->H - ph + 1) / 2; c.OWc = (d->W - pw + 1) / 2;
            if (c.OHc <= 0 || c.OWc <= 0) continue;
            for (int kh = 0; kh < d->KH; ++kh) {
                if ((ph + d->pad - kh) & 1) continue;
                const int dh = (ph + d->pad - kh) / 2;           // dz row = i + dh, in {0, 1} for the supported shapes
                for (int kw = 0; kw < d->KW; ++kw) {
                    if ((pw + d->pad - kw) & 1) continue;
                    const int dw = (pw + d->pad - kw) / 2;
                    const unsigned wt = (unsigned)(taps - 1 - (kh * d->KW + kw));     // tap index in the flipped weight pack
                    c.code |= ((unsigned)dh | ((unsigned)dw << 1) | (wt << 2)) << (8 * c.nt);
                    ++c.nt;
                }
            }
            if (c.nt == 0 && accumulate) continue;
            int rc = conv_launch(&g, dz, w, nullptr, nullptr, dx, sums, z_in, bn_vec, act, stream, &c);
            if (rc) return rc;
        }
    return ADAMML_OK;
}

static bool dgrad_stride2_ok(const adamml_conv_desc_t* d) {
    const bool k3 = d->KH == 3 && d->KW == 3 && d->pad == 1, k1 = d->KH == 1 && d->KW == 1 && d->pad == 0;
    return d->stride == 2 && (k3 || k1) && (d->up <= 1) && ilog2_exact(d->Cout) >= 0 &&
           d->OH == (d->H + 2 * d->pad - d->KH) / 2 + 1 && d->OW == (d->W + 2 * d->pad - d->KW) / 2 + 1;
}

extern "C" int adamml_conv_bwd_data_bn(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx,
                                       const void* z_in, const float* bn_vec, int act, double* sums, hipStream_t stream) {
    if (!d || !z_in || !bn_vec || !sums) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_bn: null argument");
    if (dgrad_stride2_ok(d)) return conv_dgrad_stride2(d, dz, w_dgrad_packed, dx, 0, sums, z_in, bn_vec, act, stream);
    const adamml_conv_desc_t g = dgrad_desc(d, 0, true);
    return conv_launch(&g, dz, w_dgrad_packed, nullptr, nullptr, dx, sums, z_in, bn_vec, act, stream);
}

// Measured on MI355X (tools/bench_fused.py, B = 72): against apply + data gradient the dual loader wins for K = Cout <= 512
// (layer 1: 3.8 vs 4.2 ms, layer 2: 1.01 vs 1.05 ms) and loses beyond (layer 3: 0.33 vs 0.30 ms; layer 4: every one of
// the 4 cout tiles repeats the affine and the vectors no longer fit the LDS table).
extern "C" int adamml_conv_bwd_data_dual_supported(const adamml_conv_desc_t* d) {
    return d && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->Cout <= 512 && d->Cin % 8 == 0 && d->Cout % 8 == 0 ? 1 : 0;
}

extern "C" int adamml_conv_bwd_data_dual(const adamml_conv_desc_t* d, const void* g, const void* z, const float* aff, void* dz_side,
                                         const void* w_dgrad_packed, void* dx, int accumulate, const void* z_in, const float* bn_vec,
                                         int act, double* sums, hipStream_t stream) {
    if (!d || !g || !z || !aff) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_dual: null argument");
    if (!adamml_conv_bwd_data_dual_supported(d))
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_dual: only 1x1 / stride-1 convs with Cout <= 512");
    if ((z_in != nullptr) != (bn_vec != nullptr) || (z_in != nullptr) != (sums != nullptr))
        return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_dual: incomplete BatchNorm epilogue operands");
    if (z_in && accumulate) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_dual: the BatchNorm epilogue does not accumulate");
    if (adamml_conv1x1_narrow_dual_supported(d))             // projection convs of the MobileNetV2s: barrier-free streaming kernel (conv1x1_narrow.hip)
        return adamml_conv1x1_narrow_dual_launch(d, g, z, aff, dz_side, w_dgrad_packed, dx, accumulate, z_in, bn_vec, act, sums, stream);
    const adamml_conv_desc_t gd = dgrad_desc(d, accumulate);
    DualIn di{z, aff, dz_side};
    return conv_launch(&gd, g, w_dgrad_packed, nullptr, nullptr, dx, sums, z_in, bn_vec, act, stream, nullptr, nullptr, &di);
}

extern "C" int adamml_conv_bwd_data_alg_streams(const adamml_conv_desc_t* d) {
    return d && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && adamml_alg_stream_supported(d->Cout, d->Cin) ? 1 : 0;
}

extern "C" int adamml_conv_bwd_data_alg(const adamml_conv_desc_t* d, const void* g, const void* a, const float* a_scale, const float* a_shift,
                                        const void* w_alg, const float* epi_add, void* dx, int accumulate, const void* z_in,
                                        const float* bn_vec, int act, double* sums, hipStream_t stream) {
    // d describes the FORWARD conv (1x1, stride 1); d->act / d->in_gstride describe the lazy transform of its input a
    if (!d || !g || !a || !w_alg || !epi_add || !dx) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_alg: null argument");
    if (!(d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_alg: only 1x1 / stride-1 convs");
    if ((z_in != nullptr) != (bn_vec != nullptr) || (z_in != nullptr) != (sums != nullptr))
        return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_alg: incomplete BatchNorm epilogue operands");
    if (z_in && accumulate) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_alg: the BatchNorm epilogue does not accumulate");
    if (adamml_alg_stream_supported(d->Cout, d->Cin))
        return adamml_alg_stream_launch(d, g, a, a_scale, a_shift, w_alg, epi_add, dx, accumulate, z_in, bn_vec, act, sums, stream);
    adamml_conv_desc_t gd = dgrad_desc(d, accumulate);
    gd.act = d->act; gd.in_gstride = d->in_gstride;          // the lazy transform of the concatenated operand a (the loader applies it to a only)
    CatIn c{a, d->Cin, (size_t)d->Cin * (d->Cout + d->Cin), epi_add};
    return conv_launch(&gd, g, w_alg, a_scale, a_shift, dx, sums, z_in, bn_vec, act, stream, nullptr, nullptr, nullptr, &c);
}

static bool res_1x1(const adamml_conv_desc_t* d) {
    return d && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->Cin % 8 == 0 && d->Cout % 8 == 0;
}

// 3x3 / pad 1 / stride 1 with as many output as input channels (conv1 of a BasicBlock without a downsample branch): the tile kernel's
// KxK loaders need a power-of-two channel count
static bool res_3x3(const adamml_conv_desc_t* d) {
    return d && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->up <= 1 && d->Cin == d->Cout && d->Cin >= 64 &&
           ilog2_exact(d->Cin) >= 0 && d->OH == d->H && d->OW == d->W;
}

extern "C" int adamml_conv_bwd_data_res_supported(const adamml_conv_desc_t* d) {
    return res_1x1(d) || res_3x3(d) ? 1 : 0;
}

// 64 channels (layer 1 of the BasicBlock nets): the resident-weight kernel of conv3x3_c64.hip, which has no second BatchNorm operand
static bool res_3x3_c64(const adamml_conv_desc_t* d) {
    if (!res_3x3(d)) return false;
    const adamml_conv_desc_t g = dgrad_desc(d, 0, true);
    return adamml_conv3x3_c64_res_supported(&g);
}

extern "C" int adamml_conv_bwd_data_res_streams(const adamml_conv_desc_t* d) {
    if (res_3x3_c64(d)) return 2;
    return res_1x1(d) && adamml_res_stream_supported(d) ? 1 : 0;
}

extern "C" int adamml_conv_bwd_data_res(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx,
                                        int accumulate, const void* res_out, const uint8_t* res_mask, int res_act, const void* z_a, const float* vec_a,
                                        double* sums_a, const void* z_b, const float* vec_b, double* sums_b,
                                        hipStream_t stream) {
    if (!d || !res_out || !sums_a || (z_a && !vec_a)) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_res: null argument");
    if ((z_b != nullptr) != (vec_b != nullptr) || (z_b != nullptr) != (sums_b != nullptr))
        return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_res: incomplete second BatchNorm operand");
    if (!adamml_conv_bwd_data_res_supported(d))
        return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_res: only 1x1 / stride-1 convs and 3x3 / pad-1 / stride-1 convs with Cin == Cout (a power of two >= 64)");
    if (accumulate && res_mask && !z_a && res_1x1(d) && adamml_res_stream_supported(d))       // (the algebraic backward's form at the layer-2 shape)
        return adamml_res_stream_launch(d, dz, w_dgrad_packed, dx, res_mask, sums_a, z_b, vec_b, sums_b, stream);
    const adamml_conv_desc_t g = dgrad_desc(d, accumulate, d->KH > 1);       // (3x3: pad KH - 1 - pad for the flipped taps, as adamml_conv_bwd_data)
    if (!z_b && res_3x3_c64(d))
        return adamml_conv3x3_c64_res_launch(&g, dz, w_dgrad_packed, dx, res_out, res_mask, res_act, z_a, vec_a, sums_a, stream);
    ResEpi r{res_out, res_mask, res_act, z_b, vec_b, sums_b};
    return conv_launch(&g, dz, w_dgrad_packed, nullptr, nullptr, dx, sums_a, z_a, vec_a, ACT_NONE, stream, nullptr, &r);
}

extern "C" size_t adamml_conv_bwd_data_res_prod_workspace(const adamml_conv_desc_t* d) {
    if (!d) return 0;
    if (adamml_res_prod_stream_supported(d, 64)) return adamml_res_prod_stream_workspace(d);
    const int groups = d->groups < 1 ? 1 : d->groups;
    const int n_ptiles = ceil_div(d->N * d->OH * d->OW, BP), n_ctiles = ceil_div(d->Cin, 128);      // (dgrad: the output channels are d->Cin)
    long nsp = 1536 / ((long)n_ctiles * groups);
    if (nsp < 1) nsp = 1;
    const int tpb = ceil_div(n_ptiles, (int)nsp);
    return (size_t)groups * n_ctiles * ceil_div(n_ptiles, tpb < 1 ? 1 : tpb) * 128 * 64 * sizeof(float);
}

extern "C" int adamml_conv_bwd_data_res_prod_supported(const adamml_conv_desc_t* d, int a_channels) {
    if (res_1x1(d) && adamml_res_prod_stream_supported(d, a_channels)) return 1;
    return res_1x1(d) && d->Cin % 128 == 0 && a_channels == 64 &&
           (long)ceil_div(d->N * d->OH * d->OW, BP) * (d->Cin / 128) * (d->groups < 1 ? 1 : d->groups) >= 4096 ? 1 : 0;
}

extern "C" int adamml_conv_bwd_data_res_prod_streams(const adamml_conv_desc_t* d, int a_channels) {
    return res_1x1(d) && adamml_res_prod_stream_supported(d, a_channels) ? 1 : 0;
}

extern "C" int adamml_conv_bwd_data_res_prod(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx,
                                             const uint8_t* res_mask, int res_act, double* sums_a, const void* a, const float* a_scale,
                                             const float* a_shift, int a_act, int a_gstride, int a_channels, float* prod,
                                             void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!adamml_conv_bwd_data_res_prod_supported(d, a_channels)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_bwd_data_res_prod: unsupported shape");
    if (!res_mask || !sums_a || !a || !prod) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data_res_prod: null argument");
    if (adamml_res_prod_stream_supported(d, a_channels))
        return adamml_res_prod_stream_launch(d, dz, w_dgrad_packed, dx, res_mask, sums_a, a, a_scale, a_shift, a_act, a_gstride, prod, workspace,
                                             workspace_bytes, stream);
    const adamml_conv_desc_t dd = dgrad_desc(d, 1);
    ResEpi r{dx, res_mask, res_act, nullptr, nullptr, nullptr};       // (res_out is never read in the mask form)
    PfIn pf{a, a_scale, a_shift, a_act, a_gstride, a_channels, prod, workspace, workspace_bytes};
    return conv_launch(&dd, dz, w_dgrad_packed, nullptr, nullptr, dx, sums_a, nullptr, nullptr, 0, stream, nullptr, &r, nullptr, nullptr, nullptr, &pf);
}

extern "C" int adamml_conv_bwd_data(const adamml_conv_desc_t* d, const void* dz, const void* w_dgrad_packed, void* dx,
                                    int accumulate, hipStream_t stream) {
    // d describes the FORWARD conv; the data gradient is a stride-1 conv of the (zero-upsampled) dz with the
    // flipped / transposed weight pack (adamml_pack_conv_weight, mode 1).
    if (!d) return adamml_set_error(ADAMML_EINVAL, "conv_bwd_data: null desc");
    if (dgrad_stride2_ok(d)) return conv_dgrad_stride2(d, dz, w_dgrad_packed, dx, accumulate, nullptr, nullptr, nullptr, 0, stream);
    const adamml_conv_desc_t g = dgrad_desc(d, accumulate, true);
    return adamml_conv_fwd(&g, dz, w_dgrad_packed, nullptr, nullptr, dx, nullptr, stream);
}
