// Weight-streaming forward 1x1 / stride-1 conv for serving-size batches (model.online(), online.Pool: one to eight videos per step).
// The deep 1x1 convs of ResNet-50 layers 3-4 and the tail of the sound MobileNetV2 then have a few dozen to a few hundred pixels and
// 256 .. 2048 channels on both sides: the launch is its weight matrix read once.  The tile kernel (conv_gemm.hip) tiles 128 pixels x 64
// channels and walks all of K inside one workgroup -- 2048 -> 512 at 49 pixels is 8 workgroups on 256 CUs, each waiting for one K step of
// HBM latency after the other.  Here the roles are swapped:
//   * the WEIGHTS are the streamed operand.  A wave owns 16 output channels for a chunk of 16 / 32 / 64 pixels; its weight rows go from
//     global memory straight into MFMA A fragments (16-byte loads along K from the mode-0 pack [Cout][Cin]; no LDS, no repack), through a
//     register ring that runs SK_PD panels = 16 MFMA K steps ahead: a wave keeps 16 KB of weights in flight, the grid of 2048 -> 512 at
//     49 pixels (128 waves) the whole matrix.
//   * the ACTIVATIONS are the resident operand.  The four waves of a workgroup (four neighbouring channel slices) share the pixel chunk:
//     panel by panel (128 channels) it goes through the same register ring -- requested together with the panel's weights, so that every
//     wait of the in-order load counter is for the OLDEST bundle and leaves SK_PD - 1 bundles in flight -- and into a double-buffered,
//     XOR-swizzled LDS panel, the lazy input transform (in_scale / in_shift / act, per group) applied on the way in as the tile kernel's
//     loader applies it.  One barrier per panel (4 MFMA K steps) publishes it; there is none inside a panel.
//   * every load of the steady state is unconditional, from a clamped address: no load sits behind a branch, so the compiler's wait
//     counts are exact (conv_gemm.hip, UNC).  Rows past P and channels past K are zeroed on the way into LDS; panels past the last one
//     are requested, never multiplied.
// Numerics: v_mfma_f32_16x16x32_bf16 with the weights as A and the pixels as B, K steps in ascending order into one fp32 accumulator
// per output, one rounding to bf16 -- the instruction, operand roles, K order and rounding point of conv_gemm_kernel's MODE 0
// instances: outputs are bit-identical to the tile kernel's (tests/test_conv1x1_skinny_gpu.py compares them).  No split K, no atomics.
// adamml_conv_fwd dispatches here from its arguments alone (adamml_conv1x1_skinny_supported); training launches pass `stats` and keep
// the tile kernel.
#include "common.h"
#include "conv_internal.h"
#include "../../include/adamml_hip.h"

namespace {

constexpr int SK_NW = 4;                // waves per workgroup: 4 slices of 16 output channels share a pixel chunk
constexpr int SK_NT = SK_NW * 64;
constexpr int SK_KP = 128;              // channels per panel = 4 MFMA K steps
constexpr int SK_PD = 4;                // panels in flight per wave
constexpr int SK_ROWB = SK_KP * 2;      // bytes of a pixel row of an LDS panel: 16 chunks of 16 bytes = all 64 banks
constexpr int SK_MAXK = 2048;           // the lazy vectors live in LDS: 2 x 8 KB
// the tile kernel's own grid arithmetic (conv_plan: 128 pixels x 64 channels per workgroup for small problems): the kernel serves
// launches that give the tile kernel fewer than one workgroup per CU ...
constexpr int SK_TILE_WG = 256;
// ... up to this many pixels per group (the measured cut-over: see adamml_conv1x1_skinny_supported): the tile kernel's time grows with
// its K loop, this kernel's with the pixel chunks that re-read the weight rows, so long-K layers keep winning four times further
constexpr int SK_MAX_P = 392;
constexpr int SK_LONG_K = 1024, SK_MAX_P_LONG_K = 1568;

struct SkP {
    const bf16_t* x;
    const bf16_t* w;
    const float* in_scale;
    const float* in_shift;
    bf16_t* y;
    int P, K, Cout, act, in_gs;
};

// NPT: 16-pixel MFMA tiles of a chunk.  LDS: 2 panels x NPT x 4 KB + 16 KB of vectors = 24 .. 48 KB: >= 3 workgroups per CU.
template <int NPT>
__global__ __launch_bounds__(SK_NT, 2) void conv1x1_skinny_kernel(SkP p) {
    constexpr int ROWS = 16 * NPT;
    constexpr int PANEL_BYTES = ROWS * SK_ROWB;
    __shared__ __attribute__((aligned(16))) char s_act[2 * PANEL_BYTES];
    __shared__ __attribute__((aligned(16))) float s_vec[2 * SK_MAXK];       // scale at [0, K), shift at [SK_MAXK, SK_MAXK + K)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int g = blockIdx.z, K = p.K;
    const int p0 = blockIdx.y * ROWS;
    const int c0 = (blockIdx.x * SK_NW + wave) * 16;
    const bool active = c0 < p.Cout;                                        // (Cout % 64 != 0: the last workgroup has idle slices)
    const bf16_t* x = p.x + (size_t)g * p.P * K;
    bf16_t* y = p.y + (size_t)g * p.P * p.Cout;
    const bool lazy = p.in_scale != nullptr;
    if (lazy) {
        const float* sc = p.in_scale + (size_t)g * p.in_gs;
        const float* sh = p.in_shift + (size_t)g * p.in_gs;
        for (int i = tid; i < K; i += SK_NT) { s_vec[i] = sc[i]; s_vec[SK_MAXK + i] = sh[i]; }
        __syncthreads();
    }
    const float lo = act_lo(p.act), hi = act_hi(p.act);

    // staging share of this thread: chunk sc (8 channels) of rows (tid >> 4) + 16 i.  LDS position of chunk c of row r: c ^ (r & 15) --
    // the 16 lanes of a ds_write_b128 / ds_read_b128 service group touch 16 distinct chunks = all 64 banks
    const int sc8 = (tid & 15) * 8;
    const bf16_t* xrow[NPT];
    bool rok[NPT];
    int sdst[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int r = (tid >> 4) + 16 * i;
        rok[i] = p0 + r < p.P;
        xrow[i] = x + (size_t)(rok[i] ? p0 + r : p.P - 1) * K;
        sdst[i] = r * SK_ROWB + (((tid & 15) ^ (r & 15)) << 4);
    }
    // A fragment of K step ks: lane (li, lg) holds channels 32 ks + 8 lg .. + 7 of weight row c0 + li
    const bf16_t* wrow = p.w + (size_t)((active ? c0 : 0) + li) * K + lg * 8;

    bf16x8 ra[SK_PD][NPT], rw[SK_PD][4];
    auto issue = [&](auto slot_c, int pn) {
        constexpr int SL = decltype(slot_c)::value;
        const int kb = pn * SK_KP;
        const int ka = min(kb + sc8, K - 8);                                // clamped: a chunk past K is re-read, then zeroed / never used
#pragma unroll
        for (int i = 0; i < NPT; ++i) ra[SL][i] = *reinterpret_cast<const bf16x8*>(xrow[i] + ka);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) rw[SL][ks] = *reinterpret_cast<const bf16x8*>(wrow + min(kb + ks * 32, K - 32));
    };

    f32x4 acc[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int np = (K + SK_KP - 1) / SK_KP;
    static_for<SK_PD>([&](auto sc) { issue(sc, (int)decltype(sc)::value); });
    // K <= SK_MAXK: at most 4 trips, unrolled with early exits -- straight-line code, so that the wait for a slot is counted exactly
    // (rolled, the compiler's wait counts merge at the loop header and drain three of the four slots there)
#pragma unroll
    for (int pn0 = 0; pn0 < SK_MAXK / SK_KP; pn0 += SK_PD) {
        if (pn0 >= np) break;
        static_for<SK_PD>([&](auto sc) {
            constexpr int SL = decltype(sc)::value;
            const int pn = pn0 + SL, kb = pn * SK_KP;
            char* buf = s_act + (pn & 1) * PANEL_BYTES;
            // the oldest bundle has landed: its activations -> LDS (everyone left this buffer before the previous panel's barrier)
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                bf16x8 v = ra[SL][i];
                const bool ok = rok[i] && kb + sc8 < K;
                if (lazy && ok) {
                    const f32x8 s = load_f32x8(s_vec + kb + sc8), h = load_f32x8(s_vec + SK_MAXK + kb + sc8);
                    f32x8 f = bf8_to_f32(v);
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = clamp_act(fmaf(f[j], s[j], h[j]), lo, hi);
                    v = f32_to_bf8(f);
                }
                if (!ok) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                *reinterpret_cast<bf16x8*>(buf + sdst[i]) = v;
            }
            __syncthreads();
            if (pn < np) {                                                  // (uniform; LDS reads and MFMAs only behind it)
                const int nks = min(4, (K - kb) >> 5);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < nks) {
#pragma unroll
                        for (int t = 0; t < NPT; ++t) {
                            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(buf + (t * 16 + li) * SK_ROWB + (((ks * 4 + lg) ^ li) << 4));
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rw[SL][ks], fa, acc[t], 0, 0, 0);
                        }
                    }
                }
            }
            // refill the slot AFTER its last use (requested ahead of it, the new values would need registers of their own and the loop
            // would end in a copy of the whole ring: a full drain of the load counter per trip).  Unconditional, clamped address
            issue(sc, pn + SK_PD);
        });
    }
    // the tile kernel's plain epilogue: one rounding to bf16; lane (li, lg) holds channels c0 + 4 lg .. + 3 of pixel 16 t + li
    if (active) {
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int pix = p0 + t * 16 + li;
            if (pix < p.P) *reinterpret_cast<bf16x4*>(y + (size_t)pix * p.Cout + c0 + lg * 4) = f32_to_bf4(acc[t]);
        }
    }
}

template <int NPT>
void skinny_launch(const SkP& p, int groups, hipStream_t stream) {
    const dim3 grid(ceil_div(p.Cout, 16 * SK_NW), ceil_div(p.P, 16 * NPT), groups);
    hipLaunchKernelGGL(conv1x1_skinny_kernel<NPT>, grid, dim3(SK_NT), 0, stream, p);
}

}  // namespace

// Serves the adamml_conv_fwd launch of descriptor d (has_stats: the call passes a statistics accumulator)?  Forward 1x1 / stride 1,
// no accumulation, no statistics (eval / no-grad: runtime.conv_bn passes none), Cin and Cout multiples of 32, Cin <= 2048, not a shape
// of the narrow MobileNetV2 kernels, and few pixels: the tile kernel's grid -- ceil(P / 128) * ceil(Cout / 64) * groups workgroups --
// stays below one workgroup per CU (256), and P per group <= 392 (Cin < 1024) or <= 1568 (Cin >= 1024).
// Cut-over, measured (profiles/conv1x1_skinny.json: tools/bench_conv1x1_skinny.py against the tile kernel of the parent build on the
// same tensors, alternating, with P <= 3136 admitted): up to 392 pixels the kernel wins on every layer-3/4 and sound-tail shape, plain
// and lazy, by more than the spread (1.1x .. 5.6x).  Beyond, the short-K shapes with a plain input lose (256 -> 1024 at 784: 0.97x,
// 320 -> 1280 at 512: within the spread, 512 -> 2048 at 784: 0.80x) while Cin >= 1024 still wins at 1568 (1.3x .. 2.8x) and 1024 -> 512
// loses at 3136 (0.80x): two cut-overs, each the largest measured pixel count at which no shape of its class loses.
extern "C" int adamml_conv1x1_skinny_supported(const adamml_conv_desc_t* d, int has_stats) {
    if (!d || has_stats || d->accumulate) return 0;
    if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0 || d->up > 1 || d->OH != d->H || d->OW != d->W) return 0;
    if (d->Cin < 32 || d->Cin % 32 || d->Cout < 32 || d->Cout % 32 || d->Cin > SK_MAXK) return 0;
    const long P = (long)d->N * d->OH * d->OW;
    const int groups = d->groups < 1 ? 1 : d->groups;
    if (P < 1 || P > (d->Cin >= SK_LONG_K ? SK_MAX_P_LONG_K : SK_MAX_P) || groups > 65535) return 0;
    if ((long)ceil_div((int)P, 128) * ceil_div(d->Cout, 64) * groups >= SK_TILE_WG) return 0;
    return adamml_conv1x1_narrow_fwd_supported(d) ? 0 : 1;
}

int adamml_conv1x1_skinny_launch(const adamml_conv_desc_t* d, const void* x, const void* w_packed, const float* in_scale, const float* in_shift,
                                 void* y, hipStream_t stream) {
    if (!adamml_conv1x1_skinny_supported(d, 0)) return adamml_set_error(ADAMML_EUNSUPPORTED, "conv_fwd (skinny): not a serving-size 1x1 shape");
    if (!x || !w_packed || !y) return adamml_set_error(ADAMML_EINVAL, "conv_fwd (skinny): null argument");
    SkP p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w_packed; p.in_scale = in_scale; p.in_shift = in_scale ? in_shift : nullptr; p.y = (bf16_t*)y;
    p.P = d->N * d->OH * d->OW; p.K = d->Cin; p.Cout = d->Cout; p.act = d->act; p.in_gs = d->in_gstride;
    const int groups = d->groups < 1 ? 1 : d->groups;
    // the largest pixel chunk that still gives every CU two waves; the smallest one below that (a short K walk per wave matters more
    // than the weight rows being requested by up to four chunks: they meet in L2)
    const long slices = (long)(p.Cout / 16) * groups;
    if (slices * ceil_div(p.P, 64) >= 512) skinny_launch<4>(p, groups, stream);
    else if (slices * ceil_div(p.P, 32) >= 512) skinny_launch<2>(p, groups, stream);
    else skinny_launch<1>(p, groups, stream);
    return adamml_check_launch("conv_fwd (skinny)");
}
