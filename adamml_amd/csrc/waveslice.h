// What the barrier-free "wave-slice" streaming kernels (conv1x1_stream.hip, conv1x1_fadd_stream.hip, conv1x1_fadd_next.hip,
// conv1x1_narrow.hip, conv1x1_wide.hip, res_prod_stream.hip, tpool_bwd_prod.hip) share: a wave owns a channel slice or a pixel tile, keeps
// its operands in registers or a wave-private LDS area and runs without a workgroup barrier in the loop.  The idioms of that protocol --
// wave-uniform clamp bounds, the lazy-operand vectors and transform, the staging rows and their transpose reads, the chunk-lane sums, the
// persistent grid -- are here ONCE: these kernels promise the tile kernels' bits through "same rounding points, same epilogue expression".
// Loop-invariant lane arithmetic (li, lg, trow, zch, zpx) stays in the caller and is passed in: computed inside a helper it is recomputed
// per use (tr_frag with its own trow: 2224 -> 2286 instructions in tpool_bwd_prod_kernel).  A helper is used only where the kernel's
// device code stays byte-identical with it (tools/device_code_digest.py); the sites and idioms where it does not -- a wrapper moves the
// point where an argument is evaluated, and the scheduler follows -- keep their own text: profiles/r11_bench_parent_vs_waveslice.txt.
// Internal linkage throughout (non-RDC build).
#pragma once
#include "common.h"
#include "../../include/adamml_hip.h"

namespace {

// a wave-uniform value pinned to a scalar register (as vector registers the clamp bounds were spilled to scratch and re-read per tile)
__device__ __forceinline__ float wave_uniform(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// clamp bounds of a lazy operand act(scale * raw + shift): [-inf, inf] when there is no transform (scale == nullptr)
__device__ __forceinline__ float lazy_lo(const float* scale, int act) { return wave_uniform(scale ? act_lo(act) : -INFINITY); }
__device__ __forceinline__ float lazy_hi(const float* scale, int act) { return wave_uniform(scale ? act_hi(act) : INFINITY); }

// s_vec [2][n] = scale, shift of the lazy operand of group g (p.in_scale, p.in_shift, group stride p.in_gs; identity when there is none).
// It takes the kernel's parameter block by reference and reads the fields where the loop it replaces read them: with the pointers passed by
// value, in_shift is loaded from the kernel arguments in front of the branch that needs it -- other code.
template <class P>
__device__ __forceinline__ void fill_lazy_vec(float* s_vec, int n, const P& p, int g, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) {
        s_vec[i] = p.in_scale ? p.in_scale[(size_t)g * p.in_gs + i] : 1.f;
        s_vec[n + i] = p.in_scale ? p.in_shift[(size_t)g * p.in_gs + i] : 0.f;
    }
}

// the lazy transform of 8 channels, rounded as every loader rounds it: bf16(act(scale * raw + shift))
__device__ __forceinline__ bf16x8 lazy8(bf16x8 raw, f32x8 sc, f32x8 sh, float lo, float hi) {
    f32x8 v = bf8_to_f32(raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = clamp_act(fmaf(v[i], sc[i], sh[i]), lo, hi);
    return f32_to_bf8(v);
}

// a 16-byte chunk of a staging row as two 8-byte LDS accesses (the rows are 8-byte aligned only)
__device__ __forceinline__ void stage8(char* dst, bf16x8 v) {
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.v = v;
    *reinterpret_cast<s16x4*>(dst) = u.s.a;
    *reinterpret_cast<s16x4*>(dst + 8) = u.s.b;
}
__device__ __forceinline__ bf16x8 unstage8(const char* src) {
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = *reinterpret_cast<const s16x4*>(src);
    u.s.b = *reinterpret_cast<const s16x4*>(src + 8);
    return u.v;
}

// MFMA fragment of the 16-channel block `blk` of a staged 32-row tile, pixels = the reduction dimension: two hardware transpose reads
// (trow = 8 lg + (li >> 2), computed once by the caller; the read pair itself is common.h's tr_rows, which the tile kernels use too)
__device__ __forceinline__ bf16x8 tr_frag(const char* base, int row_bytes, int blk, int trow, int li) {
    return tr_rows(base + trow * row_bytes + (blk * 16 + 4 * (li & 3)) * 2, row_bytes);
}

// acc[mt][nt] += Z^T X over the 32 rows of two staged tiles (the fragments of the NARROWER operand are held, the other side streams)
template <int MT, int NT>
__device__ __forceinline__ void staged_outer_product(f32x4 (&acc)[MT][NT], const char* zs, int zrow, const char* xs, int xrow, int trow, int li) {
    if constexpr (NT <= MT) {
        bf16x8 fb[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) fb[nt] = tr_frag(xs, xrow, nt, trow, li);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const bf16x8 fa = tr_frag(zs, zrow, mt, trow, li);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[nt], acc[mt][nt], 0, 0, 0);
        }
    } else {
        bf16x8 fa[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) fa[mt] = tr_frag(zs, zrow, mt, trow, li);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bf16x8 fb = tr_frag(xs, xrow, nt, trow, li);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb, acc[mt][nt], 0, 0, 0);
        }
    }
}

// per-channel sums of the (pixel, 8-channel chunk) lanes: the eight lanes that share a chunk (lane % 8) fold their pixels; lanes 0..7 then
// hold the wave's sums of channels 8 lane .. + 7 and publish them (that `if (lane < 8 && v != 0.f) stat_publish(..)` stays with the callers:
// behind a helper the tail of tpool_bwd_prod_kernel was scheduled differently -- same resources, other instruction order)
__device__ __forceinline__ float chunk_lane_fold(float v) {
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// ---- host side
// workgroups per group of a persistent launch: one per work item, at most per_cu on each of the 256 CUs over all groups
inline int persistent_blocks(long work_items, int groups, int per_cu) {
    long cap = 256L * per_cu / (groups < 1 ? 1 : groups);
    if (cap < 1) cap = 1;
    return (int)(work_items < cap ? work_items : cap);
}

}  // namespace
