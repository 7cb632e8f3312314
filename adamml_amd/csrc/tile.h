// Tile primitives that more than one of the MFMA tile kernel files (conv_gemm.hip, conv_wgrad.hip, gram.hip) uses: the workgroup size, the
// transpose-read LDS image, LDS-DMA staging.  Everything has internal linkage: the build is non-RDC, so a device global -- the zero page -- cannot be shared
// between translation units and every file that includes this header gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int NTHREADS = 256;

// LDS image of one K step: [32 pixels][CH channels] bf16, row-major, 8-byte units XOR-swizzled so that the
// ds_read_b64_tr_b16 of a 32-lane service group (rows {r..r+3} U {r+8..r+11}) touches 64 distinct banks.
template <int CH>
__device__ __forceinline__ int tr_swz(int row) {
    if (CH >= 128) return ((row & 3) | (((row >> 3) & 1) << 2)) << 2;       // 256-byte rows: all rows start at bank 0
    return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 2;               // 128-byte rows: parity picks the bank half
}

// MFMA fragment of the 8-byte unit column u of such an image (common.h: tr_pair).  lo / hi = byte offsets of this lane's row trow = 8 lg +
// (li >> 2) and of row trow + 4, x_lo / x_hi = tr_swz of the two: loop-invariant, computed once by the caller.
__device__ __forceinline__ bf16x8 tr_swz_frag(const char* base, int lo, int x_lo, int hi, int x_hi, int u) {
    return tr_pair(base + lo + ((u ^ x_lo) << 3), base + hi + ((u ^ x_hi) << 3));
}

__device__ const uint4 g_zero_page[4] = {};          // 64 zero bytes: source of the out-of-range chunks of an LDS-DMA tile

__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_uniform) : "memory");
}

inline int ilog2_exact(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return (1 << s) == v ? s : -1;
}

}  // namespace
