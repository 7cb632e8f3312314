// What the HBM-bound elementwise files (bn.hip, pool.hip, head.hip, clip_input.hip, param.hip) and the depthwise kernels of dwconv_gemm32.hip
// share: the workgroup size, the thread map of the row-walking kernels, the per-channel publication of a workgroup's sums, the launchers' grid
// arithmetic and two compile-time dispatch helpers.  Internal linkage throughout (non-RDC build: every includer gets its own copy).
#pragma once
#include "common.h"
#include "../../include/adamml_hip.h"
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int MAXC = 2048;

// thread -> (pixel slot, channel chunk) mapping that keeps a thread's channel chunk fixed across its pixels
struct ChanMap {
    int nchunk, rows_per_pass, chunk, rslot;
    bool active;
    __device__ ChanMap(int C, int tid) {
        nchunk = C >> 3;
        rows_per_pass = NT / nchunk;
        if (rows_per_pass < 1) rows_per_pass = 1;
        active = tid < rows_per_pass * nchunk;
        chunk = tid % nchunk;
        rslot = tid / nchunk;
    }
};

// Per-channel sums of a workgroup (s, q: the 8-channel partials of this thread): row slot r of the thread map deposits its partials in LDS
// row r [2C]; one thread per channel folds the rows in row order and publishes the workgroup's partial exactly (common.h: reproducible
// reductions).  rows_per_pass * 2C <= 16 NT floats = the 2 * MAXC floats every caller provides.
__device__ __forceinline__ void block_channel_publish(const float (&s)[8], const float (&q)[8], const ChanMap& m, float* smem,
                                                      int C, double* out) {
    if (m.active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            smem[m.rslot * 2 * C + m.chunk * 8 + i] = s[i];
            smem[m.rslot * 2 * C + C + m.chunk * 8 + i] = q[i];
        }
    }
    __syncthreads();
    const unsigned slot = blockIdx.x & (ADAMML_STAT_SLOTS - 1);
    for (int i = threadIdx.x; i < 2 * C; i += NT) {
        float v = 0.f;
        for (int r = 0; r < m.rows_per_pass; ++r) v += smem[r * 2 * C + i];
        stat_publish(out + i, 2 * (size_t)C, slot, v);
    }
}

// ---- host side
#define CHECK_C(C, name)                                                                                     \
    if ((C) % 8 != 0 || (C) > MAXC || (C) <= 0)                                                              \
        return adamml_set_error(ADAMML_EINVAL, name ": C=%d must be a multiple of 8 in (0, %d]", (C), MAXC);

inline int grid_for(size_t work, int per_block = NT, int cap = 256 * 16) {
    size_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > (size_t)cap) g = cap;
    return (int)g;
}

inline int rows_per_pass(int C) { return NT / (C / 8) > 0 ? NT / (C / 8) : 1; }       // ChanMap::rows_per_pass on the host (C: checked by CHECK_C)

// rows per workgroup and workgroups per group of the row-walking kernels: >= 16 passes per thread, <= ~cap_total workgroups over all groups
struct RowGrid { size_t ppb, nblk; };
inline RowGrid rowwalk_grid(size_t P, int C, int groups, int cap_total) {
    const int rows = rows_per_pass(C);
    size_t ppb = (size_t)rows * 16;
    size_t nblk = (P + ppb - 1) / ppb;
    const size_t cap = cap_total / (groups < 1 ? 1 : groups) + 1;
    if (nblk > cap) { ppb = ((P + cap - 1) / cap + rows - 1) / rows * rows; nblk = (P + ppb - 1) / ppb; }
    return {ppb, nblk};
}
inline RowGrid reduce_grid(size_t P, int C, int groups) { return rowwalk_grid(P, C, groups, 2048); }

// bytes of a [groups][P][C] bf16 tensor, and whether it is larger than the 256 MB Infinity Cache: the kernels with a STREAM form then use
// non-temporal accesses (nothing is re-used from cache)
inline size_t tensor_bytes(size_t P, int C, int groups) { return (size_t)groups * P * C * 2; }
inline bool exceeds_infinity_cache(size_t P, int C, int groups) { return tensor_bytes(P, C, groups) > ((size_t)256 << 20); }

// A runtime choice as a template argument: f receives std::bool_constant<b> / std::integral_constant<int, T>, so a launcher writes the
// argument list of its kernel once (f: a generic lambda, the value is decltype(arg)::value).
template <class F>
inline void dispatch_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F>
inline void dispatch_frames_8_4_2(int T, F&& f) {           // the frame counts of the hot path (the caller has checked T)
    if (T == 8) f(std::integral_constant<int, 8>{}); else if (T == 4) f(std::integral_constant<int, 4>{}); else f(std::integral_constant<int, 2>{});
}

}  // namespace
