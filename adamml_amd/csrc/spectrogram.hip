// Log-power spectrogram of raw waveforms (the sound input of utils/video_dataset.py:93-132 load_sound, librosa.stft semantics):
// wave [N, L] fp32 -> y [N, F, T] fp32, y[k, t] = log(Re^2 + Im^2 + eps), F = n_fft/2 + 1, T = 1 + (L + 2*(n_fft/2) - n_fft) / hop.
//
// Structure: per clip, a GEMM of the [win x 2F] windowed cos/sin basis (caller-owned, built once in fp64 on the host) with the
// [win x T] frame matrix, on the exact-fp32 matrix cores (mfma_f32_32x32x2f32: a k-ordered fmaf chain).  A workgroup owns one clip,
// a block of TB = 32*NT frames and WAVES*32 frequency bins.  Its frames overlap by win - hop samples, so the workgroup stages the
// sample slab they cover in LDS once (zeros outside [0, L): center=True, pad_mode='constant') and forms every frame row from it;
// for hop > win the frames are packed at a stride of win instead (no unused samples).  Each wave owns 32 bins: per K step of 2
// taps it reads the cos and sin basis values of its bins (one float per lane each, L2-resident) and NT frame values from LDS, and
// issues 2*NT MFMAs.  The cos and sin accumulators of a (bin, frame) pair sit in the same register of the same lane, so the
// epilogue (fmaf power, accurate logf) runs in registers.  The accumulator column is the frame: stores are 128-byte rows along t.
//
// NaN: a tap outside the support (m >= win) reads zero for BOTH operands, so a NaN / Inf sample reaches exactly the frames whose
// support holds it, and there every bin (0 * NaN = NaN, also where the Hann window or the sine is zero).
#include "common.h"
#include "../../include/adamml_hip.h"

namespace {

constexpr int SPEC_WAVES = 4;               // waves per workgroup: 4 x 32 bins
constexpr int SPEC_KC = 8;                  // K steps (2 taps each) per register batch of basis values
constexpr int SPEC_MAX_NFFT = 512;          // documented bound (include/adamml_hip.h); keeps the LDS slab <= 64 KiB at NT = 1
constexpr int SPEC_LDS_BYTES = 65536;

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
__global__ void __launch_bounds__(64 * SPEC_WAVES) __attribute__((amdgpu_waves_per_eu(2)))     // <= 256 registers: 2 workgroups per CU
log_spectrogram_kernel(const float* __restrict__ wave, const float* __restrict__ basis, float* __restrict__ y, int L, int F, int T, int win,
                       int hop, int fs, int s_off, int ntb, float eps) {
    extern __shared__ float slab[];
    const int n = blockIdx.x / ntb;
    const int t0 = (blockIdx.x - n * ntb) * (32 * NT);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* x = wave + (size_t)n * L;

    // slab: frame tl of the block, tap m at slab[tl*fs + m]; clip sample of frame t, tap m = t*hop + s_off + m
    const int slab_len = (32 * NT - 1) * fs + win;
    const int s_lo = t0 * hop + s_off;
    for (int i = threadIdx.x; i < slab_len; i += 64 * SPEC_WAVES) {
        int s;
        if (fs == hop) {
            s = s_lo + i;
        } else {                                       // hop > win: frames packed at stride win
            const int tl = i / win;
            s = s_lo + tl * hop + (i - tl * win);
        }
        slab[i] = (s >= 0 && s < L) ? x[s] : 0.f;
    }
    __syncthreads();

    const int kb = (blockIdx.y * SPEC_WAVES + wv) * 32;            // first bin of this wave
    if (kb >= F) return;                                           // no barrier follows
    const int twoF = 2 * F;
    const int col = lane & 31, half = lane >> 5;
    const bool bin_ok = kb + col < F;
    const float* bc = basis + kb + col;                            // cos column of bin kb+col; sin at +F
    const float* fr = slab + col * fs + half;                      // frame col of tile 0, tap 'half' of the K step

    f32x16 re[NT], im[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) re[j][r] = im[j][r] = 0.f;

    const int ksteps = (win + 1) >> 1;
    for (int k0 = 0; k0 < ksteps; k0 += SPEC_KC) {
        float a_c[SPEC_KC], a_s[SPEC_KC];
#pragma unroll
        for (int kk = 0; kk < SPEC_KC; ++kk) {
            const int m = 2 * (k0 + kk) + half;
            const bool ok = bin_ok && m < win;
            a_c[kk] = ok ? bc[(size_t)m * twoF] : 0.f;
            a_s[kk] = ok ? bc[(size_t)m * twoF + F] : 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < SPEC_KC; ++kk) {
            const int m = 2 * (k0 + kk) + half;
            const bool ok = m < win;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float b = ok ? fr[j * 32 * fs + 2 * (k0 + kk)] : 0.f;
                re[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c[kk], b, re[j], 0, 0, 0);
                im[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_s[kk], b, im[j], 0, 0, 0);
            }
        }
    }

    // C/D map: column (frame) = lane & 31, row (bin) = (r & 3) + 8*(r >> 2) + 4*(lane >> 5)
    float* yn = y + (size_t)n * F * T;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int t = t0 + j * 32 + col;
        if (t >= T) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = kb + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (k < F) {
                const float p = fmaf(re[j][r], re[j][r], im[j][r] * im[j][r]);
                yn[(size_t)k * T + t] = logf(p + eps);
            }
        }
    }
}

size_t slab_bytes(int nt, int fs, int win) { return (size_t)((32 * nt - 1) * fs + win) * sizeof(float); }

}  // namespace

extern "C" int adamml_log_spectrogram(const float* wave, const float* basis, float* y, int N, int L, int n_fft, int win, int hop, float eps,
                                      hipStream_t stream) {
    if (N < 0 || L < 1) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: bad N = %d / L = %d", N, L);
    if (n_fft < 2 || n_fft > SPEC_MAX_NFFT)
        return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: n_fft = %d outside [2, %d]", n_fft, SPEC_MAX_NFFT);
    if (win < 1 || win > n_fft) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: win = %d outside [1, n_fft = %d]", win, n_fft);
    if (hop < 1) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: hop = %d < 1", hop);
    if (!(eps >= 0.f)) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: eps must be >= 0");
    if (L > (1 << 30)) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: L = %d too large", L);
    if (N == 0) return ADAMML_OK;
    if (!wave || !basis || !y) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: null argument");
    const int F = n_fft / 2 + 1;
    const int T = 1 + (L + 2 * (n_fft / 2) - n_fft) / hop;
    const int fs = hop < win ? hop : win;                            // LDS stride between the frames of a block
    const int s_off = (n_fft - win) / 2 - n_fft / 2;                 // lpad - n_fft/2: clip sample of frame 0, tap 0
    int nt = 4;
    while (nt > 1 && (32 * (nt / 2) >= T || slab_bytes(nt, fs, win) > SPEC_LDS_BYTES)) nt /= 2;
    const int ntb = (T + 32 * nt - 1) / (32 * nt);
    if ((int64_t)N * ntb > 0x7fffffff) return adamml_set_error(ADAMML_EINVAL, "log_spectrogram: N = %d too large", N);
    const dim3 grid((unsigned)(N * ntb), (unsigned)((F + 32 * SPEC_WAVES - 1) / (32 * SPEC_WAVES)));
    const size_t lds = slab_bytes(nt, fs, win);
    switch (nt) {
        case 4:
            hipLaunchKernelGGL(log_spectrogram_kernel<4>, grid, dim3(64 * SPEC_WAVES), lds, stream, wave, basis, y, L, F, T, win, hop, fs,
                               s_off, ntb, eps);
            break;
        case 2:
            hipLaunchKernelGGL(log_spectrogram_kernel<2>, grid, dim3(64 * SPEC_WAVES), lds, stream, wave, basis, y, L, F, T, win, hop, fs,
                               s_off, ntb, eps);
            break;
        default:
            hipLaunchKernelGGL(log_spectrogram_kernel<1>, grid, dim3(64 * SPEC_WAVES), lds, stream, wave, basis, y, L, F, T, win, hop, fs,
                               s_off, ntb, eps);
    }
    return adamml_check_launch("log_spectrogram");
}
