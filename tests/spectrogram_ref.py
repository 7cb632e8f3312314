"""float64 restatement of the sound input of utils/video_dataset.py:93-132 (load_sound) and the error model the HIP spectrogram is
checked with.  Plain numpy (no torch.cuda): tests/test_spectrogram_cpu.py and tests/test_spectrogram_gpu.py both import it.

STFT.  librosa.stft(x, n_fft, hop_length=hop, win_length=win, window='hann', center=True, pad_mode='constant'): the periodic Hann
window of length win is zero-padded to n_fft, centred ((n_fft - win) // 2 zeros on the left), the signal is padded with n_fft // 2
zeros on both sides, and frame t is padded[t * hop : t * hop + n_fft] times that window; X[k, t] = sum_n frame[n] e^{-2 pi i k n / n_fft},
k < n_fft // 2 + 1.  The image is log(|X|^2 + eps).

Error model.  The kernel computes Re and Im as fp32 dot products of length win over the fp32 operands w[m] x[m] (basis rounded once
from fp64), so |Re_h - Re| and |Im_h - Im| are at most gamma * A with A = sum_m |w[m] x[m]| over the frame's support and
gamma = (win + 2) * 2^-24 (win accumulations, the basis rounding, one spare).  That propagates to the power as
dP = 2 (|Re| + |Im|) gamma A + 2 (gamma A)^2, plus 3 fp32 roundings of the power and of P + eps (3 * 2^-24 (P + eps)).  The accepted
band for log(P + eps) is [log(max(P + eps - dP, eps (1 - 2^-23))), log(P + eps + dP)], widened by logf's own error (2 ulps of the result,
with a 2^-24 floor).  The lower edge is clamped at eps: a near-silent bin (P below the rounding noise of its frame) may come out as
anything between log(eps) and its upper edge -- the slack any fp32 STFT needs there, librosa's included.
"""
import math

import numpy as np

U32 = 2.0 ** -24


def sizes(L, n_fft, hop):
    """(F, T) of the spectrogram of L samples."""
    return n_fft // 2 + 1, 1 + (L + 2 * (n_fft // 2) - n_fft) // hop


def hann(win, periodic=True):
    n = np.arange(win, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (win if periodic else win - 1))


def frames(x, n_fft, win, hop, window=None, pad_mode="constant"):
    """[T, n_fft] windowed frames of one clip (float64), librosa's centred framing."""
    x = np.asarray(x, dtype=np.float64)
    if window is None:
        window = hann(win)
    full = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    full[lpad:lpad + win] = window
    h = n_fft // 2
    padded = np.pad(x, h, mode=pad_mode)
    T = 1 + (len(padded) - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return padded[idx] * full[None, :], np.abs(padded[idx]) * full[None, :]


def stft(x, n_fft=511, win=240, hop=120, window=None, pad_mode="constant"):
    """(Re, Im, A) [F, T] in float64: X = Re - i Im, A = sum over the frame of |w x| (the error model's scale)."""
    fr, fa = frames(x, n_fft, win, hop, window, pad_mode)
    F = n_fft // 2 + 1
    n = np.arange(n_fft)
    ang = 2.0 * np.pi * ((np.arange(F)[:, None] * n[None, :]) % n_fft) / n_fft
    re = np.cos(ang) @ fr.T
    im = np.sin(ang) @ fr.T
    return re, im, np.broadcast_to(fa.sum(axis=1)[None, :], re.shape)


def log_power(x, n_fft=511, win=240, hop=120, eps=1e-6, **kw):
    re, im, _ = stft(x, n_fft, win, hop, **kw)
    return np.log(re * re + im * im + eps)


def numpy_f32(x, n_fft=511, win=240, hop=120, eps=1e-6, window=None, pad_mode="constant", bin_shift=0):
    """The same image computed in float32 with numpy (fp32 basis, fp32 matmul, fp32 log) -- what an ordinary fp32 STFT gives.
    window / pad_mode / bin_shift plant the defects the checker must reject."""
    fr, _ = frames(x, n_fft, win, hop, window, pad_mode)
    F = n_fft // 2 + 1
    n = np.arange(n_fft)
    k = np.arange(F) + bin_shift
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft) / n_fft
    fr32 = fr.astype(np.float32)
    re = np.cos(ang).astype(np.float32) @ fr32.T
    im = np.sin(ang).astype(np.float32) @ fr32.T
    p = re * re + im * im
    with np.errstate(divide="ignore"):
        return np.log(p + np.float32(eps)) if eps else np.log(p)


def tolerance(x, n_fft=511, win=240, hop=120, eps=1e-6):
    """(ref, lo, hi): the float64 image and the accepted band of the error model, each [F, T]."""
    re, im, A = stft(x, n_fft, win, hop)
    p = re * re + im * im
    ref = np.log(p + eps)
    gamma = (win + 2) * U32
    e = gamma * A
    dp = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e + 3.0 * U32 * (p + eps)
    hi = np.log(p + eps + dp)
    lo = np.log(np.maximum(p + eps - dp, eps * (1.0 - 2.0 * U32)))
    slack = 2.0 * 2.0 * U32 * np.maximum(np.abs(ref), 1.0) + U32
    return ref, lo - slack, hi + slack


def check(y, x, n_fft=511, win=240, hop=120, eps=1e-6):
    """max err / tol of an image y [F, T] of clip x: <= 1 is accepted.  err/tol of an element is its distance from the float64
    value over the distance from that value to the band edge on its side; non-finite or misshapen output is rejected (inf)."""
    ref, lo, hi = tolerance(x, n_fft, win, hop, eps)
    y = np.asarray(y, dtype=np.float64)
    if y.shape != ref.shape or not np.all(np.isfinite(y)):
        return math.inf
    above = y >= ref
    tol = np.where(above, hi - ref, ref - lo)
    return float(np.max(np.abs(y - ref) / tol))


def sound_slice_bounds(n, idx, start_frame, fps=29.97, audio_length=1.28, resampling_rate=24000):
    """(a, b, required): load_sound's slice samples[a:b] of an n-sample track (video_dataset.py:96-114), restated with explicit
    index ranges.  In the track b - a may be required +- 1 (its two round() calls)."""
    need = int(round(resampling_rate * audio_length))
    t_mid = (start_frame + idx) / fps
    t_lo, t_hi = t_mid - audio_length / 2.0, t_mid + audio_length / 2.0
    if t_lo < 0:
        return 0, min(need, n), need                             # window starts before the track: its first samples
    if t_hi > n / float(resampling_rate):
        return max(n - need, 0), n, need                         # window ends after the track: its last samples
    return int(round(t_lo * resampling_rate)), int(round(t_hi * resampling_rate)), need


def load_sound_slice(samples, idx, start_frame, **kw):
    """load_sound's choice of samples (video_dataset.py:96-119).  The slice of the in-track case is kept as the reference takes it,
    so the result may be one sample longer than required; a result shorter than required repeats the slice from its start
    (np.tile then truncation is index i -> i mod len)."""
    a, b, need = sound_slice_bounds(samples.shape[0], idx, start_frame, **kw)
    got = samples[a:b]
    if got.shape[0] >= need:
        return got
    return got[np.arange(need) % got.shape[0]]
