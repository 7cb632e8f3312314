"""CPU checks of the sound-spectrogram input (no GPU): the float64 restatement of load_sound's STFT (tests/spectrogram_ref.py) agrees
with torch.stft, its error model accepts an ordinary fp32 STFT and rejects the defects a kernel could plausibly have, the host-side
window selection (adamml_amd.audio.sound_window) equals load_sound's in every branch, and the C ABI declares and exports
adamml_log_spectrogram."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from adamml_amd import abi, audio
from adamml_amd.runtime import spectrogram_basis
from tests import spectrogram_ref as R

L = 30720


def _noise_with_gap(seed=0):
    """White noise with a silent stretch in the middle (frames of zero power: where eps matters) and loud edges."""
    x = np.random.default_rng(seed).standard_normal(L)
    x[12000:16000] = 0.0
    return x.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n_fft,win,hop,length", [(511, 240, 120, L), (511, 160, 80, 20480), (256, 200, 64, 5000)])
def test_reference_equals_torch_stft_in_float64(n_fft, win, hop, length):
    x = np.random.default_rng(1).standard_normal(length)
    ref = R.log_power(x, n_fft, win, hop)
    X = torch.stft(torch.from_numpy(x), n_fft=n_fft, hop_length=hop, win_length=win,
                   window=torch.hann_window(win, periodic=True, dtype=torch.float64), center=True, pad_mode="constant",
                   return_complex=True)
    got = torch.log(X.real ** 2 + X.imag ** 2 + 1e-6).numpy()
    assert ref.shape == got.shape == R.sizes(length, n_fft, hop)
    d = float(np.abs(ref - got).max())
    print("  max |log ref - log torch.stft| = %.3g" % d)
    assert d <= 1e-10


def test_checker_accepts_numpy_float32():
    x = _noise_with_gap()
    worst = R.check(R.numpy_f32(x), x)
    print("  numpy fp32: max err/tol = %.3f" % worst)
    assert worst <= 1.0
    for scale in (1e-3, 3e4):
        xs = x * scale
        assert R.check(R.numpy_f32(xs), xs) <= 1.0


def _defects(x):
    yield "symmetric Hann", R.numpy_f32(x, window=R.hann(240, periodic=False))
    yield "n_fft = 512", R.numpy_f32(x, n_fft=512)[:256, :256]
    yield "hop + 1", R.numpy_f32(np.concatenate([x, x[:400]]), hop=121)[:, :256]        # (T = 256 needs 30 976 samples)
    yield "hop - 1", R.numpy_f32(x, hop=119)[:, :256]
    yield "no eps", R.numpy_f32(x, eps=0.0)
    yield "reflect padding", R.numpy_f32(x, pad_mode="reflect")
    yield "bin off by one", R.numpy_f32(x, bin_shift=1)


def test_checker_rejects_planted_defects():
    x = _noise_with_gap()
    for name, y in _defects(x):
        worst = R.check(y, x)
        print("  %-16s max err/tol = %.3g" % (name, worst))
        assert worst >= 2.0, name
    # the symmetric window is a small change: median |dlog| ~ 1e-2 on noise
    sym = R.numpy_f32(x, window=R.hann(240, periodic=False))
    assert np.median(np.abs(sym - R.log_power(x))) > 3e-3


def test_host_basis_matches_the_float64_dft():
    b = spectrogram_basis(511, 240)
    assert b.dtype == np.float32 and b.shape == (240, 512)
    m, k = np.arange(240)[:, None], np.arange(256)[None, :]
    w = R.hann(240)[:, None]
    assert np.abs(b[:, :256] - w * np.cos(2 * np.pi * k * m / 511)).max() < 1e-7
    assert np.abs(b[:, 256:] - w * np.sin(2 * np.pi * k * m / 511)).max() < 1e-7
    assert np.all(b[0] == 0) and np.all(b[:, 256] == 0)            # w[0] = 0; sin of bin 0


def test_stft_sizes_round_as_load_sound():
    assert audio.stft_sizes() == (240, 120)
    assert audio.stft_sizes(16000) == (160, 80)
    assert audio.stft_sizes(22050) == (220, 110)         # round(220.5) = 220, round(110.25) = 110


def _check_window(track, idx, start, **kw):
    want = R.load_sound_slice(track, idx, start, **kw)
    req = int(round(kw.get("resampling_rate", 24000) * kw.get("audio_length", 1.28)))
    got = audio.sound_window(track, idx, start, **kw)
    assert got.dtype == np.float32 and got.shape == (req,)
    assert len(want) in (req, req + 1)
    np.testing.assert_array_equal(got, want[:req].astype(np.float32))
    a, b, _ = R.sound_slice_bounds(track.shape[0], idx, start, **kw)
    return b - a - req


def test_sound_window_every_branch():
    rng = np.random.default_rng(3)
    track = rng.standard_normal(24000 * 10).astype(np.float32)           # 10 s at 24 kHz
    _check_window(track, 5, 0)                                            # left_sec < 0: the first samples
    _check_window(track, 290, 5)                                          # right_sec > duration: the last samples
    _check_window(track, 150, 0)                                          # in the track
    _check_window(track, 3, 100, fps=25.0)
    short = rng.standard_normal(7000).astype(np.float32)                  # shorter than the window: tiled
    for idx in (0, 5, 200):
        _check_window(short, idx, 0)
    _check_window(rng.standard_normal(20000).astype(np.float32), 10, 0, resampling_rate=16000)
    # the two round() calls: in-track slices of required + 1 and required - 1 samples (rate * length / 2 not an integer)
    seen = set()
    for idx in range(20, 260, 3):
        for length in (1.28, 1.00005, 0.64003):
            seen.add(_check_window(track, idx, 0, fps=29.97, audio_length=length))
            seen.add(_check_window(track, idx, 7, fps=23.976, audio_length=length))
    print("  slice length - required seen:", sorted(seen))
    assert {-1, 0, 1} <= seen


def test_sound_window_rejects_an_empty_track():
    with pytest.raises(ValueError):
        audio.sound_window(np.zeros(0, np.float32), 0, 0)


def test_header_declares_and_library_exports_log_spectrogram():
    assert str(abi.FUNCTIONS["adamml_log_spectrogram"]) == (
        "int adamml_log_spectrogram(const float* wave, const float* basis, float* y, int N, int L, "
        "int n_fft, int win, int hop, float eps, hipStream_t stream)")
    ge.build()
    lib = ctypes.CDLL(ge.LIB)
    assert hasattr(lib, "adamml_log_spectrogram")
    assert lib.adamml_version() >= 102
    from adamml_amd import hip
    assert "adamml_log_spectrogram" in hip.SIGNATURES
