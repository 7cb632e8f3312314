"""Sound input without librosa: the two halves of utils/video_dataset.py:93-132 (load_sound).

    window = sound_window(samples, centre_frame, start_frame)            # host numpy: the 1.28 s the STFT sees
    image = log_spectrogram(torch.from_numpy(window).cuda())             # GPU: [256, 256] fp32 log-power spectrogram

`sound_window` is the loader's slicing and tiling; `log_spectrogram` is librosa.stft(n_fft=511, window='hann', win_length,
hop_length, center=True, pad_mode='constant') followed by log(|X|^2 + eps), computed by the HIP kernel adamml_log_spectrogram.
AdaMML.forward also takes the sound modality as waveforms [B, S, L] and runs `log_spectrogram` itself; a loader that
has to say which clips had no track hands over a `Waveforms` (adamml_amd/data.py)."""
import copy

import numpy as np
import torch

from . import hip, runtime

__all__ = ['Waveforms', 'log_spectrogram', 'sound_window', 'stft_sizes']


def stft_sizes(sample_rate=24000, window_ms=10, step_ms=5):
    """(win, hop) in samples, rounded as load_sound does (video_dataset.py:126-127)."""
    return int(round(window_ms * sample_rate / 1e3)), int(round(step_ms * sample_rate / 1e3))


def log_spectrogram(wave, sample_rate=24000, window_ms=10, step_ms=5, n_fft=511, eps=1e-6):
    """Waveforms [..., L] on the GPU -> log-power spectrograms [..., F, T] fp32, F = n_fft // 2 + 1 (frequency = row),
    T = 1 + (L + 2 * (n_fft // 2) - n_fft) // hop (time = column); the defaults give 256 x 256 for L = 30720 (1.28 s at 24 kHz).

    Floating-point input of another precision is converted to fp32 and non-contiguous input is copied; integer samples (whose
    scale the caller must choose) and CPU tensors are rejected.  Runs on the current stream; no host synchronisation."""
    if not isinstance(wave, torch.Tensor):
        raise TypeError("log_spectrogram: expected a torch.Tensor, got %s" % type(wave).__name__)
    hip.require_gpu(wave)
    if not wave.is_floating_point():
        raise TypeError("log_spectrogram: expected floating-point samples, got %s (convert to float32 at the intended scale)" % wave.dtype)
    if wave.dim() < 1 or wave.shape[-1] < 1:
        raise ValueError("log_spectrogram: expected [..., L] samples with L >= 1, got shape %s" % (tuple(wave.shape),))
    win, hop = stft_sizes(sample_rate, window_ms, step_ms)
    lead, length = wave.shape[:-1], wave.shape[-1]
    flat = wave.to(torch.float32).contiguous().reshape(-1, length)
    y = runtime.log_spectrogram(flat, n_fft, win, hop, eps)
    return y.view(*lead, y.shape[1], y.shape[2])


def sound_window(samples, centre_frame, start_frame, fps=29.97, audio_length=1.28, resampling_rate=24000):
    """The round(resampling_rate * audio_length) samples load_sound (video_dataset.py:96-119) passes to the STFT, as float32.

    samples: the decoded mono track at resampling_rate.  The window is centred on frame start_frame + centre_frame; a window
    that starts before the track takes the first samples, one that ends after it the last ones, and a track shorter than the
    window is tiled.  The reference's two round() calls can make its slice one sample longer than required: its STFT then has one
    more column (257 with the defaults).  Here the first `required` samples are kept instead: with the defaults frame t reads samples
    120 t - 120 .. 120 t + 119, so columns 0 .. 255 never see the extra sample, are exactly the reference's, and only its 257th
    column is dropped."""
    samples = np.asarray(samples)
    if samples.ndim != 1 or samples.shape[0] == 0:
        raise ValueError("sound_window: expected a non-empty 1-D track, got shape %s" % (samples.shape,))
    centre_sec = (start_frame + centre_frame) / fps
    left_sec = centre_sec - audio_length / 2.0
    right_sec = centre_sec + audio_length / 2.0
    duration = samples.shape[0] / float(resampling_rate)
    required = int(round(resampling_rate * audio_length))
    if left_sec < 0:
        out = samples[:required]
    elif right_sec > duration:
        out = samples[-required:]
    else:
        out = samples[int(round(left_sec * resampling_rate)):int(round(right_sec * resampling_rate))]
    if out.shape[0] == 0:
        raise ValueError("sound_window: empty slice (audio_length * resampling_rate too small)")
    if out.shape[0] < required:
        out = np.tile(out, int(required / out.shape[0] + 0.5) + 1)
    return np.ascontiguousarray(out[:required], dtype=np.float32)


class Waveforms:
    """A batch of sound windows as a loader hands it over: wave [B, S, L] float32 (`sound_window` of every clip) and missing [B, S]
    bool, set where the video has no track.  The reference's loader substitutes an all-zero image there, not the log(eps) image of
    silence (video_dataset.py:102-103), so `spectrogram` sets those images to exactly 0.  A plain class, like video.Frames:
    DistributedDataParallel's input scatter passes it through as it is."""

    def __init__(self, wave, missing=None):
        wave = torch.as_tensor(wave)
        if wave.dim() != 3 or wave.dtype != torch.float32 or wave.shape[-1] < 1:
            raise ValueError("Waveforms: expected float32 samples [B, S, L], got %s %s" % (wave.dtype, tuple(wave.shape)))
        missing = torch.zeros(wave.shape[:2], dtype=torch.bool) if missing is None else torch.as_tensor(missing)
        if missing.dtype != torch.bool or missing.shape != wave.shape[:2]:
            raise ValueError("Waveforms: expected bool flags %s, got %s %s" % (tuple(wave.shape[:2]), missing.dtype, tuple(missing.shape)))
        self.wave, self.missing = wave, missing
        # known on the host, so that `spectrogram` decides without reading the flags back from the GPU
        self.num_missing = int(missing.sum())

    @property
    def device(self):
        return self.wave.device

    @property
    def shape(self):
        """Shape of the waveforms: [B, S, L]."""
        return self.wave.shape

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def to(self, device, non_blocking=False):
        out = copy.copy(self)
        out.wave = self.wave.to(device, non_blocking=non_blocking)
        out.missing = self.missing.to(device, non_blocking=non_blocking)
        return out

    def pin_memory(self):
        out = copy.copy(self)
        out.wave, out.missing = self.wave.pin_memory(), self.missing.pin_memory()
        return out

    def spectrogram(self, sample_rate=24000, window_ms=10, step_ms=5, n_fft=511, eps=1e-6):
        """[B, S, F, T] fp32 on the GPU: `log_spectrogram` of the windows, exactly 0 for the missing clips.  When every clip of the
        batch is missing the spectrogram kernel is not launched."""
        hip.require_gpu(self.wave)
        if self.num_missing == self.missing.numel():
            _, hop = stft_sizes(sample_rate, window_ms, step_ms)
            frames = 1 + (self.wave.shape[-1] + 2 * (n_fft // 2) - n_fft) // hop
            return torch.zeros(*self.wave.shape[:2], n_fft // 2 + 1, frames, dtype=torch.float32, device=self.wave.device)
        spec = log_spectrogram(self.wave, sample_rate, window_ms, step_ms, n_fft, eps)
        if self.num_missing:
            spec.masked_fill_(self.missing[:, :, None, None], 0.0)
        return spec

    def __repr__(self):
        return "Waveforms(%s, %d missing, %s)" % (tuple(self.wave.shape), self.num_missing, self.device)
