"""The sound spectrogram on the GPU (adamml_log_spectrogram, adamml_amd.audio): within the float64 error model of
tests/spectrogram_ref.py on every kind of input a loader produces, reproducible, NaN-propagating per frame, argument-checked,
replayable from a launch plan, and fed to AdaMML as raw waveforms it gives bit for bit what the spectrogram input gives."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import adamml, audio, hip, plan, runtime, synth  # noqa: E402
from tests import spectrogram_ref as R  # noqa: E402

DEV = "cuda"
L = 30720


def _gpu(x, **kw):
    return audio.log_spectrogram(torch.as_tensor(np.asarray(x, dtype=np.float32)).to(DEV), **kw).cpu().numpy()


def _check_rows(name, xs, ys, n_fft=511, win=240, hop=120):
    worst = max(R.check(y, x, n_fft, win, hop) for x, y in zip(xs, ys))
    print("  %-28s max err/tol = %.4f" % (name, worst))
    assert worst <= 1.0, name


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def test_white_noise():
    xs = _f32(np.random.default_rng(0).standard_normal((8, L)) * 0.1)
    ys = _gpu(xs)
    assert ys.shape == (8, 256, 256) and ys.dtype == np.float32
    _check_rows("white noise", xs, ys)


def test_sinusoids_on_and_between_bins():
    t = np.arange(L)
    xs = _f32([np.sin(2 * np.pi * k * t / 511 + 0.3) for k in (0.0, 1.0, 37.0, 37.5, 100.25, 255.0, 255.5)])
    _check_rows("sinusoids", xs, _gpu(xs))


def test_silence_is_exactly_log_eps():
    y = _gpu(np.zeros((3, L)))
    want = np.float32(math.log(np.float32(1e-6)))                # the correctly rounded logf(1e-6f)
    v = np.unique(y)
    print("  silence ->", v, "want", want)
    assert v.size == 1 and abs(int(v[0].view(np.int32)) - int(want.view(np.int32))) <= 1
    # and the device's own logf(1e-6f)
    assert v[0] == torch.log(torch.tensor([1e-6], dtype=torch.float32, device=DEV)).item()


def test_int16_scale_amplitude():
    rng = np.random.default_rng(1)
    xs = np.clip(rng.standard_normal((4, L)) * 8000.0, -32768, 32767).round()
    xs[1, :5000] = 32767.0                                        # a clipped (constant) stretch
    xs[2] = np.round(20000 * np.sin(2 * np.pi * 440.0 * np.arange(L) / 24000))
    xs = _f32(xs)
    _check_rows("int16 scale", xs, _gpu(xs))


def test_tiled_short_track():
    rng = np.random.default_rng(2)
    track = rng.standard_normal(7001).astype(np.float32)
    xs = _f32([audio.sound_window(track, idx, 0) for idx in (0, 3)])
    np.testing.assert_array_equal(xs[0][:7001], track)
    _check_rows("tiled short track", xs, _gpu(xs))


def test_n360_default_recipe():
    rng = np.random.default_rng(3)
    xs = rng.standard_normal((360, L)).astype(np.float32) * np.float32(0.05)
    xs[::7, 10000:20000] = 0                                    # some silent stretches
    ys = _gpu(xs)
    assert ys.shape == (360, 256, 256)
    _check_rows("N = 360", _f32(xs[::5]), ys[::5])


def test_16khz_parameters():
    xs = _f32(np.random.default_rng(4).standard_normal((3, 20480)))
    ys = _gpu(xs, sample_rate=16000)
    assert ys.shape == (3, 256, 256)
    _check_rows("16 kHz (win 160, hop 80)", xs, ys, win=160, hop=80)


@pytest.mark.parametrize("n_fft,win,hop,length", [(256, 200, 64, 5000), (128, 101, 150, 3001), (512, 512, 1, 300), (2, 1, 1, 1)])
def test_other_sizes_through_the_function(n_fft, win, hop, length):
    """Non-square images, odd windows, hop > win (frames packed), the n_fft bound and the smallest case."""
    xs = _f32(np.random.default_rng(5).standard_normal((2, length)))
    ys = runtime.log_spectrogram(torch.from_numpy(xs.astype(np.float32)).to(DEV), n_fft, win, hop, 1e-6).cpu().numpy()
    assert ys.shape == (2,) + R.sizes(length, n_fft, hop)
    _check_rows("n_fft %d win %d hop %d L %d" % (n_fft, win, hop, length), xs, ys, n_fft, win, hop)


def test_two_runs_are_bitwise_identical():
    x = torch.randn(45, L, device=DEV)
    a, b = audio.log_spectrogram(x), audio.log_spectrogram(x)
    assert torch.equal(a, b)


def test_nan_reaches_exactly_its_frames():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, L)).astype(np.float32)
    clean = _gpu(x)
    bad = x.copy()
    for s in (0, 5000, 5040, L - 1):
        bad[1, s] = np.nan
    bad[0, 777] = np.inf
    y = _gpu(bad)
    for clip, samples in ((0, (777,)), (1, (0, 5000, 5040, L - 1))):
        # frame t covers samples 120 t - 120 .. 120 t + 119
        hit = sorted({t for s in samples for t in range(256) if 120 * t - 120 <= s <= 120 * t + 119})
        bad_cols = np.where(~np.isfinite(y[clip]).all(axis=0))[0].tolist()
        assert bad_cols == hit, (clip, bad_cols, hit)
        if clip == 1:
            assert np.isnan(y[clip][:, hit]).all()
        else:                                                    # Inf: +Inf power, NaN where a basis value is 0 (sine of bin 0)
            assert not np.isfinite(y[clip][:, hit]).any() and np.isnan(y[clip][0, hit]).all()
        keep = [t for t in range(256) if t not in hit]
        assert np.array_equal(y[clip][:, keep], clean[clip][:, keep])


def test_bad_arguments_raise_with_the_library_message():
    x = torch.randn(2, 1000, device=DEV)
    for kw, msg in (((1024, 240, 120, 1e-6), "n_fft = 1024 outside"), ((511, 600, 120, 1e-6), "win = 600 outside"),
                    ((511, 0, 120, 1e-6), "win = 0 outside"), ((511, 240, 0, 1e-6), "hop = 0"),
                    ((511, 240, 120, -1.0), "eps must be >= 0")):
        with pytest.raises(RuntimeError, match=msg):
            runtime.log_spectrogram(x, *kw)
    with pytest.raises(RuntimeError, match="null argument"):
        hip.call("adamml_log_spectrogram", None, None, None, 1, 1000, 511, 240, 120, 1e-6)
    with pytest.raises(RuntimeError, match="bad N"):
        hip.call("adamml_log_spectrogram", None, None, None, -1, 1000, 511, 240, 120, 1e-6)
    hip.call("adamml_log_spectrogram", None, None, None, 0, 1000, 511, 240, 120, 1e-6)         # N == 0: a no-op
    with pytest.raises(TypeError):
        audio.log_spectrogram(torch.zeros(2, L, dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        audio.log_spectrogram(torch.zeros(2, L))
    # other floating dtypes and strided input are converted
    x = torch.randn(3, 2 * L, device=DEV)
    ref = audio.log_spectrogram(x[:, ::2].contiguous())
    assert torch.equal(audio.log_spectrogram(x[:, ::2]), ref)
    assert audio.log_spectrogram(x[:, ::2].double()).shape == ref.shape


def test_replays_from_a_launch_plan():
    x1, x2 = torch.randn(4, L, device=DEV), torch.randn(4, L, device=DEV)
    audio.log_spectrogram(x1)                                      # basis cached
    rec = plan.Recorder(x1)
    hip.recorder = rec
    try:
        y = runtime.log_spectrogram(x1, 511, 240, 120, 1e-6)
    finally:
        hip.recorder = None
    assert rec.failed is None and len(rec.cur) == 1
    rec.end_forward()
    p = plan.Plan(rec, y)
    out, _ = p.forward(x2)
    assert torch.equal(out, audio.log_spectrogram(x2))


# ---- AdaMML fed raw waveforms ---------------------------------------------------------------------------------------------------

def _model(S, sd=None):
    model = adamml(groups=8, modality=["rgb", "sound"], input_channels=[3, 1], num_segments=S, rng_policy=False, rng_threshold=0.5,
                   causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.0, pooling_method="max",
                   fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True, resampling_rate=24000,
                   audio_length=1.28)
    sd = sd or synth.synth_state_dict(model.state_dict(), seed=1234)
    model.load_state_dict(sd)
    return model.to(DEV), sd


def _inputs(B, S):
    rgb = synth.synth_inputs(["rgb"], B, S, 8, 64, seed=5)[0].to(DEV)
    wave = (torch.randn(B, S, L, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    expo = synth.synth_gumbel_exponential(S, 2, B, seed=11).to(DEV)
    return rgb, wave, expo


def test_adamml_waveform_input_train_is_bitwise_the_spectrogram_input():
    B, S = 2, 2
    rgb, wave, expo = _inputs(B, S)
    spec = audio.log_spectrogram(wave)
    assert spec.shape == (B, S, 256, 256)
    res = []
    sd = None
    for snd in (wave, spec):
        model, sd = _model(S, sd)
        model.freeze_policy_net()
        model.train()
        logits, sel = model([rgb, snd], gumbel_exponential=expo)
        logits.sum().backward()
        torch.cuda.synchronize()
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        res.append((logits.detach().clone(), sel.detach().clone(), grads))
    (la, da, ga), (lb, db, gb) = res
    assert torch.equal(la, lb) and torch.equal(da, db)
    assert len(ga) == len(gb) > 0 and all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_adamml_waveform_input_eval_skipping():
    B, S = 2, 2
    rgb, wave, expo = _inputs(B, S)
    model, _ = _model(S)
    model.eval()
    assert model.skip_unselected
    with torch.no_grad():
        a, da = model([rgb, wave], gumbel_exponential=expo)
        b, db = model([rgb, audio.log_spectrogram(wave)], gumbel_exponential=expo)
    assert model.last_skip_stats is not None
    assert torch.equal(a, b) and torch.equal(da, db)


def test_adamml_rejects_a_wrong_waveform_length():
    B, S = 2, 2
    rgb, wave, expo = _inputs(B, S)
    model, _ = _model(S)
    model.eval()
    with torch.no_grad(), pytest.raises(ValueError, match="30720"):
        model([rgb, wave[..., :-1]], gumbel_exponential=expo)
