#!/usr/bin/env python3
"""Micro-benchmark of adamml_log_spectrogram (the sound input of load_sound, utils/video_dataset.py:93-132) against the torch.stft
composite (torch.stft + |X|^2 + log, ROCm) on the same data in the same process.

N = 360 clips is one C2 step's sound input (B*S = 72*5), N = 45 the per-GPU share of the reference recipe (B = 9).  Each clip is
L = 30720 samples (1.28 s at 24 kHz), n_fft 511, win 240, hop 120 -> a 256 x 256 fp32 image.  Counted work: the GEMM of the windowed
cos/sin basis with the frames, 2*N*T*win*2F FLOP (the log and the power are not counted); counted bytes: the waveforms in and the
images out (the 480 KiB basis is read from L2).  Times: device events around `--iters` back-to-back calls, after `--warmup`
calls, median of `--repeats` windows.  Prints one line per (N, path) and a JSON summary line.
Usage: python tools/bench_spectrogram.py [--iters 50] [--repeats 7] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adamml_amd import audio  # noqa: E402

PEAK_TF = 157.3          # fp32 matrix peak (MI355X_MICROARCH.md)
PEAK_GBS = 8000.0        # HBM
L, N_FFT, WIN, HOP, EPS = 30720, 511, 240, 120, 1e-6


def timed(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / iters)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="360,45")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectrogram: no GPU (there is no CPU measurement path)")
    dev = "cuda"
    window = torch.hann_window(WIN, periodic=True, dtype=torch.float32, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "rows": []}
    for n in [int(v) for v in a.sizes.split(",")]:
        wave = torch.randn(n, L, generator=torch.Generator().manual_seed(n)).mul_(0.1).to(dev)
        T = 1 + (L + 2 * (N_FFT // 2) - N_FFT) // HOP
        F = N_FFT // 2 + 1
        flop = 2.0 * n * T * WIN * 2 * F
        nbytes = 4.0 * n * (L + F * T)

        def hip_path():
            return audio.log_spectrogram(wave, n_fft=N_FFT)

        def torch_path():
            X = torch.stft(wave, n_fft=N_FFT, hop_length=HOP, win_length=WIN, window=window, center=True, pad_mode="constant",
                           return_complex=True)
            return torch.log(X.abs() ** 2 + EPS)

        y_h, y_t = hip_path(), torch_path()
        diff = float((y_h - y_t).abs().max())
        for name, fn in (("hip", hip_path), ("torch.stft", torch_path)):
            med, lo, hi = timed(fn, a.iters, a.repeats, a.warmup)
            tf = flop / (med * 1e-3) / 1e12
            gbs = nbytes / (med * 1e-3) / 1e9
            floor_ms = max(flop / (PEAK_TF * 1e12), nbytes / (PEAK_GBS * 1e9)) * 1e3
            row = {"N": n, "path": name, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "tflops": round(tf, 2),
                   "pct_fp32_matrix_peak": round(100 * tf / PEAK_TF, 1), "gbs": round(gbs, 1), "floor_ms": round(floor_ms, 4)}
            out["rows"].append(row)
            print("N=%4d %-11s %8.4f ms (min %.4f max %.4f)  %6.2f TF/s = %5.1f %% of %.0f TF  %7.1f GB/s  (floor %.4f ms)"
                  % (n, name, med, lo, hi, tf, row["pct_fp32_matrix_peak"], PEAK_TF, gbs, floor_ms))
        print("N=%4d max |hip - torch.stft| in log = %.3g" % (n, diff))
        out["rows"][-1]["max_abs_log_diff_vs_hip"] = diff
    print(json.dumps(out))


if __name__ == "__main__":
    main()
