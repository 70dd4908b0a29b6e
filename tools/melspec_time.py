#!/usr/bin/env python3
"""Time the mel-spectrogram engine against the torch composition a user would write today, on one MI355X.

For each shape (8 x 420 000 samples = configs[4]'s 8 clips x 1000 frames, and 1 x 12 600 samples = one clip of 30
frames) at the HiFi-GAN config (2048 / 420 / 2048, 64 mels, sr 11413, fmax 8000):

* ``m2s``    ``MelSpectrogram.hifigan(h).forward(wav)``: one call = the DFT/mel kernel and the reduction kernel
* ``torch``  ``F.pad(reflect)`` + ``torch.stft`` (rocFFT) + ``sqrt(re^2 + im^2 + 1e-9)`` + matmul + ``log(clamp)``

Every call is bracketed by its own pair of device events on the current stream; the two versions alternate inside
one timed loop after a warm-up of both, and the median over the timed calls is reported with the 10th and 90th
percentiles.  ``gemm_tflops`` is the DFT counted as the GEMM the kernel runs (2 * rows * n_fft * 2 * bins) plus
the mel projection over the median time, and ``mfma_peak_frac`` its share of the 157.3 TFLOP/s fp32 MFMA peak.
Also reports the worst |difference| of the two results.  Writes one JSON file (default profiles/melspec_time.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H = dict(n_fft=2048, num_mels=64, sampling_rate=11413, hop_size=420, win_size=2048, fmin=0, fmax=8000)
SHAPES = [(8, 420000), (1, 12600)]
F32_MFMA_PEAK = 157.3e12


def torch_composition(wav, basis, window, h):
    p = (h["n_fft"] - h["hop_size"]) // 2
    y = torch.nn.functional.pad(wav[:, None], (p, p), mode="reflect")[:, 0]
    s = torch.stft(y, h["n_fft"], hop_length=h["hop_size"], win_length=h["win_size"], window=window, center=False,
                   normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-9)
    return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5))


def timed(fns, warmup, calls):
    """fns: name -> callable; the versions alternate; per-call event times in ms."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
          for k in fns}
    for i in range(calls):
        for k, f in fns.items():
            a, b = ev[k][i]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "melspec_time.json"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("melspec_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s.melspec import MelSpectrogram, slaney_mel_basis
    dev = torch.device("cuda", 0)
    eng = MelSpectrogram.hifigan(H, device=dev)
    basis = torch.from_numpy(slaney_mel_basis(H["sampling_rate"], H["n_fft"], H["num_mels"], H["fmin"], H["fmax"])).to(dev)
    window = torch.hann_window(H["win_size"], device=dev)
    res = {"device": torch.cuda.get_device_name(0), "config": H, "warmup": a.warmup, "calls": a.calls, "shapes": []}
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(B)
        wav = (0.2 * torch.randn(B, L, generator=g)).clamp(-1, 1).to(dev)
        T, bins = eng.frames(L), H["n_fft"] // 2 + 1
        fns = {"m2s": lambda: eng.forward(wav), "torch": lambda: torch_composition(wav, basis, window, H)}
        diff = float((fns["m2s"]() - fns["torch"]()).abs().max())
        ms = timed(fns, a.warmup, a.calls)
        flops = 2.0 * B * T * H["n_fft"] * 2 * bins + 2.0 * B * T * bins * H["num_mels"]
        row = {"B": B, "L": L, "frames": T, "gemm_flops": flops, "max_abs_diff_ln": diff}
        for k, v in ms.items():
            row[k] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                      "p90_ms": float(np.percentile(v, 90))}
        row["gemm_tflops"] = flops / (row["m2s"]["median_ms"] * 1e-3) / 1e12
        row["mfma_peak_frac"] = row["gemm_tflops"] * 1e12 / F32_MFMA_PEAK
        row["torch_over_m2s"] = row["torch"]["median_ms"] / row["m2s"]["median_ms"]
        res["shapes"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
