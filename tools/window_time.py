#!/usr/bin/env python3
"""Time windowed acoustic inference against what a caller could do without it, on one MI355X.

Two shapes, 1 clip x 1000 frames and 64 clips x 30 frames, window W = 4, engines bf16x3 and fp32:

* ``latest``   (a) ``bilstm_windowed(feats, lens, 4, "latest")``
* ``mean``     (b) ``bilstm_windowed(feats, lens, 4, "mean")``
* ``gather``   (c) the only route to the FULL windows without this mode: gather (S, 4, 208) windows in torch and
               call ``bilstm`` (the persistent recurrence kernels, 64 sequences a launch), the gather included;
               it cannot give the warm-up rows, a context or ``mean``
* ``windowed_frames`` / ``dense_frames``  (d) ``forward_windowed`` against the whole-clip dense ``forward`` on
               the same 256 x 256 frames (the CNN included)

The versions of a group alternate inside one timed loop after a warm-up of all of them; each sample is one pair of
device events around ``--group`` back-to-back calls of one version (a single call of (a) is tens of microseconds,
below what one event pair resolves), and the warm median per call is reported with the 10th / 90th percentiles.
``kernels`` holds one profiled call of (a) and of (c): per kernel name, launches and summed event time.
Writes one JSON file (default profiles/window_time.json).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

W = 4
SHAPES = [(1, 1000), (64, 30)]
HW = (256, 256)


def timed(fns, warmup, samples, group):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(samples)]
          for k in fns}
    for i in range(samples):
        for k, f in fns.items():
            a, b = ev[k][i]
            torch.cuda.synchronize()
            a.record()
            for _ in range(group):
                f()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) / group for a, b in v]) for k, v in ev.items()}


def stats(v):
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}


def kernels(native, f):
    native.prof_enable(True)
    try:
        native.prof_launches()
        f()
        torch.cuda.synchronize()
        rec = native.prof_launches()
    finally:
        native.prof_enable(False)
    out = {}
    for r in rec:
        e = out.setdefault(r["name"], {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += r["ms"]
    return out


def sha():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source snapshot without git
        return "unknown"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_time.json"))
    ap.add_argument("--source", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--frame-samples", type=int, default=8, help="samples of the frame-level pair (d), group 1")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("window_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import _native, runtime, synth
    dev = torch.device("cuda", 0)
    sd = synth.synth_acoustic_state(2)
    res = {"device": torch.cuda.get_device_name(0), "source": a.source or sha(), "window": W, "warmup": a.warmup,
           "samples": a.samples, "group": a.group, "rows": []}
    for dtype in ("bf16x3", "fp32"):
        eng = runtime.AcousticEngine(sd, dtype=dtype, device=dev)
        for B, T in SHAPES:
            lens = [T] * B
            g = torch.Generator().manual_seed(B)
            feats = torch.randn(B * T, 208, generator=g).to(dev)
            idx = (torch.arange(T - W + 1)[:, None] + torch.arange(W)[None]).to(dev)  # full windows of one clip

            def gather():
                blk = feats.view(B, T, 208)[:, idx].reshape(B * (T - W + 1), W, 208)
                return eng.bilstm(blk)[1][:, -1]

            fns = {"latest": lambda: eng.bilstm_windowed(feats, lens, W, "latest")[1],
                   "mean": lambda: eng.bilstm_windowed(feats, lens, W, "mean")[1], "gather": gather}
            full = torch.cat([torch.arange(b * T + W - 1, (b + 1) * T) for b in range(B)]).to(dev)
            diff = float((fns["latest"]()[full] - gather()).abs().max())
            ms = timed(fns, a.warmup, a.samples, a.group)
            row = {"dtype": dtype, "B": B, "T": T, "windows_latest": B * T, "windows_full": B * (T - W + 1),
                   "latest_vs_gather_max_abs": diff, **{k: stats(v) for k, v in ms.items()}}
            row["gather_over_latest"] = row["gather"]["median_ms"] / row["latest"]["median_ms"]
            row["kernels"] = {"latest": kernels(_native, fns["latest"]), "gather": kernels(_native, gather)}
            frames = torch.rand(B * T, *HW, generator=torch.Generator().manual_seed(T)).to(dev)
            ffns = {"windowed_frames": lambda: eng.forward_windowed(frames, lens, W, "latest"),
                    "dense_frames": lambda: eng.forward(frames.view(B, T, *HW))}
            fms = timed(ffns, 2, a.frame_samples, 1)
            row.update({k: stats(v) for k, v in fms.items()})
            row["windowed_over_dense_frames"] = row["windowed_frames"]["median_ms"] / row["dense_frames"]["median_ms"]
            eng.check()
            del frames
            res["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "kernels"}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
