#!/usr/bin/env python3
"""Time the device frame front end against the route a caller takes without it, on one MI355X.

From pinned host uint8 frames to fp32 model input on the device, for 1 x 30 and 8 x 1000 frames of 84 x 84 going to
256 x 256:

* ``fused``   upload of the native 84 x 84 frames (7 KB each) + ``preprocess_frames(x, (256, 256))``: grey, resize
              and normalisation in one kernel (csrc/frames.hip)
* ``today``   upload of frames a host resize already brought to 256 x 256 (64 KB each) + ``preprocess_frames(x)``.
              The host resize itself (cv2.resize, a serial per-frame loop) is NOT in this time: the figure is the
              device-side part of today's route only.
* ``kernel``  the fused call alone on frames already on the device, against its store-bound floor: 4 * H * W bytes a
              frame over the HBM rate (8.0 TB/s specified, 6.3 TB/s as a float4 copy reaches)

Every call is bracketed by its own pair of device events on the current stream; the versions alternate inside one
timed loop after a warm-up of all, and the median over the timed calls is reported with the 10th and 90th
percentiles.  Writes one JSON file (default profiles/frames_time.json).
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

SHAPES = [(1, 30), (8, 1000)]
SRC, DST = (84, 84), (256, 256)
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frames_time.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("frames_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import runtime
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "source": SRC, "destination": DST, "warmup": a.warmup,
           "calls": a.calls, "hbm_spec_Bps": HBM_SPEC, "hbm_copy_Bps": HBM_COPY, "shapes": []}
    for clips, T in SHAPES:
        n = clips * T
        g = torch.Generator().manual_seed(n)
        native = torch.randint(0, 256, (n, *SRC), dtype=torch.uint8, generator=g).pin_memory()
        resized = torch.randint(0, 256, (n, *DST), dtype=torch.uint8, generator=g).pin_memory()
        on_dev = native.to(dev)
        fns = {"fused": lambda: runtime.preprocess_frames(native.to(dev, non_blocking=True), DST),
               "today": lambda: runtime.preprocess_frames(resized.to(dev, non_blocking=True)),
               "kernel": lambda: runtime.preprocess_frames(on_dev, DST)}
        ms = timed(fns, a.warmup, a.calls)
        row = {"clips": clips, "frames_per_clip": T, "frames": n,
               "upload_bytes": {"fused": n * SRC[0] * SRC[1], "today": n * DST[0] * DST[1]}}
        for k, v in ms.items():
            row[k] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                      "p90_ms": float(np.percentile(v, 90))}
        out_bytes = 4.0 * n * DST[0] * DST[1]
        row["today_over_fused"] = row["today"]["median_ms"] / row["fused"]["median_ms"]
        row["kernel_floor_ms"] = {"hbm_spec": out_bytes / HBM_SPEC * 1e3, "hbm_copy": out_bytes / HBM_COPY * 1e3}
        row["kernel_store_TBps"] = out_bytes / (row["kernel"]["median_ms"] * 1e-3) / 1e12
        row["kernel_over_floor"] = row["kernel"]["median_ms"] / row["kernel_floor_ms"]["hbm_spec"]
        res["shapes"].append(row)
        print(json.dumps(row))
        del native, resized, on_dev
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
