#!/usr/bin/env python3
"""Time the Grad-CAM engine against the autograd route a caller had before it, on one MI355X.

Two bands (mel bins 9..20 and 21..38, the tool's default F1 / F2) on one 256 x 256 clip, exact fp32, at
(T frames, F target frames) = (30, 0), (30, 8), (300, 8), (1000, 16):

* ``engine``    one ``m2s.gradcam.GradCam.run`` over both bands: one train-mode forward, the 2 (1 + F) cotangents
                through the backward together, heat maps on the device
* ``autograd``  what a caller does without it: the plug-in in ``train()``, per band the module calls of the
                reference's compute_gradcam (backbone, mean, rnn, head, band power), one ``backward()`` per target
                and the torch heat-map loop over T

Both are warmed up first, then alternate inside one timed loop, each sample one pair of device events around one
call; the warm median is reported with the 10th / 90th percentiles.  ``kernels`` holds one profiled call of each
(torch.profiler device activity): per kernel name, launches and summed device time, and ``launches`` their totals;
``trace_incomplete`` marks a trace that lost events (its device time is under half the timed call).
At every shape the two routes' heat maps must agree within 1e-4 (asserted; the worst difference is recorded).
Writes one JSON file (default profiles/gradcam_time.json); ``--append`` adds rows to an existing file, so each shape
can run as a step of its own.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mri-to-speech_amd", "mri2speech_code"), os.path.join(REPO, "mri-to-speech_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(30, 0), (30, 8), (300, 8), (1000, 16)]
BANDS = {"F1": list(range(9, 21)), "F2": list(range(21, 39))}
HW = (256, 256)
SAMPLES = {30: 10, 300: 5, 1000: 3}


def heatmaps_torch(feats, grads, T, hw):
    """The reference's heat-map arithmetic as torch ops: one interpolate and one min-max per frame."""
    w = grads.mean(dim=(2, 3), keepdim=True)
    cam = torch.relu((w * feats).sum(dim=1, keepdim=True)).view(1, T, *feats.shape[-2:]).detach()
    out = []
    for t in range(T):
        c = F.interpolate(cam[:, t].unsqueeze(1), size=hw, mode="bilinear", align_corners=False).squeeze(1)
        c = c - c.amin(dim=(-2, -1), keepdim=True)
        out.append(c / (c.amax(dim=(-2, -1), keepdim=True) + 1e-6))
    return torch.stack(out, dim=1).squeeze(0)


def autograd_route(model, frames, mean, std, bands, targets):
    """frames (1,T,1,H,W); per band a train-mode forward, a backward per target, the torch heat-map loop."""
    T = frames.shape[1]
    hw = tuple(frames.shape[-2:])
    res = {}
    for name, idx in bands.items():
        model.train()
        model.rnn.dropout.train(False)
        x = frames.reshape(T, *frames.shape[2:]).repeat(1, 3, 1, 1)
        feats = model.cnn.backbone(x)[-1].requires_grad_(True)
        feats.retain_grad()
        pred = model.head(model.rnn(feats.mean(dim=(2, 3)).view(1, T, -1)))
        power = torch.pow(10.0, (pred * std + mean) / 10.0)
        band_power = power.index_select(-1, torch.as_tensor(idx, device=frames.device)).sum(-1)
        model.zero_grad(set_to_none=True)
        band_power.mean().backward(retain_graph=bool(targets))
        maps = heatmaps_torch(feats.detach(), feats.grad.detach().clone(), T, hw)
        per = {}
        for i, t in enumerate(targets):
            model.zero_grad(set_to_none=True)
            feats.grad.zero_()
            band_power[:, t].mean().backward(retain_graph=i < len(targets) - 1)
            per[t] = heatmaps_torch(feats.detach(), feats.grad.detach().clone(), T, hw)[t]
        model.eval()
        res[name] = (maps, per)
    return res


def timed(fns, warmup, samples):
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
            f()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def stats(v):
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}


def kernels(f):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        us = getattr(e, "device_time_total", None)
        if us is None:
            us = getattr(e, "cuda_time_total", 0.0)
        if us <= 0:
            continue
        name = e.key.replace("(anonymous namespace)::", "").removeprefix("void ").split("(")[0][:96]
        k = out.setdefault(name, {"launches": 0, "ms": 0.0})
        k["launches"] += int(e.count)
        k["ms"] += us / 1e3
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms"]))


def sha():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source snapshot without git
        return "unknown"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gradcam_time.json"))
    ap.add_argument("--source", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--shape", type=int, nargs=2, action="append", metavar=("T", "F"),
                    help="time only this (frames, target frames) shape; repeatable (default: all four)")
    ap.add_argument("--append", action="store_true", help="add the rows to an existing --out file")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=0, help="samples per version (default: 10 / 5 / 3 by clip length)")
    ap.add_argument("--no-kernels", action="store_true", help="skip the profiled calls")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gradcam_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import synth
    from m2s.gradcam import GradCam
    from mri_acoustic_model import build_acoustic_model
    dev = torch.device("cuda", 0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_acoustic_state(3).items()}
    model = build_acoustic_model(n_mels=64, cnn_pretrained=False, rnn_hidden=640, dropout=0.5).to(dev)
    model.load_state_dict(sd, strict=False)
    model.eval()
    cam = GradCam(sd, dev)
    mean_np, std_np = synth.synth_scaler()
    mean, std = torch.from_numpy(mean_np).to(dev), torch.from_numpy(std_np).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "source": a.source or sha(), "bands": BANDS, "frame": list(HW),
           "chunk": cam.chunk, "warmup": a.warmup, "rows": []}
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            res["rows"] = json.load(f)["rows"]
    for T, nf in [tuple(s) for s in (a.shape or SHAPES)]:
        frames = torch.from_numpy(synth.synth_frames(1, T, hw=HW, seed=T)).to(dev)
        targets = [int(t) for t in np.linspace(0, T - 1, nf).round()] if nf else []
        fns = {"engine": lambda: cam.run(frames[0], mean, std, BANDS, "mean", targets, return_dpooled=False),
               "autograd": lambda: autograd_route(model, frames[:, :, None], mean, std, BANDS, targets)}
        new, old = fns["engine"](), fns["autograd"]()
        worst = 0.0
        for name in BANDS:
            worst = max(worst, float((new[name]["heatmaps"] - old[name][0]).abs().max()))
            for t in targets:
                worst = max(worst, float((new[name]["per_frame"][t] - old[name][1][t]).abs().max()))
        assert worst <= 1e-4, f"T={T} F={nf}: the two routes' heat maps differ by {worst:.3e}"
        del new, old
        samples = a.samples or SAMPLES.get(T, 5)
        ms = timed(fns, a.warmup, samples)
        K = len(BANDS) * (1 + nf)
        row = {"T": T, "F": nf, "targets": K, "samples": samples, "heatmap_max_abs_diff": worst,
               **{k: stats(v) for k, v in ms.items()}}
        row["autograd_over_engine"] = row["autograd"]["median_ms"] / row["engine"]["median_ms"]
        if not a.no_kernels:
            row["kernels"] = {k: kernels(f) for k, f in fns.items()}
            row["launches"] = {k: sum(e["launches"] for e in v.values()) for k, v in row["kernels"].items()}
            # a trace whose device time is under half the timed call lost events (the profiler's buffer): say so
            row["trace_incomplete"] = {k: sum(e["ms"] for e in v.values()) < 0.5 * row[k]["median_ms"]
                                       for k, v in row["kernels"].items()}
        res["rows"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
        del frames
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
