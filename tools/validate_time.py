#!/usr/bin/env python3
"""Time checkpoint validation on the training pairs against what a caller could do without it, on one MI355X.

Two routes to the same numbers, on the same box in the same process, at window = 4, 256 x 256 frames, on
8 clips x 30 frames and 1 clip x 1000 frames:

* ``fused``   (a) ``forward_pairs`` (the CNN once per frame, the BiLSTM on every window, every row kept) plus ONE
              ``torch.ops.m2s.mel_metrics`` call over all P pairs in groups of 8;
* ``gather``  (b) what the engine offered before: gather the P windows of frames into (P, 4, H, W), run the dense
              ``forward`` on them (every frame goes through the CNN up to 4 times), then the reference's criterion,
              band MAEs and eval_mel's masked losses written in torch on the device, one batch of 8 at a time with
              the reference's three ``.item()`` calls per batch.  The MCD-like is NOT part of (b): the reference
              computes it on the host through librosa, which would only make (b) slower.

Also timed alone: the ``mel_metrics`` call and the torch criterion loop on the same predictions.  ``launches`` are the
engine's recorded kernel launches of one call of (a); ``torch_ops`` the ATen operators one pass of the torch criterion
dispatches (about one kernel launch each).  Each sample is one pair of device events around one call; the warm
median is reported with the 10th / 90th percentiles.  Writes one JSON file (default profiles/validate_time.json).
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
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

W = 4
GROUP = 8
SHAPES = [(8, 30), (1, 1000)]
HW = (256, 256)


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def torch_criterion(pred, target, mask, fw, tw, coeffs, bands):
    """The reference's per-batch numbers in torch ops (train_mri_acoustic_model.py:112-167,263-277, eval_mel.py:24-32),
    with the reference's host reads."""
    B, T, M = pred.shape
    fwv, twv = fw.view(1, 1, M), tw.view(1, T, 1)
    mk = mask.unsqueeze(-1)
    diff = pred - target
    w = (fwv * twv).expand(B, T, M) * mk
    den = w.sum().clamp_min(1e-6)
    mse, mae = torch.sum(diff ** 2 * w) / den, torch.sum(diff.abs() * w) / den
    d = diff[:, 1:] - diff[:, :-1]
    dw = (fwv * twv[:, 1:]).expand(B, T - 1, M) * mk[:, 1:] * mk[:, :-1]
    delta = torch.sum(d ** 2 * dw) / dw.sum().clamp_min(1e-6)
    a = diff[:, 2:] - 2 * diff[:, 1:-1] + diff[:, :-2]
    aw = (fwv * twv[:, 1:T - 1]).expand(B, T - 2, M) * mk[:, 2:] * mk[:, 1:-1] * mk[:, :-2]
    accel = torch.sum(a ** 2 * aw) / aw.sum().clamp_min(1e-6)
    lw = fwv.expand(B, 1, M)
    latest = torch.sum(diff[:, -1] ** 2 * lw[:, 0]) / lw.sum().clamp_min(1e-6)
    loss = mse + coeffs[0] * delta + coeffs[1] * accel + coeffs[2] * latest
    out = [loss.item(), mse.item(), mae.item()]
    for s, e in bands:
        out.append(float(torch.mean(torch.abs(pred[..., s:e] - target[..., s:e])).item()))
    e = diff * mk
    eden = mk.sum().clamp_min(1.0)
    emse, emae = (e ** 2).sum() / eden, e.abs().sum() / eden
    out += [(0.8 * emse + 0.2 * emae).item(), emse.item(), emae.item()]
    return out


def criterion_loop(pred, target, mask, fw, tw, coeffs, bands):
    tot = np.zeros(10)
    n = 0
    for i in range(0, pred.shape[0], GROUP):
        tot += torch_criterion(pred[i:i + GROUP], target[i:i + GROUP], mask[i:i + GROUP], fw, tw, coeffs, bands)
        n += 1
    return tot / n


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


def launches(native, f):
    native.prof_enable(True)
    try:
        native.prof_launches()
        f()
        torch.cuda.synchronize()
        rec = native.prof_launches()
    finally:
        native.prof_enable(False)
    by_stage = {}
    for r in rec:
        by_stage[r["stage"]] = by_stage.get(r["stage"], 0) + 1
    return {"total": len(rec), "by_stage": by_stage}


def sha():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source snapshot without git
        return "unknown"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "validate_time.json"))
    ap.add_argument("--source", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--dtype", default="bf16x3")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("validate_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import _native, metrics, runtime, synth
    dev = torch.device("cuda", 0)
    mean, std = synth.synth_scaler()
    eng = runtime.AcousticEngine(synth.synth_acoustic_state(2), dtype=a.dtype, device=dev)
    fw_np, tw_np, coeffs, bands = metrics.train_weights(64, W, 1.0)
    fw, tw = torch.from_numpy(fw_np).to(dev), torch.from_numpy(tw_np).to(dev)
    band_list = [bands[k] for k in metrics.BAND_NAMES]
    res = {"device": torch.cuda.get_device_name(0), "source": a.source or sha(), "window": W, "group": GROUP,
           "dtype": a.dtype, "warmup": a.warmup, "samples": a.samples, "rows": []}
    for B, T in SHAPES:
        lens = [T] * B
        frames = torch.rand(B * T, *HW, generator=torch.Generator().manual_seed(T)).to(dev)
        idx = metrics.pair_index(lens, W, dev)
        P = int(idx.shape[0])
        target = torch.randn(B * T, 64, generator=torch.Generator().manual_seed(B)).to(dev)[idx]
        mask = torch.ones(B * T, device=dev)[idx]
        mm = metrics.MelMetrics(64, mean, std, device=dev)

        def fused():
            mm.reset()
            return mm.update(eng.forward_pairs(frames, lens, W), target, mask, group=GROUP)

        def gather():
            pred = eng.forward(frames[idx])  # (P, W, H, W): every frame up to W times through the CNN
            return criterion_loop(pred, target, mask, fw, tw, coeffs, band_list)

        pred = eng.forward_pairs(frames, lens, W)

        def metrics_only():
            mm.reset()
            return mm.update(pred, target, mask, group=GROUP)

        def criterion_only():
            return criterion_loop(pred, target, mask, fw, tw, coeffs, band_list)

        got, want = fused().compute(), gather()
        agree = {"loss": [got["loss"], float(want[0])], "mse": [got["mse"], float(want[1])],
                 "eval_mse": [got["eval"]["mse"], float(want[8])]}
        ms = timed({"fused": fused, "gather": gather, "metrics_only": metrics_only, "criterion_only": criterion_only},
                   a.warmup, a.samples)
        with OpCounter() as oc:
            criterion_only()
        row = {"B": B, "T": T, "pairs": P, "agree_fused_vs_gather": agree, **{k: stats(v) for k, v in ms.items()},
               "launches_fused": launches(_native, fused), "launches_gather_engine": launches(_native, lambda: eng.forward(frames[idx])),
               "torch_ops_criterion": oc.n, "batches": (P + GROUP - 1) // GROUP}
        row["gather_over_fused"] = row["gather"]["median_ms"] / row["fused"]["median_ms"]
        row["criterion_over_metrics"] = row["criterion_only"]["median_ms"] / row["metrics_only"]["median_ms"]
        eng.check()
        res["rows"].append(row)
        print(json.dumps(row))
        del frames
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
