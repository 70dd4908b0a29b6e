#!/usr/bin/env python3
"""Time one fine-tuning step of the BiLSTM and the mel head (m2s/finetune.py) on one MI355X against the route a
caller had before it, in the same process on the same inputs, at window = 4, 64 mels:

* the reference's loader batch, 8 windows x 4 frames (``lengths = [4] * 8``);
* 8 clips x 1000 frames in one batch (P = 7976 windows).

Routes:

* ``eager``     ``HeadTuner.step`` launched from the host;
* ``graph``     the same step captured once into a graph and replayed;
* ``autograd``  what existed before: ``m2s.autograd.bilstm`` + ``linear`` on the gathered (P, 4, 208) windows, dropout
                and the criterion in torch ops, ``clip_grad_norm_``, ``torch.optim.AdamW`` (one ``.item()``-free step).

Each sample is one pair of device events around one step; the warm median is reported with the 10th / 90th
percentiles.  A separate profiled pass (the engine's per-launch events) gives the time per kernel of one eager step
and the share spent in the BPTT and dW_hh GEMMs; the achieved rate of the recurrent GEMMs is their algorithmic FLOPs
(forward 2 (W - 1) P 640 2560 2, BPTT the same, dW_hh the same) over their kernel time, against the 157.3 TFLOP/s
fp32 MFMA peak.  Writes one JSON file (default profiles/finetune_time.json).
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

W, M = 4, 64
SHAPES = [("loader_8x4", [4] * 8), ("clips_8x1000", [1000] * 8)]
PEAK_F32_MFMA = 157.3e12  # MI355X, v_mfma_f32_32x32x2_f32


def criterion(pred, target, mask, fw, tw, coeffs):
    """LOSS of MaskedMSEMAE in torch ops (train_mri_acoustic_model.py:112-167), no host read."""
    B, T, Mm = pred.shape
    fwv, twv, mk = fw.view(1, 1, Mm), tw.view(1, T, 1), mask.unsqueeze(-1)
    diff = pred - target
    w = fwv * twv * mk
    loss = torch.sum(diff ** 2 * w) / w.sum().clamp_min(1e-6)
    d = diff[:, 1:] - diff[:, :-1]
    dw = fwv * twv[:, 1:] * mk[:, 1:] * mk[:, :-1]
    loss = loss + coeffs[0] * torch.sum(d ** 2 * dw) / dw.sum().clamp_min(1e-6)
    a = diff[:, 2:] - 2 * diff[:, 1:-1] + diff[:, :-2]
    aw = fwv * twv[:, 1:T - 1] * mk[:, 2:] * mk[:, 1:-1] * mk[:, :-2]
    loss = loss + coeffs[1] * torch.sum(a ** 2 * aw) / aw.sum().clamp_min(1e-6)
    lw = fwv.expand(B, 1, Mm)[:, 0]
    return loss + coeffs[2] * torch.sum(diff[:, -1] ** 2 * lw) / lw.sum().clamp_min(1e-6)


def timed(fns, warmup, samples):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(samples)]
          for k in fns}
    for i in range(samples):  # the routes alternate within a sample
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


def sha():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source snapshot without git
        return "unknown"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "finetune_time.json"))
    ap.add_argument("--source", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("finetune_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import _native, autograd, finetune, metrics, synth
    dev = torch.device("cuda", 0)
    sd = {k: v for k, v in synth.synth_acoustic_state(2).items() if k in finetune.KEYS}
    fw_np, tw_np, coeffs, _ = metrics.train_weights(M, W, 1.0)
    fw, tw = torch.from_numpy(fw_np).to(dev), torch.from_numpy(tw_np).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "source": a.source or sha(), "window": W, "n_mels": M,
           "warmup": a.warmup, "samples": a.samples, "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12, "rows": []}
    for name, lens in SHAPES:
        rows = sum(lens)
        g = torch.Generator().manual_seed(rows)
        feats = (0.5 * torch.randn(rows, 208, generator=g)).to(dev)
        target = torch.randn(rows, M, generator=g).to(dev)
        mask = torch.ones(rows, device=dev)
        idx = metrics.pair_index(lens, W, dev)
        P = int(idx.shape[0])
        tun = finetune.HeadTuner(sd, n_mels=M, device=dev, dropout=0.5, lr=1e-4, window=W)
        cap = finetune.HeadTuner(sd, n_mels=M, device=dev, dropout=0.5, lr=1e-4, window=W)
        cap.predict(feats, lens)  # stages the window table
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap.step(feats, target, mask, lens)
        # the route that existed before: torch modules on the device, the project's autograd functions
        lstm = torch.nn.LSTM(208, 640, 1, batch_first=True, bidirectional=True).to(dev)
        head = torch.nn.Linear(640, M).to(dev)
        lstm.load_state_dict({k[len("rnn.lstm."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith("rnn.")})
        head.load_state_dict({"weight": torch.from_numpy(np.asarray(sd["head.weight"])), "bias": torch.from_numpy(np.asarray(sd["head.bias"]))})
        params = list(lstm.parameters()) + list(head.parameters())
        opt = torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)

        def route_autograd():
            opt.zero_grad(set_to_none=True)
            y = torch.nn.functional.dropout(autograd.bilstm(feats[idx], lstm), 0.5, True)
            loss = criterion(autograd.linear(y, head.weight, head.bias), target[idx], mask[idx], fw, tw, coeffs)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
            return loss

        fns = {"eager": lambda: tun.step(feats, target, mask, lens), "graph": graph.replay}
        row = {"shape": name, "lengths": [lens[0], len(lens)], "pairs": P}
        try:
            route_autograd()
            torch.cuda.synchronize()
            fns["autograd"] = route_autograd
        except Exception as e:  # noqa: BLE001 - recorded: the older route may refuse a shape
            row["autograd_error"] = f"{type(e).__name__}: {e}"
        ms = timed(fns, a.warmup, a.samples)
        row.update({k: stats(v) for k, v in ms.items()})
        if "autograd" in ms:
            row["autograd_over_eager"] = row["autograd"]["median_ms"] / row["eager"]["median_ms"]
        # one profiled eager step: the engine's own per-launch events
        _native.prof_enable(True)
        try:
            _native.prof_launches()
            tun.step(feats, target, mask, lens)
            torch.cuda.synchronize()
            rec = _native.prof_launches()
        finally:
            _native.prof_enable(False)
        per = {r["name"]: {"launches": r["launches"], "ms": r["ms"]} for r in _native.aggregate(rec, "name")}
        total = sum(r["ms"] for r in rec)
        flops_rec = 2.0 * (W - 1) * P * 640 * 2560 * 2  # forward recurrence; BPTT and dW_hh are each the same
        hot = {k: per.get(f"ft_gemm_kernel<{k}>", {"ms": 0.0})["ms"] for k in ("recurrent", "bptt", "dwhh")}
        row["profiled"] = {"launches": len(rec), "kernel_ms_total": total, "per_kernel": per,
                           "share_bptt_dwhh": (hot["bptt"] + hot["dwhh"]) / total if total else None,
                           "recurrent_flops_forward": flops_rec, "recurrent_flops_backward": 2.0 * flops_rec,
                           "achieved_tflops": {k: flops_rec / (v * 1e-3) / 1e12 if v else None for k, v in hot.items()},
                           "share_of_f32_mfma_peak": {k: flops_rec / (v * 1e-3) / PEAK_F32_MFMA if v else None
                                                      for k, v in hot.items()}}
        res["rows"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
