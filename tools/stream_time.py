#!/usr/bin/env python3
"""Time one push of the streaming vocoder against what a caller could do without it, on one MI355X.

Three shapes, 1 stream x 1 new row, 1 x 4 and 64 streams x 4, every span with the full history (``back`` rows of
context) and the full look-ahead (``ahead`` rows held back); the shipped resblock "1" generator, engines bf16x3 and
fp32, in one process:

* ``cone``      (a) ``forward_chunk`` as shipped: between stages only the rows an emitted sample depends on
* ``cone_off``  (b) ``forward_chunk`` with the cone switched off: every stage on the full spans
* ``ragged``    (c) ``forward_ragged`` on the full spans and a torch slice of the emitted rows: the only route without
                the chunk call

The versions alternate inside one timed loop after a warm-up of all of them; each sample is one pair of device events
around ``--group`` back-to-back calls of one version, and the warm median per call is reported with the 10th / 90th
percentiles, next to the real-time budget of the push (new rows x hop / sampling rate).  ``kernels`` holds one
profiled call of (a) and of (b): launches and summed event time per stage.  Writes one JSON file (default
profiles/stream_time.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from window_time import sha, stats, timed  # noqa: E402  (the same protocol)

SHAPES = [(1, 1), (1, 4), (64, 4)]


def stages(native, f):
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
        e = out.setdefault(r["stage"], {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += r["ms"]
    out["all"] = {"launches": len(rec), "ms": sum(r["ms"] for r in rec)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_time.json"))
    ap.add_argument("--source", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--group", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stream_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import _native, runtime, synth
    from m2s.config import HIFIGAN_H
    dev = torch.device("cuda", 0)
    sd = synth.synth_generator_state(2, HIFIGAN_H)
    row_ms = 1000.0 * HIFIGAN_H["hop_size"] / HIFIGAN_H["sampling_rate"]
    res = {"device": torch.cuda.get_device_name(0), "source": a.source or sha(), "warmup": a.warmup,
           "samples": a.samples, "group": a.group, "row_ms": row_ms, "rows": []}
    for dtype in ("bf16x3", "fp32"):
        eng = runtime.VocoderEngine(sd, HIFIGAN_H, dtype=dtype, device=dev)
        back, ahead = eng.reach
        hop = eng.hop
        for B, n in SHAPES:
            T = back + n + ahead
            lens, ctx, hold = [T] * B, [back] * B, [ahead] * B
            mel = torch.from_numpy(synth.synth_mel_log(B, 64, T, seed=B + n)).transpose(1, 2).reshape(B * T, 64)
            mel = mel.contiguous().to(dev)

            def chunk(cone):
                def f():
                    eng.set_chunk_cone(cone)
                    return eng.forward_chunk(mel, lens, ctx, hold)
                return f

            def ragged():
                return eng.forward_ragged(mel, lens).view(B, T * hop)[:, back * hop:(back + n) * hop].reshape(-1)

            fns = {"cone": chunk(True), "cone_off": chunk(False), "ragged": ragged}
            want = ragged()
            diff = {k: float((fns[k]() - want).abs().max()) for k in ("cone", "cone_off")}
            ms = timed(fns, a.warmup, a.samples, a.group)
            row = {"dtype": dtype, "streams": B, "new_rows": n, "span_rows": T, "budget_ms": n * row_ms,
                   "max_abs_vs_ragged": diff, **{k: stats(v) for k, v in ms.items()}}
            row["cone_off_over_cone"] = row["cone_off"]["median_ms"] / row["cone"]["median_ms"]
            row["ragged_over_cone"] = row["ragged"]["median_ms"] / row["cone"]["median_ms"]
            row["kernels"] = {"cone": stages(_native, fns["cone"]), "cone_off": stages(_native, fns["cone_off"])}
            eng.set_chunk_cone(True)
            res["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "kernels"}))
            print(json.dumps({k: v["all"] for k, v in row["kernels"].items()}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
