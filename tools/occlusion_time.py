#!/usr/bin/env python3
"""Time the masking experiment's device path against the routes a caller has without it, on one MI355X.

(a) the masked frame front end: 64 masks x 30 frames of 84 x 84 going to 256 x 256
    * ``masked``  one ``preprocess_frames_masked`` call (csrc/frames.hip, grid (frame, variant))
    * ``today``   per variant, a torch elementwise mask on the device (float multiply, clamp, uint8) and one
                  ``preprocess_frames_resize`` call: 64 x (3 elementwise kernels + 1 front-end launch)
    against the store-bound floor, 4 * H * W bytes a variant-frame over the HBM rate.
(b) the experiment: ``Pipeline.occlusion`` for 64 grid masks x 30 frames (synthetic weights, bf16x3), against the
    baseline plus 64 separate host-masked clips through ``Pipeline.forward`` (65 calls) and the scores in torch.
(c) the unmasked ``preprocess_frames_resize`` on the same frames (1 x 30 and 8 x 1000), the figure
    tools/frames_time.py reports as ``kernel``: to be compared with the parent commit's on the same machine.

Every call is bracketed by its own pair of device events on the current stream; the versions alternate inside one
timed loop after a warm-up of all, and the median over the timed calls is reported with the 10th and 90th
percentiles.  Writes one JSON file (default profiles/occlusion_time.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frames_time import DST, HBM_COPY, HBM_SPEC, SHAPES, SRC, timed  # noqa: E402

M, T = 64, 30
PATCH, STRIDE = 14, 11  # 8 x 8 squares on 84 x 84


def stats(v):
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occlusion_time.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--pipeline-calls", type=int, default=8, help="timed calls of part (b), whose calls take tens of ms")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("occlusion_time.py needs an MI355X (HIP) device: a CPU run cannot give a time")
    from m2s import occlusion, ops, runtime, synth
    from m2s.config import HIFIGAN_H
    dev = torch.device("cuda", 0)
    o = ops.load()
    res = {"device": torch.cuda.get_device_name(0), "source": SRC, "destination": DST, "masks": M, "frames": T,
           "warmup": a.warmup, "calls": a.calls}

    masks_np = occlusion.grid_masks(SRC, PATCH, STRIDE, alpha=0.1, blur_kernel=5)
    assert masks_np.shape[0] == M
    masks = torch.from_numpy(masks_np).to(dev)
    frames = torch.randint(0, 256, (T, *SRC), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)

    # ---- (a)
    def today_front():
        return [o.preprocess_frames_resize((frames.float() * masks[m]).clamp_(0.0, 255.0).to(torch.uint8), DST[0], DST[1], 0, 0)
                for m in range(M)]

    ms = timed({"masked": lambda: o.preprocess_frames_masked(frames, masks, DST[0], DST[1], 0, 0), "today": today_front},
               a.warmup, a.calls)
    assert torch.equal(o.preprocess_frames_masked(frames, masks, DST[0], DST[1], 0, 0), torch.stack(today_front()))
    out_bytes = 4.0 * M * T * DST[0] * DST[1]
    fa = {k: stats(v) for k, v in ms.items()}
    fa["today_over_masked"] = fa["today"]["median_ms"] / fa["masked"]["median_ms"]
    fa["floor_ms"] = {"hbm_spec": out_bytes / HBM_SPEC * 1e3, "hbm_copy": out_bytes / HBM_COPY * 1e3}
    fa["masked_store_TBps"] = out_bytes / (fa["masked"]["median_ms"] * 1e-3) / 1e12
    res["front_end"] = fa
    print(json.dumps({"front_end": fa}))

    # ---- (b)
    mean, std = synth.synth_scaler()
    ac = runtime.AcousticEngine(synth.synth_acoustic_state(0), dtype="bf16x3", device=dev)
    pipe = runtime.Pipeline(ac, runtime.VocoderEngine(synth.synth_generator_state(0), HIFIGAN_H, dtype="bf16x3", device=dev),
                            mean, std)
    host_masked = [frames] + [torch.from_numpy(occlusion.apply_mask_host(frames.cpu().numpy(), m)).to(dev) for m in masks_np]

    def today_experiment():
        db = [pipe.forward(runtime.preprocess_frames(f, DST)[None])["mel_db"][0] for f in host_masked]  # 65 full inferences
        return torch.stack([(d - db[0]).abs().mean() for d in db[1:]])

    ms = timed({"occlusion": lambda: pipe.occlusion(frames, masks, None, size=DST, chunk=M + 1), "today": today_experiment},
               2, a.pipeline_calls)
    ac.check()
    fb = {k: stats(v) for k, v in ms.items()}
    fb["today_over_occlusion"] = fb["today"]["median_ms"] / fb["occlusion"]["median_ms"]
    fb["note"] = "today runs the vocoder in each of its 65 calls, as Pipeline.forward does; occlusion runs it for no variant"
    res["experiment"] = fb
    print(json.dumps({"experiment": fb}))

    # ---- (c)
    res["unmasked"] = []
    for clips, t in SHAPES:
        n = clips * t
        x = torch.randint(0, 256, (n, *SRC), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).to(dev)
        row = {"frames": n, **stats(timed({"kernel": lambda: runtime.preprocess_frames(x, DST)}, a.warmup, a.calls)["kernel"])}
        res["unmasked"].append(row)
        print(json.dumps({"unmasked": row}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
