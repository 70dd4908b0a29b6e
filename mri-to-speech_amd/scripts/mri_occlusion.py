"""Command-line driver: the masking experiment of one clip on MI355X (docs/rtmri_pipeline_notes.md step 5).

The reference masks a video on the host (scripts/mask_rtmri_video.py), re-encodes it, runs a full inference per
mask and compares the generated speech by hand.  Here every mask variant of the clip goes through ONE engine call
(``m2s.runtime.Pipeline.occlusion``): the masks are applied on the device while the uint8 frames are
staged, and the loss in the predicted mel is reduced on the device to

* ``occlusion_scores.json``      per mask, per band (and "all"): mean |mel_db(masked) - mel_db(clip)| in dB, plus the
                                 per-frame scores
* ``occlusion_<band>_map.npy``   (h,w) coverage-weighted mean score at the frames' own size: which regions the band
                                 depends on, the perturbation-based counterpart of the Grad-CAM maps
* ``occlusion_<name>.wav``       with ``--wav``: the baseline's and every named mask's audio, for listening

Masks: ``--mask-type lip|tongue`` (repeatable), ``--mask-json FILE`` (repeatable) and / or ``--grid PATCH STRIDE``, one
soft square per grid position.  Bands are the Grad-CAM tool's ``--formant-band NAME:LOW-HIGH``.  The clip is a
(T,h,w[,3]) uint8 ``.npy`` stack, or a video where OpenCV is installed, at the scanner's size (no larger than the
model's 256 x 256).  The lossy mp4v re-encode of the reference's workflow is not reproduced: the model sees the
masked frames themselves.  No CPU path.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

PROJECT_ROOT = Path(__file__).resolve().parents[1]
for _p in (str(PROJECT_ROOT), str(Path(__file__).resolve().parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from m2s import occlusion, runtime  # noqa: E402
from m2s.gradcam import parse_band_arguments  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Occlusion sensitivity of the MRI -> mel model: masked variants of one clip "
                                            "in one engine call (MI355X)")
    p.add_argument("--video", required=True, help="rtMRI clip: a (T,h,w[,3]) uint8 .npy stack, or a video with OpenCV")
    p.add_argument("--mri-checkpoint", required=True, help="acoustic-model checkpoint (.pt)")
    p.add_argument("--scaler-json", required=True, help="scaler.json with the per-bin mel mean/std")
    p.add_argument("--hifigan-config", required=True, help="HiFi-GAN config.json")
    p.add_argument("--hifigan-checkpoint", required=True, help="HiFi-GAN generator checkpoint")
    p.add_argument("--output-dir", required=True, help="where the scores, maps and wavs go")
    p.add_argument("--mri-code-dir", help="directory with mri_acoustic_model.py (default: <ckpt>/../../mri2speech_code)")
    p.add_argument("--max-frames", type=int, default=None)
    p.add_argument("--n-mels", type=int, default=64)
    p.add_argument("--rnn-hidden", type=int, default=640)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--dtype", default=None, help="engine dtype (default: the engines' own)")
    p.add_argument("--sampling-rate", type=int, default=11413, help="sampling rate of the mel extraction")
    p.add_argument("--fmin", type=float, default=0.0, help="mel filter minimum frequency (Hz)")
    p.add_argument("--fmax", type=float, default=8000.0, help="mel filter maximum frequency (Hz)")
    p.add_argument("--formant-band", action="append", metavar="NAME:LOW-HIGH",
                   help="band in Hz, e.g. F1:300-900; repeatable; default F1:300-900 and F2:900-2500")
    p.add_argument("--mask-type", action="append", choices=sorted(occlusion.PRESETS), default=[],
                   help="preset region to darken; repeatable")
    p.add_argument("--mask-json", action="append", default=[], help="custom convex polygon file; repeatable")
    p.add_argument("--grid", type=int, nargs=2, metavar=("PATCH", "STRIDE"),
                   help="a sweep: one square of PATCH pixels every STRIDE pixels")
    p.add_argument("--alpha", type=float, default=0.1, help="brightness factor left inside a mask")
    p.add_argument("--blur-kernel", type=int, default=11, help="taps of the Gaussian that softens a mask's edge")
    p.add_argument("--window", type=int, default=0, help="> 0: the windowed acoustic model with that window")
    p.add_argument("--frame-interp", choices=["linear", "area"], default="linear")
    p.add_argument("--frame-norm", choices=["zscore", "unit"], default="zscore")
    p.add_argument("--chunk", type=int, default=64, help="variants per engine call, the baseline included")
    p.add_argument("--normalize", action="store_true", help="min-max scale every map to [0, 1]")
    p.add_argument("--wav", action="store_true", help="write the audio of the baseline and of every named mask")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def load_frames_u8(path: Path, max_frames=None) -> np.ndarray:
    """The clip as a uint8 (T,h,w[,3]) array at its own size."""
    path = Path(path)
    if path.suffix.lower() == ".npy":
        a = np.load(path, allow_pickle=False)
    else:
        try:
            import cv2
        except ImportError:
            raise SystemExit(f"error: {path} is a video file and OpenCV (cv2) is not installed; pass a .npy stack") from None
        cap = cv2.VideoCapture(str(path))
        if not cap.isOpened():
            raise ValueError(f"cannot open video {path}")
        fr = []
        while max_frames is None or len(fr) < max_frames:
            ok, f = cap.read()
            if not ok:
                break
            fr.append(f)
        cap.release()
        if not fr:
            raise ValueError(f"no frames could be read from {path}")
        a = np.stack(fr)
    if a.dtype != np.uint8 or a.ndim not in (3, 4):
        raise ValueError(f"expected uint8 frames (T,h,w[,3]), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a[:max_frames] if max_frames is not None else a)


def build_masks(args, shape):
    """(names, (M,h,w) float32) of every mask the flags ask for; the named ones come first."""
    names, masks = [], []
    for t in args.mask_type:
        names.append(t)
        masks.append(occlusion.preset_mask(t, shape, args.alpha, args.blur_kernel))
    for f in args.mask_json:
        names.append(Path(f).stem)
        masks.append(occlusion.custom_mask(f, shape, args.alpha, args.blur_kernel))
    n_named = len(names)
    if args.grid:
        patch, stride = args.grid
        for (y, x), m in zip(occlusion.grid_positions(shape, patch, stride),
                             occlusion.grid_masks(shape, patch, stride, args.alpha, args.blur_kernel)):
            names.append(f"grid_y{y:03d}_x{x:03d}")
            masks.append(m)
    if not masks:
        raise SystemExit("error: no mask: give --mask-type, --mask-json and / or --grid PATCH STRIDE")
    return names, np.stack(masks), n_named


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("m2s needs an MI355X (HIP) device; there is no CPU path")
    from run_mri_video_inference import TARGET, build_mri_model, load_hifigan, load_scaler, write_wav
    device = torch.device("cuda")
    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    mean, std = load_scaler(Path(args.scaler_json))
    if len(mean) != args.n_mels or len(std) != args.n_mels:
        raise ValueError("scaler mean/std length does not match --n-mels")
    bands = parse_band_arguments(args.formant_band, args.n_mels, args.sampling_rate, args.fmin, args.fmax)
    frames = load_frames_u8(Path(args.video), args.max_frames)
    names, masks, n_named = build_masks(args, frames.shape[1:3])
    model = build_mri_model(args, device)
    gen, h = load_hifigan(Path(args.hifigan_config), Path(args.hifigan_checkpoint), device, args.dtype)
    if not (hasattr(model, "_engine") and hasattr(gen, "_engine")):
        raise RuntimeError("the occlusion experiment needs the m2s acoustic and vocoder plug-ins")
    eng = model._engine(device)
    pipe = runtime.Pipeline(eng, gen._engine(device), mean, std)
    wav_variants = list(range(0, n_named + 1)) if args.wav else []
    res = pipe.occlusion(torch.from_numpy(frames).to(device), masks, bands, size=(TARGET[1], TARGET[0]),
                         interp=args.frame_interp, norm=args.frame_norm, windowed=args.window or None,
                         wav_variants=wav_variants, chunk=args.chunk, normalize=args.normalize)
    score, per_frame, maps = (res[k].cpu().numpy() for k in ("score", "per_frame", "map"))
    eng.check()
    cols = res["names"]
    report = {"unit": "dB", "frames": int(frames.shape[0]), "bands": {n: [int(i) for i in bands[n]] for n in bands},
              "masks": [{"name": n, "score": {c: float(score[m, j]) for j, c in enumerate(cols)},
                         "per_frame": {c: [float(v) for v in per_frame[m, :, j]] for j, c in enumerate(cols)}}
                        for m, n in enumerate(names)]}
    (out_dir / "occlusion_scores.json").write_text(json.dumps(report, indent=1))
    for j, c in enumerate(cols):
        np.save(out_dir / f"occlusion_{c}_map.npy", maps[j])
    for v, wav in res["wavs"].items():
        write_wav(out_dir / f"occlusion_{'baseline' if v == 0 else names[v - 1]}.wav", wav.float().cpu().numpy(),
                  int(h.get("sampling_rate", args.sampling_rate)))
    print(f"[m2s] occlusion of {frames.shape[0]} frames under {len(names)} masks, columns {cols} -> {out_dir}")
    return {"score": score, "per_frame": per_frame, "map": maps, "names": names, "columns": cols}


if __name__ == "__main__":
    main()
