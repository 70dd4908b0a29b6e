"""Command-line driver: Grad-CAM heat maps of the acoustic model's formant-band power on MI355X.

Takes the flags of the reference's scripts/mri_gradcam_formant.py (:326-368) and writes its output files
(``gradcam_{band}_sequence.npy`` (T,H,W), ``gradcam_{band}_average.png``, ``gradcam_{band}_frame{idx:04d}.png``,
``gradcam_{band}_frame{idx:04d}_detail.png``; :302-323, :419-426).  It is written for this build, not a
transcription: every band and every ``--target-frames`` entry goes through ONE ``m2s.gradcam.GradCam.run`` (one
train-mode forward, all targets through the backward together, heat maps made on the device)
instead of one autograd backward per target.  Video, scaler and checkpoint load through this repository's
run_mri_video_inference.py, so a (T,H,W) uint8 ``.npy`` stack works as the video.

``--all-frames`` (additive) asks for a per-frame target at every frame and writes
``gradcam_{band}_perframe.npy`` (T,H,W) - row t is frame t under its own target - and no per-frame PNGs.

The PNG overlays need matplotlib; without it the ``.npy`` files are still written and the PNGs are skipped with a
message.  No CPU path: ``--device cpu`` stops.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

PROJECT_ROOT = Path(__file__).resolve().parents[1]
for _p in (str(PROJECT_ROOT), str(Path(__file__).resolve().parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from m2s.gradcam import GradCam, parse_band_arguments  # noqa: E402
from run_mri_video_inference import build_mri_model, load_scaler, load_video_frames  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Grad-CAM of the CNN-BiLSTM MRI -> mel model on formant bands (MI355X)")
    p.add_argument("--video", required=True, help="rtMRI video, or a (T,H,W[,3]) uint8 .npy frame stack")
    p.add_argument("--mri-checkpoint", required=True, help="acoustic-model checkpoint (.pt)")
    p.add_argument("--scaler-json", required=True, help="scaler.json with the per-bin mel mean/std")
    p.add_argument("--output-dir", required=True, help="where the heat maps go")
    p.add_argument("--mri-code-dir", help="directory with mri_acoustic_model.py (default: <ckpt>/../../mri2speech_code)")
    p.add_argument("--n-mels", type=int, default=64)
    p.add_argument("--sampling-rate", type=int, default=11413, help="sampling rate of the mel extraction")
    p.add_argument("--fmin", type=float, default=0.0, help="mel filter minimum frequency (Hz)")
    p.add_argument("--fmax", type=float, default=8000.0, help="mel filter maximum frequency (Hz)")
    p.add_argument("--formant-band", action="append", metavar="NAME:LOW-HIGH",
                   help="target band in Hz, e.g. F1:300-900; repeatable; default F1:300-900 and F2:900-2500")
    p.add_argument("--target-frames", type=int, nargs="*", default=[],
                   help="frames that also get a heat map under their own (single-frame) target")
    p.add_argument("--reduction", choices=["mean", "sum"], default="mean",
                   help="reduction over time of the whole-clip target")
    p.add_argument("--device", choices=["auto", "cpu", "cuda"], default="auto", help="auto and cuda mean the HIP device")
    p.add_argument("--all-frames", action="store_true",
                   help="a per-frame target at every frame: writes gradcam_{band}_perframe.npy (T,H,W), no per-frame PNGs")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
        return plt
    except ImportError:
        return None


def overlay(plt, frame: np.ndarray, heat: np.ndarray, path: Path) -> None:
    """The heat map (jet, half transparent) over the grey frame."""
    fig = plt.figure(figsize=(5, 5))
    plt.imshow(frame, cmap="gray", interpolation="nearest")
    plt.imshow(heat, cmap="jet", alpha=0.5, interpolation="bilinear")
    plt.axis("off")
    plt.tight_layout(pad=0)
    fig.savefig(path, dpi=200)
    plt.close(fig)


def main(argv=None):
    args = parse_args(argv)
    if args.device == "cpu" or not torch.cuda.is_available():
        raise RuntimeError("m2s needs an MI355X (HIP) device; there is no CPU path")
    device = torch.device("cuda")
    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    mean, std = load_scaler(Path(args.scaler_json))
    if len(mean) != args.n_mels or len(std) != args.n_mels:
        raise ValueError("scaler mean/std length does not match --n-mels")
    bands = parse_band_arguments(args.formant_band, args.n_mels, args.sampling_rate, args.fmin, args.fmax)
    frames = load_video_frames(Path(args.video))  # (T,H,W) fp32 in [0,1], host
    T = frames.shape[0]
    targets = list(range(T)) if args.all_frames else list(args.target_frames)
    for t in targets:
        if not 0 <= t < T:
            raise IndexError(f"--target-frames {t} outside the clip's {T} frames")
    model_args = argparse.Namespace(mri_checkpoint=args.mri_checkpoint, n_mels=args.n_mels, rnn_hidden=640, dropout=0.5,
                                    mri_code_dir=args.mri_code_dir)
    model = build_mri_model(model_args, device)
    for name, idx in bands.items():
        print(f"[m2s] band {name}: mel bins {idx.tolist()}")
    res = GradCam(model, device).run(frames.to(device), mean, std, bands, reduction=args.reduction,
                                     frame_indices=targets, return_dpooled=False)
    plt = _pyplot()
    if plt is None:
        print("[m2s] matplotlib is not installed: the .npy files are written, the PNG overlays are skipped")
    frames_np = frames.numpy()
    for name, r in res.items():
        cams = r["heatmaps"].cpu().numpy()
        np.save(out_dir / f"gradcam_{name}_sequence.npy", cams)
        if args.all_frames:
            np.save(out_dir / f"gradcam_{name}_perframe.npy",
                    torch.stack([r["per_frame"][t] for t in range(T)]).cpu().numpy())
        if plt is None:
            continue
        overlay(plt, frames_np.mean(axis=0), cams.mean(axis=0), out_dir / f"gradcam_{name}_average.png")
        if args.all_frames:
            continue
        for t in dict.fromkeys(targets):
            overlay(plt, frames_np[t], cams[t], out_dir / f"gradcam_{name}_frame{t:04d}.png")
            overlay(plt, frames_np[t], r["per_frame"][t].cpu().numpy(), out_dir / f"gradcam_{name}_frame{t:04d}_detail.png")
    print(f"[m2s] Grad-CAM of {T} frames, bands {list(res)}, {len(targets)} frame targets -> {out_dir}")
    return res


if __name__ == "__main__":
    main()
