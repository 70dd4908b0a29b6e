#!/usr/bin/env python3
"""Apply a soft articulator mask to an rtMRI clip: the reference's scripts/mask_rtmri_video.py with its flags
(``--input --output --mask-type --alpha --blur-kernel``) plus ``--mask-json`` for a custom polygon.

A ``.npy`` stack of uint8 frames, (T,h,w) grey or (T,h,w,3) BGR, goes in and out without OpenCV.  Video files are
read and written (mp4v, as the reference) only where ``cv2`` imports; elsewhere they are refused with a message
that says so.  The mask is ``m2s.occlusion``'s restatement of ``build_mask`` (its parity with
cv2.fillConvexPoly / cv2.GaussianBlur is unpinned), the application the reference's
``(frame.astype(float32) * mask[..., None]).clip(0, 255).astype(uint8)``.

This writes the masked frames for inspection or for another tool.  The experiment itself needs no masked file:
``scripts/mri_occlusion.py`` masks on the device while it stages the frames.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from m2s import occlusion  # noqa: E402

try:
    import cv2
except ImportError:  # .npy stacks need none of it
    cv2 = None


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Darken one articulator of an rtMRI clip with a soft polygon mask")
    p.add_argument("--input", required=True, help="clip to mask: a .npy uint8 stack, or a video file where OpenCV is installed")
    p.add_argument("--output", required=True, help="where the masked clip goes (same kind as the input)")
    p.add_argument("--mask-type", default="lip", choices=sorted(occlusion.PRESETS), help="preset region to darken")
    p.add_argument("--alpha", type=float, default=0.1, help="brightness factor left inside the region, 0 = black, 1 = untouched")
    p.add_argument("--blur-kernel", type=int, default=11, help="taps of the Gaussian that softens the edge; 0 or 1 = hard edge, an even value is the next odd one")
    p.add_argument("--mask-json", default=None,
                   help='Custom convex polygon instead of a preset: [[x, y], ...] in frame pixels, or {"points": '
                        '[...], "base_size": [width, height]}')
    return p.parse_args(argv)


def make_mask(args, shape) -> np.ndarray:
    if args.mask_json:
        return occlusion.custom_mask(args.mask_json, shape, args.alpha, args.blur_kernel)
    return occlusion.preset_mask(args.mask_type, shape, args.alpha, args.blur_kernel)


def _need_cv2(path):
    if cv2 is None:
        raise SystemExit(f"error: {path} is a video file and OpenCV (cv2) is not installed; "
                         "pass a .npy stack of uint8 frames, or install OpenCV for mp4 input and output")


def mask_video(args, input_path: Path, output_path: Path) -> None:
    _need_cv2(input_path)
    cap = cv2.VideoCapture(str(input_path))
    if not cap.isOpened():
        raise RuntimeError(f"cannot open {input_path} as a video")
    fps = cap.get(cv2.CAP_PROP_FPS) or 30.0
    width, height = int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
    mask = make_mask(args, (height, width))
    writer = cv2.VideoWriter(str(output_path), cv2.VideoWriter_fourcc(*"mp4v"), fps, (width, height))
    if not writer.isOpened():
        raise RuntimeError(f"cannot open {output_path} for writing")
    try:
        while True:
            ret, frame = cap.read()
            if not ret:
                break
            writer.write(occlusion.apply_mask_host(frame[None], mask)[0])
    finally:
        cap.release()
        writer.release()


def main(argv=None) -> int:
    args = parse_args(argv)
    input_path, output_path = Path(args.input), Path(args.output)
    if not input_path.exists():
        raise FileNotFoundError(f"no such clip: {input_path}")
    output_path.parent.mkdir(parents=True, exist_ok=True)
    if input_path.suffix == ".npy":
        if output_path.suffix != ".npy":
            raise SystemExit("error: a .npy stack is written back as a .npy stack; name the output *.npy")
        frames = np.load(input_path)
        if frames.dtype != np.uint8 or frames.ndim not in (3, 4):
            raise SystemExit(f"error: expected a uint8 stack (T,h,w) or (T,h,w,3), got {frames.dtype} {frames.shape}")
        np.save(output_path, occlusion.apply_mask_host(frames, make_mask(args, frames.shape[1:3])))
    else:
        mask_video(args, input_path, output_path)
    print(f"masked clip: {output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
