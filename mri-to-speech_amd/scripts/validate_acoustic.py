"""Validate an acoustic checkpoint on its training pairs, on MI355X: the numbers of the reference's
``OTNLikeTrainer.validate()`` (mri2speech_code/train_mri_acoustic_model.py:349-384,496-499) and of ``eval_mel.py``
(:104-155,208-215) in one run.

Reads ``{processed_dir}/samples/*/{mri.npy, mel_db.npy, mask.npy}`` (what preprocess_rtmri_data.py's save_sample
writes, :155-165), NOT the materialised ``pairs_ref{N}`` files: the pairs are cut on the device.  A clip gives the
pairs pass3_save_pairs (:198-259) cuts from it: every window of ``--ref_frames`` consecutive frames, stride 1,
against ``(mel_db - mean) / std``; clips shorter than ``--ref_frames`` are skipped.  Clips are ordered by the
reference's natural sort of their folder names and pairs are numbered globally in that order, which is the index
space of FixedLenPairDataset.  ``--split val|test`` keeps the subset ``make_loaders`` (:173-206) draws:
``random_split`` of ``range(n)`` into ``int(.8 n), int(.1 n), rest`` with ``torch.Generator().manual_seed(seed)``;
the kept pairs form batches of ``--val_bs`` in the subset's order, and every loss is taken per batch and averaged
over the batches, as the reference does.

How it runs: ``--batch`` clips go through the acoustic model per call (``forward_pairs``: the CNN once per frame,
the BiLSTM from zero state on every window), the predictions of all pairs stay on the device, and ONE
``torch.ops.m2s.mel_metrics`` call computes every number.  ``--cpu`` is refused: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import re
import sys
from pathlib import Path

import numpy as np
import torch

PROJECT_ROOT = Path(__file__).resolve().parents[1]
if str(PROJECT_ROOT) not in sys.path:
    sys.path.insert(0, str(PROJECT_ROOT))


def natural_key(s: str):
    """The reference's ``_natural_key`` (dataset_fixedlen.py:13-27): digit runs compare as integers."""
    return [int(t) if t.isdigit() else t for t in re.findall(r"\d+|\D+", s)]


def split_indices(n: int, split: str, seed: int = 42):
    """Global pair indices of a split, in the order the reference's loader visits them."""
    if split == "all":
        return list(range(n))
    n_train, n_val = int(n * 0.8), int(n * 0.1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    return {"train": perm[:n_train], "val": perm[n_train:n_train + n_val], "test": perm[n_train + n_val:]}[split]


def list_clips(samples_dir: Path, ref_frames: int):
    """[(folder, T)] of the clips that give at least one pair, in the reference's order."""
    if not samples_dir.is_dir():
        raise SystemExit(f"samples directory not found: {samples_dir}")
    clips = []
    for d in sorted((p for p in samples_dir.iterdir() if p.is_dir()), key=lambda p: natural_key(p.name)):
        paths = [d / n for n in ("mri.npy", "mel_db.npy", "mask.npy")]
        if not all(p.is_file() for p in paths):
            continue
        T = min(int(np.load(p, mmap_mode="r", allow_pickle=False).shape[0]) for p in paths[:2])
        if T >= ref_frames:
            clips.append((d, T))
    return clips


def scaler_arrays(path: Path):
    st = json.loads(Path(path).read_text(encoding="utf-8"))
    mean, std = (torch.tensor(st[k], dtype=torch.float32) for k in ("mean", "std"))
    if mean.numel() != std.numel():
        raise SystemExit("Scaler mean/std length mismatch")
    return mean, std


def validate(args: argparse.Namespace) -> dict:
    if args.cpu:
        raise SystemExit("--cpu: m2s runs on MI355X only (no CPU path); drop the flag")
    if not torch.cuda.is_available():
        raise SystemExit("m2s needs an MI355X (HIP) device; none is visible")
    from m2s import drivers
    from m2s.metrics import MelMetrics, pair_index, ramp_of_step

    device = torch.device("cuda")
    mean, std = scaler_arrays(Path(args.scaler_json).resolve())
    W = args.ref_frames
    clips = list_clips(Path(args.processed_dir).resolve() / "samples", W)
    n = sum(T - W + 1 for _, T in clips)
    if n == 0:
        raise SystemExit(f"no clip of at least {W} frames under {args.processed_dir}/samples")
    sel = split_indices(n, args.split, args.seed)
    if not sel:
        raise SystemExit(f"split {args.split!r} of {n} pairs is empty")
    model = drivers.build_acoustic(Path(args.mri_checkpoint).resolve(), device, code_dir=args.mri_code_dir,
                                   n_mels=mean.numel(), dtype=args.dtype)
    mean_d, std_d = mean.to(device), std.to(device)
    preds, tgts, masks = [], [], []
    for i in range(0, len(clips), args.batch):
        part = clips[i:i + args.batch]
        lens = [T for _, T in part]
        frames = [torch.from_numpy(np.load(d / "mri.npy", allow_pickle=False)[:T].astype(np.float32, copy=False)).to(device)
                  for d, T in part]
        mel = torch.from_numpy(np.concatenate([np.load(d / "mel_db.npy", allow_pickle=False)[:T] for d, T in part])
                               .astype(np.float32, copy=False)).to(device)
        mk = torch.from_numpy(np.concatenate([np.load(d / "mask.npy", allow_pickle=False)[:T] for d, T in part])
                              .astype(np.float32, copy=False)).to(device)
        idx = pair_index(lens, W, device)
        preds.append(model.forward_pairs(frames, W))
        tgts.append(((mel - mean_d) / std_d)[idx])
        masks.append(mk[idx])
    keep = torch.tensor(sel, dtype=torch.long, device=device)
    ramp = args.ramp if args.ramp is not None else (ramp_of_step(args.step) if args.step is not None else 1.0)
    met = MelMetrics(mean.numel(), mean_d, std_d, ramp=ramp, device=device)
    met.update(torch.cat(preds).index_select(0, keep), torch.cat(tgts).index_select(0, keep),
               torch.cat(masks).index_select(0, keep), group=args.val_bs)
    res = met.compute()
    res.update(split=args.split, pairs=len(sel), clips=len(clips), ref_frames=W, ramp=ramp)
    report(res)
    if args.out:
        Path(args.out).write_text(json.dumps(res, indent=2), encoding="utf-8")
    return res


def report(res: dict) -> None:
    print(f"Val  : loss={res['loss']:.6f} mse={res['mse']:.6f} mae={res['mae']:.6f}")
    if res["band"]:
        print("    band val  : " + ", ".join(f"{k}={v:.4f}" for k, v in sorted(res["band"].items())))
    print(f"\n=== Evaluation (split: {res.get('split', 'all')}) ===")
    print("masked loss: {:.6f}".format(res["eval"]["loss"]))
    print("masked mse : {:.6f}".format(res["eval"]["mse"]))
    print("masked mae : {:.6f}".format(res["eval"]["mae"]))
    print("MCD-like   : {:.4f}".format(res["mcd_like"]) if res["mcd_like"] is not None else "MCD-like   : (no sequence)")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Validation losses of an MRI->mel checkpoint on its training pairs (MI355X).")
    p.add_argument("--processed_dir", required=True, help="rtMRI processed dataset root (contains samples/).")
    p.add_argument("--mri_checkpoint", required=True, help="Path to trained MRI->mel checkpoint (.pt).")
    p.add_argument("--scaler_json", required=True, help="Path to scaler.json (mean/std of the dB mels).")
    p.add_argument("--mri_code_dir", help="Directory containing mri_acoustic_model.py (if not importable by default).")
    p.add_argument("--ref_frames", type=int, default=4, help="frames per pair (1..16; the reference trains on 4)")
    p.add_argument("--split", choices=["all", "val", "test"], default="all",
                   help="all pairs, or the reference's validation / test subset")
    p.add_argument("--seed", type=int, default=42, help="seed of the reference's random_split")
    p.add_argument("--val_bs", type=int, default=8, help="pairs per batch of the reference's loader")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--step", type=int, default=None, help="global training step the criterion's ramp is taken at")
    g.add_argument("--ramp", type=float, default=None, help="the criterion's ramp in [0, 1] (default 1: finished)")
    p.add_argument("--dtype", choices=["bf16x3", "fp32", "bf16", "fp8"], default=None,
                   help="m2s compute dtype (default: M2S_DTYPE or bf16x3)")
    p.add_argument("--batch", type=int, default=16, help="clips per forward call")
    p.add_argument("--out", help="write the result dict as JSON here")
    p.add_argument("--cpu", action="store_true", help="Refused: m2s has no CPU execution path.")
    args = p.parse_args(argv)
    if not 1 <= args.ref_frames <= 16:
        p.error("--ref_frames must be 1..16")
    if args.val_bs < 1 or args.batch < 1:
        p.error("--val_bs and --batch must be >= 1")
    if args.ramp is not None and not 0.0 <= args.ramp <= 1.0:
        p.error("--ramp must be in [0, 1]")
    if args.step is not None and args.step < 0:
        p.error("--step must be >= 0")
    return args


def main(argv=None):
    return validate(parse_args(argv))


if __name__ == "__main__":
    main()
