"""Fine-tune the BiLSTM and the mel head of an acoustic checkpoint on MI355X with the encoder frozen: adapting the
sequence model to a new speaker or session (m2s/finetune.py, DESIGN.md "Fine-tuning").

Reads ``{processed_dir}/samples/*/{mri.npy, mel_db.npy, mask.npy}`` as scripts/validate_acoustic.py does (same clip
listing, scaler reading and split rule, imported from there).  Every clip's encoder features are computed once
(``AcousticEngine.effnet``, eval mode, running BatchNorm statistics) and stay on the device; an epoch then draws the
``train`` split's windows in a shuffled order from a seeded host generator, ``--batch_size`` windows a step, each
step one ``HeadTuner.step`` (fp32; no autocast, no GradScaler, one micro-batch).  After every epoch the ``val`` split
goes through ``HeadTuner.evaluate`` in batches of ``--batch_size`` windows; the learning rate follows the reference
trainer's ``ReduceLROnPlateau(factor 0.5, patience 5, min_lr 1e-6)`` and training stops after 20 epochs without
improvement or when the rate reaches its floor.  The best model is saved as ``{"model_state_dict": merged, "epoch",
"val_loss"}``, the layout the reference's ``resume_from_checkpoint`` and this project's loaders read.  ``--cpu`` is
refused: there is no CPU path.
"""
from __future__ import annotations

import argparse
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import torch

PROJECT_ROOT = Path(__file__).resolve().parents[1]
if str(PROJECT_ROOT) not in sys.path:
    sys.path.insert(0, str(PROJECT_ROOT))


def _validate_cli():
    """scripts/validate_acoustic.py as a module: its clip listing, scaler reading and split rule are reused as they are."""
    spec = importlib.util.spec_from_file_location("m2s_validate_cli", Path(__file__).with_name("validate_acoustic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Plateau:
    """``ReduceLROnPlateau(mode="min", factor, patience, min_lr)`` with torch's defaults (threshold 1e-4 relative,
    cooldown 0, eps 1e-8) plus the trainer's stop rules, on the host.  ``step(val_loss)`` returns the new learning
    rate; ``stop`` is None, "early" (``early_stop`` epochs without a new best) or "min_lr"."""

    def __init__(self, lr: float, factor: float = 0.5, patience: int = 5, min_lr: float = 1e-6, early_stop: int = 20):
        self.lr, self.factor, self.patience, self.min_lr, self.early_stop = float(lr), factor, patience, min_lr, early_stop
        self.sched_best, self.bad = math.inf, 0   # the scheduler's own best (relative threshold) and bad-epoch count
        self.best, self.since_best = math.inf, 0  # the trainer's best (strict <) and patience
        self.improved, self.stop = False, None

    def step(self, val_loss: float) -> float:
        v = float(val_loss)
        if v < self.sched_best * (1.0 - 1e-4):
            self.sched_best, self.bad = v, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new = max(self.lr * self.factor, self.min_lr)
            if self.lr - new > 1e-8:
                self.lr = new
            self.bad = 0
        self.improved = v < self.best and not math.isnan(v)
        if self.improved:
            self.best, self.since_best = v, 0
        else:
            self.since_best += 1
        if self.since_best >= self.early_stop:
            self.stop = "early"
        elif self.lr <= self.min_lr + 1e-12:
            self.stop = "min_lr"
        return self.lr


def window_batches(n: int, batch_size: int, generator: torch.Generator):
    """A shuffled pass over ``n`` windows in batches of ``batch_size`` (the last may be short), from a host generator."""
    perm = torch.randperm(n, generator=generator)
    return [perm[i:i + batch_size] for i in range(0, n, batch_size)]


def finetune(args: argparse.Namespace) -> dict:
    if args.cpu:
        raise SystemExit("--cpu: m2s runs on MI355X only (no CPU path); drop the flag")
    if not torch.cuda.is_available():
        raise SystemExit("m2s needs an MI355X (HIP) device; none is visible")
    from m2s import drivers, runtime
    from m2s.finetune import HeadTuner
    from m2s.metrics import MelMetrics, ramp_of_step

    cli = _validate_cli()
    device = torch.device("cuda")
    mean, std = cli.scaler_arrays(Path(args.scaler_json).resolve())
    M, W = mean.numel(), args.ref_frames
    clips = cli.list_clips(Path(args.processed_dir).resolve() / "samples", W)
    n = sum(T - W + 1 for _, T in clips)
    if n == 0:
        raise SystemExit(f"no clip of at least {W} frames under {args.processed_dir}/samples")
    ck = drivers.load_state(Path(args.mri_checkpoint).resolve())
    frozen = ck.get("model_state_dict", ck)
    ac = runtime.AcousticEngine(frozen, n_mels=M, dtype=args.dtype or "fp32", device=device)
    mean_d, std_d = mean.to(device), std.to(device)
    feats, tgts, masks, first = [], [], [], []  # per frame row; first[i] = the packed row of global window i
    off = 0
    for d, T in clips:
        fr = torch.from_numpy(np.load(d / "mri.npy", allow_pickle=False)[:T].astype(np.float32, copy=False)).to(device)
        feats.append(ac.effnet(fr[:, 0] if fr.dim() == 4 else fr))
        mel = torch.from_numpy(np.load(d / "mel_db.npy", allow_pickle=False)[:T].astype(np.float32, copy=False)).to(device)
        tgts.append((mel - mean_d) / std_d)
        masks.append(torch.from_numpy(np.load(d / "mask.npy", allow_pickle=False)[:T].astype(np.float32, copy=False)).to(device))
        first.append(off + torch.arange(T - W + 1))
        off += T
    ac.check()
    feats, tgts, masks, first = torch.cat(feats), torch.cat(tgts), torch.cat(masks), torch.cat(first).to(device)
    span = torch.arange(W, device=device)

    def gather(sel):
        """Windows ``sel`` (global indices) as a batch of len(sel) clips of W rows each."""
        rows = (first[sel.to(device)][:, None] + span[None, :]).reshape(-1)
        return feats[rows], tgts[rows], masks[rows], [W] * int(sel.numel())

    train = torch.tensor(cli.split_indices(n, "train", args.seed), dtype=torch.long)
    val = torch.tensor(cli.split_indices(n, "val", args.seed), dtype=torch.long)
    if train.numel() == 0 or val.numel() == 0:
        raise SystemExit(f"{n} windows are too few for a train and a val split")
    tuner = HeadTuner(frozen, n_mels=M, device=device, lr=args.lr, weight_decay=args.weight_decay,
                      grad_clip=args.grad_clip, dropout=args.dropout, seed=args.seed, window=W)
    sched = Plateau(args.lr)
    gen = torch.Generator().manual_seed(args.seed)
    step, result = 0, {"epochs": 0, "best_val": math.inf, "steps": 0}
    for ep in range(1, args.epochs + 1):
        slots = []
        for sel in window_batches(int(train.numel()), args.batch_size, gen):
            if args.max_train_steps is not None and step >= args.max_train_steps:
                break
            f, t, m, lens = gather(train[sel])
            slots.append(tuner.step(f, t, m, lens, ramp=ramp_of_step(step)))
            step += 1
        tr = torch.stack(slots).mean(0).cpu().tolist() if slots else [float("nan")] * 8  # one download an epoch
        met = MelMetrics(M, mean_d, std_d, ramp=ramp_of_step(step), device=device)
        for i in range(0, int(val.numel()), args.batch_size):
            f, t, m, lens = gather(val[i:i + args.batch_size])
            tuner.evaluate(f, t, m, lens, met)
        va = met.compute()
        print(f"\nEpoch {ep}/{args.epochs}")
        print(f"Train: loss={tr[0]:.6f} mse={tr[1]:.6f} mae={tr[2]:.6f}")
        print(f"Val  : loss={va['loss']:.6f} mse={va['mse']:.6f} mae={va['mae']:.6f}")
        if va["band"]:
            print("    band val  : " + ", ".join(f"{k}={v:.4f}" for k, v in sorted(va["band"].items())))
        print(f"LR: {sched.lr:.2e}")
        old = sched.lr
        new = sched.step(va["loss"])
        if new != old:
            print(f"[SCHEDULER] LR reduced: {old:.6e} -> {new:.6e}")
            tuner.set_lr(new)
        if sched.improved:
            torch.save({"epoch": ep, "model_state_dict": tuner.merged_state_dict(frozen), "val_loss": va["loss"],
                        "val_mse": va["mse"], "train_loss": tr[0]}, args.out_ckpt)
            print("[BEST] New best model saved.")
        result.update(epochs=ep, best_val=sched.best, steps=step)
        if sched.stop == "early":
            print("[STOP] Early stopping.")
            break
        if sched.stop == "min_lr":
            print("[STOP] LR reached min.")
            break
        if args.max_train_steps is not None and step >= args.max_train_steps:
            break
    return result


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Fine-tune the BiLSTM and mel head of an MRI->mel checkpoint, encoder frozen (MI355X).")
    p.add_argument("--processed_dir", required=True, help="rtMRI processed dataset root (contains samples/).")
    p.add_argument("--mri_checkpoint", required=True, help="Path to the MRI->mel checkpoint to start from (.pt).")
    p.add_argument("--scaler_json", required=True, help="Path to scaler.json (mean/std of the dB mels).")
    p.add_argument("--out_ckpt", required=True, help="Where the best checkpoint is written.")
    p.add_argument("--ref_frames", type=int, default=4, help="frames per window (1..16; the reference trains on 4)")
    p.add_argument("--epochs", type=int, default=80)
    p.add_argument("--batch_size", type=int, default=8, help="windows per optimisation step")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--grad_clip", type=float, default=1.0, help="clip_grad_norm_ max_norm (<= 0: off)")
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=42, help="seed of the split, the shuffling and the dropout stream")
    p.add_argument("--dtype", choices=["bf16x3", "fp32", "bf16", "fp8"], default=None,
                   help="compute dtype of the frozen encoder (default fp32); the tuned part is always fp32")
    p.add_argument("--max_train_steps", type=int, default=None, help="stop after this many optimisation steps")
    p.add_argument("--cpu", action="store_true", help="Refused: m2s has no CPU execution path.")
    args = p.parse_args(argv)
    if not 1 <= args.ref_frames <= 16:
        p.error("--ref_frames must be 1..16")
    if args.epochs < 1 or args.batch_size < 1:
        p.error("--epochs and --batch_size must be >= 1")
    if not 0.0 <= args.dropout < 1.0:
        p.error("--dropout must be in [0, 1)")
    if args.lr <= 0.0 or args.weight_decay < 0.0:
        p.error("--lr must be > 0 and --weight_decay >= 0")
    if args.max_train_steps is not None and args.max_train_steps < 1:
        p.error("--max_train_steps must be >= 1")
    return args


def main(argv=None):
    return finetune(parse_args(argv))


if __name__ == "__main__":
    main()
