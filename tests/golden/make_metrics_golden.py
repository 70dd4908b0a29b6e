"""Writes tests/golden/metrics_ref.npz: inputs, ramp and the values the REFERENCE's own classes give for them.

    python tests/golden/make_metrics_golden.py <reference repository>

Loaded from the reference, not restated: ``MaskedMSEMAE`` and ``OTNLikeTrainer._compute_band_mae`` of
mri2speech_code/train_mri_acoustic_model.py and ``MaskedMSEMAE`` of mri2speech_code/eval_mel.py.  Both modules
import packages a test box may lack (tensorboard, tqdm, librosa, timm) and sibling modules (the model, the
datasets) at import time; none of them is used by the three pieces called here, so whatever cannot be imported is
replaced by an empty stub module for the import.  ``mcd_like`` needs librosa itself and is therefore NOT part of
this golden: tests/metrics_ref.py restates it from librosa's documented formulas.

The file holds data only: per case ``pred, target, mask, ramp`` and ``train = [loss, mse, mae]``,
``band = [f0, f1, f2, high]`` (NaN where the reference leaves the band out), ``eval = [loss, mse, mae]``.
"""
import os
import sys
import types

import numpy as np
import torch


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def load(ref, module):
    """The reference module, executed from its source file.  The trainer's comments are not valid UTF-8, so the
    file is decoded leniently (only comments and docstrings are affected) instead of going through ``import``."""
    path = os.path.join(ref, "mri2speech_code", module + ".py")
    with open(path, "rb") as f:
        code = compile(f.read().decode("utf-8", errors="replace"), path, "exec")
    for name in ("torch.utils.tensorboard", "tqdm", "librosa", "timm"):  # optional packages: stub what is missing
        try:
            __import__(name)
        except ImportError:
            for k in [k for k in sys.modules if k == name.split(".")[-1] or k.startswith(name.split(".")[-1] + ".")]:
                del sys.modules[k]  # a half-imported package
            sys.modules[name] = _Stub(name)
    for _ in range(32):
        try:
            mod = types.ModuleType(module)
            mod.__file__ = path
            exec(code, mod.__dict__)
            return mod
        except ImportError as e:
            if not e.name or e.name in sys.modules:
                raise
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Stub(".".join(parts[:i])))
    raise ImportError(module)


CASES = {
    # name: (B, T, M, masks per sequence or None, ramp step)
    "b3_t4_m64": (3, 4, 64, [[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]], 120000),
    "half_ramp": (4, 4, 64, [[1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 0], [0.5, 0.5, 1, 1]], 60000),
    "t1": (2, 1, 64, [[1], [1]], 120000),
    "t2": (2, 2, 64, [[1, 1], [1, 0]], 120000),
    "m16": (3, 4, 16, [[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]], 120000),
    "t12_nomask": (2, 12, 64, None, 30000),
}


def main(ref):
    tr = load(ref, "train_mri_acoustic_model")
    ev = load(ref, "eval_mel")
    out = {"cases": np.array(sorted(CASES))}
    g = torch.Generator().manual_seed(20)
    for name in sorted(CASES):
        B, T, M, masks, step = CASES[name]
        pred, target = torch.randn(B, T, M, generator=g), torch.randn(B, T, M, generator=g)
        mask = None if masks is None else torch.tensor(masks, dtype=torch.float32)
        crit = tr.MaskedMSEMAE(num_mels=M)  # the criterion built for the model's n_mels (the trainer's is 64)
        crit.set_step(step)
        with torch.no_grad():
            train = [float(v) for v in crit(pred, target, mask)]
            bands = tr.OTNLikeTrainer._compute_band_mae(types.SimpleNamespace(crit=crit), pred, target)
            evals = [float(v) for v in ev.MaskedMSEMAE()(pred, target, torch.ones(B, T) if mask is None else mask)]
        out[f"{name}.pred"], out[f"{name}.target"] = pred.numpy(), target.numpy()
        out[f"{name}.mask"] = np.zeros((0,), np.float32) if mask is None else mask.numpy()
        out[f"{name}.ramp"] = np.float64(min(1.0, step / 120000.0))
        out[f"{name}.train"] = np.array(train, np.float64)
        out[f"{name}.band"] = np.array([bands.get(k, np.nan) for k in ("f0", "f1", "f2", "high")], np.float64)
        out[f"{name}.eval"] = np.array(evals, np.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(CASES)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
