"""Generate tests/golden/melspec.npz from the REFERENCE's own ``meldataset.mel_spectrogram``, on CPU:

    python tests/golden/make_melspec_golden.py PATH_TO_A_CHECKOUT_OF_THE_REFERENCE

Needed only to regenerate the fixture; the tests read the committed .npz.

The reference imports librosa, which is not installed.  Only its mel filter bank is used on this path
(meldataset.py:72-78), so a stub ``librosa`` whose ``filters.mel`` returns this project's
``m2s.melspec.slaney_mel_basis`` stands in: the fixture pins the reference's padding, window, STFT, magnitude,
matmul and log on CPU in fp32, while the Slaney basis itself stays unpinned against librosa.  The basis is stored,
so the tests feed the engine and the float64 restatement (tests/melspec_ref.py) exactly what the reference saw.

``compute_mel_db`` (preprocess_rtmri_data.py:121-147) calls ``librosa.feature.melspectrogram`` proper and cannot be
run this way: that convention is checked against the float64 restatement only.

Cases: config C (256 / 101 / 200 / 20 mels, odd n_fft - hop; noise, tone stack, zero clip) and config A
(2048 / 420 / 2048 / 64 mels, sr 11413, fmax 8000) with one clip.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO / "mri-to-speech_amd"))
sys.path.insert(0, str(HERE.parent))

import melspec_ref as R  # noqa: E402
from m2s.melspec import slaney_mel_basis  # noqa: E402


def _stub_librosa():
    lib, util, filters = types.ModuleType("librosa"), types.ModuleType("librosa.util"), types.ModuleType("librosa.filters")
    util.normalize = lambda x, *a, **k: x
    filters.mel = lambda *, sr, n_fft, n_mels, fmin, fmax: slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)
    lib.util, lib.filters = util, filters
    sys.modules.update({"librosa": lib, "librosa.util": util, "librosa.filters": filters})


def _reference_module(ref_dir: Path):
    """meldataset.py executed from its source text: the repository's own plug-in module of the same name must not
    shadow it."""
    _stub_librosa()
    mod = types.ModuleType("reference_meldataset")
    src = (ref_dir / "meldataset.py").read_text(encoding="utf-8")
    exec(compile(src, str(ref_dir / "meldataset.py"), "exec"), mod.__dict__)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = _reference_module(Path(sys.argv[1]))
    out = {}
    for name, B in (("C", 3), ("A", 1)):
        c = R.CONFIGS[name]
        wav = R.signals(B, c["L"], c["sr"], seed=7)
        with torch.no_grad():
            mel = ref.mel_spectrogram(torch.from_numpy(wav), c["n_fft"], c["n_mels"], c["sr"], c["hop"], c["win"],
                                      c["fmin"], c["fmax"], center=False)
        out[f"{name}_wav"] = wav
        out[f"{name}_basis"] = ref.mel_basis[c["fmax"]].numpy()
        out[f"{name}_mel"] = mel.numpy().astype(np.float32)
        print(name, wav.shape, "->", tuple(mel.shape))
    path = HERE / "melspec.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
