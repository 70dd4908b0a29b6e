"""Grad-CAM engine, the checks that need no GPU: the C ABI surface, the torch ops and their fake
kernels, the band arithmetic, the command line's flags, and the size queries."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from m2s import _native as N
from m2s import gradcam, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2s_gradcam_create", "m2s_gradcam_destroy", "m2s_gradcam_n_mels", "m2s_gradcam_bn_stats_floats",
       "m2s_gradcam_chunk", "m2s_gradcam_workspace_bytes", "m2s_gradcam_forward", "m2s_gradcam_cotangents",
       "m2s_bilstm_train_backward_multi_workspace_bytes", "m2s_bilstm_train_backward_multi", "m2s_cam_heatmap")
REFERENCE_FLAGS = {"--video", "--mri-checkpoint", "--scaler-json", "--output-dir", "--mri-code-dir", "--n-mels",
                   "--sampling-rate", "--fmin", "--fmax", "--formant-band", "--target-frames", "--reduction", "--device"}


def _cli():
    spec = importlib.util.spec_from_file_location(
        "m2s_gradcam_cli", os.path.join(REPO, "mri-to-speech_amd", "scripts", "mri_gradcam_formant.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_entry_points_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m2s.h")).read(), flags=re.S)
    L = N.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/m2s.h"
        f = getattr(L, name)  # exported
        assert f.argtypes is not None, f"{name} has no ctypes signature in _native.py"
        assert name in N.exported_symbols()
    assert L.m2s_abi_version() == N.ABI_VERSION == 6
    assert L.m2s_gradcam_chunk() >= 1


def test_ops_registered_and_fakes_shape_meta_tensors():
    o = ops.load()
    assert ops.GRADCAM_OPS == ("gradcam", "gradcam_cotangents", "bilstm_train_backward_multi", "cam_heatmap")
    for name in ops.GRADCAM_OPS:
        assert hasattr(o, name), name
    m = lambda *s: torch.empty(*s, device="meta")
    hs, hf, pred, dp, st = o.gradcam(1, m(6, 96, 160), m(64), m(64), m(2, 64), [0, 5, 5], 0, True)
    assert hs.shape == (2, 6, 96, 160) and hf.shape == (2, 3, 96, 160) and pred.shape == (6, 64)
    assert dp.shape == (8, 6, 208) and st.shape == (ops.CAM_BN_STATS,)
    assert o.gradcam(1, m(6, 96, 160), m(64), m(64), m(2, 64), [], 1, False)[3].shape == (0, 6, 208)
    assert o.gradcam(1, m(6, 96, 160), m(64), m(64), m(2, 64), [], 1, False)[1].shape == (2, 0, 96, 160)
    assert o.gradcam_cotangents(m(5, 64), m(64), m(64), m(2, 64), [4, 0], 0).shape == (6, 5, 64)
    w = [m(2560, 208), m(2560, 640), m(2560), m(2560)] * 2
    assert o.bilstm_train_backward_multi(m(17, 9, 640), w, m(2, 1, 9, 2560), m(2, 1, 9, 640)).shape == (17, 9, 208)
    assert o.cam_heatmap(m(3, 7, 3, 5), m(5, 7), [0, 1, 1, 2, 0], 37, 50).shape == (5, 37, 50)


def test_band_arguments_default_bins():
    """The tool's defaults: 64 mels, 11413 Hz, 0..8000 Hz.  F1 300-900 Hz -> bins 9..20, F2 900-2500 Hz -> bins
    21..38; every band edge is more than 11 Hz from the nearest bin centre."""
    bands = gradcam.parse_band_arguments(None, 64, 11413, 0.0, 8000.0)
    assert list(bands) == ["F1", "F2"]
    assert bands["F1"].tolist() == list(range(9, 21))
    assert bands["F2"].tolist() == list(range(21, 39))
    freqs = gradcam.mel_bin_frequencies(64, 11413, 0.0, 8000.0)
    assert freqs.shape == (65,)
    assert np.all(np.diff(freqs) > 0) and 0 < freqs[0] < freqs[-1] < 8000.0
    for edge in (300.0, 900.0, 2500.0):
        assert np.abs(freqs - edge).min() > 11.0
    named = gradcam.parse_band_arguments(["lo:300-900", " F3 :2500-3500"], 64, 11413, 0.0, 8000.0)
    assert list(named) == ["lo", "F3"] and named["lo"].tolist() == bands["F1"].tolist()
    # fmax <= 0 or None: Nyquist
    assert np.allclose(gradcam.mel_bin_frequencies(64, 11413, 0.0, None), gradcam.mel_bin_frequencies(64, 11413, 0.0, 5706.5))


@pytest.mark.parametrize("spec", ["F1", "F1:300", "F1:a-b", "F1:900-300", "F1:300-300"])
def test_band_arguments_malformed(spec):
    with pytest.raises(ValueError):
        gradcam.parse_band_arguments([spec], 64, 11413, 0.0, 8000.0)


def test_band_arguments_empty_and_past_the_last_bin():
    with pytest.raises(ValueError, match="no mel bin"):
        gradcam.parse_band_arguments(["X:301-302"], 64, 11413, 0.0, 8000.0)
    top = gradcam.mel_bin_frequencies(64, 11413, 0.0, 8000.0)[64]
    with pytest.raises(ValueError, match="centre index 64"):  # the 65th centre has no mel bin
        gradcam.parse_band_arguments([f"hi:7000-{top + 1.0}"], 64, 11413, 0.0, 8000.0)
    ok = gradcam.parse_band_arguments([f"hi:7000-{top - 1.0}"], 64, 11413, 0.0, 8000.0)
    assert ok["hi"][-1] == 63


def test_cli_flags_are_the_reference_set_plus_all_frames():
    cli = _cli()
    flags = {s for a in cli.build_parser()._actions for s in a.option_strings} - {"-h", "--help"}
    assert flags == REFERENCE_FLAGS | {"--all-frames"}
    req = ["--video", "v.npy", "--mri-checkpoint", "c.pt", "--scaler-json", "s.json", "--output-dir", "o"]
    a = cli.parse_args(req)
    assert (a.n_mels, a.sampling_rate, a.fmin, a.fmax) == (64, 11413, 0.0, 8000.0)
    assert a.formant_band is None and a.target_frames == [] and a.reduction == "mean" and a.device == "auto"
    assert a.all_frames is False
    a = cli.parse_args(req + ["--formant-band", "F1:300-900", "--formant-band", "F2:900-2500", "--target-frames", "0", "5",
                              "--reduction", "sum", "--all-frames"])
    assert a.formant_band == ["F1:300-900", "F2:900-2500"] and a.target_frames == [0, 5] and a.all_frames
    with pytest.raises(SystemExit):
        cli.parse_args(req + ["--reduction", "max"])
    with pytest.raises(SystemExit):
        cli.parse_args(req[2:])  # --video is required


def test_backward_multi_workspace_query():
    L = N.lib()
    q = L.m2s_bilstm_train_backward_multi_workspace_bytes
    kc = L.m2s_gradcam_chunk()
    for bad in [(0, 9, 208, 640), (3, 0, 208, 640), (3, 9, 0, 640), (3, 9, 208, 0), (3, 9, 208, 636), (-1, 9, 208, 640)]:
        assert q(*bad) == 0, bad
    sizes = [q(k, 9, 208, 640) for k in (1, 2, kc - 1, kc, kc + 1, 4 * kc)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3]  # grows with K up to the chunk
    assert sizes[3] == sizes[4] == sizes[5]  # and not past it
    # one chunk: dG (2, kc, T, 4H) + W_hh^T (2, H, 4H) + dc (2, kc, H), each a whole number of 256-byte granules
    assert sizes[3] == 4 * (2 * kc * 9 * 2560 + 2 * 640 * 2560 + 2 * kc * 640)


def test_gradcam_workspace_query_rejects_without_a_handle():
    """0 for a null handle (no device here to create one); with a device tests/test_gpu_gradcam_engine.py checks
    the rejected shapes and that the size stops growing at K = chunk."""
    assert N.lib().m2s_gradcam_workspace_bytes(None, 6, 256, 256, 2, 2) == 0
