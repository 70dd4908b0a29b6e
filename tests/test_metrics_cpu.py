"""Validation metrics and pair outputs, the parts that need no GPU: the float64 restatement against the reference's
own classes, the weights, the C ABI / binding / op registration, and the command line's split rule and flags."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as MR  # tests/metrics_ref.py
from m2s import _native as N
from m2s import metrics, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2s_acoustic_pairs_workspace_bytes", "m2s_bilstm_pairs", "m2s_acoustic_forward_pairs",
       "m2s_mel_metrics_workspace_bytes", "m2s_mel_metrics")
GOLDEN = os.path.join(REPO, "tests", "golden", "metrics_ref.npz")


def _cli():
    spec = importlib.util.spec_from_file_location(
        "m2s_validate_cli", os.path.join(REPO, "mri-to-speech_amd", "scripts", "validate_acoustic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the restatement against the reference's classes (tests/golden/make_metrics_golden.py) -------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_holds_every_case(golden):
    assert set(golden["cases"].tolist()) == {"b3_t4_m64", "half_ramp", "m16", "t12_nomask", "t1", "t2"}


@pytest.mark.parametrize("case", ["b3_t4_m64", "half_ramp", "m16", "t12_nomask", "t1", "t2"])
def test_restatement_matches_the_reference_classes(golden, case):
    """The reference computes in float32 (sums of a few hundred terms): 2e-5 relative is ~100 float32 ulps."""
    pred, target, ramp = golden[f"{case}.pred"], golden[f"{case}.target"], float(golden[f"{case}.ramp"])
    mask = golden[f"{case}.mask"]
    mask = None if mask.size == 0 else mask
    B, T, M = pred.shape
    fw, tw, coeffs, bands = metrics.train_weights(M, T, ramp)
    out, _ = MR.metrics(pred, target, mask, 0, fw, tw, coeffs, [bands[k] for k in metrics.BAND_NAMES])
    tr, ev, bd = golden[f"{case}.train"], golden[f"{case}.eval"], golden[f"{case}.band"]
    np.testing.assert_allclose([out["loss"], out["mse"], out["mae"]], tr, rtol=2e-5, atol=0)
    np.testing.assert_allclose([out["eval_loss"], out["eval_mse"], out["eval_mae"]], ev, rtol=2e-5, atol=0)
    for i, name in enumerate(metrics.BAND_NAMES):
        start, end = bands[name]
        if min(end, M) <= start:
            assert np.isnan(bd[i]) and out[f"band{i}"] == 0.0, name  # the reference leaves the band out
        else:
            np.testing.assert_allclose(out[f"band{i}"], bd[i], rtol=2e-5, atol=0, err_msg=name)
    assert out["groups"] == 1


def test_groups_are_the_reference_batches(golden):
    """group = 2 on five sequences: the sums of three separate batches, the last one short."""
    g = np.random.default_rng(5)
    pred, target = g.standard_normal((5, 4, 64)), g.standard_normal((5, 4, 64))
    mask = (g.random((5, 4)) > 0.3).astype(np.float64)
    fw, tw, coeffs, bands = metrics.train_weights(64, 4, 1.0)
    bl = [bands[k] for k in metrics.BAND_NAMES]
    whole, _ = MR.metrics(pred, target, mask, 2, fw, tw, coeffs, bl)
    parts = [MR.metrics(pred[s], target[s], mask[s], 0, fw, tw, coeffs, bl)[0] for s in (slice(0, 2), slice(2, 4), slice(4, 5))]
    for k in MR.SLOTS:
        np.testing.assert_allclose(whole[k], sum(p[k] for p in parts), rtol=1e-12, err_msg=k)
    assert whole["groups"] == 3


def test_mcd_like_restatement_properties():
    """No librosa here: the restatement is checked against what the formulas imply.  Equal inputs give 0; a
    constant dB offset c on every bin moves only coefficient 0, by c sqrt(M); top_db floors at max - 80."""
    g = np.random.default_rng(6)
    M = 64
    mean, std = g.uniform(-50, -30, M), g.uniform(5, 15, M)
    x = g.standard_normal((7, M))
    assert MR.mcd_like(x, x, mean, std) == 0.0
    c = 3.0
    got = MR.mcd_like(x + c / std, x, mean, std)
    np.testing.assert_allclose(got, (10 / np.log(10)) * np.sqrt(2) * c * np.sqrt(M), rtol=1e-12)
    db = np.array([[0.0, -50.0, -90.0, -120.0]])
    np.testing.assert_allclose(MR.power_to_db_of_db(db), [[0.0, -50.0, -80.0, -80.0]], atol=1e-9)
    np.testing.assert_allclose(MR.power_to_db_of_db(db - 30.0), [[-30.0, -80.0, -100.0, -100.0]], atol=1e-9)


# ---- 2. train_weights against values written out by hand ----------------------------------------------------------
def test_train_weights_n64_by_hand():
    fw, tw, coeffs, bands = metrics.train_weights(64, 10, 1.0)
    want = [2.0] * 6 + [3.0] * 10 + [2.4] * 16 + [1.6] * 16 + [1.8] * 16
    np.testing.assert_array_equal(fw, np.array(want, np.float32))
    np.testing.assert_array_equal(tw, np.array([1.6, 1.45, 1.3, 1.2, 1.15, 1.1, 1.05, 1.02, 1.0, 1.0], np.float32))
    assert coeffs == pytest.approx((0.45, 0.15, 0.4))
    assert bands == {"f0": (0, 6), "f1": (6, 16), "f2": (16, 32), "high": (48, 64)}
    fw, tw, coeffs, _ = metrics.train_weights(64, 2, 0.5)
    np.testing.assert_allclose(fw[[0, 6, 16, 32, 48]], [1.5, 2.0, 1.7, 1.3, 1.4], rtol=1e-6)
    np.testing.assert_allclose(tw, [1.3, 1.225], rtol=1e-6)
    assert coeffs == pytest.approx((0.375, 0.125, 0.3))
    fw, tw, coeffs, _ = metrics.train_weights(64, 3, 0.0)
    assert (fw == 1).all() and (tw == 1).all() and coeffs == pytest.approx((0.3, 0.1, 0.2))


def test_train_weights_n16_later_ranges_override():
    fw, tw, _, bands = metrics.train_weights(16, 4, 1.0)
    np.testing.assert_array_equal(fw, np.full(16, 1.8, np.float32))  # high = (0, 16) is applied last
    assert bands == {"f0": (0, 6), "f1": (6, 16), "f2": (16, 16), "high": (0, 16)}  # f2 empty, high overlaps both


def test_train_weights_past_max_frames_is_one():
    _, tw, _, _ = metrics.train_weights(64, 130, 1.0)
    assert tw.shape == (130,) and (tw[8:] == 1).all() and tw[0] == np.float32(1.6)
    assert metrics.ramp_of_step(60000) == 0.5 and metrics.ramp_of_step(10 ** 7) == 1.0


def test_result_dict_names_and_averages():
    acc = np.zeros(len(metrics.SLOTS))
    a = dict(zip(metrics.SLOTS, range(len(metrics.SLOTS))))
    acc[a["loss"]], acc[a["groups"]], acc[a["band2"]], acc[a["band3"]] = 6.0, 3.0, 9.0, 1.5
    acc[a["eval_mse"]], acc[a["mcd_sum"]], acc[a["mcd_count"]] = 12.0, 10.0, 4.0
    _, _, _, bands = metrics.train_weights(16, 4, 1.0)
    r = metrics.result_dict(acc, bands, 16)
    assert set(r) >= {"loss", "mse", "mae", "delta", "accel", "latest", "band", "eval", "mcd_like"}
    assert r["loss"] == 2.0 and r["eval"]["mse"] == 4.0 and r["mcd_like"] == 2.5 and r["batches"] == 3
    assert set(r["band"]) == {"f0", "f1", "high"} and r["band"]["high"] == 0.5  # f2 is empty at 16 mels
    acc[a["mcd_count"]] = 0
    assert metrics.result_dict(acc, bands, 16)["mcd_like"] is None
    with pytest.raises(N.M2SError):
        metrics.result_dict(np.zeros(len(metrics.SLOTS)), bands, 16)


def test_pair_index_is_the_reference_pair_order():
    idx = metrics.pair_index([5, 4], 4)
    assert idx.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [5, 6, 7, 8]]
    with pytest.raises(N.M2SError):
        metrics.pair_index([5, 3], 4)


def test_cpu_tensors_are_refused():
    with pytest.raises(N.M2SError):
        metrics.mel_metrics(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), None, 0, torch.ones(64), torch.ones(4),
                            (0.3, 0.1, 0.2), [], None, None, 13, torch.zeros(len(metrics.SLOTS), dtype=torch.float64))


# ---- 3. header, exports, bindings ---------------------------------------------------------------------------------
def test_new_entry_points_declared_exported_and_bound():
    raw = open(os.path.join(REPO, "include", "m2s.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = N.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/m2s.h"
        f = getattr(L, name)  # exported
        assert f.argtypes is not None, f"{name} has no ctypes signature in _native.py"
        assert name in N.exported_symbols()
    assert L.m2s_abi_version() == N.ABI_VERSION == 6  # additive: the version stays
    enum = re.search(r"enum m2s_metrics_slot \{(.*?)\}", src, flags=re.S).group(1)
    names = [t.split("=")[0].strip() for t in enum.split(",") if t.strip()]
    assert names == ["M2S_MET_" + s.upper() for s in N.METRICS_SLOTS] + ["M2S_METRICS_SLOTS"]
    for cite in ("train_mri_acoustic_model.py:57-167,263-277", "eval_mel.py:19-32,39-82,104-155",
                 "preprocess_rtmri_data.py:198-259"):
        assert cite in raw, cite


def test_size_queries_without_a_device():
    L = N.lib()
    assert L.m2s_mel_metrics_workspace_bytes(0) == 0
    assert L.m2s_mel_metrics_workspace_bytes(3) == 512  # 3 x 32 floats, to the 256-byte granule
    assert L.m2s_mel_metrics_workspace_bytes(1000) == 128000
    assert L.m2s_acoustic_pairs_workspace_bytes(None, None, 0, 0, 0, 4) == 0  # null handle


# ---- 4. ops and fake kernels --------------------------------------------------------------------------------------
def test_ops_registered_and_fakes_shape_meta_tensors():
    o = ops.load()
    assert ops.PAIR_OPS == ("bilstm_pairs", "acoustic_forward_pairs") and ops.METRIC_OPS == ("mel_metrics",)
    assert not set(ops.PAIR_OPS + ops.METRIC_OPS) & (set(ops.OPS) | set(ops.RAGGED_OPS) | set(ops.WINDOWED_OPS))
    for name in ops.PAIR_OPS + ops.METRIC_OPS:
        assert hasattr(o, name), name
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    y, mn = o.bilstm_pairs(1, m(16, 208), [4, 7, 5], 4, 640, 64)
    assert y.shape == (7, 4, 640) and mn.shape == (7, 4, 64)  # P = 1 + 4 + 2
    y, mn = o.bilstm_pairs(1, m(33, 208), [17, 16], 16, 640, 64)
    assert y.shape == (3, 16, 640) and mn.shape == (3, 16, 64)
    assert o.bilstm_pairs(1, m(9, 208), [4, 5], 1, 640, 64)[1].shape == (9, 1, 64)
    assert o.acoustic_forward_pairs(1, m(40, 96, 80), [36, 4], 4, 64).shape == (34, 4, 64)
    out, per_seq = o.mel_metrics(m(5, 4, 64), m(5, 4, 64), m(5, 4), 2, m(64), m(4), [0.45, 0.15, 0.4],
                                 [0, 6, 6, 16, 16, 32, 48, 64], m(64), m(64), 13,
                                 m(len(N.METRICS_SLOTS), dtype=torch.float64))
    assert out.shape == (len(N.METRICS_SLOTS),) and out.dtype == torch.float32 and per_seq.shape == (5, 3)
    out, _ = o.mel_metrics(m(2, 1, 16), m(2, 1, 16), None, 0, m(16), m(1), [0.3, 0.1, 0.2], [], None, None, 13,
                           m(len(N.METRICS_SLOTS), dtype=torch.float64))
    assert out.shape == (20,)


# ---- 5. the command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 10, 53])
@pytest.mark.parametrize("seed", [42, 7])
def test_split_rule_is_random_split(tmp_path, n, seed):
    """On a toy directory: the clips found, their pair count, and the subsets against torch's random_split."""
    from torch.utils.data import random_split
    cli = _cli()
    lens = {"clip10": 6, "clip2": 4, "clip1": 3, "clipA": n - 4 + 3}  # clip1 is shorter than the window
    for stem, T in lens.items():
        d = tmp_path / "samples" / stem
        d.mkdir(parents=True)
        np.save(d / "mri.npy", np.zeros((T, 8, 8), np.float32))
        np.save(d / "mel_db.npy", np.zeros((T, 64), np.float32))
        np.save(d / "mask.npy", np.ones((T,), np.float32))
    (tmp_path / "samples" / "broken").mkdir()
    clips = cli.list_clips(tmp_path / "samples", 4)
    assert [d.name for d, _ in clips] == ["clip2", "clip10", "clipA"]  # natural order, the short clip skipped
    total = sum(T - 3 for _, T in clips)
    assert total == n
    n_train, n_val = int(n * 0.8), int(n * 0.1)
    tr, va, te = random_split(range(n), [n_train, n_val, n - n_train - n_val],
                              generator=torch.Generator().manual_seed(seed))
    assert cli.split_indices(n, "val", seed) == list(va.indices)
    assert cli.split_indices(n, "test", seed) == list(te.indices)
    assert cli.split_indices(n, "all", seed) == list(range(n))


def test_natural_key_is_the_reference_rule():
    cli = _cli()
    names = ["s10", "s2", "s1_b", "s1_a10", "s1_a9", "x"]
    assert sorted(names, key=cli.natural_key) == ["s1_a9", "s1_a10", "s1_b", "s2", "s10", "x"]
    assert cli.natural_key("ab12cd003") == ["ab", 12, "cd", 3]


def test_cli_flags():
    cli = _cli()
    req = ["--processed_dir", "p", "--mri_checkpoint", "c.pt", "--scaler_json", "s.json"]
    a = cli.parse_args(req)
    assert (a.ref_frames, a.split, a.seed, a.val_bs, a.step, a.ramp, a.batch, a.dtype, a.out, a.cpu) == \
        (4, "all", 42, 8, None, None, 16, None, None, False)
    a = cli.parse_args(req + ["--split", "test", "--step", "60000", "--val_bs", "4", "--ref_frames", "8",
                              "--mri_code_dir", "x", "--dtype", "fp32", "--batch", "2", "--out", "r.json", "--seed", "1"])
    assert (a.split, a.step, a.val_bs, a.ref_frames, a.mri_code_dir, a.dtype, a.batch, a.out, a.seed) == \
        ("test", 60000, 4, 8, "x", "fp32", 2, "r.json", 1)
    for bad in (["--step", "5", "--ramp", "0.5"], ["--ramp", "1.5"], ["--ref_frames", "17"], ["--split", "train"],
                ["--val_bs", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(req + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["--processed_dir", "p"])
    with pytest.raises(SystemExit, match="no CPU path"):
        cli.validate(cli.parse_args(req + ["--cpu"]))
