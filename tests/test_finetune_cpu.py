"""Fine-tuning, the parts that need no GPU: the yardstick (tests/finetune_ref.py) against the reference's criterion,
the dropout mix, the precondition of the GPU trajectory test, the exported checkpoint's layout, the C ABI / binding /
op registration, and the command line's flags and schedule."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import finetune_ref as FR  # tests/finetune_ref.py
import metrics_ref as MR   # tests/metrics_ref.py
from m2s import _native as N
from m2s import finetune, metrics, ops, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "metrics_ref.npz")
NEW = ("m2s_finetune_create", "m2s_finetune_destroy", "m2s_finetune_n_mels", "m2s_finetune_set_hyper",
       "m2s_finetune_workspace_bytes", "m2s_finetune_step", "m2s_finetune_forward", "m2s_finetune_grads",
       "m2s_finetune_export", "m2s_finetune_import_moments")
TRAJ = dict(kind="synth", lens=(4, 7, 36), W=4, M=64, lr=1e-3, seed=11, steps=5)  # as tests/test_gpu_finetune.py


def _cli():
    spec = importlib.util.spec_from_file_location(
        "m2s_finetune_cli", os.path.join(REPO, "mri-to-speech_amd", "scripts", "finetune_head.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the differentiable criterion against the reference's class ----------------------------------------------
@pytest.mark.parametrize("case", ["b3_t4_m64", "half_ramp", "m16", "t12_nomask", "t1", "t2"])
def test_criterion_matches_the_reference_class_and_the_restatement(case):
    g = np.load(GOLDEN)
    pred, target, ramp = g[f"{case}.pred"], g[f"{case}.target"], float(g[f"{case}.ramp"])
    mask = g[f"{case}.mask"]
    mask = None if mask.size == 0 else mask
    _, T, M = pred.shape
    fw, tw, coeffs, _ = metrics.train_weights(M, T, ramp)
    out = FR.criterion(torch.from_numpy(pred).double(), torch.from_numpy(target).double(), mask, fw, tw, coeffs)
    np.testing.assert_allclose([float(out[k]) for k in ("loss", "mse", "mae")], g[f"{case}.train"], rtol=2e-5, atol=0)
    want = MR.train_criterion(pred, target, mask, fw, tw, coeffs)
    for k in ("loss", "mse", "mae", "delta", "accel", "latest"):
        np.testing.assert_allclose(float(out[k]), want[k], rtol=1e-12, atol=1e-300, err_msg=k)


def test_criterion_gradient_is_the_hand_derivative():
    """The closed form the kernel implements (csrc/finetune.hip) against autograd, in float64."""
    rng = np.random.default_rng(0)
    P, W, M = 5, 4, 16
    pred = torch.from_numpy(rng.normal(size=(P, W, M))).requires_grad_(True)
    target = torch.from_numpy(rng.normal(size=(P, W, M)))
    mask = rng.choice([0.0, 0.5, 1.0], size=(P, W))
    fw, tw, coeffs, _ = metrics.train_weights(M, W, 0.7)
    FR.criterion(pred, target, mask, fw, tw, coeffs)["loss"].backward()
    d = (pred.detach() - target).numpy()
    fw64, tw64 = fw.astype(np.float64), tw.astype(np.float64)
    sfw = fw64.sum()
    k_mse = 2.0 / max(sfw * (tw64[None] * mask).sum(), 1e-6)
    rwd = tw64[None, 1:] * mask[:, 1:] * mask[:, :-1]
    rwa = tw64[None, 1:-1] * mask[:, 2:] * mask[:, 1:-1] * mask[:, :-2]
    k_d, k_a = 2.0 * coeffs[0] / max(sfw * rwd.sum(), 1e-6), 2.0 * coeffs[1] / max(sfw * rwa.sum(), 1e-6)
    k_l = 2.0 * coeffs[2] / max(P * sfw, 1e-6)
    g = k_mse * (tw64[None] * mask)[:, :, None] * d
    dl = (d[:, 1:] - d[:, :-1]) * rwd[:, :, None] * k_d
    g[:, 1:] += dl
    g[:, :-1] -= dl
    ac = (d[:, 2:] - 2 * d[:, 1:-1] + d[:, :-2]) * rwa[:, :, None] * k_a
    g[:, 2:] += ac
    g[:, 1:-1] -= 2 * ac
    g[:, :-2] += ac
    g[:, -1] += k_l * d[:, -1]
    np.testing.assert_allclose(g * fw64[None, None, :], pred.grad.numpy(), rtol=1e-10, atol=1e-14)


# ---- 2. the dropout mix ---------------------------------------------------------------------------------------------
def test_dropout_mix_statistics():
    shape = (38, 4, 640)
    n = int(np.prod(shape))
    k1, k2 = (finetune.dropout_keep(shape, 0.5, 3, t) for t in (1, 2))
    sd = np.sqrt(0.25 / n)
    assert abs(k1.mean() - 0.5) <= 5 * sd and abs(k2.mean() - 0.5) <= 5 * sd
    assert (k1 != k2).mean() > 1.0 / 3.0
    assert (finetune.dropout_keep(shape, 0.5, 4, 1) != k1).mean() > 1.0 / 3.0  # the seed moves it too
    assert finetune.dropout_keep(shape, 0.0, 3, 1).all()
    assert abs(finetune.dropout_keep(shape, 0.25, 3, 1).mean() - 0.75) <= 5 * np.sqrt(0.1875 / n)
    # the mix itself, by hand: element 0, seed 0, step 0 is the finaliser of 0
    assert int(finetune.dropout_mix([0], 0, 0)[0]) == 0
    x = (1 * 0x9E3779B1 + 3 * 0x85EBCA77 + 2 * 0xC2B2AE3D) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(finetune.dropout_mix([1], 3, 2)[0]) == x


# ---- 3. the reference trajectory: the precondition of the GPU trajectory test -------------------------------------
def test_reference_loss_falls_at_every_step():
    c = TRAJ
    sd = FR.state_of(c["kind"], c["M"])
    feats, target, mask = FR.inputs(c["lens"], c["M"], c["seed"])
    t = FR.RefTuner(sd, c["M"], c["lr"], 1e-4, 1.0, 0.0, 3, c["W"])
    losses = [t.step(feats, target, mask, c["lens"])["loss"] for _ in range(c["steps"])]
    print("float64 losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    moved = [float((t.state()[k] - torch.from_numpy(sd[k]).double().reshape(t.state()[k].shape)).abs().max()) for k in FR.KEYS]
    assert min(moved) > 0.0  # every one of the 10 tensors is updated


def test_reference_step_is_clip_then_adamw():
    """RefTuner against the float64 formula of adamw_update on its own gradients (what the GPU optimiser test uses)."""
    sd = FR.state_of("synth", 16)
    feats, target, mask = FR.inputs((4, 7), 16, 5)
    t = FR.RefTuner(sd, 16, 1e-3, 1e-2, 1e-3, 0.0, 3, 4)
    w0 = t.state()
    r = t.step(feats, target, mask, (4, 7))
    assert r["clip_coef"] < 1.0
    for k in FR.KEYS:
        w, _, _ = FR.adamw_update(w0[k].numpy(), t.grads[k].numpy(), 0.0, 0.0, 1, 1e-3, 1e-2, r["clip_coef"])
        np.testing.assert_allclose(t.state()[k].numpy(), w, rtol=1e-9, atol=1e-12, err_msg=k)


# ---- 4. export and symbols ----------------------------------------------------------------------------------------
def test_merged_state_dict_loads_strictly_into_the_plugin_module():
    from mri_acoustic_model import build_acoustic_model
    full = synth.synth_acoustic_state(0)
    tuned = {k: np.asarray(full[k]) + 1.0 for k in finetune.KEYS}
    merged = finetune.merge_state_dict(full, tuned)
    model = build_acoustic_model(n_mels=64, cnn_pretrained=False, rnn_hidden=640, dropout=0.5)
    assert set(merged) == set(full)
    model.load_state_dict(merged, strict=True)  # unfiltered: a missing or an unexpected key fails here
    assert set(finetune.KEYS) <= set(model.state_dict())
    for k in finetune.KEYS:
        assert torch.equal(model.state_dict()[k], torch.from_numpy(tuned[k])), k
    assert torch.equal(merged["cnn.backbone.conv_stem.weight"], torch.from_numpy(np.asarray(full["cnn.backbone.conv_stem.weight"])))
    with pytest.raises(N.M2SError):
        finetune.merge_state_dict(full, {k: tuned[k] for k in finetune.KEYS[:9]})


def test_new_entry_points_declared_exported_and_bound():
    raw = open(os.path.join(REPO, "include", "m2s.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = N.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/m2s.h"
        f = getattr(L, name)
        assert f.argtypes is not None, f"{name} has no ctypes signature in _native.py"
        assert name in N.exported_symbols()
    declared = set(re.findall(r"\b(m2s_finetune_\w+)\s*\(", src))
    assert declared == set(NEW)
    assert L.m2s_abi_version() == N.ABI_VERSION == 6  # additive: the version stays
    assert L.m2s_finetune_workspace_bytes(None, None, 0, 4) == 0 and L.m2s_finetune_n_mels(None) == 0
    assert [n for n, _ in N.FinetuneHyper._fields_] == ["lr", "weight_decay", "max_norm", "dropout", "seed", "delta_coeff",
                                                        "accel_coeff", "latest_coeff"]


def test_ops_registered_and_fakes_shape_meta_tensors():
    o = ops.load()
    assert ops.FINETUNE_OPS == ("finetune_step", "finetune_forward", "finetune_grads", "finetune_export",
                                "finetune_import")
    assert not set(ops.FINETUNE_OPS) & (set(ops.OPS) | set(ops.PAIR_OPS) | set(ops.METRIC_OPS))
    for name in ops.FINETUNE_OPS:
        assert hasattr(o, name), name
    assert ops.FINETUNE_KEYS[0] == "rnn.lstm.weight_ih_l0" and ops.FINETUNE_KEYS[5] == "rnn.lstm.weight_hh_l0_reverse"
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)  # noqa: E731
    assert o.finetune_step(1, m(47, 208), m(47, 64), None, [4, 7, 36], 4).shape == (len(ops.FINETUNE_SLOTS),)
    ops._FINETUNE_MELS[1] = 16
    try:
        assert o.finetune_forward(1, m(47, 208), [4, 7, 36], 4, False).shape == (38, 4, 16)
        g = o.finetune_grads(1, m(1))
        assert [tuple(t.shape) for t in g[:4]] == [(2560, 208), (2560, 640), (2560,), (2560,)]
        assert tuple(g[8].shape) == (16, 640) and tuple(g[9].shape) == (16,)
    finally:
        ops._FINETUNE_MELS.pop(1)
    with pytest.raises(N.M2SError):
        finetune.HeadTuner({}, device="cpu")


# ---- 5. the command line ------------------------------------------------------------------------------------------
def test_cli_flags_and_cpu_refusal():
    cli = _cli()
    req = ["--processed_dir", "p", "--mri_checkpoint", "c.pt", "--scaler_json", "s.json", "--out_ckpt", "o.pt"]
    a = cli.parse_args(req)
    assert (a.ref_frames, a.epochs, a.batch_size, a.lr, a.weight_decay, a.grad_clip, a.dropout, a.seed, a.dtype,
            a.max_train_steps, a.cpu) == (4, 80, 8, 1e-4, 1e-4, 1.0, 0.5, 42, None, None, False)
    a = cli.parse_args(req + ["--ref_frames", "8", "--epochs", "3", "--batch_size", "32", "--lr", "3e-4",
                              "--weight_decay", "0", "--grad_clip", "0", "--dropout", "0.1", "--seed", "1", "--dtype",
                              "bf16x3", "--max_train_steps", "10"])
    assert (a.ref_frames, a.epochs, a.batch_size, a.lr, a.weight_decay, a.grad_clip, a.dropout, a.seed, a.dtype,
            a.max_train_steps) == (8, 3, 32, 3e-4, 0.0, 0.0, 0.1, 1, "bf16x3", 10)
    for bad in (["--ref_frames", "17"], ["--dropout", "1.0"], ["--lr", "0"], ["--batch_size", "0"],
                ["--max_train_steps", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(req + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(req[:-2])
    with pytest.raises(SystemExit, match="no CPU path"):
        cli.finetune(cli.parse_args(req + ["--cpu"]))
    # the clip listing, scaler reading and split rule are validate_acoustic.py's, by import
    v = cli._validate_cli()
    assert v.split_indices(10, "train", 42) == torch.randperm(10, generator=torch.Generator().manual_seed(42)).tolist()[:8]


def test_plateau_follows_torch_and_the_trainers_stop_rules():
    cli = _cli()
    losses = [1.0, 0.9, 0.9, 0.91, 0.9, 0.95, 0.9, 0.92, 0.89999, 0.93, 0.8] + [0.85] * 30
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-4)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=5, min_lr=1e-6)
    s = cli.Plateau(1e-4)
    best, since = float("inf"), 0
    for i, v in enumerate(losses):
        ref.step(v)
        lr = s.step(v)
        assert lr == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12), i
        improved = v < best
        best, since = (v, 0) if improved else (best, since + 1)
        assert s.improved == improved and s.best == best
        if since >= 20:
            assert s.stop == "early"
            break
        assert s.stop is None
    else:
        raise AssertionError("the scripted sequence should stop early")
    s = cli.Plateau(3e-6)
    stops = [(s.step(1.0), s.stop) for _ in range(14)]
    assert stops[-1][0] == 1e-6 and stops[-1][1] == "min_lr" and stops[0][1] is None
    g = torch.Generator().manual_seed(1)
    b = cli.window_batches(10, 4, g)
    assert [len(x) for x in b] == [4, 4, 2] and sorted(torch.cat(b).tolist()) == list(range(10))
