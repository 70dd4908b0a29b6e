"""Grad-CAM engine on the GPU: its three kernels against CPU references, the engine end to end
against the oracle and against the existing autograd route, the workspace contract through the C ABI, the torch
ops, and the command line.  Shapes are a few frames: every case runs in seconds."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_hard as LH
import ws_harness as H
from m2s import _native, ops, synth
from m2s.gradcam import GradCam
from oracle import gradcam as oracle_gradcam

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = {"A": list(range(5, 20)), "B": list(range(21, 39))}
LSTM_NAMES = [f"rnn.lstm.{n}_l0{s}" for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _bits(a, b):
    return H.bits_equal(a, b)


def _kc():
    return _native.lib().m2s_gradcam_chunk()


@pytest.fixture(scope="module")
def sd3():
    return synth.synth_acoustic_state(3)


@pytest.fixture(scope="module")
def engine(sd3):
    return GradCam(sd3, DEV)


@pytest.fixture(scope="module")
def clip6():
    return torch.from_numpy(synth.synth_frames(1, 6, seed=11))  # (1, 6, 256, 256)


@pytest.fixture(scope="module")
def oracle_runs(sd3, clip6):
    """oracle.gradcam.gradcam per (reduction, band) on the 6-frame clip, computed once per session."""
    cache = {}
    mean, std = synth.synth_scaler()

    def get(reduction, band):
        key = (reduction, band)
        if key not in cache:
            cache[key] = oracle_gradcam.gradcam(_t(sd3), clip6[:, :, None], mean, std, BANDS[band], reduction, [0, 5])
        return cache[key]

    return get


# ---- 1. heat maps -------------------------------------------------------------------------------------------------
def _heatmap_cpu(feats, weights, frame, size):
    cam = torch.relu((weights[:, :, None, None] * feats[frame]).sum(dim=1, keepdim=True))
    c = F.interpolate(cam, size=size, mode="bilinear", align_corners=False)[:, 0]
    c = c - c.amin(dim=(-2, -1), keepdim=True)
    return c / (c.amax(dim=(-2, -1), keepdim=True) + 1e-6)


@pytest.mark.parametrize("chw,size", [((7, 3, 5), (37, 50)), ((208, 8, 8), (256, 256)), ((4, 1, 1), (4, 4)),
                                      ((5, 2, 3), (2, 3))])
def test_cam_heatmap_matches_interpolate(chw, size):
    """cam_heatmap vs weights . feats -> relu -> F.interpolate(bilinear, align_corners=False) -> min-max on the CPU,
    1e-4 absolute (the bar of test_gradcam_matches_oracle).  M = 5 maps over N = 3 frames, frame 1 twice; map 1 has
    all-negative weights on positive features (cam = 0), map 3 a constant cam of exactly 2 (one channel of ones,
    weight 2): both come out exactly zero.  The others have cams with spread of order one.  The worst |d| of each
    shape is printed; DESIGN.md §20 records what an MI355X gave."""
    Cc, h, w = chw
    g = torch.Generator().manual_seed(Cc * 100 + h)
    feats = torch.rand(3, Cc, h, w, generator=g)
    feats[2, 0] = 1.0
    weights = torch.randn(5, Cc, generator=g) * (4.0 / Cc ** 0.5)
    weights[1] = -torch.rand(Cc, generator=g) - 0.1
    weights[3] = 0.0
    weights[3, 0] = 2.0
    frame = [0, 1, 1, 2, 2]
    got = ops.load().cam_heatmap(feats.to(DEV), weights.to(DEV), frame, *size).cpu()
    ref = _heatmap_cpu(feats, weights, frame, size)
    assert got.shape == (5, *size)
    # A map whose source cam is constant (map 1: all zero, map 3: all 2, and every map of a 1 x 1 source) is held to
    # the exact answer, zero, not to the CPU: F.interpolate returns c -+ 1 ulp for a constant c when the scale is not
    # dyadic or c no power of two (a constant 2 at 3x5 -> 37x50 gives 1.99999976 .. 2.00000024), and the 1e-6 in the
    # min-max denominator turns that ulp into values up to 0.3.  Every other map is compared with the CPU at 1e-4.
    cam = torch.relu((weights[:, :, None, None] * feats[frame]).sum(dim=1))
    const = (cam.amax(dim=(1, 2)) == cam.amin(dim=(1, 2))).tolist()
    assert const[1] and const[3] and (h * w == 1 or const == [False, True, False, True, False])
    per_map = (got - ref).abs().amax(dim=(1, 2))
    print(f"cam_heatmap {chw} -> {size}: |d| per map {[f'{float(d):.3e}' for d in per_map]}, constant source {const}")
    for m in range(5):
        if const[m]:
            assert torch.count_nonzero(got[m]) == 0, m
        else:
            assert float(per_map[m]) <= 1e-4, (m, float(per_map[m]))
    if h * w > 1:
        for m in (0, 2, 4):  # spread maps are min-max normalised: they reach 0 and (nearly) 1
            assert float(got[m].min()) == 0.0 and float(got[m].max()) > 0.99
    with pytest.raises(IndexError):
        ops.load().cam_heatmap(feats.to(DEV), weights.to(DEV), [0, 1, 3, 2, 2], *size)


# ---- 2. many cotangents through one saved forward -------------------------------------------------------------------
def _cotangents(K, T, Hd, seed):
    """dense, all zeros, only t = 0, only t = T - 1, then dense ones"""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(K, T, Hd, generator=g)
    if K > 1:
        dy[1] = 0.0
    if K > 2:
        dy[2, 1:] = 0.0
    if K > 3:
        dy[3, :-1] = 0.0
    return dy


@pytest.mark.parametrize("T", [1, 2, 9])
def test_backward_multi_matches_single_backward_and_torch(sd3, T):
    """bilstm_train_backward_multi for K in {1, 3, KC + 1}: dx[k] within 1e-5 relative of bilstm_train_backward with
    that cotangent alone and of torch-CPU autograd through nn.LSTM (the bars of test_bilstm_autograd_matches_torch);
    the zero cotangent gives exactly zero; a cotangent of the K = KC + 1 call (first and second chunk) has the bits
    of a K = 1 call with it alone."""
    o = ops.load()
    kc = _kc()
    sd = _t(sd3)
    w = [sd[n].to(DEV) for n in LSTM_NAMES]
    x = torch.randn(1, T, 208, generator=torch.Generator().manual_seed(40 + T))
    y, gates, cells, hid = o.bilstm_train_forward(x.to(DEV), w)
    lstm = torch.nn.LSTM(208, 640, 1, batch_first=True, bidirectional=True)
    lstm.load_state_dict({k[len("rnn.lstm."):]: v for k, v in sd.items() if k.startswith("rnn.lstm.")})
    xr = x.clone().requires_grad_(True)
    yr = lstm(xr)[0]
    yr = yr[..., :640] + yr[..., 640:]
    full = _cotangents(kc + 1, T, 640, seed=7 * T)
    dx_full = None
    for K in (1, 3, kc + 1):
        dy = full[:K]
        dx = o.bilstm_train_backward_multi(dy.to(DEV), w, gates, cells)
        assert dx.shape == (K, T, 208)
        if K == kc + 1:
            dx_full = dx
        for k in range(K):
            single, _ = o.bilstm_train_backward(dy[k:k + 1].to(DEV), x.to(DEV), w, gates, cells, hid)
            (ref,) = torch.autograd.grad(yr, xr, dy[k:k + 1], retain_graph=True)
            if float(dy[k].abs().max()) == 0.0:
                assert torch.count_nonzero(dx[k]) == 0, "a zero cotangent must give exactly zero"
                continue
            assert _rel(dx[k].cpu(), single[0].cpu()) < 1e-5, (K, k)
            assert _rel(dx[k].cpu(), ref[0]) < 1e-5, (K, k)
    for j in (0, 2, kc - 1, kc):  # first chunk, its last column, and the second chunk
        alone = o.bilstm_train_backward_multi(full[j:j + 1].to(DEV), w, gates, cells)
        assert _bits(alone[0], dx_full[j]), f"cotangent {j} depends on its batch"
    shuffled = o.bilstm_train_backward_multi(full.flip(0).to(DEV), w, gates, cells)
    assert _bits(shuffled.flip(0), dx_full), "a cotangent's result depends on its position"


@pytest.mark.parametrize("kind", ["hard", "sat"])
@pytest.mark.parametrize("T", [9, 40])
def test_train_forward_and_backward_multi_on_hard_weights(kind, T):
    """bilstm_train_forward's y, gates, cells and hidden states against the float64 loop, and
    bilstm_train_backward_multi with K = 3 (dense, all zeros, only t = 0) against float64 torch autograd and against
    bilstm_train_backward, on the weights of tests/lstm_hard.py: "hard" has forget gates at 0.87 and
    W_hh at gain one, "sat" gates at exactly 0 and 1 and cell states up to T.  1e-5 relative to the largest element,
    the bar of the test above; everything finite, the zero cotangent exactly zero."""
    o = ops.load()
    sd = LH.state_of(kind)
    w = [sd[n].to(DEV) for n in LSTM_NAMES]
    x, _ = LH.train_inputs(1, T)
    y, gates, cells, hid = o.bilstm_train_forward(x.to(DEV), w)
    y64, st = LH.bilstm_f64(sd, x, state=True)
    fwd = {"y": _rel(y.cpu(), y64), "gates": _rel(gates.cpu(), st["gates"]), "cells": _rel(cells.cpu(), st["c"]),
           "hid": _rel(hid.cpu(), st["h"])}
    dy = _cotangents(3, T, 640, seed=7 * T)
    ref = LH.lstm_autograd(sd, x, dy[:, None])["dx"][:, 0]
    dx = o.bilstm_train_backward_multi(dy.to(DEV), w, gates, cells)
    assert dx.shape == (3, T, 208) and torch.isfinite(dx).all() and torch.isfinite(y).all()
    assert torch.count_nonzero(dx[1]) == 0, "a zero cotangent must give exactly zero"
    bwd = {}
    for k in (0, 2):
        single, _ = o.bilstm_train_backward(dy[k:k + 1].to(DEV), x.to(DEV), w, gates, cells, hid)
        bwd[f"dx[{k}]"] = _rel(dx[k].cpu(), ref[k])
        bwd[f"single[{k}]"] = _rel(single[0].cpu(), ref[k])
    print(f"train {kind} 1 x {T}: " + ", ".join(f"{k} {v:.1e}" for k, v in {**fwd, **bwd}.items()))
    for k, v in {**fwd, **bwd}.items():
        assert v < 1e-5, (k, v)


def test_backward_multi_launch_count(sd3):
    """T * ceil(K / KC) launches of the step kernel, never K * T: 9 for K = 6, 18 for K = KC + 1 at T = 9."""
    o = ops.load()
    kc = _kc()
    w = [_t(sd3)[n].to(DEV) for n in LSTM_NAMES]
    x = torch.randn(1, 9, 208, generator=torch.Generator().manual_seed(3)).to(DEV)
    _, gates, cells, _ = o.bilstm_train_forward(x, w)
    for K, want in ((6, 9), (kc + 1, 18)):
        dy = torch.randn(K, 9, 640, generator=torch.Generator().manual_seed(K)).to(DEV)
        torch.cuda.synchronize()
        _native.prof_enable(True)
        try:
            o.bilstm_train_backward_multi(dy, w, gates, cells)
            torch.cuda.synchronize()
            launches = _native.prof_launches()
        finally:
            _native.prof_enable(False)
        steps = [r for r in launches if r["name"] == "lstm_bptt_multi_step"]
        assert len(steps) == want, (K, len(steps))


# ---- 3. band cotangents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_cotangents_match_autograd(reduction):
    """gradcam_cotangents vs autograd of oracle/gradcam.py's band-power expression on the CPU: T = 5, two bands,
    frames [4, 0], 1e-5 relative per target."""
    mean, std = synth.synth_scaler()
    pred = torch.randn(1, 5, 64, generator=torch.Generator().manual_seed(9)).requires_grad_(True)
    fidx = [4, 0]
    mask = torch.zeros(2, 64)
    for b, idx in enumerate(BANDS.values()):
        mask[b, idx] = 1.0
    got = ops.load().gradcam_cotangents(pred[0].detach().to(DEV), torch.from_numpy(mean).to(DEV),
                                        torch.from_numpy(std).to(DEV), mask.to(DEV), fidx,
                                        0 if reduction == "mean" else 1).cpu()
    assert got.shape == (6, 5, 64)
    power = torch.pow(10.0, (pred * torch.from_numpy(std) + torch.from_numpy(mean)) / 10.0)
    k = 0
    for idx in BANDS.values():
        band_power = power.index_select(-1, torch.as_tensor(idx)).sum(-1)
        targets = [band_power.mean() if reduction == "mean" else band_power.sum()] + [band_power[:, t].mean() for t in fidx]
        for j, target in enumerate(targets):
            (ref,) = torch.autograd.grad(target, pred, retain_graph=True)
            assert _rel(got[k], ref[0]) < 1e-5, (k, _rel(got[k], ref[0]))
            if j > 0:  # a frame target touches its frame only
                other = [t for t in range(5) if t != fidx[j - 1]]
                assert torch.count_nonzero(got[k][other]) == 0
            k += 1


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_engine_matches_oracle(engine, clip6, oracle_runs, reduction):
    """Both bands and frames [0, 5] in one GradCam.run: heat maps within 1e-4 absolute of oracle.gradcam run per band,
    dpooled / P within 1e-4 relative of its feats.grad, pred_norm within 1e-4 relative."""
    mean, std = synth.synth_scaler()
    out = engine.run(clip6[0].to(DEV), mean, std, BANDS, reduction, [0, 5])
    for band in BANDS:
        rmaps, rper, rgrads = oracle_runs(reduction, band)
        r = out[band]
        assert r["heatmaps"].shape == (6, 256, 256) and set(r["per_frame"]) == {0, 5}
        d = float((r["heatmaps"].cpu() - rmaps).abs().max())
        print(f"gradcam engine {reduction} {band}: heat maps worst |d| {d:.3e}")
        assert d <= 1e-4
        for t in (0, 5):
            assert float((r["per_frame"][t].cpu() - rper[t]).abs().max()) <= 1e-4
        P = rgrads.shape[2] * rgrads.shape[3]
        assert r["dpooled"].shape == (3, 6, 208)
        got = (r["dpooled"][0].cpu() / P)[:, :, None, None].expand_as(rgrads)
        assert _rel(got, rgrads) < 1e-4
    sd = _t(synth.synth_acoustic_state(3))
    pred, _ = oracle_gradcam.forward_with_features({k: v.clone() for k, v in sd.items()}, clip6[:, :, None])
    assert _rel(out["A"]["pred_norm"].cpu(), pred[0].detach()) < 1e-4


@pytest.mark.parametrize("T,hw", [(1, (256, 256)), (3, (96, 160))])
def test_engine_other_shapes(engine, sd3, T, hw):
    """One frame, and a 96 x 160 clip whose last map is 3 x 5: neither square nor a power of two."""
    mean, std = synth.synth_scaler()
    fr = torch.from_numpy(synth.synth_frames(1, T, hw=hw, seed=13))
    out = engine.run(fr.to(DEV)[:, :, None], mean, std, {"A": BANDS["A"]}, "mean", [T - 1])  # (1,T,1,H,W) form
    rmaps, rper, rgrads = oracle_gradcam.gradcam(_t(sd3), fr[:, :, None], mean, std, BANDS["A"], "mean", [T - 1])
    assert tuple(rgrads.shape[2:]) == ((8, 8) if hw == (256, 256) else (3, 5))
    assert out["A"]["heatmaps"].shape == (T, *hw)
    assert float((out["A"]["heatmaps"].cpu() - rmaps).abs().max()) <= 1e-4
    assert float((out["A"]["per_frame"][T - 1].cpu() - rper[T - 1]).abs().max()) <= 1e-4


def test_engine_frame_lists_and_determinism(engine, clip6):
    mean, std = synth.synth_scaler()
    fr = clip6[0].to(DEV)
    none = engine.run(fr, mean, std, BANDS, "mean", ())
    assert all(r["per_frame"] == {} and r["dpooled"].shape == (1, 6, 208) for r in none.values())
    o = ops.load()
    mask = engine.band_mask(BANDS).to(DEV)
    mu, sd = torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
    a = o.gradcam(engine.handle, fr, mu, sd, mask, [5, 0, 5], 0, True)
    b = o.gradcam(engine.handle, fr, mu, sd, mask, [5, 0, 5], 0, True)
    for x, y in zip(a, b):
        assert _bits(x, y), "the same call twice must give the same bits"
    assert a[1].shape == (2, 3, 256, 256) and _bits(a[1][:, 0], a[1][:, 2]), "a repeated frame index, different maps"
    assert _bits(a[3][1], a[3][3]) and _bits(a[3][5], a[3][7])
    for b_, name in enumerate(BANDS):  # the whole-clip maps do not depend on the frame list
        assert _bits(a[0][b_], none[name]["heatmaps"])
    # the maps of frame targets chunk with the other cotangents: all frames at once = one by one
    every = engine.run(fr, mean, std, {"A": BANDS["A"]}, "sum", list(range(6)) * 3)  # K = 19: two chunks
    one = engine.run(fr, mean, std, {"A": BANDS["A"]}, "sum", [4])
    assert _bits(every["A"]["per_frame"][4], one["A"]["per_frame"][4])
    assert _bits(every["A"]["heatmaps"], one["A"]["heatmaps"])


def test_engine_argument_errors(engine, clip6):
    mean, std = synth.synth_scaler()
    fr = clip6[0].to(DEV)
    with pytest.raises(IndexError):
        engine.run(fr, mean, std, BANDS, "mean", [6])
    with pytest.raises(IndexError):
        ops.load().gradcam(engine.handle, fr, torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV),
                           engine.band_mask(BANDS).to(DEV), [-1], 0, False)
    with pytest.raises(ValueError):
        engine.run(fr, mean, std, {}, "mean")
    with pytest.raises(ValueError):
        engine.run(fr, mean, std, {"A": []}, "mean")
    with pytest.raises(ValueError):
        engine.run(fr, mean, std, BANDS, "max")
    with pytest.raises(_native.M2SError):
        engine.run(clip6[0], mean, std, BANDS)  # a CPU tensor
    with pytest.raises(ValueError):
        engine.run(torch.zeros(2, 6, 1, 256, 256, device=DEV), mean, std, BANDS)  # one clip per call


def test_engine_running_stats(sd3, clip6):
    """The module's BatchNorm buffers are untouched by default; update_running_stats=True applies torch's train-mode
    update once (num_batches_tracked 1, running statistics within 1e-4 relative of the oracle's)."""
    from mri_acoustic_model import build_acoustic_model
    m = build_acoustic_model(n_mels=64, cnn_pretrained=False, rnn_hidden=640, dropout=0.5).to(DEV)
    m.load_state_dict(_t(sd3), strict=False)
    m.eval()
    mean, std = synth.synth_scaler()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    cam = GradCam(m, DEV)
    cam.run(clip6[0].to(DEV), mean, std, BANDS)
    assert not m.training
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    cam.run(clip6[0].to(DEV), mean, std, BANDS, update_running_stats=True)
    ref = {k: v.clone() for k, v in _t(sd3).items()}
    oracle_gradcam.forward_with_features(ref, clip6[:, :, None])
    msd = m.state_dict()
    for key in ("cnn.backbone.bn1", "cnn.backbone.blocks.1.0.bn2", "cnn.backbone.blocks.5.9.bn3"):
        for b in ("running_mean", "running_var"):
            assert _rel(msd[f"{key}.{b}"].cpu(), ref[f"{key}.{b}"]) < 1e-4, (key, b)
        assert int(msd[f"{key}.num_batches_tracked"]) == 1


# ---- 5. agreement with the existing autograd route ------------------------------------------------------------------
def test_engine_agrees_with_autograd_route(engine, sd3, clip6):
    from mri_acoustic_model import build_acoustic_model
    from test_gpu_gradcam import run_gradcam
    m = build_acoustic_model(n_mels=64, cnn_pretrained=False, rnn_hidden=640, dropout=0.5).to(DEV)
    m.load_state_dict(_t(sd3), strict=False)
    m.eval()
    mean, std = synth.synth_scaler()
    out = engine.run(clip6[0].to(DEV), mean, std, BANDS, "mean", [0, 5])
    for band, idx in BANDS.items():
        maps, per, _ = run_gradcam(m, clip6[:, :, None].to(DEV), mean, std, idx, "mean", [0, 5])
        d = float((out[band]["heatmaps"] - maps).abs().max())
        print(f"engine vs autograd route, band {band}: worst |d| {d:.3e}")
        assert d <= 1e-4
        for t in (0, 5):
            assert float((out[band]["per_frame"][t] - per[t]).abs().max()) <= 1e-4


# ---- 6. workspace contract through the C ABI ------------------------------------------------------------------------
def _sync():
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_workspace_contract_gradcam_forward(engine):
    """m2s_gradcam_forward at T = 2, 64 x 96 frames, two bands, frames [1, 0, 1]: guards intact, outputs complete and
    bit-equal under every workspace fill, one granule short refused with nothing written; a frame index of T is
    refused the same way; the size query rejects what the call rejects and stops growing at K = chunk."""
    L = _native.lib()
    kc = _kc()
    T, Hh, Ww, nb, fidx = 2, 64, 96, 2, [1, 0, 1]
    Fn, K = len(fidx), nb * (1 + len(fidx))
    mean, std = synth.synth_scaler()
    mask = engine.band_mask(BANDS).numpy()
    frames = synth.synth_frames(1, T, hw=(Hh, Ww), seed=2)[0]
    h = engine._h
    nws = L.m2s_gradcam_workspace_bytes(h, T, Hh, Ww, nb, Fn)
    assert nws > 0 and nws % 256 == 0
    for bad in [(0, Hh, Ww, nb, Fn), (T, 16, Ww, nb, Fn), (T, Hh, Ww, 0, Fn), (T, Hh, Ww, nb, -1)]:
        assert L.m2s_gradcam_workspace_bytes(h, *bad) == 0, bad
    assert L.m2s_gradcam_workspace_bytes(h, T, Hh, Ww, 1, kc - 1) == L.m2s_gradcam_workspace_bytes(h, T, Hh, Ww, 1, 4 * kc - 1)
    assert L.m2s_gradcam_workspace_bytes(h, T, Hh, Ww, 1, 0) < L.m2s_gradcam_workspace_bytes(h, T, Hh, Ww, 1, kc - 1)
    arena = H.Arena(DEV, [("frames", "in", frames), ("mean", "in", mean), ("std", "in", std),
                          ("heat_seq", "out", (nb, T, Hh, Ww)), ("heat_frame", "out", (nb, Fn, Hh, Ww)),
                          ("pred", "out", (T, 64)), ("dpooled", "out", (K, T, 208)),
                          ("bn_stats", "out", (ops.CAM_BN_STATS,)), ("ws", "ws", nws)])
    cmask = mask.astype(np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def call(a, n=None, idx=fidx):
        ci = (C.c_int * len(idx))(*idx)
        return L.m2s_gradcam_forward(h, a.ptr("frames"), T, Hh, Ww, a.ptr("mean"), a.ptr("std"), cmask, nb, ci, len(idx), 0,
                                     a.ptr("heat_seq"), a.ptr("heat_frame"), a.ptr("pred"), a.ptr("dpooled"),
                                     a.ptr("bn_stats"), a.ptr("ws"), a.nbytes("ws") if n is None else n, _stream())

    rep = H.check_contract(arena, call, sync=_sync, what="gradcam_forward")
    assert rep.deterministic
    H.check_undersized(arena, call, rep.outs["zero"], sync=_sync, what="gradcam_forward")
    arena.prepare("nan")
    _sync()
    assert call(arena, idx=[1, T, 0]) == H.M2S_E_ARG  # same count, one index outside the clip
    _sync()
    assert not arena.violations(outputs_written=False)
    assert all(bool(torch.isnan(t).all()) for t in arena.outputs().values()), "a refused call wrote an output"
    bad_mask = mask.astype(np.float32).copy()
    bad_mask[1] = 0.0
    assert L.m2s_gradcam_forward(h, arena.ptr("frames"), T, Hh, Ww, arena.ptr("mean"), arena.ptr("std"),
                                 bad_mask.ctypes.data_as(C.POINTER(C.c_float)), nb, (C.c_int * 3)(*fidx), 3, 0,
                                 arena.ptr("heat_seq"), arena.ptr("heat_frame"), arena.ptr("pred"), arena.ptr("dpooled"),
                                 arena.ptr("bn_stats"), arena.ptr("ws"), nws, _stream()) == H.M2S_E_ARG
    assert all(bool(torch.isnan(t).all()) for t in arena.outputs().values())
    # the results of the guarded run are the op's
    got = ops.load().gradcam(engine.handle, torch.from_numpy(frames).to(DEV), torch.from_numpy(mean).to(DEV),
                             torch.from_numpy(std).to(DEV), torch.from_numpy(mask).to(DEV), fidx, 0, True)
    for name, t in zip(("heat_seq", "heat_frame", "pred", "dpooled", "bn_stats"), got):
        assert _bits(t, rep.outs["zero"][name]), name


def test_workspace_contract_backward_multi(sd3):
    L = _native.lib()
    kc = _kc()
    K, T, Cc, Hd = kc + 1, 3, 208, 640
    sd = _t(sd3)
    w = [sd[n] for n in LSTM_NAMES]
    x = torch.randn(1, T, Cc, generator=torch.Generator().manual_seed(5))
    _, gates, cells, _ = ops.load().bilstm_train_forward(x.to(DEV), [t.to(DEV) for t in w])
    dy = _cotangents(K, T, Hd, seed=6)
    nws = L.m2s_bilstm_train_backward_multi_workspace_bytes(K, T, Cc, Hd)
    arena = H.Arena(DEV, [("dy", "in", dy), ("gates", "in", gates.cpu()), ("cells", "in", cells.cpu())] +
                    [(f"w{i}", "in", t) for i, t in enumerate(w)] + [("dx", "out", (K, T, Cc)), ("ws", "ws", nws)])

    def call(a, n=None):
        wp = (C.c_void_p * 8)(*[a.ptr(f"w{i}") for i in range(8)])
        return L.m2s_bilstm_train_backward_multi(a.ptr("dy"), K, T, Cc, Hd, wp, a.ptr("gates"), a.ptr("cells"),
                                                 a.ptr("dx"), a.ptr("ws"), a.nbytes("ws") if n is None else n, _stream())

    rep = H.check_contract(arena, call, sync=_sync, what="bilstm_train_backward_multi")
    assert rep.deterministic
    H.check_undersized(arena, call, rep.outs["zero"], sync=_sync, what="bilstm_train_backward_multi")
    got = ops.load().bilstm_train_backward_multi(dy.to(DEV), [t.to(DEV) for t in w], gates, cells)
    assert _bits(got, rep.outs["zero"]["dx"])


def test_guarded_cam_heatmap():
    """m2s_cam_heatmap has no workspace: guards around its inputs and its output, every element written, for an
    output whose maps are 16-byte aligned (4 x 8) and one whose maps are not (5 x 7)."""
    L = _native.lib()
    g = torch.Generator().manual_seed(1)
    feats, weights = torch.rand(2, 6, 2, 3, generator=g), torch.randn(3, 6, generator=g)
    frame = torch.tensor([1, 0, 1], dtype=torch.int32)
    for size in ((4, 8), (5, 7)):
        arena = H.Arena(DEV, [("feats", "in", feats), ("weights", "in", weights), ("frame", "in", frame),
                              ("out", "out", (3, *size))])
        arena.prepare("zero")
        _sync()
        rc = L.m2s_cam_heatmap(arena.ptr("feats"), 2, 6, 2, 3, arena.ptr("weights"), arena.ptr("frame"), 3, size[0], size[1],
                               arena.ptr("out"), _stream())
        _sync()
        assert rc == H.M2S_OK
        assert not arena.violations()
        ref = _heatmap_cpu(feats, weights, frame.tolist(), size)
        assert float((arena.view("out").cpu() - ref).abs().max()) <= 1e-4
    assert L.m2s_cam_heatmap(arena.ptr("feats"), 2, 6, 200, 200, arena.ptr("weights"), arena.ptr("frame"), 3, 5, 7,
                             arena.ptr("out"), _stream()) == H.M2S_E_ARG  # the source map must fit the LDS


# ---- 7. opcheck -----------------------------------------------------------------------------------------------------
def test_opcheck_gradcam_ops(engine, sd3):
    o = ops.load()
    mean, std = (torch.from_numpy(v).to(DEV) for v in synth.synth_scaler())
    fr = torch.from_numpy(synth.synth_frames(1, 2, hw=(64, 64), seed=4)[0]).to(DEV)
    mask = engine.band_mask(BANDS).to(DEV)
    w = [_t(sd3)[n].to(DEV) for n in LSTM_NAMES]
    x = torch.randn(1, 2, 208, device=DEV)
    _, gates, cells, _ = o.bilstm_train_forward(x, w)
    cases = {
        "gradcam": [(engine.handle, fr, mean, std, mask, [1], 0, True), (engine.handle, fr, mean, std, mask, [], 1, False)],
        "gradcam_cotangents": [(torch.randn(2, 64, device=DEV), mean, std, mask, [1, 0], 0)],
        "bilstm_train_backward_multi": [(torch.randn(2, 2, 640, device=DEV), w, gates, cells)],
        "cam_heatmap": [(torch.rand(2, 4, 2, 2, device=DEV), torch.randn(3, 4, device=DEV), [0, 1, 1], 6, 8)],
    }
    assert set(cases) == set(ops.GRADCAM_OPS)
    for name, argsets in cases.items():
        for args in argsets:
            torch.library.opcheck(getattr(o, name).default, args,
                                  test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))


# ---- 8. command line ------------------------------------------------------------------------------------------------
def _cli(name):
    spec = importlib.util.spec_from_file_location(
        "m2s_gradcam_cli", os.path.join(REPO, "mri-to-speech_amd", "scripts", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(tmp_path, sd3):
    """A 6-frame .npy stack, a synth checkpoint and a scaler.json: the sequence files are (6, 256, 256) and have the
    bits of GradCam.run on the same frames; the PNGs exist when matplotlib imports; --all-frames writes the per-frame
    stack, whose rows 0 and 5 are the --target-frames maps."""
    cli = _cli("mri_gradcam_formant.py")
    mean, std = synth.synth_scaler()
    torch.save({"model_state_dict": _t(sd3)}, tmp_path / "best.pt")
    (tmp_path / "scaler.json").write_text(json.dumps({"mean": mean.tolist(), "std": std.tolist()}))
    np.save(tmp_path / "clip.npy", np.random.default_rng(0).integers(0, 256, size=(6, 256, 256), dtype=np.uint8))
    base = ["--video", str(tmp_path / "clip.npy"), "--mri-checkpoint", str(tmp_path / "best.pt"),
            "--scaler-json", str(tmp_path / "scaler.json"),
            "--mri-code-dir", os.path.join(REPO, "mri-to-speech_amd", "mri2speech_code")]
    res = cli.main(base + ["--output-dir", str(tmp_path / "a"), "--target-frames", "0", "5"])
    assert list(res) == ["F1", "F2"]
    frames = cli.load_video_frames(tmp_path / "clip.npy")
    bands = cli.parse_band_arguments(None, 64, 11413, 0.0, 8000.0)
    want = GradCam(sd3, DEV).run(frames.to(DEV), mean, std, bands, "mean", [0, 5])
    try:
        import matplotlib  # noqa: F401
        have_plt = True
    except ImportError:
        have_plt = False
    for band in ("F1", "F2"):
        seq = np.load(tmp_path / "a" / f"gradcam_{band}_sequence.npy")
        assert seq.shape == (6, 256, 256) and seq.dtype == np.float32
        assert _bits(torch.from_numpy(seq), want[band]["heatmaps"].cpu())
        if have_plt:
            names = [f"gradcam_{band}_average.png"] + [f"gradcam_{band}_frame{t:04d}{s}.png" for t in (0, 5)
                                                        for s in ("", "_detail")]
            for n in names:
                assert (tmp_path / "a" / n).stat().st_size > 0, n
    cli.main(base + ["--output-dir", str(tmp_path / "b"), "--all-frames"])
    for band in ("F1", "F2"):
        per = np.load(tmp_path / "b" / f"gradcam_{band}_perframe.npy")
        assert per.shape == (6, 256, 256)
        for t in (0, 5):
            assert _bits(torch.from_numpy(per[t]), want[band]["per_frame"][t].cpu())
        assert _bits(torch.from_numpy(np.load(tmp_path / "b" / f"gradcam_{band}_sequence.npy")), want[band]["heatmaps"].cpu())
        assert not list((tmp_path / "b").glob(f"gradcam_{band}_frame*.png"))
