"""Pair outputs of the windowed engine on the GPU (include/m2s.h "pair outputs"): the model on every
window of W consecutive frames of a clip, all W rows kept.

Expected values are tests/windowed_ref.py's M(x) run on every window (imported, not restated), at the bars of
tests/test_gpu_windowed.py's ``_check`` (imported).  The bit-identity tests tie the new rows to the existing
``latest`` output: row W - 1 of a pair and ``latest``'s row of the same frame are the same cells of the same step
launches, so a wrong window, step or direction index shows as a bit difference.  Frames are 96 x 80.  GPU box only.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR  # tests/metrics_ref.py
import windowed_ref as R  # tests/windowed_ref.py
import ws_harness as H    # tests/ws_harness.py
from m2s import _native, metrics, ops, runtime, synth
from oracle import effnet
from test_gpu_windowed import _check, _dev, _feats, ac, ac_sd, sd, voc  # noqa: F401 - fixtures and the model bars

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HW = (96, 80)
ERRORS = (_native.M2SError, RuntimeError)
CASES = {"w4": (4, [4, 7, 5]), "w1": (1, [3, 2]), "w16": (16, [17, 16]), "w4_tile": (4, [36, 4])}  # 33 pairs: tile + 1


def pairs_ref(sd, clips, W):
    """(y (P, W, 640), mel_norm (P, W, 64)): M on every window, clips in order, windows ascending."""
    ys, ms = [], []
    for x in clips:
        for i in range(x.shape[0] - W + 1):
            y, m = R.M(sd, x[i:i + W])
            ys.append(y)
            ms.append(m)
    return torch.stack(ys).numpy(), torch.stack(ms).numpy()


@pytest.fixture(scope="module")
def refs(sd):
    cache = {}

    def get(case):
        if case not in cache:
            W, lens = CASES[case]
            feats = _feats(lens, seed=len(lens) + 10 * W)
            cache[case] = (feats, *pairs_ref(sd, feats, W))
        return cache[case]
    return get


# ---- 1. against the oracle on every window ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,case", [(d, c) for d in ("fp32", "bf16x3") for c in CASES] + [("bf16", "w4")])
def test_bilstm_pairs_vs_oracle(ac, refs, case, dtype):
    W, lens = CASES[case]
    feats, y_ref, m_ref = refs(case)
    eng = ac(dtype)
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        y, mn = eng.bilstm_pairs(_dev(feats), None, W)
        eng.check()
        rec = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    names = [r["name"] for r in rec]
    assert names.count("lstm_window_pairs_kernel") == 1 and "lstm_window_mean_kernel" not in names, names
    assert len([n for n in names if n.startswith("lstm_window_step_kernel")]) == W - 1
    P = sum(n - W + 1 for n in lens)
    assert y.shape == (P, W, 640) and mn.shape == (P, W, 64)
    _check(f"bilstm_pairs {case} {dtype} mel_norm", mn, m_ref)
    _check(f"bilstm_pairs {case} {dtype} y", y, y_ref)


# ---- 2. ties to latest and mean --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(CASES))
def test_last_row_of_a_pair_is_latest_bit_for_bit(ac, refs, case, dtype):
    W, lens = CASES[case]
    feats = _dev(refs(case)[0])
    eng = ac(dtype)
    y, mn = eng.bilstm_pairs(feats, None, W)
    yl, ml = eng.bilstm_windowed(feats, None, W, "latest")
    eng.check()
    off = np.cumsum([0] + lens[:-1])
    rows = torch.cat([torch.arange(o + W - 1, o + n) for o, n in zip(off.tolist(), lens)]).to(DEV)  # frames with a full window
    assert torch.equal(y[:, W - 1], yl[rows]), float((y[:, W - 1] - yl[rows]).abs().max())
    assert torch.equal(mn[:, W - 1], ml[rows]), float((mn[:, W - 1] - ml[rows]).abs().max())
    if W > 1:  # and the other rows are other numbers: the rows of a pair are not copies of one another
        assert float((y[:, 0] - y[:, W - 1]).abs().max()) > 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_averaging_the_pair_rows_per_frame_is_mean(ac, refs, dtype):
    W, lens = CASES["w4"]
    feats = _dev(refs("w4")[0])
    eng = ac(dtype)
    y, mn = eng.bilstm_pairs(feats, None, W)
    ym, mm = eng.bilstm_windowed(feats, None, W, "mean")
    eng.check()
    y, mn = y.cpu().double(), mn.cpu().double()
    ys, ms, base = [], [], 0
    for n in lens:
        nwin = n - W + 1
        for t in range(n):
            ws = range(max(0, t - W + 1), min(t, nwin - 1) + 1)  # ascending window order
            ys.append(torch.stack([y[base + w, t - w] for w in ws]).mean(0))
            ms.append(torch.stack([mn[base + w, t - w] for w in ws]).mean(0))
        base += nwin
    _check(f"pairs averaged vs mean {dtype} y", ym, torch.stack(ys).float().numpy())
    _check(f"pairs averaged vs mean {dtype} mel_norm", mm, torch.stack(ms).float().numpy())


# ---- 3. invariance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_permuting_the_clips_permutes_the_pairs(ac, dtype):
    eng, W, lens = ac(dtype), 4, [7, 4, 9, 5]
    clips = _dev(_feats(lens, seed=700))
    counts = [n - W + 1 for n in lens]
    y, mn = eng.bilstm_pairs(clips, None, W)
    perm = [2, 0, 3, 1]
    yp, mp = eng.bilstm_pairs([clips[i] for i in perm], None, W)
    eng.check()
    ys, ms = torch.split(y, counts), torch.split(mn, counts)
    yps, mps = torch.split(yp, [counts[i] for i in perm]), torch.split(mp, [counts[i] for i in perm])
    for pos, i in enumerate(perm):
        assert torch.equal(yps[pos], ys[i]) and torch.equal(mps[pos], ms[i]), i


# ---- 4. composition --------------------------------------------------------------------------------------------------
def _frames(lens, seed=100):
    return torch.from_numpy(np.concatenate([synth.synth_frames(1, n, hw=HW, seed=seed + 17 * b)[0]
                                            for b, n in enumerate(lens)]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_forward_pairs_is_effnet_then_bilstm_pairs(ac, dtype):
    eng, lens = ac(dtype), [7, 4, 5]
    fr = _frames(lens).to(DEV)
    mn = eng.forward_pairs(fr, lens, 4)
    _, want = eng.bilstm_pairs(eng.effnet(fr), lens, 4)
    eng.check()
    assert mn.shape == (7, 4, 64) and torch.equal(mn, want)
    assert torch.equal(eng.forward_pairs(fr[:, None], lens, 4), mn)  # (N,1,H,W) frames


def test_plugin_forward_pairs(ac, ac_sd):
    from mri_acoustic_model import build_acoustic_model
    model = build_acoustic_model(n_mels=64).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ac_sd.items()}, strict=False)
    model.m2s_dtype = "bf16x3"
    fr = _frames([6, 6], seed=200).view(2, 6, 1, *HW).to(DEV)
    with pytest.raises(NotImplementedError):
        model.train().forward_pairs(fr, 4)
    model.eval()
    out = model.forward_pairs(fr, 4)
    assert out.shape == (2, 3, 4, 64)
    assert torch.equal(out.reshape(6, 4, 64), ac("bf16x3").forward_pairs(fr.view(12, *HW), [6, 6], 4))
    packed = model.forward_pairs([fr[0], fr[1, :5]], 4)
    assert packed.shape == (5, 4, 64) and torch.equal(packed[:3], out[0])
    with pytest.raises(ValueError):
        model.forward_pairs(fr[:, :3], 4)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------
BAD = {"short_clip": dict(lens=[3, 2], window=3), "window0": dict(lens=[3, 2], window=0), "window17": dict(lens=[3, 2], window=17),
       "empty": dict(lens=[]), "sum_short": dict(lens=[4]), "sum_long": dict(lens=[4, 4]), "zero_length": dict(lens=[5, 0])}


@pytest.mark.parametrize("bad", list(BAD))
def test_argument_errors_raise_before_any_launch(ac, bad):
    a, o = ac("bf16x3"), ops.load()
    kw = dict(window=4)
    kw.update(BAD[bad])  # short_clip: the second clip has 2 rows, the window 3
    fr, ft = torch.zeros(5, *HW, device=DEV), torch.zeros(5, 208, device=DEV)
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        for call in (lambda: o.bilstm_pairs(a.handle, ft, kw["lens"], kw["window"], 640, 64),
                     lambda: o.acoustic_forward_pairs(a.handle, fr, kw["lens"], kw["window"], 64)):
            with pytest.raises(ERRORS):
                call()
        assert _native.prof_launches() == []
    finally:
        _native.prof_enable(False)
    a.check()
    if bad.startswith("sum_"):
        return  # the query takes no row count: these lengths are valid on their own
    cl = (C.c_int * max(1, len(kw["lens"])))(*kw["lens"])
    assert _native.lib().m2s_acoustic_pairs_workspace_bytes(a._h, cl, len(kw["lens"]), 0, 0, kw["window"]) == 0


# ---- 6. workspace contract through the C ABI -------------------------------------------------------------------------
def _contract(eng, arena, call, what):
    L = _native.lib()
    sync = lambda: torch.cuda.synchronize(DEV)
    status = lambda: L.m2s_acoustic_status(eng._h)
    (ws,) = arena.names("ws")
    rep = H.check_contract(arena, lambda a: call(a, a.nbytes(ws)), sync=sync, status=status, what=what)
    assert rep.deterministic, what
    H.check_undersized(arena, call, rep.outs["zero"], sync=sync, status=status, what=what)  # exact to the granule
    return rep


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("W", [4, 1])
def test_workspace_contract_bilstm_pairs(ac, sd, dtype, W):
    lens = [7, 4, 5]
    eng, L = ac(dtype), _native.lib()
    feats = _feats(lens, seed=3)
    N, P = sum(lens), sum(n - W + 1 for n in lens)
    cl = (C.c_int * len(lens))(*lens)
    nws = L.m2s_acoustic_pairs_workspace_bytes(eng._h, cl, len(lens), 0, 0, W)
    assert nws > 0
    arena = H.Arena(DEV, [("feats", "in", torch.cat(feats)), ("y", "out", (P, W, 640)), ("mel_norm", "out", (P, W, 64)),
                          ("ws", "ws", nws)])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(a, n):
        return L.m2s_bilstm_pairs(eng._h, a.ptr("feats"), cl, len(lens), N, W, a.ptr("y"), a.ptr("mel_norm"), a.ptr("ws"),
                                  n, stream)

    what = f"bilstm_pairs W={W} {dtype} {lens}"
    rep = _contract(eng, arena, call, what)
    y_ref, m_ref = pairs_ref(sd, feats, W)
    _check(f"{what} mel_norm", rep.outs["nan"]["mel_norm"], m_ref)
    _check(f"{what} y", rep.outs["nan"]["y"], y_ref)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_workspace_contract_acoustic_forward_pairs(ac, dtype):
    lens, W = [7, 4, 5], 4
    eng, L = ac(dtype), _native.lib()
    fr = _frames(lens)
    N, P = sum(lens), sum(n - W + 1 for n in lens)
    cl = (C.c_int * len(lens))(*lens)
    nws = L.m2s_acoustic_pairs_workspace_bytes(eng._h, cl, len(lens), HW[0], HW[1], W)
    assert nws > L.m2s_acoustic_pairs_workspace_bytes(eng._h, cl, len(lens), 0, 0, W) > 0
    arena = H.Arena(DEV, [("frames", "in", fr), ("mel_norm", "out", (P, W, 64)), ("ws", "ws", nws)])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(a, n):
        return L.m2s_acoustic_forward_pairs(eng._h, a.ptr("frames"), cl, len(lens), N, HW[0], HW[1], W, a.ptr("mel_norm"),
                                            a.ptr("ws"), n, stream)

    rep = _contract(eng, arena, call, f"acoustic_forward_pairs {dtype} {lens}")
    want = eng.forward_pairs(fr.to(DEV), lens, W)
    eng.check()
    assert torch.equal(rep.outs["nan"]["mel_norm"], want)


# ---- 7. opcheck ------------------------------------------------------------------------------------------------------
def test_opcheck_both_pair_ops(ac):
    a, o = ac("bf16x3"), ops.load()
    lens = [5, 4]
    cases = {"bilstm_pairs": [(a.handle, torch.randn(9, 208, device=DEV), lens, 4, 640, 64),
                              (a.handle, torch.randn(9, 208, device=DEV), lens, 1, 640, 64)],
             "acoustic_forward_pairs": [(a.handle, _frames(lens).to(DEV), lens, 4, 64)]}
    assert set(cases) == set(ops.PAIR_OPS)
    for name, argsets in cases.items():
        for args in argsets:
            torch.library.opcheck(getattr(o, name).default, args,
                                  test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))


# ---- 8. the driver ---------------------------------------------------------------------------------------------------
def test_pipeline_validate_vs_oracle_windows(ac, voc, sd):
    """Pipeline.validate on two synthetic clips, select + group = 8, against tests/metrics_ref.py on the oracle's
    windows (oracle CNN, then M on every window).

    How the bars combine.  The metric bar (tests/test_gpu_metrics.py: twice (terms per lane + 8 + 4) 2^-24, relative)
    covers the kernel on the engine's own predictions.  The engine's predictions differ from the oracle's by at most
    eps = 1e-4 per element (the model bar of ``_check``).  A weighted mean square Q is the square of a seminorm, so
    |sqrt(Q') - sqrt(Q)| <= the seminorm of the perturbation <= eps_k, i.e. |Q' - Q| <= 2 eps_k sqrt(Q) + eps_k^2, with
    eps_k = eps for mse and latest, 2 eps for delta (a difference of two rows), 4 eps for accel (1 + 2 + 1), and
    eps sqrt(M) for eval's mse, whose denominator counts frames, not frames x M.  The weighted mean absolute values
    move by at most eps (mae, bands) or M eps (eval's mae).  loss adds its terms' bounds with its coefficients.
    The MCD-like moves by at most (10 / ln 10) sqrt(2) |c' - c|_2 <= that constant x std_max eps sqrt(M) (the
    orthonormal DCT does not lengthen a vector, truncation and the floors only shorten it)."""
    from test_gpu_metrics import loss_bar, mcd_bar
    W, lens, eps = 4, [9, 6], 1e-4
    mean, std = synth.synth_scaler()
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    pipe = runtime.Pipeline(ac("bf16x3"), voc("bf16x3"), mean, std)
    fr = _frames(lens, seed=400)
    g = np.random.default_rng(9)
    N = sum(lens)
    mel_db = (mean + std * g.standard_normal((N, 64))).astype(np.float32)
    mask = np.ones(N, np.float32)
    mask[[2, 11]] = 0.0
    P = sum(n - W + 1 for n in lens)  # 9
    select = [8, 0, 3, 4, 1, 7, 2, 6]  # eight of the nine pairs, in another order: one group of 8
    mm = pipe.validate(fr.to(DEV), lens, torch.from_numpy(mel_db).to(DEV), torch.from_numpy(mask).to(DEV),
                       window=W, select=select, group=8)
    pipe.ac.check()
    got = mm.compute()
    # the oracle's windows
    feats = effnet.effnet_gap(sd, fr)
    clips = list(torch.split(feats, lens))
    _, pred = pairs_ref(sd, clips, W)
    idx = metrics.pair_index(lens, W).numpy()
    tgt = ((mel_db - mean) / std)[idx]
    assert pred.shape == tgt.shape == (P, W, 64)
    fw, tw, coeffs, bands = metrics.train_weights(64, W, 1.0)
    want, want_seq = MR.metrics(pred[select].astype(np.float32), tgt[select], mask[idx][select], 8, fw, tw, coeffs,
                                [bands[k] for k in metrics.BAND_NAMES], mean.astype(np.float64), std.astype(np.float64))
    assert got["batches"] == 1 and want["groups"] == 1
    bar = loss_bar(W, 64)
    quad = lambda q, e: 2 * e * math.sqrt(q) + e * e
    model = {"mse": quad(want["mse"], eps), "delta": quad(want["delta"], 2 * eps), "accel": quad(want["accel"], 4 * eps),
             "latest": quad(want["latest"], eps), "mae": eps}
    model["loss"] = model["mse"] + coeffs[0] * model["delta"] + coeffs[1] * model["accel"] + coeffs[2] * model["latest"]
    for k in ("loss", "mse", "mae", "delta", "accel", "latest"):
        err = abs(got[k] - want[k])
        print(f"validate {k}: got {got[k]:.6f} want {want[k]:.6f} err {err:.2e} bar {bar * want[k] + model[k]:.2e}")
        assert err <= bar * want[k] + model[k], k
    for i, k in enumerate(metrics.BAND_NAMES):
        assert abs(got["band"][k] - want[f"band{i}"]) <= bar * want[f"band{i}"] + eps, k
    ev = {"mse": quad(want["eval_mse"], eps * 8), "mae": 64 * eps}
    ev["loss"] = 0.8 * ev["mse"] + 0.2 * ev["mae"]
    for k in ("loss", "mse", "mae"):
        assert abs(got["eval"][k] - want[f"eval_{k}"]) <= bar * want[f"eval_{k}"] + ev[k], k
    mb = mcd_bar(pred[select], tgt[select], mask[idx][select], mean.astype(np.float64), std.astype(np.float64)).max()
    mcd_model = (10 / math.log(10)) * math.sqrt(2) * float(std.max()) * eps * 8
    print(f"validate mcd_like: got {got['mcd_like']:.5f} want {want['mcd_sum'] / want['mcd_count']:.5f}")
    assert got["mcd_sequences"] == want["mcd_count"] == 8
    assert abs(got["mcd_like"] - want["mcd_sum"] / want["mcd_count"]) <= mb + mcd_model
