"""The fine-tuning engine on the GPU (include/m2s.h "fine-tuning", DESIGN.md "Fine-tuning") against
tests/finetune_ref.py: torch on the CPU in float64.

The calibrated bar.  Every quantity compared with float64 is also computed by the same torch code in fp32 on the CPU;
the device may be 4 times as far from float64 as that run is (tiled reductions add in another order), with a floor of
2e-6 of the quantity's largest magnitude, the project's fp32-autograd bar
(test_lstm_hard_cpu.py::test_fp32_autograd_is_within_2e_6_of_float64).  Each test prints both errors.

Shapes: lengths (4, 7, 36) at window 4 give P = 1 + 4 + 33 = 38 windows: a one-window clip and a clip that spills
into a second 32-window tile; split-K runs on the head (K = 152, 3 parts) and on dW_hh (K = 114, 2 parts).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import finetune_ref as FR  # tests/finetune_ref.py
import ws_harness as H     # tests/ws_harness.py
from m2s import _native, finetune, metrics, runtime, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LENS = (4, 7, 36)
U = 2.0 ** -24
# (weights, lengths, window, n_mels)
CASES = [(k, LENS, w, m) for k in ("synth", "hard") for w in (1, 2, 4) for m in (64, 16)] + \
        [(k, (16, 20), 16, 64) for k in ("synth", "hard")]
IDS = [f"{k}-W{w}-M{m}" for k, _, w, m in CASES]
TRAJ = dict(kind="synth", lens=LENS, W=4, M=64, lr=1e-3, seed=11, steps=5)  # tests/test_finetune_cpu.py asserts its precondition


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def calibrated(name, got, ref64, ref32):
    """Assert max |got - ref64| <= max(4 max |ref32 - ref64|, 2e-6 max |ref64|); prints the figures."""
    g, a, b = (np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float64) for v in (got, ref64, ref32))
    scale = max(float(np.abs(a).max()), 1e-30)
    e_dev, e_cpu = float(np.abs(g - a).max()), float(np.abs(b - a).max())
    bar = max(4.0 * e_cpu, 2e-6 * scale)
    print(f"{name}: device {e_dev / scale:.2e}, CPU fp32 {e_cpu / scale:.2e}, bar {bar / scale:.2e} (relative to max |x|)")
    assert e_dev <= bar, f"{name}: device error {e_dev:.3e} > bar {bar:.3e} (CPU fp32 error {e_cpu:.3e}, scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def reference(kind, lens, W, M, p=0.0, masked="some", lr=1e-4, wd=1e-4, clip=1.0, steps=1, seed=5):
    """One float64 and one fp32 CPU run of `steps` steps: per dtype {pred_eval, pred_train, steps: [slots], grads
    (of the last step), w0, w}.  Computed once per process, read-only."""
    sd = FR.state_of(kind, M)
    feats, target, mask = FR.inputs(lens, M, seed, masked)
    out = {"inputs": (feats, target, mask), "sd": sd}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        t = FR.RefTuner(sd, M, lr, wd, clip, p, 3, W, dt)
        r = {"w0": t.state()}
        with torch.no_grad():
            r["pred_eval"] = t.predict(feats, lens)
            r["pred_train"] = t.predict(feats, lens, train=True)
        r["steps"] = [t.step(feats, target, mask, lens) for _ in range(steps)]
        r["grads"], r["w"] = t.grads, t.state()
        out[name] = r
    return out


def tuner(sd, M, W, **kw):
    kw.setdefault("seed", 3)
    return finetune.HeadTuner(sd, n_mels=M, device=DEV, window=W, **kw)


# ---- 1. forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,lens,W,M", CASES, ids=IDS)
def test_predict_eval_and_train(kind, lens, W, M):
    ref = reference(kind, lens, W, M, p=0.5)
    feats = dev(ref["inputs"][0])
    t = tuner(ref["sd"], M, W, dropout=0.5)
    calibrated("predict eval", t.predict(feats, lens), ref["f64"]["pred_eval"], ref["f32"]["pred_eval"])
    # p = 0.5: the restated mask (numpy) on the merged rows, then the head
    calibrated("predict train", t.predict(feats, lens, train=True), ref["f64"]["pred_train"], ref["f32"]["pred_train"])


@pytest.mark.parametrize("kind", ["synth", "hard"])
def test_predict_matches_the_inference_engine(kind):
    """predict(train=False) against AcousticEngine(fp32).bilstm_pairs on the same weights at the window bar 2e-5;
    and the train-mode output is the restated mask applied to those merged rows."""
    full = synth.synth_acoustic_state(0)
    sd = FR.state_of(kind, 64)
    full.update(sd)
    feats = dev(FR.inputs(LENS, 64, 5)[0])
    ac = runtime.AcousticEngine(full, dtype="fp32", device=DEV)
    y, mel = ac.bilstm_pairs(feats, list(LENS), 4)
    ac.check()
    t = tuner(sd, 64, 4, dropout=0.5)
    d = float((t.predict(feats, LENS) - mel).abs().max())
    print(f"{kind}: predict vs bilstm_pairs max |d| = {d:.2e}")
    assert d <= 2e-5
    keep = torch.from_numpy(finetune.dropout_keep(tuple(y.shape), 0.5, 3, 1)).to(DEV)
    want = (y.double() * keep / 0.5) @ dev(sd["head.weight"]).double().T + dev(sd["head.bias"]).double()
    got = t.predict(feats, LENS, train=True)
    d = float((got - want).abs().max())
    print(f"{kind}: train-mode predict vs masked merged rows max |d| = {d:.2e}")
    assert d <= 2e-5 * max(1.0, float(want.abs().max()))
    dropped = (y.double() * (~keep)).abs().sum() > 0  # the mask does drop something that matters
    assert bool(dropped) and 0.4 < float(keep.double().mean()) < 0.6


# ---- 2 / 3. gradients, loss slots, norm ----------------------------------------------------------------------------
def _check_step(name, t, ref, slots):
    g = t.grads()
    for k in finetune.KEYS:
        calibrated(f"{name} grad {k}", g[k], ref["f64"]["grads"][k], ref["f32"]["grads"][k])
    for sfx in ("", "_reverse"):
        assert torch.equal(g[f"rnn.lstm.bias_ih_l0{sfx}"], g[f"rnn.lstm.bias_hh_l0{sfx}"])
    s = dict(zip(finetune.SLOTS, slots.cpu().tolist()))
    a, b = ref["f64"]["steps"][-1], ref["f32"]["steps"][-1]
    for k in ("loss", "mse", "mae", "delta", "accel", "latest", "grad_norm", "clip_coef"):
        calibrated(f"{name} slot {k}", [s[k]], [a[k]], [b[k]])
    return s


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("kind,lens,W,M", CASES, ids=IDS)
def test_gradients_and_slots(kind, lens, W, M, p):
    ref = reference(kind, lens, W, M, p=p)
    feats, target, mask = (dev(a) for a in ref["inputs"])
    t = tuner(ref["sd"], M, W, dropout=p)
    slots = t.step(feats, target, mask, lens)
    _check_step(f"{kind} W{W} M{M} p{p}", t, ref, slots)


def test_fully_masked_batch_gives_the_latest_term_alone():
    ref = reference("synth", LENS, 4, 64, masked="all")
    a = ref["f64"]["steps"][-1]
    assert a["mse"] == 0.0 and a["delta"] == 0.0 and a["accel"] == 0.0 and a["latest"] > 0.0
    feats, target, mask = (dev(v) for v in ref["inputs"])
    t = tuner(ref["sd"], 64, 4, dropout=0.0)
    s = _check_step("fully masked", t, ref, t.step(feats, target, mask, LENS))
    assert s["mse"] == 0.0 and s["delta"] == 0.0 and s["accel"] == 0.0 and s["latest"] > 0.0


@pytest.mark.parametrize("masked", ["some", "none"])
@pytest.mark.parametrize("W,M", [(4, 64), (2, 16), (1, 64)])
def test_slots_equal_mel_metrics(W, M, masked):
    """p = 0: the loss slots are MelMetrics' numbers on the eval-mode predictions, to the metrics suite's bar."""
    sd = FR.state_of("synth", M)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, M, 5, masked))
    t = tuner(sd, M, W, dropout=0.0)
    mm = metrics.MelMetrics(M, ramp=1.0, device=DEV)
    t.evaluate(feats, target, mask, LENS, mm)
    want = mm.last.cpu().numpy()
    got = t.step(feats, target, mask, LENS).cpu().numpy()
    bar = 2.0 * (-(-W * M // 256) + 8 + 4) * U  # test_gpu_metrics.py loss_bar
    for i, k in enumerate(finetune.SLOTS[:6]):
        assert abs(got[i] - want[i]) <= bar * abs(want[i]), (k, got[i], want[i])


# ---- 4. optimiser alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [1, 3])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", [1e-3, 1e6])
def test_adamw_update_on_the_devices_own_gradients(clip, wd, nsteps):
    """|w - w_ref| <= 4 ulp(|w|) + 1e-5 lr against the float64 formula on the device's fp32 gradients and moments:
    a dozen fp32 roundings on the update term with 16x margin (derived).  Steps before the last run at lr = 0,
    wd = 0: the parameters stay, the moments and the step count advance."""
    lr = 1e-3
    sd = FR.state_of("synth", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    t = tuner(sd, 64, 4, dropout=0.0, lr=0.0, weight_decay=0.0, grad_clip=clip)
    for _ in range(nsteps - 1):
        t.step(feats, target, mask, LENS)
    before, opt = t.state_dict(), t.optimizer_state()
    assert int(opt["step"].item()) == nsteps - 1
    for k in finetune.KEYS:
        assert torch.equal(before[k].cpu(), torch.from_numpy(sd[k]).reshape(before[k].shape)), k
    t.set_hyper(lr=lr, weight_decay=wd)
    slots = dict(zip(finetune.SLOTS, t.step(feats, target, mask, LENS).cpu().tolist()))
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in t.grads().items()}
    norm = np.sqrt(sum((v ** 2).sum() for v in g.values()))
    coef = min(1.0, clip / (norm + 1e-6))
    assert (coef < 1.0) == (clip < 1.0) and abs(slots["clip_coef"] - coef) <= 4 * U * coef
    assert abs(slots["grad_norm"] - norm) <= 4 * U * norm
    after, opt2 = t.state_dict(), t.optimizer_state()
    assert int(opt2["step"].item()) == nsteps
    for k in finetune.KEYS:
        w, m, v = FR.adamw_update(before[k].cpu().numpy(), g[k], opt["m"][k].cpu().numpy(), opt["v"][k].cpu().numpy(),
                                  nsteps, lr, wd, coef)
        got = after[k].cpu().numpy().astype(np.float64)
        bar = 4.0 * np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) + 1e-5 * lr
        worst = float(np.max(np.abs(got - w) - bar))
        print(f"{k}: max |w - w_ref| = {np.abs(got - w).max():.2e}, update {np.abs(w - before[k].cpu().numpy()).max():.2e}")
        assert worst <= 0.0, (k, worst)
        # the moments.  v = b2 v + (1 - b2) (g coef)^2 in fp32 is at most 6 roundings from the float64 formula (coef,
        # g coef counted twice through the square, the fp32 constant, two products, the sum) on non-negative terms:
        # 8 U relative.  m's two terms may cancel, so the same 8 U is taken on their magnitudes.
        m0 = np.abs(opt["m"][k].cpu().numpy().astype(np.float64))
        assert (np.abs(opt2["m"][k].cpu().numpy() - m) <= 8 * U * (m0 + np.abs(g[k] * coef)) + 1e-38).all(), k
        np.testing.assert_allclose(opt2["v"][k].cpu().numpy(), v, rtol=8 * U, atol=1e-38)


# ---- 5. trajectory -------------------------------------------------------------------------------------------------
def test_trajectory_of_five_steps():
    c = TRAJ
    ref = reference(c["kind"], c["lens"], c["W"], c["M"], p=0.0, lr=c["lr"], steps=c["steps"], seed=c["seed"])
    feats, target, mask = (dev(a) for a in ref["inputs"])
    t = tuner(ref["sd"], c["M"], c["W"], dropout=0.0, lr=c["lr"])
    losses = [float(t.step(feats, target, mask, c["lens"])[0]) for _ in range(c["steps"])]
    l64 = [s["loss"] for s in ref["f64"]["steps"]]
    l32 = [s["loss"] for s in ref["f32"]["steps"]]
    print("losses device", losses, "float64", l64)
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    for i in range(c["steps"]):
        calibrated(f"loss at step {i + 1}", [losses[i]], [l64[i]], [l32[i]])
    got = t.state_dict()
    for k in finetune.KEYS:
        w0, w64, w32 = (r[k].double().reshape(-1) for r in (ref["f64"]["w0"], ref["f64"]["w"], ref["f32"]["w"]))
        travelled = float((w64 - w0).norm())
        r_dev = float((got[k].cpu().double().reshape(-1) - w64).norm()) / travelled
        r_cpu = float((w32 - w64).norm()) / travelled
        print(f"{k}: |w_dev - w_64| / |w_64 - w_0| = {r_dev:.2e}, CPU fp32 {r_cpu:.2e}")
        assert r_dev <= max(4.0 * r_cpu, 2e-6), (k, r_dev, r_cpu)


# ---- 6. reproducibility and capture ----------------------------------------------------------------------------------
def _all_state(t):
    o = t.optimizer_state()
    return [t.state_dict()[k] for k in finetune.KEYS] + [o["m"][k] for k in finetune.KEYS] + \
        [o["v"][k] for k in finetune.KEYS] + [o["step"]]


def test_two_tuners_are_bit_equal_after_three_steps():
    sd = FR.state_of("hard", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    states = []
    for _ in range(2):
        t = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
        slots = [t.step(feats, target, mask, LENS) for _ in range(3)]
        states.append(_all_state(t) + slots)
    assert all(torch.equal(a, b) for a, b in zip(*states))
    assert not torch.equal(states[0][-1], states[0][-2])  # the dropout stream moves with the step count


def test_captured_step_replayed_equals_eager_steps():
    sd = FR.state_of("synth", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    eager = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
    for _ in range(3):
        want_slots = eager.step(feats, target, mask, LENS)
    t = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
    t.predict(feats, LENS)  # stages the window table of these lengths
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slots = t.step(feats, target, mask, LENS)
    assert int(t.optimizer_state()["step"].item()) == 0  # capturing ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize(DEV)
    assert torch.equal(slots, want_slots)
    assert all(torch.equal(a, b) for a, b in zip(_all_state(t), _all_state(eager)))
    # afterwards eager calls of this engine and of the inference engine still work
    a, b = t.step(feats, target, mask, LENS), eager.step(feats, target, mask, LENS)
    assert torch.equal(a, b) and int(t.optimizer_state()["step"].item()) == 4
    ac = runtime.AcousticEngine(synth.synth_acoustic_state(0), dtype="fp32", device=DEV)
    _, mel = ac.bilstm_pairs(feats, list(LENS), 4)
    ac.check()
    assert bool(torch.isfinite(mel).all())


def test_capture_with_an_unstaged_table_is_refused():
    sd = FR.state_of("synth", 64)
    feats = dev(FR.inputs(LENS, 64, 5)[0])
    t = tuner(sd, 64, 4)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises((_native.M2SError, RuntimeError), match="not staged"):
        with torch.cuda.graph(graph):
            t.predict(feats, LENS)
    torch.cuda.synchronize(DEV)
    assert bool(torch.isfinite(t.predict(feats, LENS)).all())


# ---- 7. workspace contract and argument errors ---------------------------------------------------------------------
def _contract_setup(W, M):
    sd = FR.state_of("synth", M)
    t = tuner(sd, M, W, dropout=0.0, lr=0.0, weight_decay=0.0)  # lr = 0: every run of the harness sees the same state
    L = _native.lib()
    lens = list(LENS)
    cl = (C.c_int * len(lens))(*lens)
    nws = L.m2s_finetune_workspace_bytes(t._h, cl, len(lens), W)
    assert nws > 0
    return t, L, lens, cl, nws


@pytest.mark.parametrize("W,M", [(4, 64), (1, 16)])
def test_workspace_contract(W, M):
    t, L, lens, cl, nws = _contract_setup(W, M)
    feats, target, mask = FR.inputs(LENS, M, 5)
    N, P = sum(lens), sum(n - W + 1 for n in lens)
    sync = lambda: torch.cuda.synchronize(DEV)  # noqa: E731
    stream = torch.cuda.current_stream(DEV).cuda_stream
    arena = H.Arena(DEV, [("feats", "in", feats), ("target", "in", target), ("mask", "in", mask),
                          ("slots", "out", (8,)), ("ws", "ws", nws)])

    def step(a, n):
        return L.m2s_finetune_step(t._h, a.ptr("feats"), a.ptr("target"), a.ptr("mask"), cl, len(lens), N, W,
                                   a.ptr("slots"), a.ptr("ws"), n, stream)

    rep = H.check_contract(arena, lambda a: step(a, nws), sync=sync, what=f"finetune_step W={W} M={M}")
    assert rep.deterministic
    H.check_undersized(arena, step, rep.outs["zero"], sync=sync, what=f"finetune_step W={W} M={M}")
    assert all(bool(torch.isfinite(g).all()) for g in t.grads().values())
    arena = H.Arena(DEV, [("feats", "in", feats), ("mel_norm", "out", (P, W, M)), ("ws", "ws", nws)])

    def fwd(a, n):
        return L.m2s_finetune_forward(t._h, a.ptr("feats"), cl, len(lens), N, W, 0, a.ptr("mel_norm"), a.ptr("ws"), n,
                                      stream)

    rep = H.check_contract(arena, lambda a: fwd(a, nws), sync=sync, what=f"finetune_forward W={W} M={M}")
    assert rep.deterministic
    H.check_undersized(arena, fwd, rep.outs["zero"], sync=sync, what=f"finetune_forward W={W} M={M}")
    assert torch.equal(rep.outs["nan"]["mel_norm"], t.predict(dev(feats), lens))


BAD = {"window_0": dict(W=0), "window_17": dict(W=17), "short_clip": dict(lens=[4, 3, 36]), "no_clips": dict(B=0),
       "sum_lengths": dict(N=46), "other_window": dict(W=2), "zero_length": dict(lens=[4, 0, 36])}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_argument_errors_write_nothing(bad):
    t, L, lens, cl, nws = _contract_setup(4, 64)
    feats, target, mask = FR.inputs(LENS, 64, 5)
    kw = dict(W=4, lens=lens, N=sum(lens))
    kw.update(BAD[bad])
    kw.setdefault("B", len(kw["lens"]))
    cl = (C.c_int * len(kw["lens"]))(*kw["lens"])
    arena = H.Arena(DEV, [("feats", "in", feats), ("target", "in", target), ("mask", "in", mask),
                          ("slots", "out", (8,)), ("mel_norm", "out", (38, 4, 64)), ("ws", "ws", nws)])
    arena.prepare("nan")
    stream = torch.cuda.current_stream(DEV).cuda_stream
    before = _all_state(t)
    rc = L.m2s_finetune_step(t._h, arena.ptr("feats"), arena.ptr("target"), arena.ptr("mask"), cl, kw["B"], kw["N"],
                             kw["W"], arena.ptr("slots"), arena.ptr("ws"), nws, stream)
    assert rc == H.M2S_E_ARG, (bad, rc, L.m2s_last_error())
    if bad != "other_window":  # eval-mode forward takes any window
        rc = L.m2s_finetune_forward(t._h, arena.ptr("feats"), cl, kw["B"], kw["N"], kw["W"], 0, arena.ptr("mel_norm"),
                                    arena.ptr("ws"), nws, stream)
        assert rc == H.M2S_E_ARG, (bad, rc)
    torch.cuda.synchronize(DEV)
    assert not arena.violations(outputs_written=False)
    assert bool(torch.isnan(arena.view("slots")).all()) and bool(torch.isnan(arena.view("mel_norm")).all())
    assert bool((arena.raw("ws") == 0xFF).all())
    assert all(torch.equal(a, b) for a, b in zip(before, _all_state(t)))
    assert L.m2s_finetune_workspace_bytes(t._h, cl, kw["B"], kw["W"]) == 0 or bad in ("sum_lengths", "other_window")


# ---- 8. round trip -------------------------------------------------------------------------------------------------
def test_round_trip_through_the_inference_engine_and_the_optimizer_state():
    full = synth.synth_acoustic_state(0)
    sd = FR.state_of("synth", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    t = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
    for _ in range(3):
        t.step(feats, target, mask, LENS)
    merged = t.merged_state_dict(full)
    assert set(merged) == set(full)
    assert not torch.equal(merged["head.weight"], torch.from_numpy(np.asarray(full["head.weight"])))
    ac = runtime.AcousticEngine(merged, dtype="fp32", device=DEV)
    _, mel = ac.bilstm_pairs(feats, list(LENS), 4)
    ac.check()
    d = float((mel - t.predict(feats, LENS)).abs().max())
    print(f"AcousticEngine(merged) vs predict: max |d| = {d:.2e}")
    assert d <= 2e-5
    u = tuner(t.state_dict(), 64, 4, dropout=0.5, lr=1e-3)
    u.load_optimizer_state(t.optimizer_state())
    a, b = t.step(feats, target, mask, LENS), u.step(feats, target, mask, LENS)
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(_all_state(t), _all_state(u)))


# ---- 9. a captured step and calls with other lengths in between --------------------------------------------------
def test_replay_survives_calls_with_other_lengths():
    """A captured step holds its window table's address.  Eager calls with other lengths between the replays (a
    validation batch: a larger table, then a smaller one) stage tables of their own and leave that one alone."""
    sd = FR.state_of("synth", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    other = (60, 9, 5)
    f2, t2, m2 = (dev(a) for a in FR.inputs(other, 64, 6))
    eager = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
    t = tuner(sd, 64, 4, dropout=0.5, lr=1e-3)
    t.predict(feats, LENS)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slots = t.step(feats, target, mask, LENS)
    for i in range(3):
        want = eager.step(feats, target, mask, LENS)
        a, b = eager.predict(f2, other), eager.predict(feats[:9], (4, 5))
        graph.replay()
        assert torch.equal(slots, want), i
        assert torch.equal(t.predict(f2, other), a) and torch.equal(t.predict(feats[:9], (4, 5)), b)
        mm = metrics.MelMetrics(64, ramp=1.0, device=DEV)
        t.evaluate(f2, t2, m2, other, mm)
    torch.cuda.synchronize(DEV)
    assert all(torch.equal(x, y) for x, y in zip(_all_state(t), _all_state(eager)))


def test_set_hyper_is_refused_on_a_capturing_stream():
    """A step captured with another ramp than the last one would capture a copy from host memory that is gone at
    replay: refused with M2S_E_STATE before anything is recorded, and the engine works afterwards."""
    sd = FR.state_of("synth", 64)
    feats, target, mask = (dev(a) for a in FR.inputs(LENS, 64, 5))
    t = tuner(sd, 64, 4, dropout=0.0)
    want = tuner(sd, 64, 4, dropout=0.0).step(feats, target, mask, LENS, ramp=0.5)
    t.predict(feats, LENS)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises((_native.M2SError, RuntimeError), match="cannot be captured"):
        with torch.cuda.graph(graph):
            t.step(feats, target, mask, LENS, ramp=0.5)
    torch.cuda.synchronize(DEV)
    assert int(t.optimizer_state()["step"].item()) == 0
    assert torch.equal(t.step(feats, target, mask, LENS, ramp=0.5), want)


# ---- 10. the command line, end to end ------------------------------------------------------------------------------
def test_finetune_head_script_on_a_toy_dataset(tmp_path):
    """scripts/finetune_head.py on three synthetic clips: two epochs run, the loss lines print, and the checkpoint it
    writes loads strictly into the plug-in's module tree with cnn.* untouched and the tuned tensors changed."""
    import importlib.util
    import json
    import os
    from mri_acoustic_model import build_acoustic_model
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "m2s_finetune_cli", os.path.join(repo, "mri-to-speech_amd", "scripts", "finetune_head.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    full = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_acoustic_state(0).items()}
    torch.save({"model_state_dict": full}, tmp_path / "start.pt")
    mean, std = synth.synth_scaler()
    (tmp_path / "scaler.json").write_text(json.dumps({"mean": np.asarray(mean).tolist(), "std": np.asarray(std).tolist()}))
    rng = np.random.default_rng(0)
    for name, T in (("clip1", 14), ("clip2", 9), ("clip10", 3)):  # clip10 is shorter than the window: skipped
        d = tmp_path / "samples" / name
        d.mkdir(parents=True)
        np.save(d / "mri.npy", rng.random((T, 64, 64), dtype=np.float32))
        np.save(d / "mel_db.npy", (np.asarray(mean) + np.asarray(std) * rng.normal(size=(T, 64))).astype(np.float32))
        np.save(d / "mask.npy", np.ones(T, np.float32))
    args = cli.parse_args(["--processed_dir", str(tmp_path), "--mri_checkpoint", str(tmp_path / "start.pt"),
                           "--scaler_json", str(tmp_path / "scaler.json"), "--out_ckpt", str(tmp_path / "tuned.pt"),
                           "--epochs", "2", "--batch_size", "4", "--lr", "1e-3", "--seed", "1"])
    res = cli.finetune(args)
    n = (14 - 3) + (9 - 3)  # 17 windows: 13 train, 1 val
    assert res["epochs"] == 2 and res["steps"] == 2 * -(-int(n * 0.8) // 4) and np.isfinite(res["best_val"])
    ck = torch.load(tmp_path / "tuned.pt", map_location="cpu", weights_only=True)
    assert {"epoch", "model_state_dict", "val_loss"} <= set(ck) and ck["val_loss"] == res["best_val"]
    model = build_acoustic_model(n_mels=64, cnn_pretrained=False, rnn_hidden=640, dropout=0.5)
    model.load_state_dict(ck["model_state_dict"], strict=True)
    for k, v in full.items():
        same = torch.equal(ck["model_state_dict"][k], v)
        assert same != (k in finetune.KEYS), k
