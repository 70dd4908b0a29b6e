"""Every BiLSTM recurrence route on weights where the recurrence matters (tests/lstm_hard.py).

The suite's other BiLSTM tests run on ``synth.synth_acoustic_state``, whose untrained LSTM damps a recurrent error
by half each step: a kernel that loses one of the three split product terms passes them.  Here the engines are
built on ``hard_acoustic_state`` (orthogonal W_hh at gain 1, forget bias +2, |c| into the tens) and on
``saturating_acoustic_state`` (pre-activations past +-90, |2c| past 89), and compared with the float64 loop
``lstm_hard.bilstm_f64`` at the project's own bars, unchanged:

    fp32 engine                      atol 2e-5 on y for T <= 64, 1e-4 above
    split engines (bf16x3/bf16/fp8)  atol 1e-4
    window-4 kernels                 atol 2e-5 for every engine (a correct split sits at 2e-6 over four steps)
    mel head                         5 x the y bar

test_lstm_hard_cpu.py shows on the CPU that correct arithmetic sits 2.5 x inside these on the same inputs and that
a lost split term, a stale hand-off, swapped gate rows and a reverse pass started in the padding land 10 x outside
or more.  Each case also asserts from the launch record that the intended kernel ran (which instantiation of
lstm_small / lstm_mid a batch size selects is pinned by test_lstm_route_cpu.py), that the result is finite, and
calls ``eng.check()``.  The worst error of every case is printed; DESIGN.md §34 records what an MI355X gave.
GPU box only.
"""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_hard as LH
from lstm_hard_child import RESULT_TAG, measure, recorded, worst
from m2s import runtime

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
STEP = (("M2S_LSTM_PERSISTENT", "0"),)
NO_X3G = (("M2S_LSTM_X3G", "0"),)
CHILD_TIMEOUT = 300  # seconds; a child measures at most two 40-step calls after loading the library


@contextlib.contextmanager
def _environ(pairs):
    old = {k: os.environ.get(k) for k, _ in pairs}
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engine():
    """get(kind, dtype, env): one engine per weight set, dtype and switch setting (an engine reads its switches
    when it is built)."""
    cache = {}

    def get(kind, dtype, env=()):
        key = (kind, dtype, env)
        if key not in cache:
            st = {"hard": LH.hard_acoustic_state, "sat": LH.saturating_acoustic_state}[kind](LH.SEED)
            with _environ(env):
                cache[key] = runtime.AcousticEngine(st, dtype=dtype, device=DEV)
        return cache[key]
    return get


def _engine_class(dtype):
    return "fp32" if dtype == "fp32" else "split"


def _hold(what, res, kernel, bar):
    print(f"{what}: {kernel}, max|d y| = {res['y']:.2e}, max|d mel_norm| = {res['mel']:.2e} "
          f"(bars {bar:.0e} / {5 * bar:.0e})")
    assert res["kernels"] == [kernel], (what, res["kernels"])
    assert np.isfinite(res["y"]) and np.isfinite(res["mel"]), what
    assert res["y"] <= bar, (what, res["y"])
    assert res["mel"] <= 5 * bar, (what, res["mel"])


# ---- 1. every dense route ---------------------------------------------------------------------------------------
# (kernel, dtype, B, T, switches of the engine)
DENSE = [("lstm_step_kernel", "fp32", 2, 40, STEP), ("lstm_step_kernel", "bf16x3", 2, 40, STEP),
         ("lstm_small_kernel", "fp32", 1, 40, ()), ("lstm_small_kernel", "fp32", 4, 40, ()),
         ("lstm_small_kernel", "bf16x3", 1, 40, ()), ("lstm_small_kernel", "bf16x3", 4, 40, ()),
         ("lstm_small_kernel", "fp32", 1, 1000, ()), ("lstm_small_kernel", "bf16x3", 1, 1000, ()),
         ("lstm_mid_kernel", "fp32", 5, 40, ()), ("lstm_mid_kernel", "fp32", 8, 40, ()),      # chunks of 4, 5: ragged
         ("lstm_mid_kernel", "fp32", 5, 1000, ()),
         ("lstm_mid_kernel", "fp32", 9, 40, ()), ("lstm_mid_kernel", "fp32", 16, 40, ()),     # chunks of 8
         ("lstm_persistent_kernel", "fp32", 17, 40, ()), ("lstm_persistent_kernel", "fp32", 64, 40, ()),
         ("lstm_persistent_kernel", "fp32", 70, 40, ()),                                      # a second launch of 6
         ("lstm_persistent_kernel", "fp32", 17, 1000, ()),
         ("lstm_x3g_kernel", "bf16x3", 5, 40, ()), ("lstm_x3g_kernel", "bf16x3", 16, 40, ()),
         ("lstm_x3g_kernel", "bf16x3", 5, 1000, ()),
         ("lstm_x3_kernel", "bf16x3", 17, 40, ()), ("lstm_x3_kernel", "bf16x3", 64, 40, ()),
         ("lstm_x3_kernel", "bf16x3", 70, 40, ()), ("lstm_x3_kernel", "bf16x3", 5, 40, NO_X3G),
         ("lstm_x3_kernel", "bf16x3", 17, 1000, ()),
         # the bf16 and fp8 engines share the split recurrence: bar and record name only
         ("lstm_x3g_kernel", "bf16", 5, 40, ()), ("lstm_x3_kernel", "bf16", 17, 40, ()),
         ("lstm_x3g_kernel", "fp8", 5, 40, ()), ("lstm_x3_kernel", "fp8", 17, 40, ())]


def _dense_id(c):
    return f"{c[0][5:-7]}-{c[1]}-{c[2]}x{c[3]}" + "".join(f"-{k[4:].lower()}{v}" for k, v in c[4])


@pytest.mark.parametrize("case", DENSE, ids=_dense_id)
def test_dense_route_on_hard_weights(engine, case):
    kernel, dtype, B, T, env = case
    res = measure(engine("hard", dtype, env), "hard", B, T)
    _hold(f"hard {dtype} {B} x {T}", res, kernel, LH.bar(_engine_class(dtype), T))


# ---- 2. the instantiations behind process-wide switches, one fresh process per setting -----------------------------
FROZEN = {"small_b8": ("M2S_LSTM_SMALL_B", "8", "lstm_small_kernel", [5, 8]),   # the 8-sequence instantiation
          "mid_ch16": ("M2S_LSTM_MID_CH", "16", "lstm_mid_kernel", [16])}        # one chunk of 16


@pytest.mark.parametrize("setting", list(FROZEN))
def test_frozen_switch_instantiations_on_hard_weights(setting):
    """M2S_LSTM_SMALL_B and M2S_LSTM_MID_CH freeze at their first use in a process, and nothing else in the suite
    sets them: each setting runs in a child process of its own (never an exec of this one), under a time limit."""
    var, value, kernel, batches = FROZEN[setting]
    cases = [["hard", "fp32", B, 40] for B in batches]
    env = dict(os.environ, **{var: value})
    p = subprocess.run([sys.executable, os.path.join(HERE, "lstm_hard_child.py"), json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (line,) = [ln for ln in p.stdout.splitlines() if ln.startswith(RESULT_TAG)]
    for (_, dtype, B, T), res in zip(cases, json.loads(line[len(RESULT_TAG):])):
        _hold(f"hard {dtype} {B} x {T} {var}={value}", res, kernel, LH.bar("fp32", T))


# ---- 3. saturated gates ---------------------------------------------------------------------------------------------
# B = 2 where the ladder lets two sequences reach the kernel; lstm_x3g starts at 5 sequences, lstm_x3 and
# lstm_persistent at 17 (csrc/lstm_route.hpp), so those run the smallest batch that reaches them.  lstm_x3g and lstm_x3
# exist in the split engines only, lstm_persistent in the fp32 engine only.
SATURATED = [("lstm_small_kernel", "fp32", 2, ()), ("lstm_small_kernel", "bf16x3", 2, ()),
             ("lstm_step_kernel", "fp32", 2, STEP), ("lstm_step_kernel", "bf16x3", 2, STEP),
             ("lstm_x3g_kernel", "bf16x3", 5, ()), ("lstm_x3_kernel", "bf16x3", 17, ()),
             ("lstm_persistent_kernel", "fp32", 17, ())]


@pytest.mark.parametrize("case", SATURATED, ids=lambda c: f"{c[0][5:-7]}-{c[1]}-{c[2]}")
def test_saturated_gates_stay_finite_and_exact(engine, case):
    """Pre-activations past +-90 and |2c| up to 240: the reference's sigmoid and tanh are exactly 0, 1 and +-1
    there, and the kernels reach the same through exp2 -> inf and rcp(inf) = 0.  T = 120."""
    kernel, dtype, B, env = case
    res = measure(engine("sat", dtype, env), "sat", B, 120)
    _hold(f"sat {dtype} {B} x 120", res, kernel, LH.bar(_engine_class(dtype), 120))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_saturated_gates_in_the_window_kernels(engine, dtype):
    """lstm_window.hip on the saturating state: the latest window-4 rows of two clips of 120 frames."""
    sd = LH.state_of("sat")
    clips = LH.clip_feats([120, 120], LH.WINDOW_SEED + 1)
    y_ref, m_ref = LH.windowed_f64(sd, clips, 4, "latest")
    eng = engine("sat", dtype)
    (y, m), rec = recorded(eng, lambda: eng.bilstm_windowed([c.to(DEV) for c in clips], None, 4, "latest"))
    _hold_window(f"sat windowed latest {dtype}", y, m, y_ref, m_ref, rec, dtype)


# ---- 4. ragged batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_ragged_on_hard_weights(engine, dtype):
    """Lengths [40, 7, 1] against the float64 loop started at each clip's own last frame.  A reverse pass that
    reads into the padding moves y by more than 1 here (test_lstm_hard_cpu.py)."""
    lens = LH.RAGGED_LENS
    clips = LH.clip_feats(lens, LH.RAGGED_SEED)
    x = torch.zeros(len(lens), max(lens), LH.C_IN)
    for b, c in enumerate(clips):
        x[b, :lens[b]] = c
    sd = LH.state_of("hard")
    y64 = LH.bilstm_f64(sd, x, lens)
    y_ref = torch.cat([y64[b, :n] for b, n in enumerate(lens)])
    m_ref = LH.head_f64(sd, y_ref)
    eng = engine("hard", dtype)
    (y, m), rec = recorded(eng, lambda: eng.bilstm_ragged([c.to(DEV) for c in clips]))
    names = {r["name"] for r in rec}
    res = {"y": worst(y, y_ref.numpy()), "mel": worst(m, m_ref.numpy()),
           "kernels": sorted(n for n in names if n.startswith("lstm_"))}
    assert {"ragged_pre_scatter_kernel", "ragged_head_gather_kernel"} <= names, names
    _hold(f"hard ragged {lens} {dtype}", res, "lstm_small_kernel", LH.bar(_engine_class(dtype), max(lens)))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_equal_lengths_are_the_dense_call_bit_for_bit_on_hard_weights(engine, dtype):
    eng = engine("hard", dtype)
    x = LH.feats(3, 40).to(DEV)
    y, m = eng.bilstm(x)
    yr, mr = eng.bilstm_ragged(x.reshape(120, LH.C_IN), [40] * 3)
    eng.check()
    assert torch.equal(yr.view(3, 40, 640), y) and torch.equal(mr.view(3, 40, 64), m)


# ---- 5. windows and pairs -------------------------------------------------------------------------------------------
def _hold_window(what, y, m, y_ref, m_ref, rec, dtype, extra=()):
    names = {r["name"] for r in rec}
    step = "lstm_window_step_kernel<f32>" if dtype == "fp32" else "lstm_window_step_kernel<split>"
    assert step in names and set(extra) <= names, names
    assert not [n for n in names if n.startswith("lstm_") and not n.startswith("lstm_window")], names
    assert len([r for r in rec if r["name"] == step]) == 3  # one launch per recurrent step of a window of 4
    ey, em = worst(y, y_ref.numpy()), worst(m, m_ref.numpy())
    bar = LH.bar(_engine_class(dtype), 4, window=True)
    print(f"{what}: max|d y| = {ey:.2e}, max|d mel_norm| = {em:.2e} (bars {bar:.0e} / {5 * bar:.0e})")
    assert np.isfinite(ey) and np.isfinite(em), what
    assert ey <= bar and em <= 5 * bar, (what, ey, em)


@pytest.fixture(scope="module")
def window_refs():
    """float64 references of the window cases on the hard state, computed on first use and never modified."""
    cache = {}

    def get(form):
        if form not in cache:
            sd = LH.state_of("hard")
            clips = LH.clip_feats(LH.WINDOW_LENS, LH.WINDOW_SEED)
            if form == "pairs":
                clips = [c for c in clips if c.shape[0] >= 4]
                cache[form] = (clips,) + LH.pairs_f64(sd, clips, 4)
            elif form == "context":
                cache[form] = (clips,) + LH.windowed_f64(sd, clips, 4, "latest", LH.WINDOW_CONTEXT)
            else:
                cache[form] = (clips,) + LH.windowed_f64(sd, clips, 4, form)
        return cache[form]
    return get


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("merge", ["latest", "mean"])
def test_windowed_on_hard_weights(engine, window_refs, merge, dtype):
    """Window 4 over clips of 1, 3, 4 and 9 frames: partial windows, exactly one window, six windows."""
    clips, y_ref, m_ref = window_refs(merge)
    eng = engine("hard", dtype)
    (y, m), rec = recorded(eng, lambda: eng.bilstm_windowed([c.to(DEV) for c in clips], None, 4, merge))
    _hold_window(f"hard windowed {merge} {dtype}", y, m, y_ref, m_ref, rec, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_windowed_context_on_hard_weights(engine, window_refs, dtype):
    clips, y_ref, m_ref = window_refs("context")
    eng = engine("hard", dtype)
    packed = torch.cat(clips).to(DEV)
    (y, m), rec = recorded(eng, lambda: eng.bilstm_windowed(packed, LH.WINDOW_LENS, 4, "latest", LH.WINDOW_CONTEXT))
    assert y.shape[0] == sum(LH.WINDOW_LENS) - sum(LH.WINDOW_CONTEXT)
    _hold_window(f"hard windowed context {dtype}", y, m, y_ref, m_ref, rec, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_pairs_on_hard_weights(engine, window_refs, dtype):
    """Every row of every full window.  A clip shorter than the window has no pair and the call refuses it
    (test_gpu_pairs.py), so of the window lengths the clips of 4 and 9 frames take part: 1 + 6 pairs."""
    clips, y_ref, m_ref = window_refs("pairs")
    eng = engine("hard", dtype)
    (y, m), rec = recorded(eng, lambda: eng.bilstm_pairs([c.to(DEV) for c in clips], None, 4))
    assert y.shape == (7, 4, 640) and m.shape == (7, 4, 64)
    _hold_window(f"hard pairs {dtype}", y, m, y_ref, m_ref, rec, dtype, extra=("lstm_window_pairs_kernel",))
