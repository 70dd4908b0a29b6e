"""The hard BiLSTM weights and the bars of test_gpu_lstm_hard.py, pinned on the CPU (tests/lstm_hard.py).

Nothing here runs a kernel.  The file shows, in float64, that on ``hard_acoustic_state`` (a) the reference alone is
far inside every bar, (b) arithmetic done the way a correct kernel does it (``split``, ``act32``) stays a factor 2.5
inside, and (c) every planted defect of ``lstm_hard.MUTATIONS`` lands at 10 x the bar or more: that is what makes a
pass of the GPU tests mean something.  The last test states the opposite about the synth weights the suite used
before.  Every figure is printed (``pytest -s``); DESIGN.md §34 carries the table.
"""
import functools

import numpy as np
import pytest
import torch

import lstm_hard as LH
from m2s import synth
from oracle import acoustic

# correct arithmetic <= bar / 2.5, a defect >= 10 bar; a seed that misses is changed, not these factors
INSIDE, OUTSIDE = 2.5, 10.0

# (engine class, T) of every GPU case -> the input the table is computed on: (state, B).  Window-4 cases are
# zero-start sequences of four frames; "stale" needs a 7th step, so it does not exist there.
TABLE = {("fp32", 4): ("hard", 8), ("split", 4): ("hard", 8),
         ("fp32", 40): ("hard", 5), ("split", 40): ("hard", 5),
         ("fp32", 120): ("sat", 2), ("split", 120): ("sat", 2),
         ("fp32", 1000): ("hard", 1), ("split", 1000): ("hard", 1)}


@functools.lru_cache(maxsize=None)
def _sd(kind):
    st = {"hard": LH.hard_acoustic_state, "sat": LH.saturating_acoustic_state}[kind](LH.SEED)
    return LH.torch_state(st)


@functools.lru_cache(maxsize=None)
def _exact(kind, B, T):
    return LH.bilstm_f64(_sd(kind), LH.feats(B, T), state=True)


@functools.lru_cache(maxsize=None)
def _err(kind, B, T, mode):
    return LH.err(_sd(kind), LH.feats(B, T), mode, ref=_exact(kind, B, T)[0])


def test_states_are_deterministic_and_touch_only_the_lstm():
    a, b, s = LH.hard_acoustic_state(3), LH.hard_acoustic_state(3), synth.synth_acoustic_state(3)
    assert a.keys() == s.keys()
    changed = {k for k in a if not np.array_equal(a[k], s[k])}
    want = {f"rnn.lstm.{n}_l0{sfx}" for n in ("weight_ih", "weight_hh", "bias_ih") for sfx in ("", "_reverse")}
    assert changed == want
    for k in a:
        assert a[k].dtype == s[k].dtype and a[k].shape == s[k].shape and np.array_equal(a[k], b[k]), k
    assert not np.array_equal(LH.hard_acoustic_state(4)["rnn.lstm.weight_hh_l0"], a["rnn.lstm.weight_hh_l0"])
    w = a["rnn.lstm.weight_hh_l0"].astype(np.float64).reshape(4, 640, 640)
    for blk in w:  # orthogonal blocks at gain one
        assert np.abs(blk @ blk.T - np.eye(640)).max() < 1e-6
    sat = LH.saturating_acoustic_state(3)
    assert {k for k in sat if not np.array_equal(sat[k], a[k])} == {
        f"rnn.lstm.{n}_l0{sfx}" for n in ("weight_ih", "bias_ih") for sfx in ("", "_reverse")}


def test_loop_is_the_oracle_loop():
    """bilstm_f64 on float64 copies of the weights is oracle.acoustic.bilstm_summerge_loop in float64, dense; a
    ragged call is each clip run alone."""
    sd = _sd("hard")
    sd64 = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = LH.feats(3, 9)
    y = LH.bilstm_f64(sd, x)
    assert float((y - acoustic.bilstm_summerge_loop(sd64, x.double())).abs().max()) < 1e-13
    lens = [9, 4, 1]
    yr = LH.bilstm_f64(sd, x, lens)
    for b, n in enumerate(lens):
        assert float((yr[b, :n] - LH.bilstm_f64(sd, x[b:b + 1, :n])[0]).abs().max()) < 1e-13
        assert not yr[b, n:].any()


@pytest.mark.parametrize("T", [40, 1000])
def test_hard_state_has_a_trained_lstm_s_properties(T):
    B = TABLE["fp32", T][1]
    y, st = _exact("hard", B, T)
    f = float(st["gates"][..., 640:1280].mean())
    c = float(st["c"].abs().max())
    whh = _sd("hard")["rnn.lstm.weight_hh_l0"].double()
    rec = float((st["h"][0] @ whh.t()).abs().max())
    pre = float(st["pre"].abs().max())
    print(f"hard {B} x {T}: mean f {f:.3f}, max|c| {c:.1f}, max|W_hh h| {rec:.2f}, max|pre| {pre:.1f}, "
          f"max|y| {float(y.abs().max()):.2f}")
    assert 0.8 <= f <= 0.95
    assert c >= 10.0
    assert rec >= 1.0
    assert 1.0 <= float(y.abs().max()) <= 2.0


@pytest.mark.parametrize("T", [40, 1000])
def test_fp32_oracle_is_far_inside_every_bar(T):
    """The weight set contracts: torch's fp32 LSTM stays within 1e-5 of float64 (measured 1.0e-6 / 1.7e-6)."""
    B = TABLE["fp32", T][1]
    with torch.no_grad():
        y32 = acoustic.bilstm_summerge(_sd("hard"), LH.feats(B, T))
    d = float((y32.double() - _exact("hard", B, T)[0]).abs().max())
    print(f"hard {B} x {T}: fp32 oracle vs float64 {d:.2e}")
    assert d <= 1e-5


@pytest.mark.parametrize("engine,T", list(TABLE))
def test_sensitivity_table(engine, T):
    """One row per (engine class, T) of the GPU cases: the emulation of correct arithmetic sits 2.5 x inside the bar,
    every defect that exists for that engine 10 x outside.  The T = 1000 row is one sequence (3.7e-5 for the split);
    the worst element over more sequences is larger, 4.7e-5 at 5 x 1000 and 5.6e-5 at 17 x 1000, still under the bar
    (DESIGN.md §34 has these and the seeds tried)."""
    kind, B = TABLE[engine, T]
    bar = LH.bar(engine, T, window=T == 4)
    good = "act32" if engine == "fp32" else "split"
    bad = [m for m in LH.MUTATIONS if m != "rev_shift" and (engine == "split" or m not in LH.SPLIT_ONLY)
           and not (m == "stale" and T <= LH.STALE_EVERY)]
    row = {m: _err(kind, B, T, m) for m in [good] + bad}
    print(f"{engine} {kind} {B} x {T} bar {bar:.0e}: " + ", ".join(f"{m} {e:.2e}" for m, e in row.items()))
    assert row[good] <= bar / INSIDE, (good, row[good])
    for m in bad:
        assert row[m] >= OUTSIDE * bar, (m, row[m])


def test_reverse_start_in_the_padding_shows():
    """A reverse pass that starts at the padded end instead of each clip's last frame moves y by more than 1e-2:
    on the ragged lengths and on the partial windows of the window-4 cases."""
    sd = _sd("hard")
    lens = LH.RAGGED_LENS
    x = torch.zeros(len(lens), max(lens), LH.C_IN)
    for b, c in enumerate(LH.clip_feats(lens, LH.RAGGED_SEED)):
        x[b, :lens[b]] = c
    d = LH.err(sd, x, "rev_shift", lengths=lens)
    clips = LH.clip_feats(LH.WINDOW_LENS, LH.WINDOW_SEED)
    yw = LH.windowed_f64(sd, clips, 4, "latest")[0]
    dw = float((LH.windowed_f64(sd, clips, 4, "latest", mode="rev_shift")[0] - yw).abs().max())
    print(f"rev_shift: ragged {lens} {d:.2e}, latest windows of {LH.WINDOW_LENS} {dw:.2e}")
    assert d > 1e-2 and dw > 1e-2


def test_window_references_follow_windowed_ref():
    """windowed_f64 / pairs_f64 are tests/windowed_ref.py's definitions (fp32 oracle, one call per window) in
    float64, one ragged call per clip."""
    import windowed_ref as R
    sd = _sd("hard")
    clips = LH.clip_feats(LH.WINDOW_LENS, LH.WINDOW_SEED)
    for merge, ctx in (("latest", None), ("mean", None), ("latest", LH.WINDOW_CONTEXT)):
        y, m = LH.windowed_f64(sd, clips, 4, merge, ctx)
        yr, mr = R.windowed(sd, clips, 4, merge, ctx)
        assert y.shape == yr.shape and m.shape == mr.shape
        assert float((y - yr.double()).abs().max()) < 1e-5 and float((m - mr.double()).abs().max()) < 5e-5, merge
    full = [c for c in clips if c.shape[0] >= 4]
    y, m = LH.pairs_f64(sd, full, 4)
    want = torch.stack([R.M(sd, c[i:i + 4])[0] for c in full for i in range(c.shape[0] - 3)])
    assert y.shape == want.shape == (7, 4, 640) and m.shape == (7, 4, 64)
    assert float((y - want.double()).abs().max()) < 1e-5


def test_saturating_state_leaves_the_range_of_exp():
    """|pre| > 90 and |2c| > 89 on the test input, the exact answer is finite, the fp32 oracle stays within 1e-5 of
    it, and the kernels' activation form reaches it through exp2 -> inf / 0 without a NaN."""
    kind, B = TABLE["fp32", 120]
    y, st = _exact(kind, B, 120)
    pre, c = st["pre"], st["c"]
    share = float((pre.abs() > 90).double().mean())
    print(f"sat {B} x 120: max|pre| {float(pre.abs().max()):.1f} ({share:.1%} past 90, min {float(pre.min()):.1f}, "
          f"max {float(pre.max()):.1f}), max|2c| {2 * float(c.abs().max()):.0f}, max|y| {float(y.abs().max()):.2f}")
    assert float(pre.max()) > 90 and float(pre.min()) < -90 and share > 0.02
    assert 2 * float(c.max()) > 89 and 2 * float(c.min()) < -89
    assert torch.isfinite(y).all()
    with torch.no_grad():
        y32 = acoustic.bilstm_summerge(_sd(kind), LH.feats(B, 120))
    d = float((y32.double() - y).abs().max())
    ya = LH.bilstm_f64(_sd(kind), LH.feats(B, 120), mode="act32")
    print(f"sat {B} x 120: fp32 oracle vs float64 {d:.2e}, act32 {float((ya - y).abs().max()):.2e}")
    assert d <= 1e-5
    assert torch.isfinite(ya).all()


@pytest.mark.parametrize("kind", ["hard", "sat"])
@pytest.mark.parametrize("B,T", LH.TRAIN_SHAPES)
def test_fp32_autograd_is_within_2e_6_of_float64(kind, B, T):
    """The training-mode tests (test_gpu_gradcam.py, test_gpu_gradcam_engine.py) hold the kernels to 1e-5 relative
    against float64 autograd; fp32 torch autograd itself is within 2e-6 of it on these weights (measured: 1.2e-6 at
    worst), so the bar has the headroom it has on synth weights."""
    x, dy = LH.train_inputs(B, T)
    a, b = LH.lstm_autograd(_sd(kind), x, dy, torch.float32), LH.lstm_autograd(_sd(kind), x, dy)
    worst = max(LH.rel(a[k], b[k]) for k in b)
    print(f"{kind} {B} x {T}: fp32 autograd vs float64, worst relative {worst:.1e}")
    assert worst <= 2e-6


@pytest.mark.parametrize("T", [4, 40])
def test_synth_weights_hide_a_lost_split_term(T):
    """A statement about the OLD weights, the gap DESIGN.md §34 closes: on synth.synth_acoustic_state a recurrence
    that drops W_hi . h_lo entirely stays under the split engines' 1e-4, so no test on those weights can see it.  (On
    the hard state the same defect is 2e-3 and more: test_sensitivity_table.)"""
    sd = LH.torch_state(synth.synth_acoustic_state(LH.SEED))
    d = LH.err(sd, LH.feats(5, T), "no_hlo")
    print(f"synth 5 x {T}: no_hlo {d:.2e}, no_wlo {LH.err(sd, LH.feats(5, T), 'no_wlo'):.2e}, "
          f"split {LH.err(sd, LH.feats(5, T), 'split'):.2e}")
    assert d < 1e-4
