"""The reference side of the frame-identification tests (tests/distinct.py), no GPU.

test_gpu_distinct.py asserts ``identification_ratio(kernel output, oracle) <= 1/2`` (< 1 for fp8) under
``calibrated_acoustic_state``.  That means something only if, for the very inputs it uses, the oracle's frames are
far apart, the activations stay in a range every number format holds, the fp32 oracle is itself exact to far
below the bar, and the metric reports a wrong frame.  Those conditions are asserted here, together with the record
of the gap: under the synth state the same wrong frame passes the suite's bf16 bars.
"""
import numpy as np
import pytest
import torch

import distinct as D  # tests/distinct.py (pytest puts this directory on sys.path)
from m2s import synth

TAP_SEP_MIN, GAP_SEP_MIN, MEL_SEP_MIN, ACT_MAX, F64_REL_MAX = 0.3, 0.1, 0.05, 32.0, 1e-5
ENCODER_INPUTS = [k for k in D.INPUTS if not k.startswith(("clips", "ragged"))]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def test_state_differs_only_in_backbone_running_statistics():
    base, cal = synth.synth_acoustic_state(D.SEED), D.calibrated_acoustic_state(D.SEED)
    assert list(base) == list(cal)
    moved = 0
    for k in base:
        assert cal[k].dtype == base[k].dtype and cal[k].shape == base[k].shape, k
        stat = k.startswith(D.BN_PREFIX) and k.rsplit(".", 1)[-1] in ("running_mean", "running_var")
        if not stat:
            assert np.array_equal(cal[k], base[k]), k
        else:
            assert np.isfinite(cal[k]).all(), k
            moved += not np.array_equal(cal[k], base[k])
            if k.endswith("running_var"):
                assert (cal[k] > 0).all(), k
    assert moved == sum(k.startswith(D.BN_PREFIX) and k.endswith(("running_mean", "running_var")) for k in base)


def test_calibration_is_reproducible_bit_for_bit():
    a, b = D.calibrated_acoustic_state(D.SEED, cache=False), D.calibrated_acoustic_state(D.SEED, cache=False)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = D.calibrated_acoustic_state(D.SEED)  # the cached state hands out copies: a caller cannot spoil it
    c["cnn.backbone.bn1.running_var"][:] = 0
    assert np.array_equal(D.calibrated_acoustic_state(D.SEED)["cnn.backbone.bn1.running_var"],
                          a["cnn.backbone.bn1.running_var"])


@pytest.mark.parametrize("name", ENCODER_INPUTS)
def test_reference_conditions_on_the_gpu_tests_inputs(name):
    """Every tap's frames >= 0.3 apart (min pair distance / rms frame norm), pooled features >= 0.1, every activation
    <= 32, and the fp32 oracle within 1e-5 of the tensor max of the float64 oracle at every tap.  The oracle is
    per frame in eval mode, so for the 263-frame input float64 runs on every 8th frame."""
    ref = D.reference(name)
    seps = [D.separation(t) for t in ref]
    amax = max(float(np.abs(t).max()) for t in ref)
    fr = D.frames(name)[0]
    idx = np.arange(0, len(fr), 8 if len(fr) > 64 else 1)
    t64, g64 = D.oracle_taps(D.calibrated_acoustic_state(D.SEED), fr[idx], torch.float64)
    errs = [float(np.abs(a[idx] - b.numpy()).max() / np.abs(b.numpy()).max()) for a, b in zip(ref, t64 + [g64])]
    ratio = max(D.identification_ratio(a[idx], b) for a, b in zip(ref, t64 + [g64])) if len(idx) > 1 else 0.0
    print(f"\n{name}: min tap separation {min(seps[:29]):.3f} (tap {int(np.argmin(seps[:29]))}), pooled {seps[29]:.3f}, "
          f"max |activation| {amax:.2f}, fp32 vs float64 rel {max(errs):.2e}, ratio {ratio:.2e}")
    assert min(seps[:29]) >= TAP_SEP_MIN, seps
    assert seps[29] >= GAP_SEP_MIN
    assert amax <= ACT_MAX
    assert max(errs) <= F64_REL_MAX, errs
    assert ratio <= 1e-4


def test_mel_rows_are_separated():
    mn = D.reference_mel("clips_96x80")
    sep = min(D.separation(D.reference_mel(k).reshape(-1, mn.shape[-1])) for k in ("clips_96x80", "clips_256x256"))
    per_clip = [D.separation(m) for m in D.reference_mel("ragged_96x80")]
    print(f"\nmel_norm row separation: 3 x 5 clips {sep:.3f}, ragged per clip {' '.join(f'{s:.3f}' for s in per_clip)}")
    assert sep >= MEL_SEP_MIN and min(per_clip) >= MEL_SEP_MIN
    assert np.isfinite(mn).all() and np.abs(mn).max() <= ACT_MAX


def _faults(ref):
    """Planted wrong-frame outputs for a (9, ...) reference: name -> output."""
    n = len(ref)
    swap = ref.copy()
    swap[[2, 3]] = ref[[3, 2]]
    prev = ref.copy()
    prev[5] = ref[4]
    mean = np.broadcast_to(ref.mean(0, keepdims=True), ref.shape).copy()
    zero = ref.copy()
    zero[n - 1] = 0  # frame 8 of 9: the only image of the partial SE group
    return {"two frames swapped": swap, "frame i = frame i-1": prev, "every frame = mean frame": mean,
            "last frame of the partial group zeroed": zero}


@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_256x256"])
def test_planted_wrong_frames_are_reported(name):
    ref = D.reference(name)
    for i in (0, 8, 13, 15, 19, 28, 29):
        assert D.identification_ratio(ref[i], ref[i]) == 0.0
        for what, bad in _faults(ref[i]).items():
            r = D.identification_ratio(bad, ref[i])
            assert r >= 1.0, (i, what, r)


def test_metric_on_small_cases():
    ref = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]])
    got = ref + np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0]])  # row 0 moved 1 towards row 1: 1 / 3
    assert D.identification_ratio(got, ref) == pytest.approx(1.0 / 3.0)
    assert D.identification_ratio(ref[[1, 0, 2]], ref) == float("inf")
    nan = ref.copy()
    nan[1, 0] = np.nan
    assert D.identification_ratio(nan, ref) == float("inf")
    assert D.separation(ref) == pytest.approx(4.0 / np.sqrt(32.0 / 3.0))
    # Gram form against the direct one, in the regime of the GPU tests (many rows, long rows, small error)
    rng = np.random.default_rng(0)
    r = rng.normal(size=(40, 5000))
    g = r + 1e-3 * rng.normal(size=r.shape)
    d = np.linalg.norm(g[:, None, :] - r[None, :, :], axis=2)
    own = np.diag(d).copy()
    np.fill_diagonal(d, np.inf)
    assert D.identification_ratio(g, r) == pytest.approx(float((own / d.min(1)).max()), rel=1e-9)


@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_67x101", "blocks_256x256"])
def test_neighbour_se_gate_misses_the_per_frame_cosine_bar_not_the_ratio(name):
    """What the ratio does not see.  A kernel that gates image n with the SqueezeExcite gate of image n & ~1 writes
    the right frame's activations, mildly mis-scaled per channel: ratio 0.05-0.18, under the 1/2 bar.  On these
    weights it does move the worst frame to a cosine of 0.9955-0.9982 against its own oracle row at every tap from
    13 to 28 (pooled features: 0.9993), so the per-frame cos >= 0.999 that test_gpu_distinct.py holds fp32 / bf16x3 /
    bf16 to catches it there; under the synth state the same fault stays above 0.999 at those taps."""
    st, fr = D.calibrated_acoustic_state(D.SEED), D.frames(name)[0]
    ref = D.reference(name)
    same = D._taps_with_gate_of(st, fr, lambda n: torch.arange(n))
    for a, b in zip(same, ref):  # the restated graph is the oracle's
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max()
    bad = D.oracle_taps_neighbour_gate(st, fr)
    cos = [float(D.frame_cosines(bad[i], ref[i]).min()) for i in range(30)]
    ratio = [D.identification_ratio(bad[i], ref[i]) for i in range(30)]
    print(f"\n{name}: neighbour gate, taps 13..28: per-frame cos {min(cos[13:29]):.5f}..{max(cos[13:29]):.5f}, "
          f"ratio {min(ratio[13:29]):.3f}..{max(ratio[13:29]):.3f}; pooled cos {cos[29]:.5f} ratio {ratio[29]:.3f}")
    assert max(ratio) < 0.5       # the ratio alone passes this fault
    assert max(cos[13:29]) < 0.999  # the per-frame cosine does not
    sy = synth.synth_acoustic_state(D.SEED)
    ref_s, bad_s = D._taps_with_gate_of(sy, fr, lambda n: torch.arange(n)), D.oracle_taps_neighbour_gate(sy, fr)
    assert min(float(D.frame_cosines(bad_s[i], ref_s[i]).min()) for i in range(13, 29)) >= 0.999


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


def _cos(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def _worst_swap(ref):
    """(lowest cosine, largest rel, highest cosine, smallest rel) against ``ref`` over all 36 outputs that have
    two of the 9 frames swapped."""
    cs, rs = [], []
    for a in range(len(ref)):
        for b in range(a + 1, len(ref)):
            bad = ref.copy()
            bad[[a, b]] = ref[[b, a]]
            cs.append(_cos(bad, ref))
            rs.append(_rel(bad, ref))
            assert D.identification_ratio(bad, ref) >= 1.0, (a, b)
    return min(cs), max(rs), max(cs), min(rs)


@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_256x256"])
def test_synth_state_hides_a_swapped_frame_from_the_bf16_bars(name):
    """The record of the gap.  Under synth_acoustic_state, any two frames swapped in the oracle's own output still
    meet the bars the bf16 tests hold a kernel to: cos >= 0.999 against the oracle at every tap from 15 on (in fact
    from 13), and rel <= 2e-2, the fused-against-unfused bar, from tap 24 on and at the pooled features (taps 15-23:
    8e-2 falling to 2e-2).  Under the calibrated state every swap misses both bars at every one of these taps, and
    the ratio reports it under either state."""
    fr = D.frames(name)[0]
    taps, gap = D.oracle_taps(synth.synth_acoustic_state(D.SEED), fr)
    synth_ref = [t.numpy() for t in taps] + [gap.numpy()]
    cal_ref = D.reference(name)
    for i in range(15, 30):
        s, c = _worst_swap(synth_ref[i]), _worst_swap(cal_ref[i])
        print(f"tap {i}: synth cos >= {s[0]:.6f} rel <= {s[1]:.1e} | calibrated cos <= {c[2]:.4f} rel >= {c[3]:.1e}")
        assert s[0] >= 0.999, (i, s)           # the old cosine bar passes every wrong frame
        if i >= 24:
            assert s[1] <= 2e-2, (i, s)        # and so does the old fused / unfused bar
        assert c[2] < 0.999 and c[3] > 2e-2, (i, c)  # on the calibrated state the same bars would catch each
