"""The per-wave form of the split IR front half on 8 x 8 maps (csrc/ir_ws_wave.hpp, ir_ws_wave8: a position subtile
is two image rows, the vertical taps a half swap of the 16-lane row, the horizontal ones masked per lane at columns 0
and 7, x double-buffered) against the handed-off form it replaces there (M2S_IR_WS=handoff) and the
fp32 oracle.  Same split fp32 arithmetic up to the order of a few roundings: the bar is the parity bar of
test_ir_ws_matches_grid_kernel, relative 1e-4 of the reference array's scale.  All engines run ir_ws and se_ws at
any pass size (M2S_IRWS_MIN=0, M2S_SEWS_MIN=0).  GPU box only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from m2s import synth
from oracle import effnet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BAR = 1e-4
# 256 x 256 frames: blocks.5.x run on 8 x 8 maps at kp 224; taps after blocks 5.1, 5.5, 5.9
TAPS7, WAVE7, HAND7 = (20, 24, 28), "ir_ws_kernel<8, 7, 1>", "ir_ws_kernel<8, 7, 1, 1>"
# 128 x 128 frames: blocks.3.x and 4.x run on 8 x 8 maps at kp 128; taps after blocks 3.1, 3.3, 4.0, 4.5
TAPS4, WAVE4, HAND4 = (10, 12, 13, 18), "ir_ws_kernel<8, 4, 1>", "ir_ws_kernel<8, 4, 1, 1>"
SEED7, SEED4 = 31, 41  # pinned: test_wrong_column_mask_would_show is about these frames


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.fixture(scope="module")
def ac_state():
    return synth.synth_acoustic_state(11)


@pytest.fixture(scope="module")
def sd(ac_state):
    return {k: torch.from_numpy(v) for k, v in ac_state.items()}


@pytest.fixture(scope="module")
def engines(ac_state):
    """(per-wave form, handed-off form): the switches are read once, when an engine is created"""
    from m2s import runtime as rt
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("M2S_IRWS_MIN", "0")
        mp.setenv("M2S_SEWS_MIN", "0")
        mp.delenv("M2S_IR_WS", raising=False)
        wave = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
        mp.setenv("M2S_IR_WS", "handoff")
        hand = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
    return wave, hand


def _names(eng, x):
    from m2s import _native
    _native.prof_enable(True)
    _native.prof_launches()
    eng.effnet(x)
    torch.cuda.synchronize()
    names = {r["name"] for r in _native.prof_launches()}
    _native.prof_enable(False)
    return names


@pytest.fixture(scope="module")
def frames300():
    """300 frames (more images than workgroups, with a split tail); one frame also at the last whole-image unit and
    in the tail parts"""
    fr = torch.from_numpy(synth.synth_frames(1, 300, seed=SEED7)[0])
    for i in (255, 256, 299):
        fr[i] = fr[0]
    return fr.to(DEV)


@pytest.fixture(scope="module")
def frames128():
    return torch.from_numpy(synth.synth_frames(1, 3, hw=(128, 128), seed=SEED4)[0])


@pytest.fixture(scope="module")
def feats300(engines, frames300):
    return engines[0].effnet(frames300).clone()


@pytest.fixture(scope="module")
def oracle_taps(sd, frames300, frames128):
    """the fp32 oracle's taps of the 3 frames of either size, computed once"""
    t7, t4 = [], []
    effnet.effnet_features(sd, frames300[:3].cpu(), taps=t7)
    effnet.effnet_features(sd, frames128, taps=t4)
    return t7, t4


def _against_handed_off(engines, x, taps, wave_name, hand_name, tag):
    wave, hand = engines
    for i in taps:
        a, b = wave.probe(x, i).cpu().numpy(), hand.probe(x, i).cpu().numpy()
        r = _rel(a, b)
        print(f"{tag} tap {i}: rel {r:.3e}")
        assert np.isfinite(a).all() and r <= BAR, (i, r)
    r = _rel(wave.effnet(x).cpu().numpy(), hand.effnet(x).cpu().numpy())
    print(f"{tag} effnet: rel {r:.3e}")
    assert r <= BAR
    nw, nh = _names(wave, x), _names(hand, x)
    assert wave_name in nw and hand_name not in nw, sorted(nw)
    assert hand_name in nh and wave_name not in nh, sorted(nh)


@pytest.mark.parametrize("n", [3, 300])
def test_wave8_matches_handed_off_form_kp224(engines, frames300, n):
    _against_handed_off(engines, frames300[:n] if n == 3 else frames300, TAPS7, WAVE7, HAND7, f"kp224 n {n}")


def test_wave8_matches_handed_off_form_kp128(engines, frames128):
    _against_handed_off(engines, frames128.to(DEV), TAPS4, WAVE4, HAND4, "kp128 n 3")


def test_wave8_matches_oracle_taps(engines, frames300, frames128, oracle_taps):
    wave, _ = engines
    for tag, x, taps, ref in (("kp224", frames300[:3], TAPS7, oracle_taps[0]),
                              ("kp128", frames128.to(DEV), TAPS4, oracle_taps[1])):
        for i in taps:
            r = _rel(wave.probe(x, i).cpu().numpy(), ref[i].numpy())
            print(f"{tag} tap {i} vs oracle: rel {r:.3e}")
            assert r <= BAR, (i, r)


def _conv_wrapping(x, w, k, s, groups=1):
    """oracle._conv with the wrong column mask on 8 x 8 depthwise maps: the left tap of column 0 takes column 7 of the
    image row above and the right tap of column 7 column 0 of the row below (lane - 1 / lane + 1 of a 16-lane row that
    holds two image rows), where the right kernel takes zero"""
    if not (groups > 1 and k == 3 and s == 1 and tuple(x.shape[-2:]) == (8, 8)):
        return _CONV(x, w, k, s, groups)
    xp = F.pad(x, [1, 1, 1, 1])
    xp[..., 2:9, 0] = x[..., 0:7, 7]
    xp[..., 1:8, 9] = x[..., 1:8, 0]
    return F.conv2d(xp, w, None, 1, 0, 1, groups)


_CONV = effnet._conv


def test_wrong_column_mask_would_show(sd, frames300, frames128, oracle_taps):
    """On the CPU, the oracle alone: with the horizontal taps wrapping into the neighbouring image row instead of
    reading zero, every checked tap of the chosen frames moves by more than 10 x the bar, so the comparisons above
    cannot pass on a wrong mask"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(effnet, "_conv", _conv_wrapping)
        w7, w4 = [], []
        effnet.effnet_features(sd, frames300[:3].cpu(), taps=w7)
        effnet.effnet_features(sd, frames128, taps=w4)
    for tag, taps, bad, ref in (("kp224", TAPS7, w7, oracle_taps[0]), ("kp128", TAPS4, w4, oracle_taps[1])):
        for i in taps:
            r = _rel(bad[i].numpy(), ref[i].numpy())
            print(f"{tag} tap {i}: wrapped taps move it by {r:.3e}")
            assert r > 10 * BAR, (tag, i, r)


def test_wave8_position_independent(feats300):
    """the same frame in the first round, as the last whole-image unit and in the tail parts"""
    for i in (255, 256, 299):
        assert torch.equal(feats300[i], feats300[0]), i


def test_wave8_deterministic(engines, frames300, feats300):
    assert torch.equal(engines[0].effnet(frames300), feats300)


def test_wave8_nan_stays_in_its_frame(engines, frames300, feats300):
    bad = (5, 270)  # a whole-image unit and a tail image
    x = frames300.clone()
    for i in bad:
        x[i, 100, 100] = float("nan")
    f = engines[0].effnet(x)
    keep = torch.ones(x.shape[0], dtype=torch.bool, device=f.device)
    for i in bad:
        assert not torch.isfinite(f[i]).all(), i
        keep[i] = False
    assert torch.isfinite(f[keep]).all()
    assert torch.equal(f[keep], feats300[keep])
