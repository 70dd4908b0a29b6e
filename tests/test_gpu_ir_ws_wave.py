"""The per-wave form of the split IR front half on 16-wide maps (csrc/ir_ws_wave.hpp: expand -> SiLU -> depthwise ->
SiLU -> store -> squeeze by one wave on the expand's MFMA accumulators) against the handed-off form
it replaces there (M2S_IR_WS=handoff) and the fp32 oracle.  Both forms are the same split fp32 arithmetic up to the
squeeze's summation order, which moves a few 17-bit roundings: the bar is the parity bar of
test_ir_ws_matches_grid_kernel, relative 1e-4.  All engines run ir_ws and se_ws at any pass size (M2S_IRWS_MIN=0,
M2S_SEWS_MIN=0).  GPU box only."""
import numpy as np
import pytest
import torch

from m2s import synth
from oracle import effnet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TAPS = (10, 12, 13, 18)  # after blocks 3.1, 3.3, 4.0, 4.5: the 16-wide stride-1 IR blocks
WAVE, HAND = "ir_ws_kernel<16, 4, 1>", "ir_ws_kernel<16, 4, 1, 1>"


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.fixture(scope="module")
def ac_state():
    return synth.synth_acoustic_state(11)


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
    fr = torch.from_numpy(synth.synth_frames(1, 300, seed=31)[0])
    for i in (255, 256, 299):
        fr[i] = fr[0]
    return fr.to(DEV)


@pytest.fixture(scope="module")
def feats300(engines, frames300):
    return engines[0].effnet(frames300).clone()


@pytest.mark.parametrize("n", [3, 300])
def test_wave_form_matches_handed_off_form(engines, frames300, n):
    wave, hand = engines
    x = frames300[:n] if n == 3 else frames300
    for i in TAPS:
        a, b = wave.probe(x, i).cpu().numpy(), hand.probe(x, i).cpu().numpy()
        r = _rel(a, b)
        print(f"n {n} tap {i}: rel {r:.3e}")
        assert np.isfinite(a).all() and r <= 1e-4, (i, r)
    r = _rel(wave.effnet(x).cpu().numpy(), hand.effnet(x).cpu().numpy())
    print(f"n {n} effnet: rel {r:.3e}")
    assert r <= 1e-4
    nw, nh = _names(wave, x), _names(hand, x)
    assert WAVE in nw and HAND not in nw, sorted(nw)
    assert HAND in nh and WAVE not in nh, sorted(nh)


def test_wave_form_matches_oracle_taps(engines, ac_state, frames300):
    wave, _ = engines
    sd = {k: torch.from_numpy(v) for k, v in ac_state.items()}
    fr = frames300[:3].cpu()
    taps = []
    effnet.effnet_features(sd, fr, taps=taps)
    for i in TAPS:
        r = _rel(wave.probe(fr.to(DEV), i).cpu().numpy(), taps[i].numpy())
        print(f"tap {i} vs oracle: rel {r:.3e}")
        assert r <= 1e-4, (i, r)


@pytest.mark.parametrize("hw", [(144, 256), (32, 256)])
def test_wave_form_edge_maps(engines, ac_state, hw):
    """9 x 16 maps (an odd, partial H) and 2 x 16 maps (every output row has a vertical tap row outside the image),
    against the handed-off form and the oracle.  Two rows are the fewest an engine reaches: it takes frames of at
    least 32 rows (test_one_row_maps_are_out_of_reach).  Their 8-wide maps have H != 8 and stay on the handed-off
    form, whose record keeps its name."""
    wave, hand = engines
    sd = {k: torch.from_numpy(v) for k, v in ac_state.items()}
    fr = torch.from_numpy(synth.synth_frames(1, 3, hw=hw, seed=37)[0])
    x = fr.to(DEV)
    taps = []
    effnet.effnet_features(sd, fr, taps=taps)
    for i in TAPS:
        a = wave.probe(x, i).cpu().numpy()
        rh, ro = _rel(a, hand.probe(x, i).cpu().numpy()), _rel(a, taps[i].numpy())
        print(f"hw {hw} tap {i}: vs handed-off {rh:.3e} vs oracle {ro:.3e}")
        assert rh <= 1e-4 and ro <= 1e-4, (i, rh, ro)
    a = wave.effnet(x).cpu().numpy()
    assert _rel(a, hand.effnet(x).cpu().numpy()) <= 1e-4
    assert _rel(a, effnet.effnet_gap(sd, fr).numpy()) <= 1e-4
    nw, nh = _names(wave, x), _names(hand, x)
    assert WAVE in nw and HAND in nh and WAVE not in nh, (sorted(nw), sorted(nh))
    for names in (nw, nh):  # the 8-wide blocks: the handed-off form under its default name
        wide8 = {k for k in names if k.startswith("ir_ws_kernel<8,")}
        assert wide8 and all(k.count(",") == 2 for k in wide8), sorted(names)


def test_one_row_maps_are_out_of_reach(engines):
    """hw = (16, 256) would give 1 x 16 maps, but effnet takes no frame under 32 rows: the kernel's H = 1 path (no
    vertical tap inside the image) cannot be reached through an engine, and 2 x 16 above is the smallest map"""
    x = torch.from_numpy(synth.synth_frames(1, 3, hw=(16, 256), seed=37)[0]).to(DEV)
    with pytest.raises(RuntimeError, match="bad input size"):
        engines[0].effnet(x)


def test_wave_form_position_independent(feats300):
    """the same frame in the first round, as the last whole-image unit and in the tail parts"""
    for i in (255, 256, 299):
        assert torch.equal(feats300[i], feats300[0]), i


def test_wave_form_deterministic(engines, frames300, feats300):
    assert torch.equal(engines[0].effnet(frames300), feats300)


def test_wave_form_nan_stays_in_its_frame(engines, frames300, feats300):
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
