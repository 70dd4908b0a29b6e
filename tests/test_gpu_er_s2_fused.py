"""blocks.2.0 of the split-fp32 ("bf16x3") engine in one launch, and se_ws's tile order.

blocks.2.0 is the stride-2 EdgeResidual block (32 -> 128 -> 56 channels).  The fused path
(conv_gemm.hip EP = 1, launch_conv_gemm_er) runs conv_pwl as the epilogue GEMM of conv_exp's 128 x 128 tile:
the SiLU'd, split 128-channel map stays in LDS.  It issues the MFMAs of the two conv_gemm launches it replaces
(M2S_ER_S2_FUSED=0) in the same order on the same operands, so the two are compared bit for bit, and the
fused one against the fp32 oracle at the CNN-tap bar of tests/test_gpu_bf16x3.py (1e-4 of the tensor's scale).
Every test reads the launch log, so a silent fallback cannot pass.

The shapes are the smallest at which the tile logic can go wrong (the tile is 128 output pixels):
  3 x  96 x  96: 24x24 -> 12x12, 144 px a frame: tiles straddle frames, the last tile (48 rows) is partial
  3 x 124 x 124: 31x31 -> 16x16, odd input: TF-SAME puts one leading pad row and column
  3 x 128 x 128: 32x32 -> 16x16, even input: no leading pad
  1 x  64 x 128: one 8x16 output map = exactly one tile
At these sizes conv_gemm would split K (a handful of tiles), which keeps the two launches, so M2S_KSPLIT=1
holds nks at 1.

M2S_SEWS_REV walks se_ws's tiles newest-first; every tile is independent of the order, so on / off are
bit-identical (512 frames: the smallest pass that passes both the ir_ws and the se_ws gates; 556 frames with
M2S_SEWS_HALF=1: 44 / 22 tiles past the last full round run as half tiles).
"""
import functools
import re

import numpy as np
import pytest
import torch

from m2s import synth
from oracle import effnet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

FUSED = "conv_gemm_kernel<128, 128, 4, 4, 2, 0, 0, 1, 1>"
EXP = "conv_gemm_kernel<128, 128, 4, 4, 2, 0, 0, 1>"   # conv_exp 3x3 stride 2, split
PWL = "conv_gemm_kernel<128, 64, 4, 2, 3, 3, 0, 1>"    # conv_pwl 1x1, split
SHAPES = [(3, (96, 96)), (3, (124, 124)), (3, (128, 128)), (1, (64, 128))]
IDS = ["3x96x96", "3x124x124", "3x128x128", "1x64x128"]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.fixture(scope="module")
def rt():
    from m2s import runtime
    return runtime


@pytest.fixture(scope="module")
def ac_state():
    return synth.synth_acoustic_state(3)


@functools.lru_cache(maxsize=None)
def _frames(n, hw, seed=31):
    return torch.from_numpy(synth.synth_frames(1, n, hw=hw, seed=seed)[0])


_ORACLE = {}


def _oracle_tap6(ac_state, n, hw):
    """The fp32 oracle's map after blocks.2.0, computed once per shape."""
    if (n, hw) not in _ORACLE:
        sd = {k: torch.from_numpy(v) for k, v in ac_state.items()}
        taps = []
        effnet.effnet_features(sd, _frames(n, hw), taps=taps)
        _ORACLE[(n, hw)] = taps[6].numpy()
    return _ORACLE[(n, hw)]


def _engines(rt, ac_state, monkeypatch):
    """(fused, off): M2S_ER_S2_FUSED is read once, when an engine is created."""
    monkeypatch.delenv("M2S_ER_S2_FUSED", raising=False)
    fused = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
    monkeypatch.setenv("M2S_ER_S2_FUSED", "0")
    off = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
    monkeypatch.delenv("M2S_ER_S2_FUSED")
    return fused, off


def _names(fn):
    from m2s import _native
    _native.prof_enable(True)
    out = fn()
    torch.cuda.synchronize()
    names = [r["name"] for r in _native.prof_launches()]  # in launch order, one entry per launch
    _native.prof_enable(False)
    return out, names


@pytest.mark.parametrize("n,hw", SHAPES, ids=IDS)
def test_er_s2_fused_matches_oracle_and_two_launches(rt, ac_state, monkeypatch, n, hw):
    monkeypatch.setenv("M2S_KSPLIT", "1")  # nks = 1: the fused path's condition (a few tiles would split K)
    fused, off = _engines(rt, ac_state, monkeypatch)
    x = _frames(n, hw).to(DEV)
    a6, names_f = _names(lambda: fused.probe(x, 6))
    b6, names_o = _names(lambda: off.probe(x, 6))
    # one fused launch in place of one conv_exp and one conv_pwl launch (off 256 x 256 the stride-1 EdgeResidual
    # blocks before it run their conv_exp on the same conv_gemm instance, so the launches are counted)
    assert names_f.count(FUSED) == 1 and names_f.count(PWL) == 0, names_f
    assert names_o.count(FUSED) == 0 and names_o.count(PWL) == 1, names_o
    assert names_f.count(EXP) == names_o.count(EXP) - 1 and len(names_f) == len(names_o) - 1, (names_f, names_o)
    ref = _oracle_tap6(ac_state, n, hw)
    assert tuple(a6.shape) == ref.shape
    e_f, e_o = _rel(a6.cpu().numpy(), ref), _rel(b6.cpu().numpy(), ref)
    print(f"blocks.2.0 {n}x{hw}: fused vs oracle {e_f:.3e}, two launches vs oracle {e_o:.3e}")
    assert e_f <= 1e-4, e_f
    if hw == (124, 124):  # the shape is a fair one: the path it replaces meets the bar on it too
        assert e_o <= 1e-4, e_o
    # the same MFMAs in the same order on the same operands: bit for bit, here and downstream
    assert torch.equal(a6, b6)
    assert torch.equal(fused.probe(x, 7), off.probe(x, 7))
    assert torch.equal(fused.effnet(x), off.effnet(x))


def test_er_s2_small_pass_plan_keeps_two_launches(rt, ac_state, monkeypatch):
    """One 30-frame clip of 256 x 256: 240 tiles fill under half a round of workgroup slots, so conv_gemm cuts
    conv_exp's K into ranges (partial sums, no mid tile) and the block stays on the two launches."""
    monkeypatch.delenv("M2S_KSPLIT", raising=False)
    fused, off = _engines(rt, ac_state, monkeypatch)
    x = _frames(30, (256, 256)).to(DEV)
    a6, names = _names(lambda: fused.probe(x, 6))
    assert EXP in names and PWL in names and FUSED not in names, names
    assert torch.isfinite(a6).all() and torch.equal(a6, off.probe(x, 6))


def test_er_s2_fused_confines_a_nan_to_its_windows(rt, ac_state, monkeypatch):
    """A NaN planted in one pixel of frame 1 reaches blocks.2.0's input as a small patch; exactly the output pixels
    whose stride-2 3x3 TF-SAME window touches the patch are non-finite (every channel), the rest of frame 1 and all
    of frames 0 and 2 stay finite: a zero-page lane or a tile's unused LDS rows never reach a real output (96 x 96:
    the tiles straddle the frames and the last one is partial)."""
    monkeypatch.setenv("M2S_KSPLIT", "1")
    fused, off = _engines(rt, ac_state, monkeypatch)
    x = _frames(3, (96, 96)).clone()
    x[1, 40, 57] = float("nan")
    x = x.to(DEV)
    t5 = fused.probe(x, 5)                      # blocks.2.0's input (N, 32, 24, 24)
    t6, names = _names(lambda: fused.probe(x, 6))
    assert FUSED in names, names
    bad_in = (~torch.isfinite(t5)).any(dim=1).cpu().numpy()       # (N, IH, IW)
    assert bad_in[1].any() and not bad_in[0].any() and not bad_in[2].any()
    N, IH, IW = bad_in.shape
    OH, OW = (IH + 1) // 2, (IW + 1) // 2
    pt, pl = max((OH - 1) * 2 + 3 - IH, 0) // 2, max((OW - 1) * 2 + 3 - IW, 0) // 2
    want = np.zeros((N, OH, OW), dtype=bool)
    for f, iy, ix in zip(*np.nonzero(bad_in)):
        for oy in range(OH):
            for ox in range(OW):
                if 0 <= iy - (2 * oy - pt) < 3 and 0 <= ix - (2 * ox - pl) < 3:
                    want[f, oy, ox] = True
    bad_out = ~torch.isfinite(t6).cpu().numpy()                   # (N, C, OH, OW)
    assert tuple(t6.shape[2:]) == (OH, OW)
    assert (bad_out.all(axis=1) == want).all() and (bad_out.any(axis=1) == want).all()
    assert (bad_out == ~torch.isfinite(off.probe(x, 6)).cpu().numpy()).all()


@pytest.mark.parametrize("n,half", [(512, False), (556, True)], ids=["512", "556-half-tiles"])
def test_se_ws_reverse_walk_is_bit_identical(rt, ac_state, monkeypatch, n, half):
    if half:
        monkeypatch.setenv("M2S_SEWS_HALF", "1")
    x = _frames(n, (256, 256), seed=47).to(DEV)
    monkeypatch.delenv("M2S_SEWS_REV", raising=False)  # the default
    rev = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
    monkeypatch.setenv("M2S_SEWS_REV", "0")
    fwd = rt.AcousticEngine(ac_state, dtype="bf16x3", device=DEV)
    gr, names_r = _names(lambda: rev.effnet(x))
    gf, names_f = _names(lambda: fwd.effnet(x))
    sr = {k for k in names_r if k.startswith("se_ws_kernel")}
    sf = {k for k in names_f if k.startswith("se_ws_kernel")}
    assert len(names_r) == len(names_f)
    # both tiles (256 x 128 at 16x16, 128 x 224 at 8x8) on se_ws; the reversed instances (the order flag after the
    # six tile / ring numbers) in the REV engine only
    for s in (sr, sf):
        assert any(k.startswith("se_ws_kernel<4, 1, 8,") for k in s) and any(k.startswith("se_ws_kernel<2, 2, 7,") for k in s), s
    assert all(re.match(r"se_ws_kernel<(\d+, ){6}true, false", k) for k in sr), names_r
    assert all(re.match(r"se_ws_kernel<(\d+, ){6}false", k) for k in sf), names_f
    assert torch.isfinite(gr).all() and torch.equal(gr, gf)
    for i in (13, 20):  # after blocks.4.0 (16x16) and blocks.5.1 (8x8, skip)
        assert torch.equal(rev.probe(x, i), fwd.probe(x, i)), i
