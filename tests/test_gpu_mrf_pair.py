"""The fused ResBlock1 pair of the split-fp32 C = 64 MRF stage (conv1d_halo.hip conv1d_halo_pair_kernel; vocoder.cpp
mrf_stage_batched, engine switch M2S_MRF_PAIR) against the launch-per-conv path it replaces (M2S_MRF_PAIR=0).

Both convs of a pair keep their stage order and the tensor between them is the split4 value the c1 launch stores, so
the fused path must give the same bits: torch.equal on the wav, plus the fp32 bar (1e-4) against the oracle.  At
HIFIGAN_H the C = 64 stage has L = 210 T and the pair kernel's tile is 112 output rows.  GPU box only.
"""
import numpy as np
import pytest
import torch

from m2s import _native, synth
from m2s.config import HIFIGAN_H
from oracle import hifigan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAIR = "conv1d_halo_pair_kernel<64>"
CONV = "conv1d_halo_sp_kernel<64>"
# C = 64 stage at L = 8 T: clips shorter than one tile (T = 20: 160 rows is two tiles) and than the 64-row history
H_SHORT = dict(HIFIGAN_H, upsample_rates=[2, 2, 2, 2], upsample_kernel_sizes=[4, 4, 4, 4], hop_size=16)
# k = 13, d = 5 reaches 60 + 12 = 72 > 64 rows back: no stage may run the pair kernel
H_REACH = dict(HIFIGAN_H, resblock_kernel_sizes=[3, 7, 13])


@pytest.fixture(scope="module")
def rt():
    from m2s import runtime
    return runtime


def _engines(rt, monkeypatch, sd, h):
    """(fused, unfused) engines; the switches are read once at engine creation."""
    monkeypatch.delenv("M2S_MRF_PAIR", raising=False)
    fused = rt.VocoderEngine(sd, h, dtype="bf16x3", device=DEV)
    monkeypatch.setenv("M2S_MRF_PAIR", "0")
    plain = rt.VocoderEngine(sd, h, dtype="bf16x3", device=DEV)
    monkeypatch.delenv("M2S_MRF_PAIR")
    return fused, plain


def _oracle(sd, h, mel):
    return hifigan.generator({k: torch.from_numpy(v) for k, v in sd.items()}, h, torch.from_numpy(mel)).numpy()


def _launches(eng, mel):
    """(name, stage) of every launch of one forward."""
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        eng.forward(mel)
        torch.cuda.synchronize()
        return [(r["name"], r["stage"]) for r in _native.prof_launches()]
    finally:
        _native.prof_enable(False)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (2, 5)])
def test_pair_bit_identical_and_oracle(rt, monkeypatch, B, T):
    """(1, 1): two tiles, the first with an all-zero history, the last ragged.  (3, 2): tiles that meet a clip
    boundary (no history may leak from the previous clip).  (2, 5): interior tiles with a full history."""
    sd = synth.synth_generator_state(11, HIFIGAN_H)
    mel = synth.synth_mel_log(B, 64, T, seed=B * 7 + T)
    fused, plain = _engines(rt, monkeypatch, sd, HIFIGAN_H)
    x = torch.from_numpy(mel).to(DEV)
    a, b = fused.forward(x), plain.forward(x)
    assert torch.equal(a, b), float((a - b).abs().max())
    err = float(np.abs(a.cpu().numpy() - _oracle(sd, HIFIGAN_H, mel)).max())
    print(f"B={B} T={T}: max|fused - oracle| = {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("T", [3, 20])
def test_pair_clip_shorter_than_tile_and_history(rt, monkeypatch, T):
    """upsample_rates [2, 2, 2, 2]: L = 24 at C = 64 (shorter than the history) and L = 160 (a ragged second tile)."""
    sd = synth.synth_generator_state(5, H_SHORT)
    mel = synth.synth_mel_log(2, 64, T, seed=T)
    fused, plain = _engines(rt, monkeypatch, sd, H_SHORT)
    x = torch.from_numpy(mel).to(DEV)
    assert any(n == PAIR for n, _ in _launches(fused, x))
    a, b = fused.forward(x), plain.forward(x)
    assert torch.equal(a, b), float((a - b).abs().max())
    err = float(np.abs(a.cpu().numpy() - _oracle(sd, H_SHORT, mel)).max())
    print(f"T={T}: max|fused - oracle| = {err:.3e}")
    assert err <= 1e-4


def test_pair_fallback_when_reach_exceeds_history(rt, monkeypatch):
    """resblock_kernel_sizes [3, 7, 13]: the k = 13, d = 5 pair reaches 72 rows back, so the C = 64 stage as a
    whole stays on the launches per conv."""
    monkeypatch.delenv("M2S_MRF_PAIR", raising=False)
    sd = synth.synth_generator_state(7, H_REACH)
    mel = synth.synth_mel_log(2, 64, 3, seed=3)
    eng = rt.VocoderEngine(sd, H_REACH, dtype="bf16x3", device=DEV)
    x = torch.from_numpy(mel).to(DEV)
    rec = _launches(eng, x)
    assert not any(n == PAIR for n, _ in rec), rec
    assert any(st == "mrf_c64" for _, st in rec)
    err = float(np.abs(eng.forward(x).cpu().numpy() - _oracle(sd, H_REACH, mel)).max())
    print(f"fallback: max|wav - oracle| = {err:.3e}")
    assert err <= 1e-4


def test_pair_launch_log(rt, monkeypatch):
    """Default switches at HIFIGAN_H: the C = 64 stage runs the pair kernel and no launch per conv.  64 x 30 fills
    the chip: one launch per pair, the last with the MRF sum chained in registers (3).  One clip: the first two
    pairs batched over the resblocks, the last pair one launch per resblock for the MRF sum (2 + 3)."""
    monkeypatch.delenv("M2S_MRF_PAIR", raising=False)
    monkeypatch.delenv("M2S_MRF_CHAIN", raising=False)
    eng = rt.VocoderEngine(synth.synth_generator_state(11, HIFIGAN_H), HIFIGAN_H, dtype="bf16x3", device=DEV)
    for (B, T), want in (((64, 30), 3), ((1, 30), 5)):
        x = torch.from_numpy(synth.synth_mel_log(B, 64, T, seed=1)).to(DEV)
        c64 = [n for n, st in _launches(eng, x) if st == "mrf_c64"]
        assert CONV not in c64, c64
        assert c64 == [PAIR] * want, ((B, T), c64)


def test_pair_chained_sum_bit_identical(rt, monkeypatch):
    """A pass that fills the chip (64 clips x 5 frames: 640 tiles, the last of a clip ragged), so the last pairs
    run chained with the MRF sum in registers, gives the bits of the launch-per-conv path."""
    sd = synth.synth_generator_state(11, HIFIGAN_H)
    fused, plain = _engines(rt, monkeypatch, sd, HIFIGAN_H)
    x = torch.from_numpy(synth.synth_mel_log(64, 64, 5, seed=9)).to(DEV)
    assert [n for n, st in _launches(fused, x) if st == "mrf_c64"] == [PAIR] * 3
    a, b = fused.forward(x), plain.forward(x)
    assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (64, 7)])
def test_pair_c128_switch(rt, monkeypatch, B, T):
    """M2S_MRF_PAIR128=1 puts the C = 128 stage (L = 70 T) on the same kernel, 8 waves: clips shorter than a tile
    and than the history, clip boundaries inside a tile's history, and a pass that chains the last pairs.  Its
    sums run in another order than conv_gemm's, so the bar is the oracle's (the two smaller cases) and, at 64 x 7
    where the oracle takes too long, the default engine at the same 1e-4."""
    monkeypatch.setenv("M2S_MRF_PAIR128", "1")
    sd = synth.synth_generator_state(11, HIFIGAN_H)
    mel = synth.synth_mel_log(B, 64, T, seed=B + T)
    eng = rt.VocoderEngine(sd, HIFIGAN_H, dtype="bf16x3", device=DEV)
    monkeypatch.delenv("M2S_MRF_PAIR128")
    x = torch.from_numpy(mel).to(DEV)
    c128 = [n for n, st in _launches(eng, x) if st == "mrf_c128"]
    assert c128 == ["conv1d_halo_pair_kernel<128>"] * (3 if B == 64 else 5), c128
    wav = eng.forward(x).cpu().numpy()
    if B == 64:
        ref = rt.VocoderEngine(sd, HIFIGAN_H, dtype="bf16x3", device=DEV).forward(x).cpu().numpy()
    else:
        ref = _oracle(sd, HIFIGAN_H, mel)
    err = float(np.abs(wav - ref).max())
    print(f"C=128 B={B} T={T}: max|d| = {err:.3e}")
    assert np.isfinite(wav).all() and err <= 1e-4


def test_pair_ragged_and_chunk_calls_bit_identical(rt, monkeypatch):
    """forward_ragged (clips of 1, 4 and 2 frames in one call) and the streaming chunk call (two spans with
    context and hold) through the fused stage against M2S_MRF_PAIR=0."""
    sd = synth.synth_generator_state(11, HIFIGAN_H)
    fused, plain = _engines(rt, monkeypatch, sd, HIFIGAN_H)
    lengths = [1, 4, 2]
    mels = [torch.from_numpy(np.ascontiguousarray(synth.synth_mel_log(1, 64, t, seed=20 + t)[0].T)).to(DEV)
            for t in lengths]
    a, b = fused.forward_ragged(mels), plain.forward_ragged(mels)
    assert a.numel() == sum(lengths) * fused.hop and torch.equal(a, b)
    back, ahead = fused.reach
    spans = [torch.from_numpy(np.ascontiguousarray(synth.synth_mel_log(1, 64, t, seed=40 + t)[0].T)).to(DEV)
             for t in (back + ahead + 3, back + 2)]
    kw = dict(context=[back, back], hold=[ahead, 0])
    a, b = fused.forward_chunk(spans, **kw), plain.forward_chunk(spans, **kw)
    assert a.numel() == (3 + 2) * fused.hop and torch.equal(a, b)
