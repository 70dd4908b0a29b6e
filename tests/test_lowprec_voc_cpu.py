"""oracle/lowprec_voc.py on the CPU: the quantisation-faithful restatements of the bf16 / e4m3 vocoder kernels and their
per-element budgets, before tests/test_gpu_lowprec_voc.py holds the kernels to them through VocoderEngine.probe.

  * arith="exact" is oracle/hifigan.py at every tap and on the waveform, to float64 rounding (HIFIGAN_H and the
    ResBlock2 config of the pack tests), and the restated weight-norm fold is torch's to float32 rounding;
  * a correctly rounded stand-in (the same quantised operands in float32, another summation order, rounded where the
    kernel rounds) stays within the budget at every element, for every piece, bf16 and e4m3, on the shapes the GPU
    test uses;
  * seeded faults exceed twice the budget at some element (the table is printed, pytest -s), while the faulty stage
    carried through the rest of the exact generator passes the bars the GPU suite holds these engines to today (SNR
    >= 25 dB against the oracle for bf16, cosine >= 0.99 for fp8): the gap, shown from the reference alone.

Configs.  The MRF of HIFIGAN_H chains six convs a resblock between two taps, and a worst-case budget grows by about
sum|w| at every conv it crosses: on "h3" it is hundreds to thousands of bf16 spacings wide (the stand-in test prints
it), so hardly a fault separates there (the neighbour-clip leak at C = 32 does) and the table says so.  The one-pair configs run the same kernels two convs deep:
"one3" (three kernel sizes, dilations [[3]] * 3) and "one1" (one resblock, k = 11, d = 5).  The faults are held on
those.  Shapes: three clips, T per stage as tests/test_gpu_lowprec_voc.py has it.
"""
import json
import os

import numpy as np
import pytest
import torch

from m2s import synth
from m2s.config import HIFIGAN_H
from oracle import hifigan, lowprec_voc as V

GOLD = os.path.join(os.path.dirname(__file__), "golden")
STATE_SEED, MEL_SEED, B = 7, 11, 3
CONFIGS = {
    "h3": HIFIGAN_H,
    "one3": dict(HIFIGAN_H, resblock_dilation_sizes=[[3], [3], [3]]),
    "one1": dict(HIFIGAN_H, resblock_kernel_sizes=[11], resblock_dilation_sizes=[[5]]),
}
# mel frames per stage: the smallest T at which the stage's kernels walk three tiles with a ragged last one (module
# docstring of tests/test_gpu_lowprec_voc.py)
T_STAGE = (9, 3, 3, 2)
# (stage, MRF kernel family): what the bf16 and fp8 engines run under the defaults and the switches of the GPU test
MRF_CASES = [(0, "pairs"), (1, "pairs"), (2, "pairs"), (3, "pairs"), (2, "fused"), (3, "fused"),
             (0, "f8"), (1, "f8"), (2, "f8"), (3, "f8"), (3, "pairs8")]
BAR_SNR, BAR_COS = 25.0, 0.99  # test_gpu_parity.py / test_gpu_vocoder_stream.py (bf16); test_gpu_fp8.py (fp8)


def _r2_h():
    g = np.load(os.path.join(GOLD, "generator.npz"), allow_pickle=False)
    return json.loads(bytes(g["r2_h"]).decode())


class World:
    """Per config: the restated weights and, per stage, the stage's inputs as a bf16 engine stores them."""

    def __init__(self):
        self._w, self._x, self._exact = {}, {}, {}

    def h(self, cfg):
        return CONFIGS[cfg]

    def w(self, cfg):
        if cfg not in self._w:
            self._w[cfg] = V.voc_weights(synth.synth_generator_state(STATE_SEED, CONFIGS[cfg]), CONFIGS[cfg])
        return self._w[cfg]

    def mel(self, cfg, stage):
        return torch.from_numpy(synth.synth_mel_log(B, CONFIGS[cfg]["num_mels"], T_STAGE[stage], seed=MEL_SEED + stage))

    def taps(self, cfg, stage):
        """Taps 0 .. 2 stage + 1 of the low-precision chain (run_conv pairs in the stages before) on the stage's mel."""
        key = (cfg, stage)
        if key not in self._x:
            taps = []
            V.generator(self.w(cfg), CONFIGS[cfg], self.mel(cfg, stage), kinds=["pairs"] * 4, arith="bf16", taps=taps,
                        stop=2 * stage + 1)
            self._x[key] = taps
        return self._x[key]

    def exact_wav(self, cfg, stage):
        key = (cfg, stage)
        if key not in self._exact:
            self._exact[key] = V.generator(self.w(cfg), CONFIGS[cfg], self.mel(cfg, stage).double(), arith="exact")
        return self._exact[key]


@pytest.fixture(scope="module")
def world():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return World()


def _folded_state(w):
    """The restated float32 weights as a plain-weight state dict for oracle/hifigan.py, in float64."""
    sd = {"conv_pre.weight": w["pre"]["W"], "conv_pre.bias": w["pre"]["b"], "conv_post.weight": w["post"]["W"],
          "conv_post.bias": w["post"]["b"]}
    for i, u in enumerate(w["ups"]):
        sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"] = u["W"], u["b"]
        for j, rb in enumerate(w["rbs"][i]):
            q = f"resblocks.{i * w['nk'] + j}"
            for n in range(len(rb["dil"])):
                if rb["c2"] is None:
                    sd[f"{q}.convs.{n}.weight"], sd[f"{q}.convs.{n}.bias"] = rb["c1"][n]
                else:
                    sd[f"{q}.convs1.{n}.weight"], sd[f"{q}.convs1.{n}.bias"] = rb["c1"][n]
                    sd[f"{q}.convs2.{n}.weight"], sd[f"{q}.convs2.{n}.bias"] = rb["c2"][n]
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}


# ------------------------------------------------------------------------------ exact = the oracle
@pytest.mark.parametrize("cfg", ["r1", "r2"])
def test_exact_agrees_with_the_oracle(cfg):
    h = HIFIGAN_H if cfg == "r1" else _r2_h()
    state = synth.synth_generator_state(STATE_SEED, h)
    w = V.voc_weights(state, h)
    mel = torch.from_numpy(synth.synth_mel_log(2, h["num_mels"], 8, seed=MEL_SEED)).double()
    want, got = [], []
    wav = hifigan.generator(_folded_state(w), h, mel, taps=want)
    mine = V.generator(w, h, mel, arith="exact", taps=got)
    assert len(want) == len(got) == 1 + 2 * len(h["upsample_rates"])
    for t, (a, b) in enumerate(zip(want, got)):
        rel = float((a - b).abs().max() / a.abs().max())
        print(f"{cfg} tap {t} {tuple(a.shape)}: exact vs oracle {rel:.2e} of the tap's scale")
        assert a.shape == b.shape and rel <= 1e-12, (t, rel)
    assert float((wav - mine).abs().max()) <= 1e-12
    # the fold itself: torch's weight norm, to float32 rounding
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    for p, W in [("ups.0", w["ups"][0]["W"]), ("conv_post", w["post"]["W"]),
                 ("resblocks.0.convs1.0" if cfg == "r1" else "resblocks.0.convs.0", w["rbs"][0][0]["c1"][0][0])]:
        ref = hifigan.fold_weight({k: v.double() for k, v in sd.items() if k.startswith(p)}, p).numpy()
        assert np.abs(W - ref).max() <= 2.0 ** -22 * np.abs(ref).max(), p


# ------------------------------------------------------------------------------ a correct implementation passes
def _standin(name, f):
    ref, budget = f("float64")
    got = f("float32")
    ratio = (got.double() - ref).abs() / budget
    sp = V.spacing(ref, "bf16")
    print(f"\n{name}: stand-in worst |got - ref| / budget {float(ratio.max()):.3f}, median budget / |ref| "
          f"{float((budget / ref.abs()).median()):.4f}, median budget / bf16 spacing {float((budget / sp).median()):.2f}")
    assert torch.isfinite(ref).all() and (budget > 0).all()
    assert float(ratio.max()) <= 1.0
    return ref, budget


def test_standin_conv_pre_and_conv_post(world):
    w = world.w("h3")
    _standin("conv_pre", lambda impl: V.conv_pre(world.mel("h3", 0), w["pre"], impl=impl))
    taps = []
    V.generator(w, HIFIGAN_H, world.mel("h3", 3), kinds=["pairs"] * 4, arith="bf16", taps=taps, stop=8)
    _standin("conv_post", lambda impl: V.conv_post(taps[8], w["post"], impl=impl))


@pytest.mark.parametrize("stage", range(4))
def test_standin_upsampler(world, stage):
    w = world.w("h3")
    x = world.taps("h3", stage)[2 * stage]
    _standin(f"upsampler {stage}", lambda impl: V.upsampler(x, w["ups"][stage], impl=impl))


@pytest.mark.parametrize("stage,kind", MRF_CASES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_standin_mrf(world, cfg, stage, kind):
    w = world.w(cfg)
    x = world.taps(cfg, stage)[2 * stage + 1]
    _standin(f"{cfg} mrf {stage} {kind} {tuple(x.shape)}", lambda impl: V.mrf(x, w["rbs"][stage], kind=kind, impl=impl))


# ------------------------------------------------------------------------------ seeded faults
def _snr(got, ref):
    return float(10 * torch.log10((ref ** 2).sum() / ((got - ref) ** 2).sum()))


def _cos(a, b):
    a, b = a.flatten(), b.flatten()
    return float(a @ b / (a.norm() * b.norm()))


def _mrf_faults(kind, k, C, nk):
    tile, flat = V.tile_rows(kind, C)
    out = {"hist": (tile, 1, flat), "hist_all": (tile, None, flat), "leak": None, "tap": (tile, k - 1, flat), "dil": None,
           "kswap": (5, 9), "chan": (3, 4)}
    if kind == "fused":
        out["res10"] = None
    if nk >= 3:
        out["accum"] = None
    return out


TABLE = []
# (config, stage, kernel family, fault) the budget does not separate (ratio under 2): listed, not dropped; asserted to be
# under 2 so the list stays true.  A tap dropped on one row of a 128-row tile, or a neighbour's bias, moves a wide
# stage's output by less than the flips its two convs may carry.  hist and leak are never in this list.
NOT_SEPARATED = {
    ("one3", 0, "pairs", "tap"), ("one3", 0, "pairs", "chan"), ("one3", 0, "pairs", "kswap"), ("one3", 0, "f8", "tap"),
    ("one3", 0, "f8", "chan"), ("one3", 0, "f8", "kswap"), ("one3", 1, "pairs", "tap"), ("one3", 1, "f8", "tap"),
    ("one3", 1, "f8", "chan"), ("one3", 3, "pairs8", "tap"), ("one3", 3, "pairs8", "chan"),
    ("one1", 0, "pairs", "tap"), ("one1", 0, "pairs", "chan"), ("one1", 0, "pairs", "kswap"), ("one1", 0, "f8", "tap"),
    ("one1", 0, "f8", "chan"), ("one1", 0, "f8", "kswap"), ("one1", 1, "pairs", "chan"), ("one1", 1, "f8", "tap"),
    ("one1", 1, "f8", "chan"), ("one1", 3, "pairs8", "chan"),
    ("gemm", "conv_pre", "", "tap"),  # one look-ahead tap of 7 x 64 on one row in 128: under conv_pre's bf16 spacing
}
# faults that today's aggregate bar already rejects on that config (asserted to be under the bar): with one resblock the
# fused kernel's residual IS the stage's output
VISIBLE_TODAY = {("one1", 2, "fused", "res10")}
BARRED = ("hist", "leak", "tap", "res10")  # carried to the waveform and held to today's bar


def _judge(rows):
    """rows: (key, text, ratio, bar_ok or None).  Every row is printed and kept; then the assertions."""
    bad = []
    for key, text, ratio, bar_ok in rows:
        sep = ratio >= 2.0
        text += "" if sep else "   NOT SEPARATED"
        print(text)
        TABLE.append(text)
        if key[3] in ("hist", "leak") and key[0] != "h3":
            assert key not in NOT_SEPARATED
        if key[0] != "h3" and sep == (key in NOT_SEPARATED):
            bad.append(text + ("   (listed as not separated)" if sep else "   (under 2 and not listed)"))
        if bar_ok is not None and bar_ok == (key in VISIBLE_TODAY):
            bad.append(text + ("   (listed as visible today)" if bar_ok else "   (today's bar rejects it)"))
    assert not bad, "\n".join(bad)


def _fault_rows(world, cfg, stage, kind, at, faults, bars=True):
    w, h = world.w(cfg), world.h(cfg)
    rbs = w["rbs"][stage]
    x = world.taps(cfg, stage)[2 * stage + 1]
    ref, budget = V.mrf(x, rbs, kind=kind)
    rows = []
    for name, site in faults.items():
        got = V.stored(V.mrf(x, rbs, kind=kind, fault=(name.split("_")[0], site), at=at, want_budget=False)[0])
        ratio = float(((got - ref).abs() / budget).max())
        text = f"{cfg} mrf {stage} {kind:7s} {name:8s} worst |got - ref| / budget {ratio:10.2f}"
        bar_ok = None
        if bars and name.split("_")[0] in BARRED:
            wav = V.generator(w, h, None, arith="exact", start=2 * stage + 2, x=got)
            want = world.exact_wav(cfg, stage)
            snr, cos = _snr(wav, want), _cos(wav, want)
            text += f"   wav SNR {snr:5.1f} dB cosine {cos:.5f}"
            if name in BARRED:  # hist_all is printed only: a fault in every tile is not the gap's example
                bar_ok = cos >= BAR_COS if kind in ("f8", "pairs8") else snr >= BAR_SNR
        rows.append(((cfg, stage, kind, name), text, ratio, bar_ok))
    return rows


@pytest.mark.parametrize("stage,kind", MRF_CASES)
@pytest.mark.parametrize("cfg", ["one3", "one1"])
def test_mrf_faults_break_the_budget_and_pass_todays_bars(world, cfg, stage, kind):
    """Every fault kind that applies, seeded into the resblock with the longest kernel (its history is the longest):
    at least twice the budget at some element, or listed in NOT_SEPARATED; hist and leak always separate.  hist (one
    tile), leak, tap and res10, carried through the rest of the exact generator, pass today's aggregate bar."""
    rbs = world.w(cfg)["rbs"][stage]
    at = len(rbs) - 1
    C = world.h(cfg)["upsample_initial_channel"] >> (stage + 1)
    _judge(_fault_rows(world, cfg, stage, kind, at, _mrf_faults(kind, rbs[at]["k"], C, len(rbs))))


@pytest.mark.parametrize("stage,kind", MRF_CASES)
def test_mrf_faults_on_the_three_pair_config_are_recorded(world, stage, kind):
    """HIFIGAN_H's own MRF: six convs a resblock between the taps.  The budget is a derived worst case and mostly too
    wide there; hist and leak are recorded with what they reach (the reason the one-pair configs exist), and nothing
    is asserted of them but that they were computed."""
    tile, flat = V.tile_rows(kind, HIFIGAN_H["upsample_initial_channel"] >> (stage + 1))
    rows = _fault_rows(world, "h3", stage, kind, 2, {"hist_all": (tile, None, flat), "leak": None}, bars=False)
    _judge(rows)
    assert all(np.isfinite(r[2]) for r in rows)


def test_single_gemm_faults(world):
    """conv_pre, the upsamplers and conv_post: one GEMM deep, so the budget is about a bf16 spacing and every fault
    stands far over it."""
    w = world.w("h3")
    mel = world.mel("h3", 0)
    cases = [("conv_pre", lambda f: V.conv_pre(mel, w["pre"], fault=f),
              {"leak": None, "tap": (128, 6), "kswap": (5, 9), "chan": (3, 4)})]
    for i in range(4):
        x = world.taps("h3", i)[2 * i]
        cases.append((f"upsampler {i}", lambda f, x=x, i=i: V.upsampler(x, w["ups"][i], fault=f),
                      {"phase": None, "leak": None, "kswap": (5, 9), "chan": (3, 4)}))
    taps = []
    V.generator(w, HIFIGAN_H, world.mel("h3", 3), kinds=["pairs"] * 4, arith="bf16", taps=taps, stop=8)
    cases.append(("conv_post", lambda f: V.conv_post(taps[8], w["post"], fault=f),
                  {"leak": None, "tap": (256, 6, False), "kswap": (5, 9)}))
    rows = []
    for name, f, faults in cases:
        ref, budget = f(None)
        for kind, site in faults.items():
            got = f((kind, site))[0]
            got = got if name == "conv_post" else V.stored(got)
            ratio = float(((got - ref).abs() / budget).max())
            rows.append((("gemm", name, "", kind), f"{name:12s} {kind:6s} worst |got - ref| / budget {ratio:10.2f}", ratio,
                         None))
    _judge(rows)
