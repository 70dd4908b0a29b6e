"""The bf16 and e4m3 early-CNN kernels, element by element, against oracle/lowprec.py.  GPU box only.

tests/test_gpu_parity.py and tests/test_gpu_fp8.py hold these kernels by cosines (0.999 / 0.995) and a fused-vs-unfused
rel 2e-2, which a dropped tap on a tile edge, two exchanged K slots, a neighbour's scale or a misplaced pad all pass
(tests/test_lowprec_cpu.py shows it).  Here every output element of stem_b0, ers2_fused, er_fused, er2_fused, er8_fused,
er8w_fused and of the unfused conv sequence is compared with a float64 restatement that quantises where the kernel does,
within a budget built from the kernel's rounding points alone (oracle/lowprec.py: output rounding, fp32 accumulation,
transcendentals, intermediate flips; no multiplier).

Procedure of a case: probe(x, i - 1) twice with equal bits (the block's input, bf16 values), probe(x, i), the launch log
names the kernel, |got - ref| <= budget at every element of the images the reference is computed for; the worst ratio
and the median budget / |ref| are printed (pytest -s; DESIGN.md "Per-element budgets" holds a run's figures).

Shapes: per kernel the smallest frame at which its map has two tiles in each direction, and enough frames that a
persistent workgroup walks three or more tiles (asserted from the launcher's grid rule and the device's CU count).  The
reference is computed for the first and the last image and one of every later trip of the loop (the blocks are
per-image independent).

Left out (DESIGN.md "Per-element budgets" has the figures): er8_fused on the saturation state dict of
tests/test_lowprec_cpu.py (oracle.lowprec.saturated_state).  Where all three scaled mid channels sit at 448 and cancel in
conv_pwl, the block-scaled K = 128 MFMA's sum is off by up to 2^-13.3 of its largest product, over 4 x the fp32-ulp-per-add
term (6 of 65 536 elements over the budget, worst 2.23 x); nothing we can cite gives the accuracy of that instruction's
internal sum, so the budget has no term to hold it with, and none was invented.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from m2s import synth
from oracle import lowprec as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STATE_SEED = 8
ER = {"blocks.1.0": (1, 0, 2), "blocks.1.1": (1, 1, 1), "blocks.1.2": (1, 2, 1),
      "blocks.2.0": (2, 0, 2), "blocks.2.1": (2, 1, 1), "blocks.2.2": (2, 2, 1)}
# frame sets: (frames, (H, W), seed, the images the reference is computed for)
SETS = {
    # 64 x 128: blocks.1 maps 16 x 32 = 2 x 2 tiles of ers2_fused (8 x 16 outputs) and er8_fused (8 x 16); the stem
    # map 32 x 64 = 2 x 4 tiles of stem_b0 (16 x 16).  257 frames: 1028 tiles, a third trip for the 512 tiles a round
    # of ers2_fused<16, 64, 32> (two workgroups a CU) and of er8_fused (two half-workgroup tiles); stem_b0's 768
    # workgroups take 1028 strips of two tiles, so a quarter of them walk four (strips 96.., image 25)
    "A": (257, (64, 128), 51, (0, 25, 128, 256)),
    # 128 x 128: blocks.1 maps 32 x 32 = 2 x 2 tiles of er_fused (16 x 16); 129 frames: 516 tiles on 256 workgroups
    "B": (129, (128, 128), 52, (0, 64, 128)),
    # 256 x 256: blocks.2 maps 32 x 32 = 2 x 2 tiles of er2_fused / er8w_fused (16 x 16), 4 x 2 of
    # ers2_fused<32, 128, 64>; 129 frames: 516 / 1032 tiles on 256 workgroups (a trip of the latter = 32 images)
    "C": (129, (256, 256), 53, (0, 32, 64, 96, 128)),
    # odd sizes: TF-SAME bottom / right pads at every stride-2 conv and partial tiles (the unfused sequence)
    "D": (3, (67, 101), 54, (0, 1, 2)),
}
UNFUSED = {"M2S_STEM_FUSED": "0", "M2S_ER_FUSED": "0", "M2S_ER_S2_FUSED": "0"}
FUSED_NAMES = ("stem_b0_kernel", "ers2_fused_kernel", "er_fused_kernel", "er2_fused_kernel", "er8_fused_kernel",
               "er8w_fused_kernel")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class World:
    def __init__(self, state):
        self.w = {"stem": L.stem_weights(state), "blocks.0.0": L.cn_weights(state, 0, 0),
                  "blocks.0.1": L.cn_weights(state, 0, 1)}
        for name, (s, i, _) in ER.items():
            self.w[name] = L.er_weights(state, s, i)

    def run(self, name, x, arith):
        if name == "stem_b0":
            return L.stem_b0(x, self.w["stem"], self.w["blocks.0.0"], self.w["blocks.0.1"])
        if name == "stem":
            return L.stem(x, self.w["stem"])
        if name in ("blocks.0.0", "blocks.0.1"):
            return L.conv_bn_act(x, self.w[name])
        return L.edge_residual(x, self.w[name], arith=arith, stride=ER[name][2])


@pytest.fixture(scope="module")
def rt():
    from m2s import runtime
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return runtime


@pytest.fixture(scope="module")
def state():
    return synth.synth_acoustic_state(STATE_SEED)


@pytest.fixture(scope="module")
def world(state):
    return World(state)


@pytest.fixture(scope="module")
def frames():
    cache = {}

    def get(key):
        if key not in cache:
            n, hw, seed, _ = SETS[key]
            cache[key] = torch.from_numpy(synth.synth_frames(1, n, hw=hw, seed=seed)[0]).to(DEV)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def bf16_fused(rt, state):
    return rt.AcousticEngine(state, dtype="bf16", device=DEV)


@pytest.fixture(scope="module")
def bf16_unfused(rt, state):
    with _env(**UNFUSED):
        return rt.AcousticEngine(state, dtype="bf16", device=DEV)


@pytest.fixture(scope="module")
def fp8(rt, state):
    return rt.AcousticEngine(state, dtype="fp8", device=DEV)


def _trips(key, tile_h, tile_w, div, tiles_per_round):
    """Tiles a persistent workgroup walks at most: the launch's tiles over the tiles of one round of its grid."""
    n, (H, W), _, _ = SETS[key]
    tiles = n * (H // div // tile_h) * (W // div // tile_w)
    return -(-tiles // tiles_per_round)


def _check(eng, world, fr, key, name, arith, kernels, absent=()):
    """One case (module docstring).  kernels: launch-log names of which one must have run (prefix match)."""
    from m2s import _native
    tap = {"stem": 0, "blocks.0.0": 1, "blocks.0.1": 2}.get(name) if name not in L.TAPS else L.TAPS[name]
    idx = list(SETS[key][3])
    if name in ("stem", "stem_b0"):
        x = fr[idx].cpu()
    else:
        a, b = eng.probe(fr, tap - 1), eng.probe(fr, tap - 1)
        assert torch.equal(a, b), f"{name}: the block's input differs between two runs"
        assert torch.equal(a, a.bfloat16().float()), f"{name}: the block's input is not bf16 values"
        x = a[idx].cpu()
    _native.prof_enable(True)
    try:
        got = eng.probe(fr, tap)
        torch.cuda.synchronize()
        names = {r["name"] for r in _native.prof_launches()}
    finally:
        _native.prof_enable(False)
    eng.check()
    assert any(n.startswith(kernels) for n in names), (name, kernels, sorted(names))
    assert not any(n.startswith(absent) for n in names), (name, absent, sorted(names))
    ref, budget = world.run(name, x, arith)
    g = got[idx].cpu().double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert torch.isfinite(g).all()
    ratio = (g - ref).abs() / budget
    worst = int(ratio.argmax())
    where = np.unravel_index(worst, tuple(ratio.shape))
    print(f"\n{name} {arith} [{', '.join(sorted(n for n in names if n.startswith(kernels)))}] set {key} "
          f"{tuple(fr.shape)}: worst |got - ref| / budget {float(ratio.max()):.3f} at image {idx[where[0]]} (c, y, x) = "
          f"{tuple(int(v) for v in where[1:])}, median budget / |ref| {float((budget / ref.abs()).median()):.4f}")
    assert float(ratio.max()) <= 1.0, (name, float(ratio.max()), where)
    return ref, got


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


# ------------------------------------------------------------------------------ bf16, fused kernels
def test_bf16_stem_b0(bf16_fused, world, frames):
    n, (H, W), _, idx = SETS["A"]
    strips, wgs = n * (W // 2 // 16), 3 * _cus()  # stem_b0.hip: three workgroups a CU, a strip = 2 tiles here
    assert strips > wgs and 25 in idx  # some workgroups take a second strip: four tiles
    _check(bf16_fused, world, frames("A"), "A", "stem_b0", "bf16", ("stem_b0_kernel<16, 0>",))


def test_bf16_ers2_fused_blocks_1_0(bf16_fused, world, frames):
    assert _trips("A", 8, 16, 4, 2 * _cus()) >= 3
    _check(bf16_fused, world, frames("A"), "A", "blocks.1.0", "bf16", ("ers2_fused_kernel<16, 64, 32, false>",))


@pytest.mark.parametrize("name", ["blocks.1.1", "blocks.1.2"])
def test_bf16_er_fused(bf16_fused, world, frames, name):
    assert _trips("B", 16, 16, 4, _cus()) >= 3
    _check(bf16_fused, world, frames("B"), "B", name, "bf16", ("er_fused_kernel",))


def test_bf16_ers2_fused_blocks_2_0(bf16_fused, world, frames):
    assert _trips("C", 8, 16, 8, _cus()) >= 3
    _check(bf16_fused, world, frames("C"), "C", "blocks.2.0", "bf16", ("ers2_fused_kernel<32, 128, 64, false>",))


@pytest.mark.parametrize("name", ["blocks.2.1", "blocks.2.2"])
def test_bf16_er2_fused(bf16_fused, world, frames, name):
    assert _trips("C", 16, 16, 8, _cus()) >= 3
    _check(bf16_fused, world, frames("C"), "C", name, "bf16", ("er2_fused_kernel",))


# ------------------------------------------------------------------------------ bf16, unfused sequence
@pytest.mark.parametrize("key", ["D", "B"])
def test_bf16_unfused_sequence(bf16_unfused, world, frames, key):
    """M2S_STEM_FUSED = M2S_ER_FUSED = M2S_ER_S2_FUSED = 0: stem32_kernel, then every block as conv_gemm / conv_halo
    launches, which round where the fused kernels do (oracle/lowprec.py edge_residual).  67 x 101: TF-SAME bottom /
    right pads (stem 34 x 51, blocks.1 17 x 26, blocks.2 9 x 13) and partial tiles everywhere."""
    fr = frames(key)
    _check(bf16_unfused, world, fr, key, "stem", "bf16", ("stem32_kernel",), FUSED_NAMES)
    for name in ("blocks.0.0", "blocks.0.1") + tuple(ER):
        _check(bf16_unfused, world, fr, key, name, "bf16", ("conv_gemm_kernel", "conv_halo_kernel"), FUSED_NAMES)


# ------------------------------------------------------------------------------ fp8 engine
@pytest.mark.parametrize("name", ["blocks.1.1", "blocks.1.2"])
def test_fp8_er8_fused(fp8, world, frames, name):
    assert _trips("A", 8, 16, 4, 2 * _cus()) >= 3  # a workgroup's two halves take a tile each per round
    _check(fp8, world, frames("A"), "A", name, "e4m3", ("er8_fused_kernel",))


@pytest.mark.parametrize("name", ["blocks.2.1", "blocks.2.2"])
def test_fp8_er8w_fused(fp8, world, frames, name):
    assert _trips("C", 16, 16, 8, _cus()) >= 3
    _check(fp8, world, frames("C"), "C", name, "e4m3", ("er8w_fused_kernel<",))
