"""Frame identification on gain-one weights for every CNN path.  GPU box only.

Under ``synth_acoustic_state`` two different frames' activations have cosine >= 0.999 from blocks.4 on, so the
bf16 / fp8 bars of the other test files pass a kernel that writes another frame's result: another image of the
8-image SE group, the other image of an ir_group G = 2 workgroup, a stale ring slot of se_ws / ir_ws, the previous
pass's row.  Here the weights are ``distinct.calibrated_acoustic_state`` (frames >= 0.49 of their norm apart at
every tap, test_distinct_cpu.py) and the question is asked directly: ``identification_ratio`` = the worst, over
frames, of (distance to the frame's own oracle row) / (distance to the nearest other frame's oracle row).

Bars: fp32, bf16x3, bf16 <= 1/2 (a kernel at the bf16 bar of cos 0.999 = 0.045 of the norm sits near 0.1 at a
separation of 0.49; a wrong frame is >= 1); fp8 < 1, strict identification.  fp32 keeps rel <= 1e-4.  fp32, bf16x3
and bf16 are also held to the suite's bf16 bar, cos >= 0.999 against the oracle, for every frame on its own: the
ratio does not see a frame that is the right one but carries its neighbour's SqueezeExcite gate (ratio 0.05-0.18),
this does on these weights (cos 0.9955-0.9982, test_distinct_cpu.py).  Every case prints its worst ratio, cosine
and tap (pytest -s).  References: the fp32 CPU oracle, once per input (distinct.reference).
"""
import numpy as np
import pytest
import torch

import distinct as D  # tests/distinct.py
from m2s import _native, runtime

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POOLED = 29  # index of the pooled features in distinct.reference()
ALL = tuple(range(30))
COS_MIN = 0.999  # the suite's bf16 bar against the oracle (test_gpu_parity.py), here per frame


def _holds(dtype, ratio):
    return ratio < 1.0 if dtype == "fp8" else ratio <= 0.5


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.fixture(scope="module")
def state():
    return D.calibrated_acoustic_state(D.SEED)


@pytest.fixture(scope="module")
def engines(state):
    """Engines with the environment's default switches, one per (dtype, chunk)."""
    cache = {}

    def get(dtype, **kw):
        key = (dtype, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = runtime.AcousticEngine(state, dtype=dtype, device=DEV, **kw)
        return cache[key]
    return get


def _x(name):
    fr = D.frames(name)
    return torch.from_numpy(fr.reshape((-1,) + fr.shape[2:])).to(DEV)


def _outputs(eng, x, taps):
    """{tap: numpy} for the probe taps and, under POOLED, effnet()'s features."""
    out = {}
    for i in taps:
        got = eng.effnet(x) if i == POOLED else eng.probe(x, i)
        out[i] = got.float().cpu().numpy()
    eng.check()
    return out


def _check(dtype, got, ref, what):
    """Outputs {tap: numpy} against ``ref`` ({tap: numpy} or distinct.reference's list): shapes, the ratio bar at
    every tap, and for fp32 / bf16x3 / bf16 the per-frame cosine bar.  Prints the worst of each."""
    ratio, cos = {}, {}
    for i, g in got.items():
        assert g.shape == ref[i].shape, (i, g.shape, ref[i].shape)
        ratio[i] = D.identification_ratio(g, ref[i])
        cos[i] = float(D.frame_cosines(g, ref[i]).min())
    name = lambda i: "pooled" if i == POOLED else f"tap {i}"  # noqa: E731
    taps = [i for i in got if i != POOLED] or list(got)
    wr, wc = max(taps, key=ratio.get), min(cos, key=cos.get)
    print(f"{what}: worst tap ratio {ratio[wr]:.4f} at {name(wr)}" +
          (f", pooled ratio {ratio[POOLED]:.4f}" if POOLED in got else "") +
          f", worst per-frame cos {cos[wc]:.6f} at {name(wc)}")
    bad = {name(i): v for i, v in ratio.items() if not _holds(dtype, v)}
    assert not bad, f"{what}: ratio over the {dtype} bar at {bad}"
    if dtype != "fp8":
        bad = {name(i): v for i, v in cos.items() if v < COS_MIN}
        assert not bad, f"{what}: per-frame cosine under {COS_MIN} at {bad}"


# ---------------------------------------------------------------------------------------------- every block
@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_67x101", "blocks_256x256"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp8"])
def test_every_block_identifies_its_frame(engines, dtype, name):
    """All 29 taps and the pooled features, 9 frames (a full 8-image SE group and a partial one), at 96 x 80,
    67 x 101 (TF-SAME pads, partial tiles) and 256 x 256 (the sizes the se_ws / e4m3 kernels have forms for)."""
    ref = D.reference(name)
    got = _outputs(engines(dtype), _x(name), ALL)
    rel = max(_rel(got[i], ref[i]) for i in ALL)
    print(f"\n{dtype} {name}: worst rel {rel:.3e}")
    _check(dtype, got, ref, f"{dtype} {name}")
    if dtype == "fp32":
        assert rel <= 1e-4


# -------------------------------------------------------------------------------- bf16 fused against unfused
FUSED = [("M2S_STEM_FUSED", (2, 3, 6, 28)), ("M2S_SE_FUSED", (9, 14, 20, 28)), ("M2S_IR_FUSED", (9, 10, 18, 19, 28)),
         ("M2S_ER_FUSED", (3, 4, 5, 6, 7, 8, 28)), ("M2S_IR_S2BAND", (9, 10))]


def _pair(state, monkeypatch, dtype, env, **kw):
    monkeypatch.setenv(env, "1")
    on = runtime.AcousticEngine(state, dtype=dtype, device=DEV, **kw)
    monkeypatch.setenv(env, "0")
    off = runtime.AcousticEngine(state, dtype=dtype, device=DEV, **kw)
    return on, off


@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_67x101"])
@pytest.mark.parametrize("env,taps", FUSED, ids=[f[0] for f in FUSED])
def test_bf16_fused_kernels_identify_their_frame(state, monkeypatch, env, taps, name):
    """Each fused bf16 kernel (switch = 1) against the oracle, and against the launches it replaces (switch = 0)
    with their output as the reference, at the taps test_gpu_parity.py lists for the switch plus the pooled
    features."""
    ref, x = D.reference(name), _x(name)
    on, off = _pair(state, monkeypatch, "bf16", env)
    taps = tuple(taps) + (POOLED,)
    a, b = _outputs(on, x, taps), _outputs(off, x, taps)
    print()
    _check("bf16", a, ref, f"{env}=1 vs oracle {name}")
    _check("bf16", b, ref, f"{env}=0 vs oracle {name}")
    _check("bf16", a, b, f"{env}=1 vs =0 {name}")


# ------------------------------------------------------------------------------------------------ fp8 switches
F8 = [("M2S_F8_EXPAND", (10, 13, 18, 20, 28)), ("M2S_F8_ER", (4, 5, 7, 8, 18, 28)), ("M2S_F8_S2", (9, 10, 19, 20, 28)),
      ("M2S_SE_WS", (13, 18, 20, 28)), ("M2S_ER8_X8", (4, 5, 8)), ("M2S_SE_Y8", (10, 12, 14, 18, 20, 28))]


SAME_ARITHMETIC = ("M2S_SE_WS", "M2S_ER8_X8", "M2S_SE_Y8")


@pytest.mark.parametrize("env,taps", F8, ids=[f[0] for f in F8])
def test_fp8_switches_identify_their_frame(state, monkeypatch, env, taps):
    """Each e4m3 path of the fp8 engine on and off, 5 frames at 256 x 256 (the 8 x 8 stage's two-image tiles, the
    last one half empty): both against the oracle, and on against off, at the taps test_gpu_fp8.py lists."""
    name = "tile_256x256"
    ref, x = D.reference(name), _x(name)
    on, off = _pair(state, monkeypatch, "fp8", env)
    taps = tuple(taps) + (POOLED,)
    a, b = _outputs(on, x, taps), _outputs(off, x, taps)
    print()
    _check("fp8", a, ref, f"{env}=1 vs oracle")
    _check("fp8", b, ref, f"{env}=0 vs oracle")
    # the two forms of these three run the same e4m3 operands through the same MFMAs (test_gpu_fp8.py holds them to
    # rel <= 1e-3 or equal bits), so on against off carries no e4m3 noise and takes the tight bars: the one place a
    # neighbour's SE gate inside one fp8-only kernel shows (cos ~0.997 against an oracle-side noise of ~0.98)
    _check("bf16" if env in SAME_ARITHMETIC else "fp8", a, b, f"{env}=1 vs =0")


def test_fp8_two_images_per_workgroup(engines):
    """256 x 512, 3 frames: the 8 x 16 maps of blocks.5 put two images in one e4m3-output ir_pwdw workgroup
    (ir_group G = 2), the second workgroup half empty.  Every tap and the pooled features."""
    name = "g2_256x512"
    print()
    _check("fp8", _outputs(engines("fp8"), _x(name), ALL), D.reference(name), f"fp8 {name}")


# ------------------------------------------------------------------------------------------ persistent kernels
WS_TAPS = (10, 12, 13, 18, 19, 20, 24, 28, POOLED)


@pytest.mark.parametrize("dtype,name", [("bf16x3", "ws_256x256"), ("fp8", "ws_256x256"), ("bf16x3", "ws_128x128")])
def test_persistent_kernels_identify_their_frame(state, monkeypatch, dtype, name):
    """ir_ws / se_ws at any pass size (M2S_IRWS_MIN=0, M2S_SEWS_MIN=0): 37 frames at 256 x 256, and 263 at
    128 x 128 = more images than workgroups, where a stale ring slot or a wrong tile counter would hand a frame
    another's rows.  The launch log must name the kernels: ir_ws only exists in the split engine, se_ws not at
    128 x 128 (se_ws_supported)."""
    monkeypatch.setenv("M2S_IRWS_MIN", "0")
    monkeypatch.setenv("M2S_SEWS_MIN", "0")
    eng = runtime.AcousticEngine(state, dtype=dtype, device=DEV)
    ref, x = D.reference(name), _x(name)
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        got = _outputs(eng, x, WS_TAPS)
        torch.cuda.synchronize()
        names = {r["name"] for r in _native.prof_launches()}
    finally:
        _native.prof_enable(False)
    if name == "ws_256x256":
        assert any(n.startswith("se_ws") for n in names), sorted(names)
    if dtype == "bf16x3":
        assert any(n.startswith("ir_ws_kernel") for n in names), sorted(names)
    print(f"\n{dtype} {name} persistent: worst rel {max(_rel(got[i], ref[i]) for i in WS_TAPS):.3e}")
    _check(dtype, got, ref, f"{dtype} {name} persistent")


# ------------------------------------------------------------------------------------------------------ passes
@pytest.mark.parametrize("name", ["blocks_96x80", "blocks_256x256"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_passes_identify_their_frame(engines, dtype, name):
    """chunk = 4, 9 frames: passes of 4, 4 and 1, each over the workspace the pass before it used."""
    print()
    _check(dtype, _outputs(engines(dtype, chunk=4), _x(name), ALL), D.reference(name), f"{dtype} chunk=4 {name}")


# ------------------------------------------------------------------------------------------------------- clips
@pytest.mark.parametrize("dtype,name", [("bf16x3", "clips_96x80"), ("bf16", "clips_96x80"), ("fp8", "clips_96x80"),
                                        ("fp8", "clips_256x256")])
def test_forward_rows_identify_their_frame(engines, dtype, name):
    """forward on 3 clips x 5 frames: the ratio over all 15 mel_norm rows, so a row of another clip counts.  At
    96 x 80 the fp8 engine has no e4m3 form for any block and runs the bf16 kernels; 256 x 256 is its own path."""
    ref = D.reference_mel(name)
    eng = engines(dtype)
    mn = eng.forward(torch.from_numpy(D.frames(name)).to(DEV))
    eng.check()
    assert mn.shape == ref.shape
    r = D.identification_ratio(mn.reshape(15, -1), ref.reshape(15, -1))
    print(f"\n{dtype} forward {name}: mel_norm ratio {r:.4f}, max|d| {np.abs(mn.cpu().numpy() - ref).max():.3e}")
    assert _holds(dtype, r), r


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_forward_ragged_rows_identify_their_frame(engines, dtype):
    """forward_ragged with lengths [5, 2, 4] against the oracle run clip by clip: the ratio per clip, and over all
    11 rows (a row of another clip)."""
    ref = D.reference_mel("ragged_96x80")
    eng = engines(dtype)
    mn = eng.forward_ragged(torch.from_numpy(D.frames("ragged_96x80")[0]).to(DEV), D.RAGGED_LENS)
    eng.check()
    assert mn.shape == (sum(D.RAGGED_LENS), 64)
    got = [g.cpu().numpy() for g in runtime.split_packed(mn, D.RAGGED_LENS)]
    rs = [D.identification_ratio(g, r) for g, r in zip(got, ref)]
    r_all = D.identification_ratio(np.concatenate(got), np.concatenate(ref))
    print(f"\n{dtype} forward_ragged {D.RAGGED_LENS}: per-clip ratio {' '.join(f'{r:.4f}' for r in rs)}, all rows {r_all:.4f}")
    assert all(_holds(dtype, r) for r in rs + [r_all]), (rs, r_all)
