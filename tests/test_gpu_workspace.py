"""The workspace contract of include/m2s.h, checked through the C ABI the way a C integrator calls it.

Every other GPU test reaches the engines through torch.ops.m2s.*, where the workspace and the outputs come from
torch's caching allocator: stale but finite bytes of the previous call, sizes rounded up.  Here every buffer is carved
out of one guarded arena (tests/ws_harness.py): the workspace has exactly the bytes the *_workspace_bytes query
reports, the outputs exactly their documented size, 1 MiB of guard on both sides of each, and the workspace is
filled with zeros, NaN bit patterns, random bytes, or what a larger call of the same engine left behind.  A call
must return M2S_OK, leave every guard byte alone, write every output element, and give the same bits under every
fill; in fp32 / bf16x3 the NaN-filled run must also meet the parity bar of the entry point against the CPU oracle
(test_gpu_parity.py / test_gpu_bf16x3.py: 1e-4; BiLSTM y 2e-5 / head 5e-5 in fp32, 1e-4 / 5e-4 split).  A
workspace 256 bytes short is refused with M2S_E_ARG, writes nothing outside its buffers, and leaves the engine
giving the same bits.  That last check applies where the size query belongs to the entry point itself;
m2s_effnet_probe, m2s_bilstm_summerge(_ragged) and m2s_bilstm_train_forward use a part of what the query of the
enclosing call reports (include/m2s.h), so 256 bytes less is still enough for them.

Shapes are the smallest that reach each padded path (half-empty 8 x 8 tiles, odd geometry, short second pass,
every BiLSTM recurrence kernel, one-frame clips), not the workload.  GPU box only.
"""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

import ws_harness as H  # tests/ws_harness.py (pytest puts this directory on sys.path)
from m2s import _native, ops, synth
from m2s.config import HIFIGAN_H
from oracle import acoustic, effnet, hifigan, pipeline

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DTYPES = ["fp32", "bf16", "bf16x3", "fp8"]
EXACT = ("fp32", "bf16x3")  # engines held to the fp32 parity bars
SEED = 2
E2E_TOL = {"mel_norm": 1e-4, "mel_db": 2e-3, "mel_log": 5e-4, "wav": 1e-4}  # test_gpu_bf16x3.py end to end
# where a call turns out nondeterministic, its fills are compared at the engine's parity bar (bf16 / fp8: the bf16 bars
# of test_gpu_parity.py's end-to-end test: mel_norm 5e-2, hence mel_db = mel_norm * std with synth_scaler's std <= 15
# and mel_log = mel_db * ln(10) / 10; its 20 dB waveform SNR is 0.1 of the tanh output's unit amplitude).  No case
# needs it so far: every call has been bit-reproducible.
LOOSE_TOL = {"mel_norm": 5e-2, "mel_db": 5e-2 * 15, "mel_log": 5e-2 * 15 * 0.2303, "wav": 0.1}
NONDETERMINISTIC = []


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _sync():
    torch.cuda.synchronize(DEV)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    return _native.lib()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _hop(h):
    return int(np.prod(h["upsample_rates"]))


def _r2_h():
    g = np.load(os.path.join(GOLD, "generator.npz"), allow_pickle=False)
    return json.loads(bytes(g["r2_h"]).decode())


VOC_H = {"r1": HIFIGAN_H, "r2": _r2_h()}


# ------------------------------------------------------------------------------------------ shared state
@pytest.fixture(scope="module")
def ac_sd():
    return synth.synth_acoustic_state(SEED)


@pytest.fixture(scope="module")
def gen_sd():
    return {k: synth.synth_generator_state(SEED, h) for k, h in VOC_H.items()}


@pytest.fixture(scope="module")
def shared():
    """Engines (one per dtype / setting), oracle results (computed once, never modified) and, per engine, the
    workspace image its largest call so far left behind (the "stale" fill of the smaller calls after it)."""
    state = {"eng": {}, "ref": {}, "stale": {}}
    yield state
    for d in state.values():
        d.clear()
    torch.cuda.empty_cache()


def _acoustic(shared, ac_sd, dtype, chunk=None, persistent=None):
    """persistent: a monkeypatch -> the engine is created under M2S_IRWS_MIN=0 / M2S_SEWS_MIN=0 (read at creation)."""
    from m2s import runtime
    key = ("ac", dtype, chunk, persistent is not None)
    if key not in shared["eng"]:
        if persistent is not None:
            persistent.setenv("M2S_IRWS_MIN", "0")
            persistent.setenv("M2S_SEWS_MIN", "0")
        kw = {} if chunk is None else {"chunk": chunk}
        shared["eng"][key] = runtime.AcousticEngine(ac_sd, dtype=dtype, device=DEV, **kw)
    return key, shared["eng"][key]


def _vocoder(shared, gen_sd, dtype, rb="r1"):
    from m2s import runtime
    key = ("voc", dtype, rb)
    if key not in shared["eng"]:
        shared["eng"][key] = runtime.VocoderEngine(gen_sd[rb], VOC_H[rb], dtype=dtype, device=DEV)
    return key, shared["eng"][key]


def _ref(shared, key, fn):
    if key not in shared["ref"]:
        with torch.no_grad():
            shared["ref"][key] = fn()
    return shared["ref"][key]


def _ac_status(eng):
    return lambda: _lib().m2s_acoustic_status(eng._h)


def _run(shared, key, what, arena, call, status=lambda: H.M2S_OK, tol=None, undersized=True):
    """The fill checks and (where the size query is the entry point's own) the undersized-workspace check."""
    (ws,) = arena.names("ws")
    stale = shared["stale"].get(key)
    if stale is not None and stale.numel() <= arena.nbytes(ws):
        stale = None  # only a larger call's leftovers
    rep = H.check_contract(arena, lambda a: call(a, a.nbytes(ws)), sync=_sync, status=status, stale=stale, tol=tol,
                           what=what)
    print(f"{what}: ws {arena.nbytes(ws)} B, fills {sorted(rep.outs)}, deterministic {rep.deterministic}"
          + (f", fill differences {rep.max_fill_diff}" if rep.max_fill_diff else ""))
    if not rep.deterministic:
        NONDETERMINISTIC.append(what)
        warnings.warn(f"{what}: two zero-fill runs differ ({rep.max_fill_diff}); fills compared at {tol}")
    if undersized:
        H.check_undersized(arena, call, rep.outs["zero"], sync=_sync, status=status, exact=rep.deterministic, what=what)
    if key not in shared["stale"] or arena.nbytes(ws) > shared["stale"][key].numel():
        shared["stale"][key] = arena.workspace_image()
    return rep


def _close(what, got, ref, atol):
    got, ref = np.asarray(got.cpu() if hasattr(got, "cpu") else got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: max |d| vs reference = {err:.3e} (bar {atol:g})")
    assert err <= atol, f"{what}: max |d| = {err:.3e} > {atol:g}"


# ------------------------------------------------------------------------------------------ m2s_acoustic_forward
def _frames(B, T, H_, W_):
    return synth.synth_frames(B, T, hw=(H_, W_), seed=1000 + B * 100 + T * 10 + H_ % 7)


def _acoustic_case(shared, ac_sd, key, eng, dtype, shape, what):
    B, T, H_, W_ = shape
    fr = _frames(*shape)
    L = _lib()
    nws = L.m2s_acoustic_workspace_bytes(eng._h, B, T, H_, W_)
    assert nws > 0 and nws % 256 == 0
    arena = H.Arena(DEV, [("frames", "in", fr), ("mel_norm", "out", (B, T, 64)), ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_acoustic_forward(eng._h, a.ptr("frames"), B, T, H_, W_, a.ptr("mel_norm"), a.ptr("ws"), n, _stream())

    tol = {"mel_norm": 1e-4} if dtype in EXACT else LOOSE_TOL
    rep = _run(shared, key, what, arena, call, _ac_status(eng), tol)
    if dtype in EXACT:
        ref = _ref(shared, ("acoustic", shape), lambda: pipeline.acoustic_forward(_t(ac_sd), fr).numpy())
        _close(what, rep.outs["nan"]["mel_norm"], ref, 1e-4)
    return rep


# largest first: the later cases of an engine also run on what this one left in its workspace
AC_SHAPES = [(8, 4, 256, 256), (1, 5, 256, 256), (2, 3, 67, 101)]


@pytest.mark.parametrize("shape", AC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_acoustic_forward(shared, ac_sd, dtype, shape):
    """8x4: the small-pass plan, split K, the B > 4 recurrence; 1x5: a half-empty last two-image 8 x 8 tile; 2x3 at
    67 x 101: odd geometry, TF-SAME pads, vector-store tails."""
    key, eng = _acoustic(shared, ac_sd, dtype)
    _acoustic_case(shared, ac_sd, key, eng, dtype, shape, f"acoustic_forward {dtype} {shape}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_acoustic_forward_short_second_pass(shared, ac_sd, dtype):
    """chunk = 4, 7 frames: a 3-frame pass after a 4-frame one, so the first pass's rows lie behind the second's."""
    key, eng = _acoustic(shared, ac_sd, dtype, chunk=4)
    _acoustic_case(shared, ac_sd, key, eng, dtype, (1, 7, 96, 80), f"acoustic_forward chunk=4 {dtype} (1, 7, 96, 80)")


@pytest.mark.parametrize("shape", [(1, 5, 256, 256), (1, 3, 128, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_persistent_kernels_at_small_n(shared, ac_sd, monkeypatch, dtype, shape):
    """The headline persistent kernels (ir_ws, se_ws) on passes far smaller than their tiles: M2S_IRWS_MIN=0 and
    M2S_SEWS_MIN=0 at engine creation, as test_ir_ws_matches_grid_kernel sets them.  The launch log must name every
    one that has a form for the case: ir_ws exists only in the split engine (Acoustic::effnet_t: the fp8 engine's IR
    front half is ir_pwdw at any size), and se_ws takes 16 x 16 maps, or 8 x 8 maps with more than 128 output
    channels (se_ws_supported), which 128 x 128 frames never produce - there the SE GEMM is conv_gemm whatever the
    setting, in both engines."""
    key, eng = _acoustic(shared, ac_sd, dtype, persistent=monkeypatch)
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        _acoustic_case(shared, ac_sd, key, eng, dtype, shape, f"acoustic_forward persistent {dtype} {shape}")
        _sync()
        names = {r["name"] for r in _native.prof_launches()}
    finally:
        _native.prof_enable(False)
    if shape[2:] == (256, 256):
        assert any(n.startswith("se_ws") for n in names), sorted(names)
    if dtype == "bf16x3":
        assert any(n.startswith("ir_ws") for n in names), sorted(names)


# ------------------------------------------------------------------------------------------ m2s_effnet_probe
def _probe_dims(n_blocks, H_, W_):
    oh, ow = H_, W_
    for s in ops._FEAT_STRIDE[:n_blocks + 1]:
        if s == 2:
            oh, ow = (oh + 1) // 2, (ow + 1) // 2
    return oh, ow, ops._FEAT_CH[n_blocks]


@pytest.mark.parametrize("n_blocks", [28, 0, 9, 19])
def test_effnet_probe(shared, ac_sd, n_blocks):
    """The dense (N, OH, OW, C) tap at its exact size; the workspace is the (N, 1, H, W) acoustic query's, of which
    the probe uses the CNN part."""
    N, H_, W_ = 3, 67, 101
    key, eng = _acoustic(shared, ac_sd, "bf16x3")
    fr = synth.synth_frames(1, N, hw=(H_, W_), seed=77)[0]
    oh, ow, oc = _probe_dims(n_blocks, H_, W_)
    L = _lib()
    nws = L.m2s_acoustic_workspace_bytes(eng._h, N, 1, H_, W_)
    arena = H.Arena(DEV, [("frames", "in", fr), ("tap", "out", (N, oh, ow, oc)), ("ws", "ws", nws)])
    dims = [C.c_int(0) for _ in range(3)]

    def call(a, n):
        return L.m2s_effnet_probe(eng._h, a.ptr("frames"), N, H_, W_, n_blocks, a.ptr("tap"), C.byref(dims[0]),
                                  C.byref(dims[1]), C.byref(dims[2]), a.ptr("ws"), n, _stream())

    what = f"effnet_probe bf16x3 n_blocks={n_blocks}"
    rep = _run(shared, key, what, arena, call, _ac_status(eng), None, undersized=False)
    assert [d.value for d in dims] == [oh, ow, oc]

    def taps():
        out = []
        effnet.effnet_features(_t(ac_sd), torch.from_numpy(fr), taps=out)
        return [x.numpy() for x in out]

    ref = _ref(shared, "probe_taps", taps)[n_blocks]
    got = rep.outs["nan"]["tap"].permute(0, 3, 1, 2).cpu().numpy()
    print(f"{what}: rel err vs oracle {_rel(got, ref):.3e}")
    assert got.shape == ref.shape and _rel(got, ref) <= 1e-4, _rel(got, ref)


# ------------------------------------------------------------------------------------------ m2s_bilstm_summerge
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "y_null"])
@pytest.mark.parametrize("B,T", [(5, 17), (33, 2), (17, 3), (1, 30)])
@pytest.mark.parametrize("dtype", EXACT)
def test_bilstm_summerge(shared, ac_sd, dtype, B, T, with_y):
    """<= 4, <= 16, > 16 and > 32 sequences: every recurrence kernel; once with both outputs, once with y = NULL."""
    key, eng = _acoustic(shared, ac_sd, dtype)
    x = np.random.default_rng(B * 13 + T).normal(0, 0.5, (B, T, 208)).astype(np.float32)
    L = _lib()
    nws = L.m2s_acoustic_workspace_bytes(eng._h, B, T, 64, 64)  # what torch.ops.m2s.bilstm_summerge passes
    specs = [("feats", "in", x)] + ([("y", "out", (B, T, 640))] if with_y else []) + [("mel_norm", "out", (B, T, 64)),
                                                                                     ("ws", "ws", nws)]
    arena = H.Arena(DEV, specs)

    def call(a, n):
        return L.m2s_bilstm_summerge(eng._h, a.ptr("feats"), B, T, a.ptr("y" if with_y else None), a.ptr("mel_norm"),
                                     a.ptr("ws"), n, _stream())

    what = f"bilstm_summerge {dtype} {B}x{T}{'' if with_y else ' y=NULL'}"
    bar = {"y": 2e-5, "mel_norm": 5e-5} if dtype == "fp32" else {"y": 1e-4, "mel_norm": 5e-4}
    rep = _run(shared, key, what, arena, call, _ac_status(eng), bar, undersized=False)

    def ref():
        sd = _t(ac_sd)
        y = acoustic.bilstm_summerge(sd, torch.from_numpy(x))
        return {"y": y.numpy(), "mel_norm": acoustic.head(sd, y).numpy()}

    r = _ref(shared, ("bilstm", B, T), ref)
    for n, t in rep.outs["nan"].items():
        _close(f"{what} {n}", t, r[n], bar[n])


# ------------------------------------------------------------------------------------------ m2s_vocoder_forward
@pytest.mark.parametrize("B,T,layout", [(2, 64, 0), (3, 17, 0), (3, 17, 1), (1, 1, 0)])
@pytest.mark.parametrize("rb", ["r1", "r2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vocoder_forward(shared, gen_sd, dtype, rb, B, T, layout):
    key, voc = _vocoder(shared, gen_sd, dtype, rb)
    h = VOC_H[rb]
    mel = synth.synth_mel_log(B, h["num_mels"], T, seed=B * 100 + T)  # (B, num_mels, T)
    x = mel if layout == 0 else np.ascontiguousarray(mel.transpose(0, 2, 1))
    L = _lib()
    nws = L.m2s_vocoder_workspace_bytes(voc._h, B, T)
    arena = H.Arena(DEV, [("mel", "in", x), ("wav", "out", (B, T * _hop(h))), ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_vocoder_forward(voc._h, a.ptr("mel"), layout, B, T, a.ptr("wav"), a.ptr("ws"), n, _stream())

    what = f"vocoder_forward {dtype} {rb} {B}x{T} layout {layout}"
    rep = _run(shared, key, what, arena, call, tol={"wav": 1e-4} if dtype in EXACT else LOOSE_TOL)
    if dtype in EXACT:
        ref = _ref(shared, ("voc", rb, B, T),
                   lambda: hifigan.generator(_t(gen_sd[rb]), h, torch.from_numpy(mel))[:, 0].numpy())
        _close(what, rep.outs["nan"]["wav"], ref, 1e-4)


# ------------------------------------------------------------------------------------------ m2s_vocoder_probe
@pytest.mark.parametrize("tap", [0, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vocoder_probe(shared, gen_sd, dtype, tap):
    """The dense (B, L, C) tap at its exact size on the forward call's workspace (the probe lays out the same buffers,
    so 256 bytes less is refused): conv_pre's output, stage 1's upsampler output and the last MRF output.  bf16 / fp8:
    every value is a bf16 value; fp32 / bf16x3: the oracle's tap at 1e-4 of its scale (LeakyReLU applied to the
    oracle's where the engine reports that it holds the tensor so)."""
    B, T = 3, 17
    key, voc = _vocoder(shared, gen_sd, dtype)
    h = VOC_H["r1"]
    mel = synth.synth_mel_log(B, h["num_mels"], T, seed=B * 100 + T)
    Cc, scale = voc.tap_shape(tap)
    L = _lib()
    nws = L.m2s_vocoder_workspace_bytes(voc._h, B, T)
    arena = H.Arena(DEV, [("mel", "in", mel), ("tap", "out", (B, T * scale, Cc)), ("ws", "ws", nws)])
    dims = [C.c_int(-1) for _ in range(3)]

    def call(a, n):
        return L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, T, tap, a.ptr("tap"), C.byref(dims[0]), C.byref(dims[1]),
                                   C.byref(dims[2]), a.ptr("ws"), n, _stream())

    what = f"vocoder_probe {dtype} tap {tap} {B}x{T}"
    rep = _run(shared, key, what, arena, call, tol={"tap": 1e-4} if dtype in EXACT else None)
    assert [d.value for d in dims[:2]] == [T * scale, Cc] and dims[2].value in (0, 1)
    info = [C.c_int(-1) for _ in range(3)]
    assert L.m2s_vocoder_tap_info(voc._h, tap, T, C.byref(info[0]), C.byref(info[1]), C.byref(info[2])) == H.M2S_OK
    assert [d.value for d in info] == [d.value for d in dims]
    assert dims[2].value == 0 or dtype == "bf16x3"  # only the split engine's batched stages hand lrelu(x) on
    got = rep.outs["nan"]["tap"].permute(0, 2, 1).cpu()
    if dtype not in EXACT:
        assert torch.equal(got, got.bfloat16().float()), f"{what}: not bf16 values"
        return

    def taps():
        out = []
        hifigan.generator(_t(gen_sd["r1"]), h, torch.from_numpy(mel), taps=out)
        return [x.numpy() for x in out]

    ref = _ref(shared, ("voc_taps", B, T), taps)[tap]
    if dims[2].value:
        ref = np.where(ref > 0, ref, ref * np.float32(0.1))
    print(f"{what}: rel err vs oracle {_rel(got.numpy(), ref):.3e}")
    assert got.shape == ref.shape and _rel(got.numpy(), ref) <= 1e-4, _rel(got.numpy(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vocoder_probe_refusals(shared, gen_sd, dtype):
    """Argument errors are M2S_E_ARG before any launch: the output and the workspace keep their fill."""
    B, T = 1, 2
    key, voc = _vocoder(shared, gen_sd, dtype)
    h = VOC_H["r1"]
    mel = synth.synth_mel_log(B, h["num_mels"], T, seed=5)
    L = _lib()
    nws = L.m2s_vocoder_workspace_bytes(voc._h, B, T)
    arena = H.Arena(DEV, [("mel", "in", mel), ("tap", "out", (B, T, h["upsample_initial_channel"])), ("ws", "ws", nws)])
    n_up = len(h["upsample_rates"])
    calls = {
        "tap -1": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, T, -1, a.ptr("tap"), None, None, None,
                                                a.ptr("ws"), nws, _stream()),
        "tap past the last": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, T, 2 * n_up + 1, a.ptr("tap"), None,
                                                           None, None, a.ptr("ws"), nws, _stream()),
        "null out": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, T, 0, None, None, None, None, a.ptr("ws"),
                                                  nws, _stream()),
        "null mel": lambda a: L.m2s_vocoder_probe(voc._h, None, 0, B, T, 0, a.ptr("tap"), None, None, None, a.ptr("ws"),
                                                  nws, _stream()),
        "null ws": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, T, 0, a.ptr("tap"), None, None, None, None,
                                                 nws, _stream()),
        "layout 2": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 2, B, T, 0, a.ptr("tap"), None, None, None,
                                                  a.ptr("ws"), nws, _stream()),
        "T = 0": lambda a: L.m2s_vocoder_probe(voc._h, a.ptr("mel"), 0, B, 0, 0, a.ptr("tap"), None, None, None,
                                               a.ptr("ws"), nws, _stream()),
    }
    for name, call in calls.items():
        arena.prepare("nan")
        _sync()
        assert call(arena) == H.M2S_E_ARG, name
        _sync()
        bad = arena.violations(outputs_written=False)
        assert not bad, f"vocoder_probe {dtype} {name}: " + "; ".join(bad)
        assert bool((arena.workspace_image() == H.POISON).all()), f"{name}: the workspace was written"
        assert bool((arena.raw("tap") == H.POISON).all()), f"{name}: the output was written"


# ------------------------------------------------------------------------------------------ m2s_pipeline_forward
def _scaler_specs():
    mean, std = synth.synth_scaler()
    return mean, std, [("mean", "in", mean), ("std", "in", std)]


@pytest.mark.parametrize("mels", [True, False], ids=["mels", "mels_null"])
@pytest.mark.parametrize("shape", [(1, 5, 256, 256), (2, 3, 67, 101)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_pipeline_forward(shared, ac_sd, gen_sd, dtype, shape, mels):
    B, T, H_, W_ = shape
    _, ac = _acoustic(shared, ac_sd, dtype)
    _, voc = _vocoder(shared, gen_sd, dtype)
    key = ("pipe", dtype)
    fr = _frames(*shape)
    mean, std, sc = _scaler_specs()
    L = _lib()
    nws = L.m2s_pipeline_workspace_bytes(ac._h, voc._h, B, T, H_, W_)
    outs = [(n, "out", (B, T, 64)) for n in ("mel_norm", "mel_db", "mel_log")] if mels else []
    arena = H.Arena(DEV, [("frames", "in", fr)] + sc + outs + [("wav", "out", (B, T * voc.hop)), ("ws", "ws", nws)])
    p = (lambda a, n: a.ptr(n)) if mels else (lambda a, n: None)

    def call(a, n):
        return L.m2s_pipeline_forward(ac._h, voc._h, a.ptr("frames"), B, T, H_, W_, a.ptr("mean"), a.ptr("std"),
                                      p(a, "mel_norm"), p(a, "mel_db"), p(a, "mel_log"), a.ptr("wav"), a.ptr("ws"), n,
                                      _stream())

    what = f"pipeline_forward {dtype} {shape}{'' if mels else ' mel_*=NULL'}"
    rep = _run(shared, key, what, arena, call, _ac_status(ac), E2E_TOL if dtype in EXACT else LOOSE_TOL)
    if dtype in EXACT:
        ref = _ref(shared, ("e2e", shape), lambda: pipeline.e2e(_t(ac_sd), _t(gen_sd["r1"]), HIFIGAN_H, fr, mean, std))
        for n, t in rep.outs["nan"].items():
            _close(f"{what} {n}", t, ref[n], E2E_TOL[n])


# ------------------------------------------------------------------------------------------ ragged entry points
def _lens(lens):
    return (C.c_int * len(lens))(*lens)


def _per_clip(what, packed, lens, per, dense, atol):
    """Clip b of a packed output against the dense call on that clip alone (test_gpu_ragged.py's bars)."""
    off, packed = 0, packed.reshape(-1)
    assert packed.size == sum(lens) * per
    for b, n in enumerate(lens):
        _close(f"{what} clip {b} (len {n}) vs its dense call", packed[off * per:(off + n) * per],
               dense[b].reshape(-1).cpu().numpy(), atol)
        off += n


@pytest.mark.parametrize("dtype", EXACT)
def test_acoustic_forward_ragged(shared, ac_sd, dtype):
    lens, (H_, W_) = [5, 1, 3], (96, 80)
    key, eng = _acoustic(shared, ac_sd, dtype)
    clips = [synth.synth_frames(1, n, hw=(H_, W_), seed=100 + 17 * b)[0] for b, n in enumerate(lens)]
    L, cl, N = _lib(), _lens(lens), sum(lens)
    nws = L.m2s_acoustic_ragged_workspace_bytes(eng._h, cl, len(lens), H_, W_)
    arena = H.Arena(DEV, [("frames", "in", np.concatenate(clips)), ("mel_norm", "out", (N, 64)), ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_acoustic_forward_ragged(eng._h, a.ptr("frames"), cl, len(lens), N, H_, W_, a.ptr("mel_norm"),
                                             a.ptr("ws"), n, _stream())

    what = f"acoustic_forward_ragged {dtype} {lens}"
    rep = _run(shared, key, what, arena, call, _ac_status(eng), {"mel_norm": 1e-4})
    dense = [eng.forward(torch.from_numpy(c[None]).to(DEV))[0] for c in clips]
    _per_clip(what, rep.outs["nan"]["mel_norm"].cpu().numpy(), lens, 64, dense, 1e-4)


@pytest.mark.parametrize("dtype", EXACT)
def test_bilstm_summerge_ragged(shared, ac_sd, dtype):
    lens = [33, 1, 8]
    key, eng = _acoustic(shared, ac_sd, dtype)
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(n, 208, generator=g) for n in lens]
    L, cl, N = _lib(), _lens(lens), sum(lens)
    nws = L.m2s_acoustic_ragged_workspace_bytes(eng._h, cl, len(lens), 64, 64)  # as torch.ops.m2s passes it
    arena = H.Arena(DEV, [("feats", "in", torch.cat(feats)), ("y", "out", (N, 640)), ("mel_norm", "out", (N, 64)),
                          ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_bilstm_summerge_ragged(eng._h, a.ptr("feats"), cl, len(lens), N, a.ptr("y"), a.ptr("mel_norm"),
                                            a.ptr("ws"), n, _stream())

    what = f"bilstm_summerge_ragged {dtype} {lens}"
    rep = _run(shared, key, what, arena, call, _ac_status(eng), {"y": 1e-4, "mel_norm": 1e-4}, undersized=False)
    dense = [eng.bilstm(x[None].to(DEV)) for x in feats]
    _per_clip(f"{what} y", rep.outs["nan"]["y"].cpu().numpy(), lens, 640, [d[0] for d in dense], 1e-4)
    _per_clip(f"{what} mel_norm", rep.outs["nan"]["mel_norm"].cpu().numpy(), lens, 64, [d[1] for d in dense], 1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vocoder_forward_ragged(shared, gen_sd, dtype):
    """Every dtype: the ragged query counts the fp8 engine's sixth buffer and the split engine's per-resblock ones."""
    lens = [17, 1, 9]
    key, voc = _vocoder(shared, gen_sd, dtype)
    mels = [np.ascontiguousarray(synth.synth_mel_log(1, 64, n, seed=40 + 11 * b)[0].T) for b, n in enumerate(lens)]
    L, cl, N = _lib(), _lens(lens), sum(lens)
    nws = L.m2s_vocoder_ragged_workspace_bytes(voc._h, cl, len(lens))
    arena = H.Arena(DEV, [("mel", "in", np.concatenate(mels)), ("wav", "out", (N * voc.hop,)), ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_vocoder_forward_ragged(voc._h, a.ptr("mel"), cl, len(lens), N, a.ptr("wav"), a.ptr("ws"), n,
                                            _stream())

    what = f"vocoder_forward_ragged {dtype} {lens}"
    rep = _run(shared, key, what, arena, call, tol={"wav": 1e-4} if dtype in EXACT else LOOSE_TOL)
    if dtype in EXACT:
        dense = [voc.forward(torch.from_numpy(m[None]).to(DEV), layout=1) for m in mels]
        _per_clip(what, rep.outs["nan"]["wav"].cpu().numpy(), lens, voc.hop, dense, 1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pipeline_forward_ragged(shared, ac_sd, gen_sd, dtype):
    from m2s import runtime
    lens, (H_, W_) = [5, 1, 3], (96, 80)
    _, ac = _acoustic(shared, ac_sd, dtype)
    _, voc = _vocoder(shared, gen_sd, dtype)
    clips = [synth.synth_frames(1, n, hw=(H_, W_), seed=300 + 17 * b)[0] for b, n in enumerate(lens)]
    mean, std, sc = _scaler_specs()
    L, cl, N = _lib(), _lens(lens), sum(lens)
    nws = L.m2s_pipeline_ragged_workspace_bytes(ac._h, voc._h, cl, len(lens), H_, W_)
    arena = H.Arena(DEV, [("frames", "in", np.concatenate(clips))] + sc +
                    [(n, "out", (N, 64)) for n in ("mel_norm", "mel_db", "mel_log")] +
                    [("wav", "out", (N * voc.hop,)), ("ws", "ws", nws)])

    def call(a, n):
        return L.m2s_pipeline_forward_ragged(ac._h, voc._h, a.ptr("frames"), cl, len(lens), N, H_, W_, a.ptr("mean"),
                                             a.ptr("std"), a.ptr("mel_norm"), a.ptr("mel_db"), a.ptr("mel_log"),
                                             a.ptr("wav"), a.ptr("ws"), n, _stream())

    what = f"pipeline_forward_ragged {dtype} {lens}"
    rep = _run(shared, ("pipe", dtype), what, arena, call, _ac_status(ac), E2E_TOL if dtype in EXACT else LOOSE_TOL)
    if dtype not in EXACT:
        return
    pipe = runtime.Pipeline(ac, voc, mean, std)
    dense = [pipe.forward(torch.from_numpy(c[None]).to(DEV)) for c in clips]
    for n, atol in E2E_TOL.items():
        _per_clip(f"{what} {n}", rep.outs["nan"][n].cpu().numpy(), lens, voc.hop if n == "wav" else 64,
                  [d[n] for d in dense], atol)


def test_size_queries_return_zero_for_null_handles():
    """The dense size queries, like every other one (include/m2s.h): 0 for a null handle, and no engine is needed."""
    L = _lib()
    assert L.m2s_acoustic_workspace_bytes(None, 2, 3, 64, 64) == 0
    assert L.m2s_vocoder_workspace_bytes(None, 2, 3) == 0
    assert L.m2s_pipeline_workspace_bytes(None, None, 2, 3, 64, 64) == 0


# ------------------------------------------------------------------------------------------ Grad-CAM path
CAM_TAPS = ((16, 2, 2), (32, 4, 5), (56, 8, 8), (120, 16, 18), (208, 32, 28))  # channels, stride, oracle tap index


@pytest.mark.parametrize("hw", [(67, 101), (64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_cam_backbone(shared, ac_sd, hw):
    """Train-mode backbone: the five taps against oracle.effnet with train=True and every BatchNorm layer's batch
    statistics through the running-statistics update torch does with them (test_gpu_gradcam.py's references, 1e-4)."""
    from m2s import autograd
    key = ("cam",)
    if key not in shared["eng"]:
        shared["eng"][key] = autograd.CamEngine(ac_sd, DEV)
    cam = shared["eng"][key]
    N, (H_, W_) = 3, hw
    fr = synth.synth_frames(1, N, hw=hw, seed=21)[0]
    L = _lib()
    shapes = []
    for c, red, _ in CAM_TAPS:
        oh, ow, r = H_, W_, 1
        while r < red:
            oh, ow, r = (oh + 1) // 2, (ow + 1) // 2, r * 2
        shapes.append((N, c, oh, ow))
    nws = L.m2s_cam_workspace_bytes(cam._h, N, H_, W_)
    arena = H.Arena(DEV, [("frames", "in", fr)] + [(f"tap{i}", "out", s) for i, s in enumerate(shapes)] +
                    [("bn_stats", "out", (ops.CAM_BN_STATS,)), ("ws", "ws", nws)])

    def call(a, n):
        taps = (C.c_void_p * 5)(*[a.ptr(f"tap{i}") for i in range(5)])
        return L.m2s_cam_backbone(cam._h, a.ptr("frames"), N, H_, W_, taps, a.ptr("bn_stats"), a.ptr("ws"), n, _stream())

    what = f"cam_backbone N={N} {hw}"
    tol = {f"tap{i}": 1e-4 for i in range(5)}
    tol["bn_stats"] = 1e-4
    rep = _run(shared, key, what, arena, call, tol=tol)
    sd = {k: v.clone() for k, v in _t(ac_sd).items()}
    ref = []
    with torch.no_grad():
        effnet.effnet_features(sd, torch.from_numpy(fr)[:, None], taps=ref, train=True)  # updates sd's running stats
    got = rep.outs["nan"]
    for i, (_, _, k) in enumerate(CAM_TAPS):
        r = _rel(got[f"tap{i}"].cpu().numpy(), ref[k].numpy())
        print(f"{what} tap{i}: rel err {r:.3e}")
        assert r < 1e-4, (i, r)
    buffers = {k: v.clone() for k, v in _t(ac_sd).items()}
    cam.update_running_stats(buffers, got["bn_stats"].cpu(), N, H_, W_, {name: 0.1 for name, _, _ in cam.layers})
    worst = max(_rel(buffers[f"{name}.{b}"].numpy(), sd[f"{name}.{b}"].numpy())
                for name, _, _ in cam.layers for b in ("running_mean", "running_var"))
    print(f"{what} bn_stats: worst running-statistic rel err over {len(cam.layers)} layers {worst:.3e}")
    assert worst < 1e-4, worst


@pytest.mark.parametrize("B,T", [(2, 3), (1, 1)])
def test_bilstm_train_forward_backward(shared, ac_sd, B, T):
    """m2s_bilstm_train_forward / _backward at (B, T, 208, 640): y, dx and every weight gradient against
    torch.nn.LSTM autograd on the CPU (1e-5 relative, test_gpu_gradcam.py); gates / cells / hid go from the guarded
    forward into the guarded backward."""
    Cc, Hd = 208, 640
    sd = _t(ac_sd)
    names = [f"rnn.lstm.{n}_l0{s}" for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    g = torch.Generator().manual_seed(B * 100 + T)
    x, wy = torch.randn(B, T, Cc, generator=g), torch.randn(B, T, Hd, generator=g)
    L = _lib()
    nws = L.m2s_bilstm_train_workspace_bytes(B, T, Cc, Hd)
    wspec = [(f"w{i}", "in", sd[n]) for i, n in enumerate(names)]

    def wptrs(a):
        return (C.c_void_p * 8)(*[a.ptr(f"w{i}") for i in range(8)])

    fwd = H.Arena(DEV, [("x", "in", x)] + wspec + [("y", "out", (B, T, Hd)), ("gates", "out", (2, B, T, 4 * Hd)),
                                                  ("cells", "out", (2, B, T, Hd)), ("hid", "out", (2, B, T, Hd)),
                                                  ("ws", "ws", nws)])

    def call_f(a, n):
        return L.m2s_bilstm_train_forward(a.ptr("x"), B, T, Cc, Hd, wptrs(a), a.ptr("y"), a.ptr("gates"),
                                          a.ptr("cells"), a.ptr("hid"), a.ptr("ws"), n, _stream())

    what = f"bilstm_train_forward {B}x{T}"
    tol5 = {n: 1e-5 for n in ("y", "gates", "cells", "hid")}
    # the forward takes two of the four buffers the (shared) query counts: 256 bytes less still fit
    rf = _run(shared, ("lstm_train",), what, fwd, call_f, tol=tol5, undersized=False)

    lstm = torch.nn.LSTM(Cc, Hd, 1, batch_first=True, bidirectional=True)
    lstm.load_state_dict({k[len("rnn.lstm."):]: v for k, v in sd.items() if k.startswith("rnn.lstm.")})
    xr = x.clone().requires_grad_(True)
    yr = lstm(xr)[0]
    yr = yr[..., :Hd] + yr[..., Hd:]
    (yr * wy).sum().backward()
    r = _rel(rf.outs["nan"]["y"].cpu().numpy(), yr.detach().numpy())
    print(f"{what} y: rel err {r:.3e}")
    assert r < 1e-5, r

    saved = {n: rf.outs["nan"][n].cpu() for n in ("gates", "cells", "hid")}
    gshape = [(4 * Hd, Cc), (4 * Hd, Hd), (4 * Hd,)] * 2
    bwd = H.Arena(DEV, [("x", "in", x), ("dy", "in", wy)] + wspec + [(n, "in", t) for n, t in saved.items()] +
                  [("dx", "out", (B, T, Cc))] + [(f"g{i}", "out", s) for i, s in enumerate(gshape)] + [("ws", "ws", nws)])

    def call_b(a, n):
        grads = (C.c_void_p * 6)(*[a.ptr(f"g{i}") for i in range(6)])
        return L.m2s_bilstm_train_backward(a.ptr("x"), a.ptr("dy"), B, T, Cc, Hd, wptrs(a), a.ptr("gates"),
                                           a.ptr("cells"), a.ptr("hid"), a.ptr("dx"), grads, a.ptr("ws"), n, _stream())

    what = f"bilstm_train_backward {B}x{T}"
    rb = _run(shared, ("lstm_train",), what, bwd, call_b, tol={n: 1e-5 for n in ["dx"] + [f"g{i}" for i in range(6)]})
    refs = {"dx": xr.grad}
    for d, s in enumerate(("", "_reverse")):
        for j, n in enumerate(("weight_ih", "weight_hh", "bias_ih")):
            refs[f"g{3 * d + j}"] = getattr(lstm, f"{n}_l0{s}").grad
    for n, ref in refs.items():
        r = _rel(rb.outs["nan"][n].cpu().numpy(), ref.numpy())
        print(f"{what} {n}: rel err {r:.3e}")
        assert r < 1e-5, (n, r)
