"""Windowed acoustic inference on the GPU (include/m2s.h "windowed inference", DESIGN.md "Windowed acoustic
inference"): the BiLSTM on sliding windows of W frames, one-shot and streaming.

Expected values come from tests/windowed_ref.py, the three definitions restated on the CPU oracle one window at a
time.  On these inputs (seeded randn features, synth weights) every plausible wrong result lies 0.08 or more from
the right one in max |d mel_norm| per frame (whole-clip forward instead of a window, W off by one, a window shifted
by a frame: 0.8), so the project's bar, atol = 1e-4, separates them by three orders of magnitude.  The BiLSTM-level
tests prove WHICH window produced a row (the synth CNN collapses frames); the frame-level tests prove the wiring.
Frames are 96 x 80 as in test_gpu_ragged.py.  GPU box only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import windowed_ref as R  # tests/windowed_ref.py
import ws_harness as H    # tests/ws_harness.py
from m2s import _native, ops, runtime, synth
from m2s.config import HIFIGAN_H
from m2s.stream import AcousticStream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HW = (96, 80)
LENS = [7, 1, 4, 7, 3]
ERRORS = (_native.M2SError, RuntimeError)
OLD_RECURRENCES = ("lstm_small", "lstm_mid", "lstm_x3", "lstm_persistent", "lstm_step")  # lstm_x3 covers lstm_x3g


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.fixture(scope="module")
def ac_sd():
    return synth.synth_acoustic_state(2)


@pytest.fixture(scope="module")
def sd(ac_sd):
    return _t(ac_sd)


@pytest.fixture(scope="module")
def ac(ac_sd):
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = runtime.AcousticEngine(ac_sd, dtype=dtype, device=DEV)
        return cache[dtype]
    return get


@pytest.fixture(scope="module")
def voc():
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = runtime.VocoderEngine(synth.synth_generator_state(2, HIFIGAN_H), HIFIGAN_H, dtype=dtype,
                                                 device=DEV)
        return cache[dtype]
    return get


def _feats(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 208, generator=g) for n in lens]


def _dev(xs):
    return [x.to(DEV) for x in xs]


CASES = {"w4_small": (4, [5, 2]), "w4_mid": (4, LENS), "w4_tile": (4, [35]), "w4_many": (4, [300, 40]),
         "w3": (3, [9, 6]), "w1": (1, [4]), "w8": (8, [20, 8, 5])}


@pytest.fixture(scope="module")
def refs(sd):
    """(feats, y, mel_norm) of every (case, merge), computed on first use and never modified."""
    cache = {}

    def get(case, merge):
        if (case, merge) not in cache:
            W, lens = CASES[case]
            feats = _feats(lens, seed=len(lens) + 10 * W)
            y, m = R.windowed(sd, feats, W, merge)
            cache[case, merge] = (feats, y.numpy(), m.numpy())
        return cache[case, merge]
    return get


def _check(what, got, want, atol=1e-4):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    print(f"{what}: max|d| = {err:.2e}")
    np.testing.assert_allclose(got, want, atol=atol, rtol=0, err_msg=what)


# ---- 1. bilstm_windowed against the helper ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("merge", ["latest", "mean"])
@pytest.mark.parametrize("case", list(CASES))
def test_bilstm_windowed_vs_oracle(ac, refs, case, merge, dtype):
    W, lens = CASES[case]
    feats, y_ref, m_ref = refs(case, merge)
    eng = ac(dtype)
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        y, mn = eng.bilstm_windowed(_dev(feats), None, W, merge)
        eng.check()
        rec = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    names = {r["name"] for r in rec}
    assert any(n.startswith("lstm_window") for n in names), names
    assert not [n for n in names if n.startswith(OLD_RECURRENCES)], names
    assert all(r["stage"] in ("bilstm", "head") for r in rec if r["name"].startswith("lstm_window")), rec
    steps = [r for r in rec if r["name"].startswith("lstm_window_step_kernel")]
    assert len(steps) == W - 1, (len(steps), W)  # one launch per recurrent step
    _check(f"bilstm_windowed {case} {merge} {dtype} mel_norm", mn, m_ref)
    _check(f"bilstm_windowed {case} {merge} {dtype} y", y, y_ref)


# ---- 2. the remaining engines: their recurrence is the split one ------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("merge", ["latest", "mean"])
def test_bilstm_windowed_other_engines(ac, refs, merge, dtype):
    feats, y_ref, m_ref = refs("w4_mid", merge)
    eng = ac(dtype)
    y, mn = eng.bilstm_windowed(_dev(feats), None, 4, merge)
    eng.check()
    _check(f"bilstm_windowed w4_mid {merge} {dtype} mel_norm", mn, m_ref)
    _check(f"bilstm_windowed w4_mid {merge} {dtype} y", y, y_ref)


# ---- 3. context ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_context_rows_are_the_no_context_rows(ac, sd, dtype):
    lens, ctx, W = [6, 4, 9], [3, 0, 2], 4
    feats = _feats(lens, seed=77)
    y_ref, m_ref = R.windowed(sd, feats, W, "latest", ctx)
    eng = ac(dtype)
    packed = torch.cat(feats).to(DEV)
    y, mn = eng.bilstm_windowed(packed, lens, W, "latest", ctx)
    y0, mn0 = eng.bilstm_windowed(packed, lens, W, "latest")
    eng.check()
    assert mn.shape == (sum(lens) - sum(ctx), 64) and y.shape == (sum(lens) - sum(ctx), 640)
    _check(f"context {dtype} mel_norm", mn, m_ref.numpy())
    _check(f"context {dtype} y", y, y_ref.numpy())
    keep = torch.cat([torch.arange(o + c, o + n) for o, n, c in zip(np.cumsum([0] + lens[:-1]).tolist(), lens, ctx)])
    assert torch.equal(mn, mn0[keep.to(DEV)]) and torch.equal(y, y0[keep.to(DEV)])


# ---- 4. streaming -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_stream_chunkings_are_the_whole_clip_bit_for_bit(ac, dtype):
    eng = ac(dtype)
    clip = torch.from_numpy(synth.synth_frames(1, 25, hw=HW, seed=41)[0]).to(DEV)
    other = torch.from_numpy(synth.synth_frames(1, 6, hw=HW, seed=42)[0]).to(DEV)
    whole = eng.forward_windowed(clip)
    st = AcousticStream(eng, window=4)
    for chunk in (1, 2, 5, 17):
        st.reset()
        got = torch.cat([st.push(clip[i:i + chunk]) for i in range(0, 25, chunk)])
        d = float((got - whole).abs().max())
        print(f"stream {dtype} chunks of {chunk}: max|d| vs whole clip = {d:.2e}")
        assert got.shape == whole.shape == (25, 64)
        assert torch.equal(got, whole), (chunk, d)
    st.reset()
    st.push(other)  # a first clip ...
    st.reset()
    again = torch.cat([st.push(clip[:10]), st.push(clip[10:])])  # ... leaves no trace in the second
    eng.check()
    assert torch.equal(again, whole)


def test_stream_on_frames_the_cnn_tells_apart():
    """The same on gain-one weights (tests/distinct.py), where every frame has its own feature row: a chunk whose
    rows were prepended in the wrong order, or a CNN pass whose result depended on its size, would show here."""
    import distinct
    eng = runtime.AcousticEngine(distinct.calibrated_acoustic_state(0), dtype="bf16x3", device=DEV)
    clip = torch.from_numpy(synth.synth_frames(1, 25, hw=HW, seed=41)[0]).to(DEV)
    feats = eng.effnet(clip)
    assert float((feats[1:] - feats[:-1]).abs().amax(1).min()) > 0.05  # neighbouring frames differ
    whole = eng.forward_windowed(clip)
    assert float((whole[1:] - whole[:-1]).abs().amax(1).min()) > 1e-3
    st = AcousticStream(eng, window=4)
    for chunk in (1, 5, 17):
        st.reset()
        got = torch.cat([st.push(clip[i:i + chunk]) for i in range(0, 25, chunk)])
        assert torch.equal(got, whole), chunk
    eng.check()


# ---- 5. invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", ["latest", "mean"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_batch_order_and_neighbours_do_not_matter(ac, dtype, merge):
    eng = ac(dtype)
    clips = _dev(_feats(LENS, seed=500))

    def run(cs):
        lens = [int(c.shape[0]) for c in cs]
        y, mn = eng.bilstm_windowed(cs, None, 4, merge)
        return runtime.split_packed(y, lens), runtime.split_packed(mn, lens)

    base = run(clips)
    perm = [3, 2, 4, 0, 1]
    moved = run([clips[i] for i in perm])
    for k in (0, 1):
        for pos, i in enumerate(perm):
            assert torch.equal(moved[k][pos], base[k][i]), (k, i)
    other = list(clips)
    other[0] = torch.randn(LENS[0], 208, generator=torch.Generator().manual_seed(999)).to(DEV)
    swapped = run(other)
    eng.check()
    assert not torch.equal(swapped[1][0], base[1][0])
    for k in (0, 1):
        for i in range(1, len(LENS)):
            assert torch.equal(swapped[k][i], base[k][i]), (k, i)


# ---- 6. ties to the existing path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_mean_with_a_window_past_every_clip_is_the_ragged_forward(ac, dtype):
    eng = ac(dtype)
    clips = _dev(_feats(LENS, seed=600))
    y, mn = eng.bilstm_windowed(clips, None, 16, "mean")
    yr, mnr = eng.bilstm_ragged(clips)
    eng.check()
    _check(f"mean W=16 vs bilstm_ragged {dtype} mel_norm", mn, mnr.cpu().numpy())
    _check(f"mean W=16 vs bilstm_ragged {dtype} y", y, yr.cpu().numpy())


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_latest_full_windows_are_the_gathered_dense_call(ac, dtype):
    """The composition available without this mode: gather (S, W, 208) windows, run the dense BiLSTM, take the last
    step.  It covers the full windows only."""
    eng, W, n = ac(dtype), 4, 12
    x = _feats([n], seed=601)[0].to(DEV)
    y, mn = eng.bilstm_windowed(x, None, W, "latest")
    block = torch.stack([x[t - W + 1:t + 1] for t in range(W - 1, n)])  # (S, W, 208)
    yd, mnd = eng.bilstm(block)
    eng.check()
    _check(f"latest vs gathered dense {dtype} mel_norm", mn[W - 1:], mnd[:, -1].cpu().numpy())
    _check(f"latest vs gathered dense {dtype} y", y[W - 1:], yd[:, -1].cpu().numpy())


# ---- 7. composition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", ["latest", "mean"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_forward_windowed_is_effnet_then_bilstm_windowed(ac, dtype, merge):
    eng = ac(dtype)
    fr = torch.from_numpy(np.concatenate([synth.synth_frames(1, n, hw=HW, seed=100 + 17 * b)[0]
                                          for b, n in enumerate(LENS)])).to(DEV)
    mn = eng.forward_windowed(fr, LENS, 4, merge)
    _, want = eng.bilstm_windowed(eng.effnet(fr), LENS, 4, merge)
    eng.check()
    assert mn.shape == (sum(LENS), 64) and torch.equal(mn, want)


def test_pipeline_forward_windowed_wav_is_the_ragged_vocoder_on_its_mel(ac, voc):
    lens = [6, 2, 4]
    clips = [torch.from_numpy(synth.synth_frames(1, n, hw=HW, seed=300 + 17 * b)[0]).to(DEV)
             for b, n in enumerate(lens)]
    mean, std = synth.synth_scaler()
    pipe = runtime.Pipeline(ac("bf16x3"), voc("bf16x3"), mean, std)
    out = pipe.forward_windowed(clips)
    pipe.ac.check()
    assert out["mel_norm"].shape == (12, 64) and out["wav"].shape == (12 * pipe.voc.hop,)
    assert torch.equal(out["mel_norm"], pipe.ac.forward_windowed(clips))
    assert torch.equal(out["wav"], pipe.voc.forward_ragged(out["mel_log"], lens))


# ---- 8. opcheck ---------------------------------------------------------------------------------------------------
def test_opcheck_every_windowed_op(ac):
    a = ac("bf16x3")
    o = ops.load()
    lens = [3, 1, 2]
    fr = torch.from_numpy(np.concatenate([synth.synth_frames(1, n, hw=HW, seed=7 + 17 * b)[0]
                                          for b, n in enumerate(lens)])).to(DEV)
    cases = {
        "bilstm_windowed": [(a.handle, torch.randn(6, 208, device=DEV), lens, [], 4, 0, 640, 64),
                            (a.handle, torch.randn(6, 208, device=DEV), lens, [2, 0, 1], 4, 0, 640, 64),
                            (a.handle, torch.randn(6, 208, device=DEV), lens, [], 2, 1, 640, 64)],
        "acoustic_forward_windowed": [(a.handle, fr, lens, [], 4, 0, 64), (a.handle, fr, lens, [], 2, 1, 64)],
    }
    assert set(cases) == set(ops.WINDOWED_OPS)
    for name, argsets in cases.items():
        for args in argsets:
            torch.library.opcheck(getattr(o, name).default, args,
                                  test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))


# ---- 9. argument errors -------------------------------------------------------------------------------------------
BAD = {"window0": dict(lens=[3, 2], window=0), "window17": dict(lens=[3, 2], window=17),
       "merge7": dict(lens=[3, 2], merge=7), "context_with_mean": dict(lens=[3, 2], merge=1, context=[1, 0]),
       "context_is_W": dict(lens=[5], window=4, context=[4]), "context_is_len": dict(lens=[3, 2], context=[0, 2]),
       "zero_length": dict(lens=[3, 0, 2]), "short": dict(lens=[3, 1]), "long": dict(lens=[4, 2]),
       "empty": dict(lens=[])}


@pytest.mark.parametrize("bad", list(BAD))
def test_argument_errors_raise_before_any_launch(ac, bad):
    a = ac("bf16x3")
    o = ops.load()
    kw = dict(window=4, merge=0, context=[])
    kw.update(BAD[bad])
    fr = torch.zeros(5, *HW, device=DEV)
    ft = torch.zeros(5, 208, device=DEV)
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()  # start from an empty record
        for call in (lambda: o.bilstm_windowed(a.handle, ft, kw["lens"], kw["context"], kw["window"], kw["merge"], 640, 64),
                     lambda: o.acoustic_forward_windowed(a.handle, fr, kw["lens"], kw["context"], kw["window"],
                                                         kw["merge"], 64)):
            with pytest.raises(ERRORS):
                call()
        assert _native.prof_launches() == []
    finally:
        _native.prof_enable(False)
    a.check()


def test_unknown_merge_name_is_refused(ac):
    with pytest.raises(ERRORS):
        ac("bf16x3").bilstm_windowed(torch.zeros(5, 208, device=DEV), [5], 4, "median")


# ---- 10. workspace contract through the C ABI ---------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v) if v is not None else None


def _contract(eng, arena, call, what):
    L = _native.lib()

    def sync():
        torch.cuda.synchronize(DEV)

    def status():
        return L.m2s_acoustic_status(eng._h)

    (ws,) = arena.names("ws")
    rep = H.check_contract(arena, lambda a: call(a, a.nbytes(ws)), sync=sync, status=status, what=what)
    assert rep.deterministic, what
    H.check_undersized(arena, call, rep.outs["zero"], sync=sync, status=status, what=what)
    return rep


WS_MODES = {"latest_ctx": (0, [2, 0, 3]), "mean": (1, None)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("mode", list(WS_MODES))
def test_workspace_contract_bilstm_windowed(ac, sd, mode, dtype):
    lens, W = [7, 1, 4], 4
    merge, ctx = WS_MODES[mode]
    if ctx is not None:
        ctx = [2, 0, 3]
    eng, L = ac(dtype), _native.lib()
    feats = _feats(lens, seed=3)
    N, Rr = sum(lens), sum(lens) - sum(ctx or [])
    cl, cc = _ints(lens), _ints(ctx)
    nws = L.m2s_acoustic_windowed_workspace_bytes(eng._h, cl, cc, len(lens), 0, 0, W, merge)
    assert nws > 0
    arena = H.Arena(DEV, [("feats", "in", torch.cat(feats)), ("y", "out", (Rr, 640)), ("mel_norm", "out", (Rr, 64)),
                          ("ws", "ws", nws)])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(a, n):
        return L.m2s_bilstm_windowed(eng._h, a.ptr("feats"), cl, cc, len(lens), N, W, merge, a.ptr("y"),
                                     a.ptr("mel_norm"), a.ptr("ws"), n, stream)

    what = f"bilstm_windowed {mode} {dtype} {lens}"
    rep = _contract(eng, arena, call, what)
    y_ref, m_ref = R.windowed(sd, feats, W, "mean" if merge else "latest", ctx)
    _check(f"{what} mel_norm", rep.outs["nan"]["mel_norm"], m_ref.numpy())
    _check(f"{what} y", rep.outs["nan"]["y"], y_ref.numpy())


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("mode", list(WS_MODES))
def test_workspace_contract_acoustic_forward_windowed(ac, mode, dtype):
    lens, W = [7, 1, 4], 4
    merge, ctx = WS_MODES[mode]
    eng, L = ac(dtype), _native.lib()
    clips = [synth.synth_frames(1, n, hw=HW, seed=100 + 17 * b)[0] for b, n in enumerate(lens)]
    N, Rr = sum(lens), sum(lens) - sum(ctx or [])
    cl, cc = _ints(lens), _ints(ctx)
    nws = L.m2s_acoustic_windowed_workspace_bytes(eng._h, cl, cc, len(lens), HW[0], HW[1], W, merge)
    assert nws > 0
    arena = H.Arena(DEV, [("frames", "in", np.concatenate(clips)), ("mel_norm", "out", (Rr, 64)), ("ws", "ws", nws)])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(a, n):
        return L.m2s_acoustic_forward_windowed(eng._h, a.ptr("frames"), cl, cc, len(lens), N, HW[0], HW[1], W, merge,
                                               a.ptr("mel_norm"), a.ptr("ws"), n, stream)

    what = f"acoustic_forward_windowed {mode} {dtype} {lens}"
    rep = _contract(eng, arena, call, what)
    want = eng.forward_windowed(torch.from_numpy(np.concatenate(clips)).to(DEV), lens, W, "mean" if merge else "latest",
                                ctx)
    eng.check()
    assert torch.equal(rep.outs["nan"]["mel_norm"], want)


# ---- 11. command line ---------------------------------------------------------------------------------------------
def test_export_script_window_flag(tmp_path):
    """scripts/export_predicted_mels.py --window 4 writes the windowed model's ln-mels; without the flag it writes
    what the dense call gives, as before."""
    import importlib.util
    import json
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "m2s_export_mels_windowed", os.path.join(repo, "mri-to-speech_amd", "scripts", "export_predicted_mels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mean, std = synth.synth_scaler()
    state = synth.synth_acoustic_state(6)
    ck = tmp_path / "best.pt"
    torch.save({"model_state_dict": _t(state)}, ck)
    (tmp_path / "scaler.json").write_text(json.dumps({"mean": mean.tolist(), "std": std.tolist()}))
    rng = np.random.default_rng(3)
    clips = {"utt_a": 6, "utt_b": 3}
    frames = {}
    for stem, n in clips.items():
        d = tmp_path / "proc" / "samples" / stem
        d.mkdir(parents=True)
        frames[stem] = (rng.integers(0, 256, (n, *HW)) / 255.0).astype(np.float32)
        np.save(d / "mri.npy", frames[stem])
    common = ["--processed_dir", str(tmp_path / "proc"), "--mri_checkpoint", str(ck), "--scaler_json",
              str(tmp_path / "scaler.json"), "--mri_code_dir", os.path.join(repo, "mri-to-speech_amd", "mri2speech_code"),
              "--dtype", "bf16x3"]
    got = mod.main([*common, "--output_dir", str(tmp_path / "win"), "--window", "4"])
    plain = mod.main([*common, "--output_dir", str(tmp_path / "dense")])
    assert sorted(p.name for p in got) == sorted(p.name for p in plain) == ["utt_a.npy", "utt_b.npy"]
    eng = runtime.AcousticEngine(state, dtype="bf16x3", device=DEV)
    for stem, n in clips.items():
        x = torch.from_numpy(frames[stem]).to(DEV)
        win = runtime.mel_glue(eng.forward_windowed(x, None, 4, "latest"), mean, std)[1].t().cpu().numpy()
        dense = runtime.mel_glue(eng.forward(x[None])[0], mean, std)[1].t().cpu().numpy()
        a, b = np.load(tmp_path / "win" / f"{stem}.npy"), np.load(tmp_path / "dense" / f"{stem}.npy")
        assert a.shape == b.shape == (64, n) and a.dtype == b.dtype == np.float32
        assert np.array_equal(a, win), stem
        assert np.array_equal(b, dense), stem
    eng.check()
