"""The device frame front end on the GPU (csrc/frames.hip): native-size uint8 frames -> resized, normalised fp32
frames, against the numpy restatement of its resize rule (tests/frames_ref.py) and the oracle's normalisation.

* UNIT outputs are compared with torch.equal: the resize is integers and float32 division is correctly rounded.
* ZSCORE_MINMAX outputs are held to atol = 1e-6 of oracle.acoustic.preprocess_frame on the reference-resized frame,
  the bar of test_gpu_parity.test_preprocess_vs_oracle_shapes_and_bgr.
* Frames of a batch are distinct random images, so a wrong frame index fails.
"""
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import frames_ref as FR     # tests/frames_ref.py
import ws_harness as H      # tests/ws_harness.py
from m2s import _native, ops, runtime, synth
from m2s.config import HIFIGAN_H
from oracle import acoustic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR, AREA, ZSCORE, UNIT = 0, 1, 0, 1
PAIRS_ALL = [(LINEAR, ZSCORE), (LINEAR, UNIT), (AREA, ZSCORE), (AREA, UNIT)]
PAIRS_REF = [(LINEAR, ZSCORE), (AREA, UNIT)]  # the reference's inference and training conventions

# name -> (n, source shape, (H, W))
CASES = {
    "5x7": (3, (5, 7), (32, 32)),              # unaligned frame bases, borders dominate
    "84": (2, (84, 84), (256, 256)),
    "68": (2, (68, 68), (256, 256)),
    "bgr": (2, (31, 33, 3), (64, 96)),         # W != H catches a transposition
    "odd_out": (2, (31, 33), (37, 50)),        # output base of frame 1 is not 16-byte aligned
    "one_axis": (1, (32, 17), (32, 40)),
    "1x1": (1, (1, 1), (32, 32)),
    "limits": (1, (256, 256, 3), (256, 256)),  # both 65536-pixel limits at once: no room for coefficient tables
    "long_row": (2, (1, 16), (1, 16000)),      # 8 bytes of table per row and column would pass 128 KB: no tables
}
SWEEP = [(c, p) for c in CASES for p in (PAIRS_ALL if c in ("5x7", "84") else PAIRS_REF)]


@functools.lru_cache(maxsize=None)
def _frames(case):
    n, shape, _ = CASES[case]
    seed = sorted(CASES).index(case)
    a = np.random.default_rng(seed).integers(0, 256, size=(n, *shape), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _resized(case, interp):
    a = FR.frames_ref(_frames(case), *CASES[case][2], interp)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _expected(case, interp, norm):
    r = _resized(case, interp)
    a = FR.unit(r) if norm == UNIT else np.stack([acoustic.preprocess_frame(f) for f in r])
    a.setflags(write=False)
    return a


def _run(frames_u8, size, interp, norm):
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(DEV)
    return ops.load().preprocess_frames_resize(x, size[0], size[1], interp, norm)


@pytest.mark.parametrize("case,pair", SWEEP, ids=[f"{c}-{'LA'[p[0]]}{'ZU'[p[1]]}" for c, p in SWEEP])
def test_matches_the_reference(case, pair):
    interp, norm = pair
    n, _, size = CASES[case]
    out = _run(_frames(case), size, interp, norm).cpu()
    want = torch.from_numpy(_expected(case, interp, norm))
    assert out.shape == (n, *size) and out.dtype == torch.float32
    d = float((out - want).abs().max())
    print(f"{case} interp {interp} norm {norm}: max |d| = {d:.3e}")
    if norm == UNIT:
        assert torch.equal(out, want)
    else:
        assert d <= 1e-6
        if float(want.max()) > 0:  # not a constant frame: the extremes are exact
            assert float(out.min()) == 0.0 and float(out.max()) == 1.0


@pytest.mark.parametrize("case", ["5x7", "84", "bgr", "odd_out"])
def test_constant_frames(case):
    _, shape, size = CASES[case]
    levels = [0, 1, 100, 255]
    x = np.stack([np.full(shape, g, np.uint8) for g in levels])
    for interp in (LINEAR, AREA):
        z = _run(x, size, interp, ZSCORE)
        assert torch.equal(z, torch.zeros_like(z))
        u = _run(x, size, interp, UNIT).cpu()
        want = (torch.tensor(levels, dtype=torch.float32) / torch.tensor(255, dtype=torch.float32))[:, None, None]
        assert torch.equal(u, want.expand_as(u))


@pytest.mark.parametrize("case", ["5x7", "odd_out", "bgr"])
def test_a_frame_alone_and_in_any_batch_position_is_bit_identical(case):
    _, shape, size = CASES[case]
    a = np.random.default_rng(77).integers(0, 256, size=(5, *shape), dtype=np.uint8)
    x = torch.from_numpy(a).to(DEV)
    o = ops.load()
    for interp, norm in PAIRS_REF:
        batch = o.preprocess_frames_resize(x, size[0], size[1], interp, norm)
        for i in range(5):
            alone = o.preprocess_frames_resize(x[i:i + 1], size[0], size[1], interp, norm)  # a view: unaligned base
            assert H.bits_equal(alone[0], batch[i]), (interp, norm, i)
        perm = [3, 0, 4, 1, 2]
        moved = o.preprocess_frames_resize(x[perm].contiguous(), size[0], size[1], interp, norm)
        assert H.bits_equal(moved, batch[perm])
        tail = o.preprocess_frames_resize(x[2:], size[0], size[1], interp, norm)
        assert H.bits_equal(tail, batch[2:])


@pytest.mark.parametrize("shape", [(3, 40, 36), (2, 33, 31, 3), (1, 256, 256), (2, 5, 7)])
def test_equal_sizes_are_preprocess_frames(shape):
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    want = runtime.preprocess_frames(x)
    assert torch.equal(runtime.preprocess_frames(x, size=shape[1:3]), want)
    assert torch.equal(runtime.preprocess_frames(x[1:], size=shape[1:3]), want[1:])
    # the training convention at equal size: the identity resize, / 255
    grey = torch.from_numpy(FR.frames_ref(x.cpu().numpy(), shape[1], shape[2], FR.AREA))
    assert torch.equal(runtime.preprocess_frames(x, interp="area", norm="unit").cpu(), grey.float() / 255.0)


def test_runtime_names_map_to_the_conventions():
    a = torch.from_numpy(_frames("84")).to(DEV)
    for (iname, interp), (nname, norm) in [(("linear", LINEAR), ("zscore", ZSCORE)), (("area", AREA), ("unit", UNIT)),
                                           (("linear", LINEAR), ("unit", UNIT))]:
        got = runtime.preprocess_frames(a, (256, 256), iname, nname)
        assert torch.equal(got, ops.load().preprocess_frames_resize(a, 256, 256, interp, norm))
    with pytest.raises(_native.M2SError):
        runtime.preprocess_frames(a, (256, 256), "cubic")
    with pytest.raises((RuntimeError, _native.M2SError)):
        runtime.preprocess_frames(a, (64, 64))  # shrinking


# ---- the C ABI between guard bands -----------------------------------------------------------------------------------
def _abi(arena, n, h, w, ch, oh, ow, interp, norm):
    return _native.lib().m2s_preprocess_frames_resize(arena.ptr("frames"), n, h, w, ch, oh, ow, interp, norm,
                                                      arena.ptr("out"), None)


@pytest.mark.parametrize("case", ["5x7", "84", "bgr", "odd_out", "limits"])
def test_c_abi_writes_exactly_its_output(case):
    n, shape, size = CASES[case]
    ch = 3 if len(shape) == 3 else 1
    arena = H.Arena(DEV, [("frames", "in", _frames(case)), ("out", "out", (n, *size))])
    for interp, norm in PAIRS_REF:
        arena.prepare("nan")  # the output holds NaN on entry, the guards their patterns
        torch.cuda.synchronize()
        rc = _abi(arena, n, shape[0], shape[1], ch, size[0], size[1], interp, norm)
        torch.cuda.synchronize()
        assert rc == H.M2S_OK, _native.lib().m2s_last_error()
        assert not arena.violations(), arena.violations()
        assert H.bits_equal(arena.view("out"), _run(_frames(case), size, interp, norm))


def test_c_abi_refusals_launch_nothing():
    n, (h, w), (oh, ow) = 2, (84, 84), (256, 256)
    arena = H.Arena(DEV, [("frames", "in", _frames("84")), ("out", "out", (n, oh, ow))])
    L = _native.lib()
    bad = {
        "channels 2": (n, h, w, 2, oh, ow, LINEAR, ZSCORE), "channels 4": (n, h, w, 4, oh, ow, LINEAR, ZSCORE),
        "channels 0": (n, h, w, 0, oh, ow, LINEAR, ZSCORE),
        "h > out_h": (n, h, w, 1, h - 1, ow, LINEAR, ZSCORE), "w > out_w": (n, h, w, 1, oh, w - 1, AREA, UNIT),
        "source pixels": (1, 257, 256, 1, 257, 256, LINEAR, ZSCORE),
        "destination pixels": (n, h, w, 1, 257, 256, LINEAR, ZSCORE),
        "interp 2": (n, h, w, 1, oh, ow, 2, ZSCORE), "interp -1": (n, h, w, 1, oh, ow, -1, ZSCORE),
        "norm 2": (n, h, w, 1, oh, ow, LINEAR, 2), "norm -1": (n, h, w, 1, oh, ow, LINEAR, -1),
        "n < 0": (-1, h, w, 1, oh, ow, LINEAR, ZSCORE), "h = 0": (n, 0, w, 1, oh, ow, LINEAR, ZSCORE),
    }
    for what, args in bad.items():
        arena.prepare("nan")
        torch.cuda.synchronize()
        rc = _abi(arena, *args)
        torch.cuda.synchronize()
        assert rc == H.M2S_E_ARG, (what, rc)
        assert L.m2s_last_error(), what
        assert not arena.violations(outputs_written=False), what
        assert bool((arena.raw("out") == H.POISON).all()), what  # nothing was launched
    arena.prepare("nan")
    assert L.m2s_preprocess_frames_resize(None, n, h, w, 1, oh, ow, 0, 0, arena.ptr("out"), None) == H.M2S_E_ARG
    assert _abi(arena, 0, h, w, 1, oh, ow, LINEAR, ZSCORE) == H.M2S_OK  # n = 0 is a no-op
    torch.cuda.synchronize()
    assert bool((arena.raw("out") == H.POISON).all()) and not arena.violations(outputs_written=False)
    assert _abi(arena, n, h, w, 1, oh, ow, LINEAR, ZSCORE) == H.M2S_OK  # and the call still works
    torch.cuda.synchronize()
    assert not arena.violations()


def test_empty_batch_through_the_op():
    out = ops.load().preprocess_frames_resize(torch.empty(0, 84, 84, dtype=torch.uint8, device=DEV), 256, 256, 0, 0)
    assert out.shape == (0, 256, 256)


# ---- torch surface -----------------------------------------------------------------------------------------------------
def test_opcheck_the_frame_op():
    o = ops.load()
    assert ops.FRAME_OPS == ("preprocess_frames_resize",)
    for args in [(torch.from_numpy(_frames("5x7")).to(DEV), 32, 32, LINEAR, ZSCORE),
                 (torch.from_numpy(_frames("bgr")).to(DEV), 64, 96, AREA, UNIT)]:
        torch.library.opcheck(o.preprocess_frames_resize.default, args,
                              test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))


def test_graph_capture_replays_to_the_same_bits():
    o = ops.load()
    a = np.random.default_rng(9).integers(0, 256, size=(2, 3, 84, 84), dtype=np.uint8)
    x = torch.from_numpy(a[0]).to(DEV)
    eager = [o.preprocess_frames_resize(torch.from_numpy(a[k]).to(DEV), 256, 256, LINEAR, ZSCORE) for k in (0, 1)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = o.preprocess_frames_resize(x, 256, 256, LINEAR, ZSCORE)
    for k in (0, 1, 0):
        x.copy_(torch.from_numpy(a[k]))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert H.bits_equal(y, eager[k]), k


# ---- streams and the command line --------------------------------------------------------------------------------------
def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def test_speech_stream_takes_uint8_native_frames():
    from m2s.stream import AcousticStream, SpeechStream
    mean, std = synth.synth_scaler()
    ac = runtime.AcousticEngine(synth.synth_acoustic_state(2), dtype="bf16x3", device=DEV)
    pipe = runtime.Pipeline(ac, runtime.VocoderEngine(synth.synth_generator_state(2), HIFIGAN_H, dtype="bf16x3",
                                                      device=DEV), mean, std)
    u8 = torch.from_numpy(np.random.default_rng(11).integers(0, 256, size=(6, 84, 84), dtype=np.uint8)).to(DEV)
    f32 = runtime.preprocess_frames(u8, (256, 256))
    assert f32.shape == (6, 256, 256)
    a, b = SpeechStream(pipe, window=4), SpeechStream(pipe, window=4)
    for lo, hi in [(0, 1), (1, 4), (4, 6)]:
        oa, ob = a.push(u8[lo:hi]), b.push(f32[lo:hi])
        for k in ("mel_norm", "mel_db", "mel_log", "wav"):
            assert H.bits_equal(oa[k], ob[k]), (k, lo)
    ac.check()
    # a stream built for the training convention, BGR frames, another size
    bgr = torch.from_numpy(_frames("bgr")).to(DEV)
    s = AcousticStream(ac, window=2, size=(96, 80), interp="area", norm="unit")  # a size the CNN tests run at
    want = AcousticStream(ac, window=2).push(runtime.preprocess_frames(bgr, (96, 80), "area", "unit"))
    assert H.bits_equal(s.push(bgr), want)
    ac.check()


def test_cli_runs_a_native_size_stack_without_opencv(tmp_path, monkeypatch):
    """An 84 x 84 .npy stack through the command line on a machine without OpenCV: the reference's output files,
    and the mel of the oracle on the reference-resized frames."""
    from oracle import effnet
    T = 4
    ac_sd, gen_sd = synth.synth_acoustic_state(4), synth.synth_generator_state(4)
    mean, std = synth.synth_scaler()
    ckdir = tmp_path / "ck" / "mri"
    ckdir.mkdir(parents=True)
    torch.save({"model_state_dict": _t(ac_sd)}, ckdir / "best.pt")
    torch.save({"generator": _t(gen_sd)}, tmp_path / "g_00000001")
    (tmp_path / "config.json").write_text(json.dumps(dict(HIFIGAN_H)))
    (tmp_path / "scaler.json").write_text(json.dumps({"mean": mean.tolist(), "std": std.tolist()}))
    video = np.random.default_rng(12).integers(0, 256, size=(T + 1, 84, 84), dtype=np.uint8)
    np.save(tmp_path / "clip84.npy", video)
    spec = importlib.util.spec_from_file_location(
        "m2s_cli_frames_gpu", os.path.join(REPO, "mri-to-speech_amd", "scripts", "run_mri_video_inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    monkeypatch.setattr(cli, "cv2", None)
    common = ["--video", str(tmp_path / "clip84.npy"), "--mri-checkpoint", str(ckdir / "best.pt"),
              "--scaler-json", str(tmp_path / "scaler.json"), "--hifigan-config", str(tmp_path / "config.json"),
              "--hifigan-checkpoint", str(tmp_path / "g_00000001"),
              "--mri-code-dir", os.path.join(REPO, "mri-to-speech_amd", "mri2speech_code"),
              "--max-frames", str(T), "--dtype", "fp32", "--decode-chunk", "3"]
    res = cli.main(common + ["--output-dir", str(tmp_path / "out")])
    for f in ("clip84_generated.wav", "clip84_mel.npy", "clip84_mel_log.npy"):
        assert (tmp_path / "out" / f).exists(), f
    mel_db = np.load(tmp_path / "out" / "clip84_mel.npy")
    assert mel_db.shape == (T, 64) and res["audio"].shape == (T * 420,)
    frames = np.stack([acoustic.preprocess_frame(f) for f in FR.frames_ref(video[:T], 256, 256, FR.LINEAR)])
    sd = _t(ac_sd)
    mn = acoustic.head(sd, acoustic.bilstm_summerge(sd, effnet.effnet_gap(sd, torch.from_numpy(frames)).view(1, T, -1)))[0]
    np.testing.assert_allclose(mel_db, acoustic.denormalize_mel(mn, mean, std).numpy(), atol=2e-3, rtol=0)
    # the training convention through the flags gives other frames, hence another mel
    res2 = cli.main(common + ["--output-dir", str(tmp_path / "out2"), "--frame-interp", "area", "--frame-norm", "unit"])
    assert res2["mel_db"].shape == (T, 64) and np.abs(res2["mel_db"] - res["mel_db"]).max() > 0
    got = cli.FrameStream(tmp_path / "clip84.npy", DEV, T, interp="area", norm="unit").read()
    assert torch.equal(got.cpu(), torch.from_numpy(FR.unit(FR.frames_ref(video[:T], 256, 256, FR.AREA))))
