"""The device frame front end without a GPU: properties of its numpy reference (tests/frames_ref.py, the resize rule
of csrc/frames.hip), parity of that reference with cv2.resize where OpenCV is installed, the fake op's shapes, the
C ABI declaration, and the command line's new flags and native-size frame route."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import frames_ref as FR
from m2s import _native as N
from m2s import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source (h, w), destination (H, W)): the scanner sizes to the model's input, and small odd shapes where the borders
# dominate, one axis stays equal, and W != H
SHAPES = [((84, 84), (256, 256)), ((68, 68), (256, 256)), ((104, 68), (256, 256)), ((64, 64), (256, 256)),
          ((5, 7), (32, 32)), ((1, 1), (32, 32)), ((31, 33), (64, 96)), ((32, 17), (32, 40))]
IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES]
BOTH = [FR.LINEAR, FR.AREA]


def _image(hw, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=hw, dtype=np.uint8)


@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_weights_sum_to_one(src, dst, interp):
    for s, d in zip(src, dst):
        t0, t1, w0, w1 = FR.axis_coefficients(s, d, interp)
        assert np.array_equal(w0 + w1, np.full(d, FR.COEF_ONE))
        assert w0.min() >= 0 and w1.min() >= 0
        assert t0.min() >= 0 and t1.max() <= s - 1 and np.all(t1 - t0 <= 1) and np.all(t1 >= t0)


@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_constant_frame_stays_constant(src, dst, interp):
    for g in (0, 1, 127, 254, 255):
        out = FR.resize(np.full(src, g, np.uint8), *dst, interp)
        assert out.shape == dst and np.all(out == g), g


@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("hw", [(84, 84), (5, 7), (1, 1), (31, 33), (256, 256)])
def test_equal_sizes_are_the_identity(hw, interp):
    img = _image(hw, 1)
    assert np.array_equal(FR.resize(img, *hw, interp), img)


@pytest.mark.parametrize("src,dst", [((64, 64), (256, 256)), ((1, 1), (32, 32)), ((32, 17), (32, 34)),
                                     ((5, 7), (15, 14))])
def test_integer_factor_area_is_replication(src, dst):
    img = _image(src, 2)
    ky, kx = dst[0] // src[0], dst[1] // src[1]
    assert np.array_equal(FR.resize(img, *dst, FR.AREA), np.repeat(np.repeat(img, ky, axis=0), kx, axis=1))


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_linear_within_one_level_of_float64_bilinear(src, dst):
    """The 11-bit weights and the three truncating shifts cost less than one grey level (worst seen on these
    shapes: 0.747)."""
    worst = 0.0
    for seed in range(3):
        img = _image(src, 10 + seed)
        d = np.abs(FR.resize(img, *dst, FR.LINEAR).astype(np.float64) - FR.bilinear_f64(img, *dst)).max()
        worst = max(worst, float(d))
    print(f"max |fixed - float64| = {worst:.3f}")
    assert worst < 1.0


def test_bgr_goes_grey_before_the_resize():
    bgr = np.random.default_rng(3).integers(0, 256, size=(2, 31, 33, 3), dtype=np.uint8)
    grey = FR.bgr_to_grey(bgr)
    assert grey.shape == (2, 31, 33) and grey.dtype == np.uint8
    assert np.array_equal(FR.frames_ref(bgr, 64, 96, FR.LINEAR), FR.frames_ref(grey, 64, 96, FR.LINEAR))
    white = np.full((1, 2, 2, 3), 255, np.uint8)
    assert np.all(FR.bgr_to_grey(white) == 255) and np.all(FR.bgr_to_grey(white * 0) == 0)


def test_shrinking_axis_is_refused():
    with pytest.raises(ValueError):
        FR.resize(_image((8, 8)), 8, 7, FR.LINEAR)


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_reference_is_cv2_resize_bit_for_bit(src, dst):
    """The pin of the rule to OpenCV, wherever OpenCV is installed."""
    cv2 = pytest.importorskip("cv2")
    for interp, flag in ((FR.LINEAR, cv2.INTER_LINEAR), (FR.AREA, cv2.INTER_AREA)):
        for seed in range(2):
            img = _image(src, 20 + seed)
            want = cv2.resize(img, (dst[1], dst[0]), interpolation=flag)
            assert np.array_equal(FR.resize(img, *dst, interp), want), (interp, seed)


def test_bgr_grey_is_cv2_cvtcolor_bit_for_bit():
    cv2 = pytest.importorskip("cv2")
    bgr = np.random.default_rng(4).integers(0, 256, size=(31, 33, 3), dtype=np.uint8)
    assert np.array_equal(FR.bgr_to_grey(bgr), cv2.cvtColor(bgr, cv2.COLOR_BGR2GRAY))


# ------------------------------------------------------------------------------------------ op, ABI, Python surface
def test_fake_op_shapes_on_meta():
    o = ops.load()
    assert ops.FRAME_OPS == ("preprocess_frames_resize",)
    assert not set(ops.FRAME_OPS) & (set(ops.OPS) | set(ops.RAGGED_OPS) | set(ops.ANALYSIS_OPS))
    schema = str(torch.ops.m2s.preprocess_frames_resize.default._schema)
    assert schema.startswith("m2s::preprocess_frames_resize(Tensor frames, int out_h, int out_w, int interp, int norm)")
    grey = torch.empty(5, 84, 84, dtype=torch.uint8, device="meta")
    out = o.preprocess_frames_resize(grey, 256, 256, 0, 0)
    assert out.shape == (5, 256, 256) and out.dtype == torch.float32
    bgr = torch.empty(2, 31, 33, 3, dtype=torch.uint8, device="meta")
    assert o.preprocess_frames_resize(bgr, 64, 96, 1, 1).shape == (2, 64, 96)
    assert o.preprocess_frames_resize(grey[:0], 256, 200, 0, 1).shape == (0, 256, 200)
    assert ops.FRAME_INTERPS == {"linear": 0, "area": 1} and ops.FRAME_NORMS == {"zscore": 0, "unit": 1}


def test_header_declares_the_call_and_native_lists_it():
    src = open(os.path.join(REPO, "include", "m2s.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int m2s_preprocess_frames_resize(const uint8_t* frames, int n, int h, int w, int channels, int out_h, "
            "int out_w, int interp, int norm, float* out, void* stream);") in flat
    assert "enum m2s_frame_interp { M2S_FRAME_LINEAR = 0, M2S_FRAME_AREA = 1 };" in flat
    assert "enum m2s_frame_norm { M2S_FRAME_ZSCORE_MINMAX = 0, M2S_FRAME_UNIT = 1 };" in flat
    assert "#define M2S_ABI_VERSION 6" in src
    # both reference sites and the limits are named where the integrator reads them
    assert "run_mri_video_inference.py:34-54" in src and "preprocess_rtmri_data.py:99-113" in src and "65536" in src
    assert "m2s_preprocess_frames_resize" in N.exported_symbols()
    L = N.lib()
    assert hasattr(L, "m2s_preprocess_frames_resize") and len(L.m2s_preprocess_frames_resize.argtypes) == 11
    assert "frames.hip" in open(os.path.join(REPO, "mri-to-speech_amd", "csrc", "Makefile")).read()


def test_runtime_refuses_before_the_device():
    from m2s import runtime
    with pytest.raises(N.M2SError):
        runtime.preprocess_frames(torch.zeros(1, 8, 8), size=(16, 16))  # not uint8
    with pytest.raises(N.M2SError):
        runtime.preprocess_frames(torch.zeros(1, 8, 8, dtype=torch.uint8), size=(16, 16))  # not on the device
    import inspect
    sig = inspect.signature(runtime.preprocess_frames)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == \
        [("size", None), ("interp", "linear"), ("norm", "zscore")]


def _cli(name="m2s_cli_frames"):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(REPO, "mri-to-speech_amd", "scripts", "run_mri_video_inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_REQ = ["--video", "v.npy", "--mri-checkpoint", "a.pt", "--scaler-json", "s.json", "--hifigan-config", "c.json",
        "--hifigan-checkpoint", "g", "--output-dir", "out"]


def test_new_flags_parse_and_defaults_are_the_inference_convention():
    cli = _cli()
    a = cli.parse_args(_REQ)
    assert (a.device_resize, a.frame_interp, a.frame_norm) == (False, "linear", "zscore")
    assert (a.window, a.stream, a.decode_chunk, a.max_frames, a.dtype) == (0, 0, 64, None, None)
    a = cli.parse_args(_REQ + ["--device-resize", "--frame-interp", "area", "--frame-norm", "unit"])
    assert (a.device_resize, a.frame_interp, a.frame_norm) == (True, "area", "unit")
    for bad in (["--frame-interp", "cubic"], ["--frame-norm", "minmax"]):
        with pytest.raises(SystemExit):
            cli.parse_args(_REQ + bad)


def test_native_frames_reach_the_device_without_opencv(tmp_path, monkeypatch):
    """An 84 x 84 .npy stack on a machine without OpenCV: the host side yields the frames as they are (the device
    resizes them) instead of raising; a frame larger than the target still needs OpenCV."""
    cli = _cli("m2s_cli_frames_nocv")
    monkeypatch.setattr(cli, "cv2", None)
    stack = np.random.default_rng(5).integers(0, 256, size=(5, 84, 84), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", stack)
    fs = cli.FrameStream(tmp_path / "clip.npy", torch.device("cpu"), chunk=3)
    assert fs.device_resize
    chunks = list(fs._host_chunks())
    assert [len(c) for c in chunks] == [3, 2]
    assert np.array_equal(np.stack([f for c in chunks for f in c]), stack)
    # BGR and non-square frames too, and max_frames still applies
    np.save(tmp_path / "bgr.npy", np.zeros((4, 68, 104, 3), np.uint8))
    got = list(cli.FrameStream(tmp_path / "bgr.npy", torch.device("cpu"), max_frames=2)._host_chunks())
    assert [f.shape for c in got for f in c] == [(68, 104, 3)] * 2
    # frames at the target size pass as before; larger ones keep the old refusal
    np.save(tmp_path / "full.npy", np.zeros((2, 256, 256), np.uint8))
    assert [f.shape for c in cli.FrameStream(tmp_path / "full.npy", torch.device("cpu"))._host_chunks() for f in c] == \
        [(256, 256)] * 2
    np.save(tmp_path / "big.npy", np.zeros((1, 300, 256), np.uint8))
    with pytest.raises(ValueError, match="OpenCV is missing"):
        list(cli.FrameStream(tmp_path / "big.npy", torch.device("cpu"))._host_chunks())
    with pytest.raises(ValueError):
        cli.FrameStream(tmp_path / "clip.npy", torch.device("cpu"), interp="cubic")


def test_training_convention_implies_the_device_path(tmp_path):
    cli = _cli("m2s_cli_frames_conv")
    p = tmp_path / "clip.npy"
    np.save(p, np.zeros((1, 84, 84), np.uint8))
    assert cli.FrameStream(p, torch.device("cpu"), interp="area").device_resize
    assert cli.FrameStream(p, torch.device("cpu"), norm="unit").device_resize
    assert cli.FrameStream(p, torch.device("cpu"), device_resize=True).device_resize
    if cli.cv2 is not None:  # with OpenCV and no flag the host resize stays
        assert not cli.FrameStream(p, torch.device("cpu")).device_resize
