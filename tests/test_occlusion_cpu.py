"""The masking experiment's host side (m2s/occlusion.py, the two command lines) and its registered surface; no GPU.

The mask rules are DESIGN.md §30's: a convex polygon filled boundary included, a separable Gaussian with OpenCV's
sigma = 0 kernels and reflect-101 borders, a clip to [alpha, 1].  Their parity with cv2 is unpinned; what is pinned
here is the rule itself, against scipy for the blur and against tests/mask_ref.py for the application.
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_ref as MR  # tests/mask_ref.py
from m2s import _native as N
from m2s import occlusion as OC
from m2s import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(REPO, "mri-to-speech_amd", "scripts")
NEW_SYMBOLS = ("m2s_preprocess_frames_masked", "m2s_occlusion_reduce")


# ------------------------------------------------------------------------------------------------------- the builder
def test_lip_preset_without_blur_fills_exactly_its_rows():
    alpha = np.float32(0.1)
    m = OC.preset_mask("lip", (256, 256), alpha=0.1, blur_kernel=1)
    assert m.dtype == np.float32 and m.shape == (256, 256)
    want = np.ones((256, 256), np.float32)
    for y in range(84, 157):  # left edge x = 8, right edge from (43, 84) to (45, 156), boundary included
        right = int(np.floor(43 + (y - 84) * 2 / 72 + 0.5))
        want[y, 8:right + 1] = alpha
    assert np.array_equal(m, want)
    assert np.all(m[:84] == 1) and np.all(m[157:] == 1) and np.all(m[:, :8] == 1) and np.all(m[:, 46:] == 1)
    assert m[84, 43] == alpha and m[84, 44] == 1 and m[156, 45] == alpha and m[120, 44] == alpha


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 21, 31])
def test_blur_kernels_sum_to_one_and_are_symmetric(k):
    g = OC.gaussian_kernel(k)
    assert g.dtype == np.float32 and g.shape == (k,)
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 1e-7
    assert np.array_equal(g, g[::-1]) and np.all(g > 0) and int(np.argmax(g)) == k // 2
    if k == 3:
        assert g.tolist() == [0.25, 0.5, 0.25]
    if k == 5:
        assert g.tolist() == [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16]
    if k == 7:
        assert g[:4].tolist() == [0.03125, 0.109375, 0.21875, 0.28125]
    if k == 11:  # sigma = 0.3 * (5 - 1) + 0.8 = 2
        x = np.arange(11) - 5.0
        e = np.exp(-x * x / 8.0)
        assert np.array_equal(g, (e / e.sum()).astype(np.float32))


def test_an_even_blur_kernel_is_the_next_odd_one():
    for even in (2, 4, 10):
        a = OC.preset_mask("tongue", (84, 84), 0.2, even)
        assert np.array_equal(a, OC.preset_mask("tongue", (84, 84), 0.2, even + 1))
    assert np.array_equal(OC.preset_mask("lip", (68, 68), 0.2, 0), OC.preset_mask("lip", (68, 68), 0.2, 1))
    with pytest.raises(ValueError):
        OC.gaussian_kernel(4)


@pytest.mark.parametrize("shape,k", [((31, 33), 3), ((84, 84), 5), ((68, 104), 7), ((40, 36), 11), ((12, 9), 15)])
def test_blur_is_scipy_correlate1d_mirror_on_both_axes(shape, k):
    ndi = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(k).random(shape).astype(np.float32)
    got = OC.gaussian_blur(img, k)
    assert got.dtype == np.float32
    kern = OC.gaussian_kernel(k).astype(np.float64)
    want = ndi.correlate1d(ndi.correlate1d(img.astype(np.float64), kern, axis=1, mode="mirror"), kern, axis=0, mode="mirror")
    assert float(np.abs(got - want).max()) <= 1e-6


@pytest.mark.parametrize("shape", [(68, 68), (84, 84), (104, 68), (256, 256)])
@pytest.mark.parametrize("name", ["lip", "tongue"])
def test_presets_scale_and_stay_in_range(shape, name):
    for alpha, k in ((0.1, 11), (0.0, 5), (0.5, 1)):
        m = OC.preset_mask(name, shape, alpha, k)
        assert m.shape == shape and m.dtype == np.float32
        assert float(m.min()) >= np.float32(alpha) and float(m.max()) <= 1.0
        assert float(m.max()) == 1.0 and float(m.min()) < 0.5 * (1 + alpha)  # an untouched rest, a darkened core
        if k == 1:
            assert float(m.min()) == np.float32(alpha) and set(np.unique(m)) == {np.float32(alpha), np.float32(1)}
    # the darkened region scales with the frame: its centroid sits where the 256 x 256 one does
    hard = OC.preset_mask(name, shape, 0.0, 1) == 0
    ref = OC.preset_mask(name, (256, 256), 0.0, 1) == 0
    cy, cx = (np.argwhere(hard).mean(axis=0) + 0.5) / np.asarray(shape)
    ry, rx = (np.argwhere(ref).mean(axis=0) + 0.5) / 256
    assert abs(cy - ry) <= 1.5 / shape[0] and abs(cx - rx) <= 1.5 / shape[1]


def test_presets_are_the_reference_regions():
    assert set(OC.PRESETS) == {"lip", "tongue"}
    assert OC.PRESETS["lip"] == ((8.0, 84.0), (43.0, 84.0), (45.0, 156.0), (8.0, 156.0))
    assert OC.PRESETS["tongue"] == ((36.1, 102.7), (63.4, 90.9), (122.7, 111.5), (133.4, 172.2), (47.6, 155.0))


def test_custom_polygons(tmp_path):
    tri = [[2, 2], [20, 4], [8, 25]]
    (tmp_path / "tri.json").write_text(json.dumps(tri))
    m = OC.custom_mask(tmp_path / "tri.json", (32, 32), 0.25, 1)
    assert m[2, 2] == 0.25 and m[4, 20] == 0.25 and m[25, 8] == 0.25 and m[0, 0] == 1 and m[30, 30] == 1
    assert np.array_equal(m, OC.build_mask((32, 32), tri, 0.25, 1))
    # base_size scales like a preset
    (tmp_path / "lip.json").write_text(json.dumps({"points": OC.PRESETS["lip"], "base_size": [256, 256]}))
    assert np.array_equal(OC.custom_mask(tmp_path / "lip.json", (84, 84), 0.1, 11), OC.preset_mask("lip", (84, 84), 0.1, 11))
    for bad in ([[0, 0], [10, 10]], [[0, 0], [10, 0], [5, 2], [10, 10], [0, 10]], [[0, 0], [5, 5], [9, 9]], [[0, 0, 1]] * 3):
        with pytest.raises(ValueError):
            OC.build_mask((32, 32), bad, 0.1, 1)
        (tmp_path / "bad.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            OC.polygon_from_json(tmp_path / "bad.json")


def test_grid_masks_cover_the_frame():
    g = OC.grid_masks((37, 50), patch=12, stride=10, alpha=0.0, blur_kernel=0)
    pos = OC.grid_positions((37, 50), 12, 10)
    assert g.shape == (len(pos), 37, 50) == (4 * 5, 37, 50) and g.dtype == np.float32
    for m, (y, x) in zip(g, pos):
        want = np.ones((37, 50), np.float32)
        want[y:y + 12, x:x + 12] = 0
        assert np.array_equal(m, want)
    assert np.all((1 - g).sum(axis=0) >= 1)  # patch >= stride: every pixel is under at least one square
    soft = OC.grid_masks((32, 32), 8, 8, alpha=0.2, blur_kernel=5)
    assert soft.shape == (16, 32, 32) and float(soft.min()) == np.float32(0.2) and float(soft.max()) == 1.0


def test_apply_mask_host_is_the_reference_expression():
    rng = np.random.default_rng(3)
    for shape in ((4, 31, 33), (3, 31, 33, 3)):
        fr = rng.integers(0, 256, size=shape, dtype=np.uint8)
        mask = (rng.random((31, 33)) * 2.2 - 0.1).astype(np.float32)  # outside [0, 1] too: the clip handles it
        got = OC.apply_mask_host(fr, mask)
        assert np.array_equal(got, MR.apply_mask(fr, mask))
        assert np.array_equal(OC.apply_mask_host(fr, np.ones((31, 33), np.float32)), fr)
    assert np.array_equal(OC.apply_mask_host(np.full((1, 2, 2), 200, np.uint8), np.full((2, 2), 2.0, np.float32)),
                          np.full((1, 2, 2), 255, np.uint8))


# ------------------------------------------------------------------------------------------------- registered surface
def test_new_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(REPO, "include", "m2s.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int m2s_preprocess_frames_masked(const uint8_t* frames, int n, int h, int w, int channels, const float* masks, "
            "int n_masks, int out_h, int out_w, int interp, int norm, float* out, void* stream);") in flat
    assert ("int m2s_occlusion_reduce(const float* mel, int V, int T, int n_mels, const float* band_mask, int n_bands, "
            "const float* masks, int h, int w, int normalize, float* score, float* per_frame, float* map, "
            "void* stream);") in flat
    assert "#define M2S_ABI_VERSION 6" in src and "masks must be finite" in re.sub(r"[\s*]+", " ", src)
    L = N.lib()
    assert L.m2s_abi_version() == N.ABI_VERSION == 6
    for name, nargs in zip(NEW_SYMBOLS, (13, 14)):
        assert name in N.exported_symbols() and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
    mk = open(os.path.join(REPO, "mri-to-speech_amd", "csrc", "Makefile")).read()
    assert "occlusion.hip" in mk and "frames.hip" in mk


def test_ops_are_registered_with_fake_kernels():
    o = ops.load()
    assert ops.OCCLUSION_OPS == ("preprocess_frames_masked", "occlusion_reduce")
    assert ops.FRAME_OPS == ("preprocess_frames_resize",)  # the unmasked front end's census is untouched
    s = str(torch.ops.m2s.preprocess_frames_masked.default._schema)
    assert s.startswith("m2s::preprocess_frames_masked(Tensor frames, Tensor masks, int out_h, int out_w, int interp, int norm)")
    s = str(torch.ops.m2s.occlusion_reduce.default._schema)
    assert s.startswith("m2s::occlusion_reduce(Tensor mel, Tensor band_mask, Tensor? masks, bool normalize, bool want_per_frame)")
    meta = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device="meta")  # noqa: E731
    out = o.preprocess_frames_masked(meta(5, 84, 84, dt=torch.uint8), meta(3, 84, 84), 256, 256, 0, 0)
    assert out.shape == (3, 5, 256, 256) and out.dtype == torch.float32
    assert o.preprocess_frames_masked(meta(0, 31, 33, 3, dt=torch.uint8), meta(2, 31, 33), 64, 96, 1, 1).shape == (2, 0, 64, 96)
    sc, pf, mp = o.occlusion_reduce(meta(5, 7, 64), meta(2, 64), meta(4, 32, 40), True, True)
    assert sc.shape == (4, 3) and pf.shape == (4, 7, 3) and mp.shape == (3, 32, 40)
    sc, pf, mp = o.occlusion_reduce(meta(2, 1, 64), meta(0, 64), None, False, False)
    assert sc.shape == (1, 1) and pf.shape == (0, 1, 1) and mp.shape == (1, 0, 0)


def test_python_surface_refuses_before_the_device():
    from m2s import runtime
    from m2s.stream import AcousticStream, SpeechStream
    import inspect
    with pytest.raises(N.M2SError):
        runtime.preprocess_frames_masked(torch.zeros(1, 8, 8), np.ones((8, 8), np.float32))  # not uint8
    with pytest.raises(N.M2SError):
        runtime.preprocess_frames_masked(torch.zeros(1, 8, 8, dtype=torch.uint8), np.ones((8, 8), np.float32))  # on the host
    with pytest.raises(N.M2SError):
        OC.reduce(torch.zeros(2, 3, 64))
    assert inspect.signature(AcousticStream.push).parameters["masks"].default is None
    assert inspect.signature(SpeechStream.push).parameters["masks"].default is None
    sig = inspect.signature(runtime.Pipeline.occlusion)
    assert list(sig.parameters)[1:9] == ["frames_u8", "masks", "bands", "size", "interp", "norm", "windowed", "wav_variants"]
    bm, names = OC.band_matrix({"F1": [3, 4, 5], "one": [63]}, 64)
    assert names == ["F1", "one", "all"] and bm.shape == (2, 64) and bm.sum(dim=1).tolist() == [3.0, 1.0]
    with pytest.raises(ValueError):
        OC.band_matrix({f"b{i}": [i] for i in range(9)}, 64)


# ------------------------------------------------------------------------------------------------------ command lines
@pytest.mark.parametrize("script", ["mask_rtmri_video.py", "mri_occlusion.py"])
def test_command_lines_print_help(script):
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, script), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--mask-type", "--alpha", "--blur-kernel", "--mask-json"):
        assert flag in r.stdout
    if script == "mri_occlusion.py":
        assert "--grid" in r.stdout and "--formant-band" in r.stdout
    else:
        assert "--input" in r.stdout and "--output" in r.stdout


def _mask_cli():
    spec = importlib.util.spec_from_file_location("m2s_mask_cli", os.path.join(SCRIPTS, "mask_rtmri_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mask_cli_masks_a_npy_stack_to_the_reference_bytes(tmp_path, monkeypatch):
    cli = _mask_cli()
    monkeypatch.setattr(cli, "cv2", None)
    rng = np.random.default_rng(8)
    for name, shape in (("grey", (5, 84, 84)), ("bgr", (3, 68, 104, 3))):
        fr = rng.integers(0, 256, size=shape, dtype=np.uint8)
        np.save(tmp_path / f"{name}.npy", fr)
        for mtype in ("lip", "tongue"):
            out = tmp_path / "out" / f"{name}_{mtype}.npy"
            assert cli.main(["--input", str(tmp_path / f"{name}.npy"), "--output", str(out), "--mask-type", mtype,
                             "--alpha", "0.2", "--blur-kernel", "10"]) == 0
            got = np.load(out)
            want = MR.apply_mask(fr, OC.preset_mask(mtype, shape[1:3], 0.2, 11))
            assert got.dtype == np.uint8 and np.array_equal(got, want)
            assert (got != fr).any() and (got <= fr).all()
    (tmp_path / "tri.json").write_text(json.dumps([[10, 10], [60, 12], [30, 70]]))
    assert cli.main(["--input", str(tmp_path / "grey.npy"), "--output", str(tmp_path / "tri.npy"), "--mask-json",
                     str(tmp_path / "tri.json")]) == 0
    fr = np.load(tmp_path / "grey.npy")
    assert np.array_equal(np.load(tmp_path / "tri.npy"),
                          MR.apply_mask(fr, OC.build_mask((84, 84), [[10, 10], [60, 12], [30, 70]], 0.1, 11)))
    a = cli.parse_args(["--input", "i", "--output", "o"])  # the reference's defaults
    assert (a.mask_type, a.alpha, a.blur_kernel, a.mask_json) == ("lip", 0.1, 11, None)
    # a video file without OpenCV: a clear refusal, not a traceback from cv2
    (tmp_path / "clip.mp4").write_bytes(b"\0")
    with pytest.raises(SystemExit, match="OpenCV"):
        cli.main(["--input", str(tmp_path / "clip.mp4"), "--output", str(tmp_path / "o.mp4")])
