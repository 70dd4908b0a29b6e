"""The packed weight bytes, pinned on the CPU: tests/pack_digest.cpp runs the acoustic and generator packers
(csrc/pack_acoustic.cpp, pack_vocoder.cpp) on the synthetic state dicts and prints size and FNV-1a digest of
every arena; tests/golden/pack_digests.json holds the values of the engines before the packers were split out
of the constructors.  The order of the Arena::add calls is the arena layout, so a digest moves when any packed
byte or its place moves: a mismatch is a packing bug, not a reason to regenerate the file."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from m2s import _native, synth
from m2s.config import HIFIGAN_H

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mri-to-speech_amd", "csrc")
H_R2 = dict(HIFIGAN_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])  # tests/test_gpu_ragged.py


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _dump(path, state):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(state)))
        for k, v in state.items():
            a = np.ascontiguousarray(v, dtype="<f4")
            name = k.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<I", a.ndim))
            f.write(struct.pack("<%dq" % a.ndim, *a.shape))
            f.write(a.tobytes())


def _config(h):
    s = _native.hifigan_h(h)
    return ",".join(str(v) for v in (C.c_int * (C.sizeof(s) // C.sizeof(C.c_int))).from_buffer_copy(s))


@pytest.fixture(scope="module")
def digests(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the packer digest program cannot be built")
    if not os.path.exists(_native.LIB_PATH):
        raise _native.M2SError(f"{_native.LIB_PATH} is not built")
    d = tmp_path_factory.mktemp("pack")
    exe = str(d / "pack_digest")
    lib_dir = os.path.dirname(_native.LIB_PATH)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-I", CSRC, os.path.join(HERE, "pack_digest.cpp"), "-o", exe,
                    "-L", lib_dir, "-lm2s", "-Wl,-rpath," + lib_dir], check=True)
    _dump(d / "acoustic.bin", synth.synth_acoustic_state(seed=0))
    _dump(d / "generator.bin", synth.synth_generator_state(seed=0))
    _dump(d / "generator_r2.bin", synth.synth_generator_state(seed=0, h=H_R2))
    cmd = [exe, str(d / "acoustic.bin"), str(d / "generator.bin"), _config(HIFIGAN_H), str(d / "generator_r2.bin"),
           _config(H_R2)]
    return [json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout) for _ in range(2)]


def test_packed_arenas_match_the_pinned_digests(digests):
    with open(os.path.join(HERE, "golden", "pack_digests.json")) as f:
        want = json.load(f)["arenas"]
    assert sorted(digests[0]) == sorted(want)
    for name in want:
        print(name, digests[0][name])
    assert digests[0] == want


def test_packing_is_deterministic(digests):
    assert digests[0] == digests[1]
