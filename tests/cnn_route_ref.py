"""Shared by tests/test_cnn_route_cpu.py and tests/test_gpu_cnn_route.py: builds and runs tests/cnn_route_dump.cpp (the
CNN's route table, csrc/cnn_route.hpp, as JSON lines) and turns a table, or a list of recorded launch names, into the
ordered list of fused-kernel records both are compared by."""
import json
import os
import subprocess

from m2s import _native, synth
from test_pack_cpu import _dump, _hipcc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")
DTYPES = ("fp32", "bf16", "bf16x3", "fp8")  # include/m2s.h m2s_dtype order
N_BLOCKS = 28

# the fused kernels' launch-record prefixes (the text before the template arguments), in no order
FUSED = {"stem_b0_kernel", "er_sp_kernel", "ers2_sp_kernel", "er8_fused_kernel", "er_fused_kernel", "er8w_fused_kernel",
         "er2_fused_kernel", "ers2_fused_kernel", "ir_ws_kernel", "ir_pwdw_kernel", "ir_pwdw_s2_kernel", "ir_s2band_kernel",
         "se_excite_kernel", "se_ws_kernel"}
# ... of which these two carry "also stores an e4m3 copy" as their last template argument
COPY_FLAG = {"er8w_fused_kernel", "ers2_fused_kernel"}


def build(tmp_dir):
    """(dump program, synthetic acoustic state dump) in tmp_dir, or None without hipcc."""
    hipcc = _hipcc()
    if hipcc is None:
        return None
    if not os.path.exists(_native.LIB_PATH):
        raise _native.M2SError(f"{_native.LIB_PATH} is not built")
    exe, lib_dir = str(tmp_dir / "cnn_route_dump"), os.path.dirname(_native.LIB_PATH)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cnn_route_dump.cpp"),
                    "-o", exe, "-L", lib_dir, "-lm2s", "-Wl,-rpath," + lib_dir], check=True)
    _dump(tmp_dir / "acoustic.bin", synth.synth_acoustic_state(seed=0))
    return exe, str(tmp_dir / "acoustic.bin")


def tables(prog, dtype, cus, shapes, env=None, x8=True):
    """{(nc, H, W): [28 block records]} of an engine of `dtype` created under the M2S_* switches `env`."""
    exe, state = prog
    base = {k: v for k, v in os.environ.items() if not k.startswith("M2S_")}
    argv = [exe, state, str(DTYPES.index(dtype)), str(cus), str(int(x8))] + ["%dx%dx%d" % s for s in shapes]
    out = subprocess.run(argv, env=dict(base, **(env or {})), check=True, capture_output=True, text=True).stdout
    rows = [json.loads(line) for line in out.splitlines()]
    assert len(rows) == N_BLOCKS * len(shapes)
    got = {s: rows[i * N_BLOCKS:(i + 1) * N_BLOCKS] for i, s in enumerate(shapes)}
    for s, t in got.items():
        assert [(r["nc"], r["H"], r["W"], r["block"]) for r in t] == [s + (k,) for k in range(N_BLOCKS)]
    return got


def predicted(table):
    """The fused-kernel records a pass on this table launches, in order: (prefix, copy flag or None)."""
    out = []
    fused_front = table[0]["stem"] == "StemB0"
    if fused_front:
        out.append(("stem_b0_kernel", None))
    for r in table[2 if fused_front else 0:]:
        if r["record"]:
            out.append((r["record"], r["y8_out"] if r["record"] in COPY_FLAG else None))
        if r["type"] == "ir":
            if r["se"] == "Excite":
                out.append(("se_excite_kernel", None))
            if r["pwl"] in ("SeWsF8", "SeWs"):
                out.append(("se_ws_kernel", None))
    return out


def recorded(names):
    """The same list from the launch-record names of one CNN pass."""
    out = []
    for name in names:
        prefix, _, args = name.partition("<")
        if prefix in FUSED:
            flag = None
            if prefix in COPY_FLAG:
                flag = args.rstrip(">").split(",")[-1].strip()
                assert flag in ("true", "false"), name
            out.append((prefix, None if flag is None else flag == "true"))
    return out
