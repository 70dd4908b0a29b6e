"""Shared by tests/test_voc_route_cpu.py and tests/test_gpu_voc_route.py: builds and runs tests/voc_route_dump.cpp (the
vocoder's route table, csrc/voc_route.hpp, as JSON lines) and turns a table, or the launch records of one generator
call, into the per-stage lists of MRF kernel records both are compared by."""
import json
import os
import subprocess

from m2s import _native, synth
from m2s.config import HIFIGAN_H
from test_pack_cpu import H_R2, _config, _dump, _hipcc
from tools import plan_dump  # noqa: F401  (VOC_ROUTE_CASES, the golden's decode)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")
DTYPES = ("fp32", "bf16", "bf16x3", "fp8")  # include/m2s.h m2s_dtype order

CONFIGS = {
    "h": HIFIGAN_H,
    "r2": H_R2,  # resblock "2": one conv per dilation, nothing fused, nothing batched
    # tests/test_gpu_mrf_pair.py H_REACH: the k = 13, d = 5 pair reaches 72 > 64 rows back
    "reach": dict(HIFIGAN_H, resblock_kernel_sizes=[3, 7, 13]),
    # the kernel sizes differ in their dilation counts: no stage batches its resblocks
    "mixed": dict(HIFIGAN_H, resblock_dilation_sizes=[[1, 3, 5], [1, 3], [1, 3, 5]]),
}

# the launch-record prefixes (the text before the template arguments) of the kernels an MRF conv can run on; the
# stage's other records (conv_gemm_ksum_kernel of a split-K conv, lrelu_e4m3_kernel) are not counted
MRF_KERNELS = {"conv1d_halo_pair_kernel", "conv1d_halo_sp_kernel", "conv_gemm_kernel", "gemm128_kernel", "rb1_fused_kernel",
               "conv_igemm_kernel"}


def build(tmp_dir):
    """(dump program, {config name: (state dump, config csv)}) in tmp_dir, or None without hipcc."""
    hipcc = _hipcc()
    if hipcc is None:
        return None
    if not os.path.exists(_native.LIB_PATH):
        raise _native.M2SError(f"{_native.LIB_PATH} is not built")
    exe, lib_dir = str(tmp_dir / "voc_route_dump"), os.path.dirname(_native.LIB_PATH)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "voc_route_dump.cpp"),
                    "-o", exe, "-L", lib_dir, "-lm2s", "-Wl,-rpath," + lib_dir], check=True)
    states = {}
    for name, h in CONFIGS.items():
        _dump(tmp_dir / f"gen_{name}.bin", synth.synth_generator_state(seed=0, h=h))
        states[name] = (str(tmp_dir / f"gen_{name}.bin"), _config(h))
    return exe, states


def table(prog, config, dtype, env=None):
    """[one record per upsampling stage] of a `dtype` engine for CONFIGS[config] created under the switches `env`."""
    exe, states = prog
    base = {k: v for k, v in os.environ.items() if not k.startswith("M2S_")}
    argv = [exe, *states[config], str(DTYPES.index(dtype))]
    out = subprocess.run(argv, env=dict(base, **(env or {})), check=True, capture_output=True, text=True).stdout
    rows = [json.loads(line) for line in out.splitlines()]
    assert [r["stage"] for r in rows] == list(range(len(CONFIGS[config]["upsample_rates"])))
    return rows


def predicted(rows, h):
    """{stage tag: [acceptable lists of MRF kernel prefixes, in launch order]} for one generator call.  The table
    does not depend on the call's shape, and only a Pair stage's launch count does: its last pairs run in one chained
    launch where chain_wanted and the pass fills the device (csrc/voc_route.hpp), so such a stage has two lists."""
    nk, res1 = len(h["resblock_kernel_sizes"]), h["resblock"] == "1"
    nps = [len(d) for d in h["resblock_dilation_sizes"]]
    out = {}
    for r in rows:
        if r["mrf"] == "Pair":  # a launch per pair but the last, then the last pairs: one per resblock, or chained
            want = [[r["record"]] * (nps[0] - 1 + n) for n in ([nk, 1] if r["chain_wanted"] else [nk])]
        elif r["mrf"] in ("HaloBatched", "GemmBatched"):  # c1 and c2 of each pair; the last c2 one per resblock
            want = [[r["record"]] * (2 * nps[0] - 1 + nk)]
        elif r["mrf"] == "F8":
            want = [[r["record"]] * (2 * sum(nps))]
        else:
            assert r["mrf"] == "PerResblock" and len(r["rb"]) == nk
            want = [[rec for route, rec, n in zip(r["rb"], r["rb_record"], nps)
                     for _ in range(1 if route == "Fused" else (2 if res1 else 1) * n)]]
        out["mrf_c%d" % r["C"]] = want
    return out


def recorded(launches):
    """{stage tag: [MRF kernel prefixes, in launch order]} from one call's launch records."""
    out = {}
    for r in launches:
        prefix = r["name"].partition("<")[0]
        if r["stage"].startswith("mrf_c"):
            out.setdefault(r["stage"], [])
            if prefix in MRF_KERNELS:
                out[r["stage"]].append(prefix)
    return out


def check_launches(rows, h, launches):
    want, got = predicted(rows, h), recorded(launches)
    assert sorted(got) == sorted(want)
    for tag in want:
        assert got[tag] in want[tag], (tag, got[tag], want[tag])
