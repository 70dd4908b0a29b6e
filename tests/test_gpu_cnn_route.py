"""The CNN's route table against what an engine launches: for the switches and sizes tests/golden/launch_plan.json does
not hold, the fused kernels one acoustic forward of 1 x 3 frames records under stage "cnn" (in order, with the "also
stores an e4m3 copy" template flags of er8w_fused and ers2_fused) are the ones tests/cnn_route_dump.cpp predicts for
nc = 3 on this device's CU count under the same switches.  tests/test_cnn_route_cpu.py checks the table itself."""
import pytest
import torch

import cnn_route_ref as ref
from m2s import _native, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

CASES = (
    # fp8, each e4m3 hand-off switch off alone
    [("fp8", {name: "0"}, (256, 256)) for name in ("M2S_ER8_X8", "M2S_SE_Y8", "M2S_F8_ER2", "M2S_F8_S2", "M2S_F8_EXPAND")]
    # 96 x 160: several *_supported predicates turn false and blocks fall to the unfused legs
    + [("fp8", {}, (96, 160)), ("bf16x3", {}, (96, 160))]
    # the persistent kernels at any pass size, the stride-2 block off ir_ws
    + [("bf16x3", {"M2S_IRWS_MIN": "0", "M2S_SEWS_MIN": "0", "M2S_IR_WS_S2": "0"}, (256, 256))]
)


def _id(case):
    dtype, env, (h, w) = case
    return "-".join([dtype] + [f"{k[4:]}={v}" for k, v in sorted(env.items())] + [f"{h}x{w}"])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    p = ref.build(tmp_path_factory.mktemp("cnn_route"))
    if p is None:
        pytest.skip("hipcc not found: the route dump program cannot be built")
    return p


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_launches_what_the_table_predicts(prog, monkeypatch, case):
    from m2s import runtime
    dtype, env, (h, w) = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the engine is created
    eng = runtime.AcousticEngine(synth.synth_acoustic_state(11), dtype=dtype, device=DEV)
    frames = torch.from_numpy(synth.synth_frames(1, 3, hw=(h, w), seed=5)).to(DEV)
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        out = eng.forward(frames)
        torch.cuda.synchronize()
        launches = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    eng.check()
    assert torch.isfinite(out).all()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table = ref.tables(prog, dtype, cus, [(3, h, w)], env)[3, h, w]
    got = ref.recorded([r["name"] for r in launches if r["stage"] == "cnn"])
    print(_id(case), got)
    assert got == ref.predicted(table)
    assert got, "the pass recorded no fused kernel"
