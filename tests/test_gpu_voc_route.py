"""The vocoder's route table against what an engine launches: for the switches and the config that the twelve
voc_forward_* cases of tests/golden/launch_plan.json do not hold (tools/plan_dump.py VOC_ROUTE_CASES), the MRF kernels
one generator forward of 1 x 8 mel frames records under each mrf_c* stage, in order, are the ones
tests/voc_route_dump.cpp predicts under the same switches, and the waveform is finite.
tests/test_voc_route_cpu.py checks the table itself."""
import pytest
import torch

import voc_route_ref as ref
from m2s import _native, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = [(dtype, env, h or "h") for _, dtype, env, h in ref.plan_dump.VOC_ROUTE_CASES]


def _id(case):
    dtype, env, config = case
    return "-".join([dtype] + [f"{k[4:]}={v}" for k, v in sorted(env.items())] + [config])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    p = ref.build(tmp_path_factory.mktemp("voc_route"))
    if p is None:
        pytest.skip("hipcc not found: the route dump program cannot be built")
    return p


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_launches_what_the_table_predicts(prog, monkeypatch, case):
    from m2s import runtime
    dtype, env, config = case
    h = ref.CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the engine is created
    eng = runtime.VocoderEngine(synth.synth_generator_state(12, h), h, dtype=dtype, device=DEV)
    mel = torch.from_numpy(synth.synth_mel_log(1, h["num_mels"], 8, seed=3)).to(DEV)
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        wav = eng.forward(mel)
        torch.cuda.synchronize()
        launches = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    assert wav.numel() == 8 * eng.hop and torch.isfinite(wav).all()
    rows = ref.table(prog, config, dtype, env)
    print(_id(case), ref.recorded(launches))
    ref.check_launches(rows, h, launches)
