"""The vocoder's route table (csrc/voc_route.hpp voc_pack_wants, voc_route), on the CPU: tests/voc_route_dump.cpp
prints, for a grid of configs, engines and switches, one record per upsampling stage; this file checks that every
LeakyReLU hand-off has both of its ends and every route the copies it reads, spells the default table out by stage,
and replays the committed launch-plan golden against it.  Needs the library built (as tests/test_pack_cpu.py does)
and no GPU.

The grid: the four configs of voc_route_ref.CONFIGS x the four dtypes x the defaults, each vocoder switch of
switches.hpp flipped alone, and three combinations whose halves interact (M2S_MRF_HALO=0 keeps the C = 128 fragments
M2S_MRF_PAIR128=1 packs from every route; M2S_F8_MRF64=1 sends the C = 64 stage to e4m3 whatever M2S_MRF_FUSED says;
both e4m3 switches together)."""
import json
import os

import pytest

import voc_route_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
# switches.hpp "vocoder": name -> the value that flips its default
ROUTE_SWITCHES = {"M2S_MRF_FUSED": "0", "M2S_MRF_BATCH": "0", "M2S_MRF_HALO": "0", "M2S_MRF_PAIR": "0", "M2S_MRF_CHAIN": "0",
                  "M2S_MRF_PAIR128": "1", "M2S_F8_MRF64": "1", "M2S_F8_MRF32": "1"}
COMBINATIONS = [{"M2S_MRF_HALO": "0", "M2S_MRF_PAIR128": "1"}, {"M2S_F8_MRF64": "1", "M2S_MRF_FUSED": "0"},
                {"M2S_F8_MRF64": "1", "M2S_F8_MRF32": "1"}]
ENVS = [{}] + [{k: v} for k, v in sorted(ROUTE_SWITCHES.items())] + COMBINATIONS
BATCHED = ("Pair", "HaloBatched", "GemmBatched")


def _env_id(env):
    return "-".join(f"{k[4:]}={v}" for k, v in sorted(env.items())) or "defaults"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    p = ref.build(tmp_path_factory.mktemp("voc_route"))
    if p is None:
        pytest.skip("hipcc not found: the route dump program cannot be built")
    return p


@pytest.fixture(scope="module")
def grid(prog):
    """grid(config, dtype, env) -> table, each computed once."""
    cache = {}

    def get(config, dtype, env):
        key = (config, dtype, _env_id(env))
        if key not in cache:
            cache[key] = ref.table(prog, config, dtype, env)
        return cache[key]

    return get


# ---- 1. hand-offs, and the copies a route reads


def check_table(rows, dtype):
    for i, r in enumerate(rows):
        where = (i, r)
        # the producer's epilogue and the consumer's operand transform agree
        assert r["in_act"] == (rows[i - 1]["mrf_act_out"] if i else r["pre_act_out"]), where
        assert r["pre_act_out"] == (dtype == "bf16x3"), where
        assert r["ups_act_out"] == (r["mrf"] in BATCHED), where
        # only a batched stage can store lrelu(S), and does wherever an upsampler follows
        assert r["mrf_act_out"] == (r["mrf"] in BATCHED and i + 1 < len(rows)), where
        if dtype != "bf16x3":
            assert r["mrf"] not in BATCHED and not (r["in_act"] or r["ups_act_out"] or r["mrf_act_out"]), where
        assert (r["mrf"] == "F8") <= (dtype == "fp8"), where
        assert r["chain_wanted"] <= (r["mrf"] == "Pair"), where
        # the packer staged what voc_pack_wants said, and every route has the copies its kernel reads
        assert r["packed"] == r["wants"], where
        need = {"Pair": "h", "HaloBatched": "h", "F8": "q"}.get(r["mrf"])
        assert all(need is None or need in w for w in r["wants"]), where
        if r["mrf"] == "PerResblock":
            assert all("f" in w for w, route in zip(r["wants"], r["rb"]) if route == "Fused"), where
            assert bool(r["rb"]) and not r["record"], where
        else:
            assert r["record"] and not r["rb"] and not r["rb_record"], where


@pytest.mark.parametrize("env", ENVS, ids=_env_id)
@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("config", sorted(ref.CONFIGS))
def test_handoffs_are_consistent(grid, config, dtype, env):
    check_table(grid(config, dtype, env), dtype)


# ---- 2. the default table for HIFIGAN_H, by stage (C = 256, 128, 64, 32)

CONVS, FUSED = "PerResblock[Convs,Convs,Convs]", "PerResblock[Fused,Fused,Fused]"
DEFAULT_TABLE = {
    "fp32": [CONVS] * 4,
    "bf16": [CONVS, CONVS, FUSED, FUSED],
    # conv_pre and every batched stage store lrelu for the upsampler that follows; the fused C = 32 stage reads raw x
    "bf16x3": ["GemmBatched+in+ups+out", "GemmBatched+in+ups+out", "Pair+chain+in+ups+out", FUSED + "+in"],
    "fp8": ["F8", "F8", FUSED, FUSED],
}


def spell(r):
    route = r["mrf"] + ("[%s]" % ",".join(r["rb"]) if r["rb"] else "")
    return route + "+chain" * r["chain_wanted"] + "+in" * r["in_act"] + "+ups" * r["ups_act_out"] + "+out" * r["mrf_act_out"]


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_default_table(grid, dtype):
    rows = grid("h", dtype, {})
    assert [r["C"] for r in rows] == [256, 128, 64, 32]
    assert [spell(r) for r in rows] == DEFAULT_TABLE[dtype]
    assert rows[0]["pre_act_out"] == (dtype == "bf16x3")


def test_other_configs_and_switches(grid):
    """What the issue's configs and combinations are in the grid for."""
    # resblock "2" and unequal dilation counts: nothing batches, nothing is fused or e4m3 (resblock "2") / the
    # split engine falls to run_conv pairs and the fused C = 32 kernel (unequal counts)
    for dtype in ref.DTYPES:
        assert [spell(r) for r in grid("r2", dtype, {})] == [CONVS + "+in" * (dtype == "bf16x3")] + [CONVS] * 3
    assert [spell(r) for r in grid("mixed", "bf16x3", {})] == [CONVS + "+in"] + [CONVS] * 2 + [FUSED]
    # one pair out of the pair kernel's reach: the C = 64 stage as a whole on the launches per conv
    assert [spell(r) for r in grid("reach", "bf16x3", {})][2] == "HaloBatched+in+ups+out"
    # C = 128 on the pair kernel; without M2S_MRF_HALO the fragments stay packed and nothing reads them
    assert [r["mrf"] for r in grid("h", "bf16x3", {"M2S_MRF_PAIR128": "1"})] == ["GemmBatched", "Pair", "Pair", "PerResblock"]
    rows = grid("h", "bf16x3", COMBINATIONS[0])
    assert [r["mrf"] for r in rows] == ["GemmBatched"] * 3 + ["PerResblock"] and rows[1]["wants"] == ["h"] * 3
    # fp8, C = 64 on e4m3: with or without the fused kernel's switch, beside its unread fragments
    for env in ({"M2S_F8_MRF64": "1"}, COMBINATIONS[1]):
        rows = grid("h", "fp8", env)
        assert [r["mrf"] for r in rows] == ["F8"] * 3 + ["PerResblock"] and rows[2]["wants"] == ["fq"] * 3
    assert [r["mrf"] for r in grid("h", "fp8", COMBINATIONS[2])] == ["F8"] * 4
    # M2S_MRF_FUSED=0: the split C = 32 stage batches on conv_gemm, so conv_post's input is the last hand-off's end
    rows = grid("h", "bf16x3", {"M2S_MRF_FUSED": "0"})
    assert [spell(r) for r in rows][3] == "GemmBatched+in+ups" and rows[3]["wants"] == ["f"] * 3


# ---- 3. the committed launch plan

GOLDEN_CASES = {
    "voc_forward_1x8_fp32": ("fp32", {}), "voc_forward_1x8_bf16": ("bf16", {}), "voc_forward_1x8_bf16x3": ("bf16x3", {}),
    "voc_forward_1x8_fp8": ("fp8", {}), "voc_forward_2x40_bf16x3": ("bf16x3", {}),
    "voc_forward_1x8_bf16x3_pair128": ("bf16x3", {"M2S_MRF_PAIR128": "1"}),
    "voc_forward_1x8_bf16x3_nopair": ("bf16x3", {"M2S_MRF_PAIR": "0"}),
    "voc_forward_1x8_bf16x3_nohalo": ("bf16x3", {"M2S_MRF_HALO": "0"}),
    "voc_forward_1x8_fp8_mrf64": ("fp8", {"M2S_F8_MRF64": "1"}),
    # ragged and chunk calls: masks and crops run between the stages, the MRF launches are the dense call's (the
    # route is the engine's, not the call's)
    "voc_forward_ragged_8_5": ("bf16x3", {}), "voc_forward_chunk_cone": ("bf16x3", {}),
    "voc_forward_chunk_zeros": ("bf16x3", {}),
}
# ... and the seven cases of the routes those twelve do not take (tools/plan_dump.py VOC_ROUTE_CASES)
MORE_CASES = {"voc_forward_1x8_" + name: (h or "h", dtype, env) for name, dtype, env, h in ref.plan_dump.VOC_ROUTE_CASES}
ALL_CASES = dict({k: ("h",) + v for k, v in GOLDEN_CASES.items()}, **MORE_CASES)


@pytest.mark.parametrize("case", sorted(ALL_CASES))
def test_table_agrees_with_the_launch_plan_golden(grid, case):
    plan_dump = ref.plan_dump
    config, dtype, env = ALL_CASES[case]
    assert len(GOLDEN_CASES) == 12 and len(MORE_CASES) == 7
    assert sorted(ALL_CASES) == sorted(c.name for c in plan_dump.CASES if c.name.startswith("voc_forward_"))
    assert {c.name: c.env for c in plan_dump.CASES}[case] == env
    with open(os.path.join(HERE, "golden", "launch_plan.json")) as f:
        plan = plan_dump.decode(json.load(f))[case]
    ref.check_launches(grid(config, dtype, env), ref.CONFIGS[config], plan)
