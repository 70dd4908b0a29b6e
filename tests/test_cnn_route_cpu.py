"""The CNN's route table (csrc/cnn_route.hpp cnn_route), on the CPU: tests/cnn_route_dump.cpp prints, for a grid of
engines, switches and pass shapes, one record per backbone block; this file checks that every e4m3 hand-off has both
of its ends, spells the default table out by block, replays the committed launch-plan golden against it and compares
the split engines' routes with the bf16 ones.  Needs the library built (as tests/test_pack_cpu.py does) and no GPU.

The grid: the four dtypes; nc around the ir_ws (M2S_IRWS_MIN = 512 frames) and se_ws (one full round of 256- or
128-row tiles on 256 CUs: 256 frames at 16 x 16, 512 at 8 x 8) thresholds; 256 x 256 and 96 x 160, where most fused
kernels decline and blocks fall to the unfused legs; the defaults, each CNN route switch of switches.hpp alone, and
M2S_IRWS_MIN=0 M2S_SEWS_MIN=0 together.  512 x 256 is added for the hand-off check alone: there blocks.3.0 stores its
e4m3 depthwise output for an e4m3 SE GEMM while blocks.3.1 runs unfused and reads no e4m3 copy."""
import json
import os

import pytest

import cnn_route_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CUS = 256
NCS = (3, 255, 256, 511, 512, 1920)
SIZES = ((256, 256), (96, 160))
SHAPES = tuple((nc, h, w) for nc in NCS for h, w in SIZES) + ((3, 512, 256),)
# switches.hpp "CNN routes": name -> the value that flips its default
ROUTE_SWITCHES = {name: "0" for name in (
    "M2S_IR_FUSED", "M2S_IR_WS", "M2S_IR_WS_S2", "M2S_IRWS_F32", "M2S_STEM_FUSED", "M2S_F8_EXPAND", "M2S_F8_S2", "M2S_F8_ER",
    "M2S_ER8_X8", "M2S_F8_ER2", "M2S_SE_Y8", "M2S_SE_FUSED", "M2S_ER_FUSED", "M2S_SE_WS", "M2S_ER_MRG", "M2S_IR_S2BAND",
    "M2S_ER_S2_FUSED", "M2S_SEWS_REV")}
ROUTE_SWITCHES["M2S_SE_SP"] = "1"
PERSISTENT = {"M2S_IRWS_MIN": "0", "M2S_SEWS_MIN": "0"}
ENVS = [{}] + [{k: v} for k, v in sorted(ROUTE_SWITCHES.items())] + [PERSISTENT]


def _env_id(env):
    return "-".join(f"{k[4:]}={v}" for k, v in sorted(env.items())) or "defaults"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    p = ref.build(tmp_path_factory.mktemp("cnn_route"))
    if p is None:
        pytest.skip("hipcc not found: the route dump program cannot be built")
    return p


@pytest.fixture(scope="module")
def grid(prog):
    """grid(env, dtype, x8=True) -> {shape: table}, each engine's tables computed once."""
    cache = {}

    def get(env, dtype, x8=True):
        key = (_env_id(env), dtype, x8)
        if key not in cache:
            cache[key] = ref.tables(prog, dtype, CUS, SHAPES, env, x8)
        return cache[key]

    return get


# ---- 1. hand-offs


def check_handoffs(table, fp8, have_x8):
    for k, r in enumerate(table):
        where = (r["name"], r["nc"], r["H"], r["W"])
        prev_y8 = k > 0 and table[k - 1]["y8_out"]
        if r["y8_out"]:
            assert k + 1 < len(table) and table[k + 1]["x8_in"], where
            c = table[k + 1]
            # the stride the consumer reads: (N, H, W, 32) / (N, H, W, 64) bytes for er8_fused / er8w_fused, rows
            # of f8x_kp bytes for an e4m3 expand
            want = {"Er8": 32, "Er8w": 64}[c["er"]] if c["type"] == "er" else c["f8x_kp"]
            assert r["ld8"] == want and want > 0, where
        else:
            assert r["ld8"] == 0, where
        assert r["convert8"] == (r["type"] == "ir" and r["x8_in"] and not prev_y8), where
        if r["x8_in"] and not prev_y8:
            assert r["type"] == "ir" and r["convert8"] and r["er"] != "Er8w", where
        if r["type"] == "er" and r["er"] == "Er8w":
            assert r["x8_in"] and prev_y8, where  # er8w_fused has no other source for its operand
        if not fp8:
            assert not (r["x8_in"] or r["y8_out"] or r["convert8"] or r["f8"]), where
        if not have_x8:
            assert not (r["x8_in"] or r["y8_out"] or r["convert8"]), where


@pytest.mark.parametrize("env", ENVS, ids=_env_id)
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_handoffs_are_consistent(grid, dtype, env):
    for shape, table in grid(env, dtype).items():
        check_handoffs(table, dtype == "fp8", dtype == "fp8")
    if dtype == "fp8":
        # without the X8 buffers nothing is handed over; the e4m3 depthwise output into the e4m3 SE GEMM needs
        # none of them, so f8 (and with it every route) stays as it is except er8w_fused, which has no operand
        for shape, table in grid(env, dtype, x8=False).items():
            check_handoffs(table, True, False)
            for r, w in zip(table, grid(env, dtype)[shape]):
                assert r["f8"] == w["f8"] and (r["front"], r["se"], r["pwl"]) == (w["front"], w["se"], w["pwl"])
                assert r["er"] == w["er"] or (w["er"] == "Er8w" and r["er"] == "Er2"), (r["name"], shape)


# ---- 2. the default table at 256 x 256, by block

CN = ["cn"] * 2
IR_GRID = ["S2Band/Excite/Conv"] + ["Pwdw/Excite/Conv"] * 9 + ["PwdwS2/Excite/Conv"] + ["Pwdw/Excite/Conv"] * 9
IR_F8 = (["S2Band/Excite/SeGemmF8+f8+y8:128"] + ["Pwdw/Excite/SeWsF8+f8+x8+y8:128"] * 9 +
         ["PwdwS2/Excite/SeWsF8+f8+x8+y8:256"] + ["Pwdw/Excite/SeWsF8+f8+x8+y8:256"] * 8 + ["Pwdw/Excite/SeWsF8+f8+x8"])
ER_BF16 = ["Ers2", "Er", "Er", "Ers2", "Er2", "Er2"]
ER_SPLIT = ["Ers2Sp", "ErSp", "ErSp", "Unfused", "ErSp", "ErSp"]
ER_F8 = ["Ers2+y8:32", "Er8+x8+y8:32", "Er8+x8", "Ers2+y8:64", "Er8w+x8+y8:64", "Er8w+x8"]
UNFUSED = CN + ["Unfused"] * 6 + ["Unfused/Convs/Conv"] * 20
DEFAULT_TABLE = {
    ("fp32", 3): ("Stem", UNFUSED),
    ("fp32", 1920): ("Stem", UNFUSED),
    ("bf16", 3): ("StemB0", CN + ER_BF16 + IR_GRID),
    ("bf16", 1920): ("StemB0", CN + ER_BF16 + IR_GRID),
    ("bf16x3", 3): ("StemB0", CN + ER_SPLIT + IR_GRID),
    # the persistent kernels, from 512 frames (ir_ws) and a full round of se_ws tiles
    ("bf16x3", 1920): ("StemB0", CN + ER_SPLIT + ["S2Band/Excite/SeWs"] + ["IrWs/Excite/SeWs+f32"] * 9 +
                       ["IrWsS2/Excite/SeWs+f32"] + ["IrWs/Excite/SeWs+f32"] * 9),
    ("fp8", 3): ("StemB0", CN + ER_F8 + IR_F8),
    ("fp8", 1920): ("StemB0", CN + ER_F8 + IR_F8),
}


def spell(r):
    route = {"cn": "cn", "er": r["er"], "ir": "/".join((r["front"], r["se"], r["pwl"]))}[r["type"]]
    return (route + "+f8" * r["f8"] + "+x8" * r["x8_in"] + "+cv" * r["convert8"] +
            ("+y8:%d" % r["ld8"] if r["y8_out"] else "") + "+f32" * r["mid_f32"])


@pytest.mark.parametrize("dtype,nc", sorted(DEFAULT_TABLE))
def test_default_table(grid, dtype, nc):
    stem, want = DEFAULT_TABLE[dtype, nc]
    table = grid({}, dtype)[nc, 256, 256]
    assert len(want) == ref.N_BLOCKS
    assert table[0]["stem"] == stem
    for r, w in zip(table, want):
        assert spell(r) == w, r["name"]
    # the geometry a 256 x 256 frame gives: TF-SAME, only a stage's first block strides
    maps = [128] * 2 + [64] * 3 + [32] * 3 + [16] * 10 + [8] * 10
    for r, m, prev in zip(table, maps, [128] + maps):
        assert (r["oh"], r["ow"], r["nh"], r["nw"]) == (prev, prev, m, m), r["name"]
        assert (r["qt"], r["ql"]) == ((0, 0) if prev != m else (1, 1)), r["name"]


# ---- 3. the committed launch plan

GOLDEN_CASES = {"ac_forward_1x3_fp32": ("fp32", {}), "ac_forward_1x3_bf16": ("bf16", {}),
                "ac_forward_1x3_bf16x3": ("bf16x3", {}), "ac_forward_1x3_fp8": ("fp8", {}),
                "ac_forward_1x3_bf16x3_persistent": ("bf16x3", PERSISTENT),
                "ac_forward_1x3_bf16x3_persistent_ksplit1": ("bf16x3", dict(PERSISTENT, M2S_KSPLIT="1"))}


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_table_agrees_with_the_launch_plan_golden(prog, case):
    from tools import plan_dump
    dtype, env = GOLDEN_CASES[case]
    assert {c.name: c.env for c in plan_dump.CASES}[case] == env
    with open(os.path.join(HERE, "golden", "launch_plan.json")) as f:
        plan = plan_dump.decode(json.load(f))[case]
    names = [r["name"] for r in plan if r["stage"] == "cnn"]
    table = ref.tables(prog, dtype, CUS, [(3, 256, 256)], env)[3, 256, 256]
    assert ref.recorded(names) == ref.predicted(table)
    assert bool(ref.recorded(names)) == (dtype != "fp32")  # the fp32 engine runs no fused kernel


# ---- 4. the split engines against bf16

SPLIT_ONLY_FRONT = ("IrWs", "IrWsS2")  # the rungs gated on the split engine
SPLIT_ONLY_PWL = ("SeWs", "SeGemmSp")


@pytest.mark.parametrize("env", ENVS, ids=_env_id)
def test_split_engines_route_like_bf16(grid, env):
    for shape, split in grid(env, "bf16x3").items():
        bf16, f32 = grid(env, "bf16")[shape], grid(env, "fp32")[shape]
        assert split[0]["stem"] == bf16[0]["stem"]
        for s, b, f in zip(split, bf16, f32):
            where = (s["name"], shape)
            assert s["se"] == b["se"], where
            assert s["front"] == b["front"] or s["front"] in SPLIT_ONLY_FRONT, where
            assert s["pwl"] == b["pwl"] or s["pwl"] in SPLIT_ONLY_PWL, where
            assert b["front"] not in SPLIT_ONLY_FRONT and b["pwl"] == "Conv", where
            assert s["er"] in ("ErSp", "Ers2Sp", "Unfused") and b["er"] in ("Er", "Er2", "Ers2", "Unfused"), where
            # the fp32 engine has no fused kernel at all
            assert (f["stem"], f["er"], f["front"], f["se"], f["pwl"]) == ("Stem", "Unfused", "Unfused", "Convs", "Conv"), where
