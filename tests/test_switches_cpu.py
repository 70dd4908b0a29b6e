"""The M2S_* switch table (csrc/switches.hpp), on the CPU: tests/switches_dump.cpp prints Switches::from_env() of
its environment as JSON and this file runs it under chosen environments.  It holds its own copy of the defaults
 and of the variable names, so a changed default, a changed parsing rule, or a switch read but not
listed (or listed but not read) fails here."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")

# variable -> (member, default): DESIGN.md §28
FLAGS = {
    "M2S_IR_FUSED": ("ir_fused", 1), "M2S_IR_WS": ("ir_ws", 1), "M2S_IR_WS_S2": ("ir_ws_s2", 1),
    "M2S_IRWS_F32": ("irws_f32", 1), "M2S_STEM_FUSED": ("stem_fused", 1), "M2S_F8_EXPAND": ("f8_expand", 1),
    "M2S_F8_S2": ("f8_s2", 1), "M2S_F8_ER": ("f8_er", 1), "M2S_ER8_X8": ("er8_x8", 1), "M2S_F8_ER2": ("f8_er2", 1),
    "M2S_SE_Y8": ("se_y8", 1), "M2S_SE_FUSED": ("se_fused", 1), "M2S_ER_FUSED": ("er_fused", 1),
    "M2S_SE_WS": ("se_ws", 1), "M2S_SE_SP": ("se_sp", 0), "M2S_ER_MRG": ("er_mrg", 1),
    "M2S_IR_S2BAND": ("ir_s2band", 1), "M2S_ER_S2_FUSED": ("er_s2_fused", 1), "M2S_SEWS_REV": ("sews_rev", 1),
    "M2S_LSTM_PERSISTENT": ("lstm_persistent", 1), "M2S_LSTM_MID": ("lstm_mid", 1), "M2S_LSTM_X3": ("lstm_x3", 1),
    "M2S_LSTM_X3G": ("lstm_x3g", 1),
    "M2S_MRF_FUSED": ("mrf_fused", 1), "M2S_MRF_BATCH": ("mrf_batch", 1), "M2S_MRF_HALO": ("mrf_halo", 1),
    "M2S_F8_MRF64": ("f8_mrf64", 0), "M2S_F8_MRF32": ("f8_mrf32", 0), "M2S_MRF_PAIR": ("mrf_pair", 1),
    "M2S_MRF_CHAIN": ("mrf_chain", 1), "M2S_MRF_PAIR128": ("mrf_pair128", 0),
}
VALUES = {
    "M2S_IRWS_MIN": ("irws_min", 512), "M2S_SEWS_MIN": ("sews_min_cus", 1), "M2S_IRWS_PARTS": ("irws_parts", 0),
    "M2S_STEM_PARTS": ("stem_parts", 0), "M2S_SEWS_HALF": ("sews_half", 0), "M2S_SE_WS_CFG": ("se_ws_cfg", 0),
    "M2S_SE_SP_WAVES": ("se_sp_waves", 8), "M2S_LSTM_SMALL_B": ("lstm_small_b", 4),
    "M2S_LSTM_MID_CH": ("lstm_mid_ch", 0), "M2S_KSPLIT": ("conv.ksplit", 0), "M2S_KSPLIT_MAX": ("conv.ksplit_max", 8),
    "M2S_KSPLIT_MINST": ("conv.ksplit_minst", 4), "M2S_CG_BN64": ("conv.bn64", 0), "M2S_CG_STAGES": ("conv.stages", 0),
}
DEFAULTS = {member: default for member, default in list(FLAGS.values()) + list(VALUES.values())}


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host compiler and no hipcc: the switch dump program cannot be built")
    exe = str(tmp_path_factory.mktemp("switches") / "switches_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "switches_dump.cpp"),
                    "-o", exe], check=True)
    base = {k: v for k, v in os.environ.items() if not k.startswith("M2S_")}

    def run(**env):
        out = subprocess.run([exe], env=dict(base, **env), check=True, capture_output=True, text=True).stdout
        return json.loads(out)

    return run


def test_defaults_with_no_switch_set(dump):
    assert dump()["values"] == DEFAULTS


def test_from_env_reads_exactly_the_listed_names_once_each(dump):
    names = dump()["names"]
    assert len(names) == len(set(names))
    assert sorted(names) == sorted(list(FLAGS) + list(VALUES))


@pytest.mark.parametrize("name", sorted(FLAGS))
def test_flag_rule(dump, name):
    """unset: the default; "0": off; anything else, the empty string too: on.  Nothing else moves."""
    member = FLAGS[name][0]
    for text, want in (("0", 0), ("1", 1), ("", 1), ("00", 1), ("off", 1)):
        assert dump(**{name: text})["values"] == dict(DEFAULTS, **{member: want}), (name, text)


# (variable, text) -> value of its member
RULES = [
    ("M2S_IRWS_MIN", "0", 0), ("M2S_IRWS_MIN", "64", 64), ("M2S_IRWS_MIN", "x", 0),  # atoi
    ("M2S_SEWS_MIN", "0", 0), ("M2S_SEWS_MIN", "3", 3),
    ("M2S_KSPLIT", "1", 1), ("M2S_KSPLIT", "6", 6), ("M2S_KSPLIT", "", 0),  # > 0 forces (conv_gemm.hip plan_ksplit)
    ("M2S_KSPLIT_MAX", "0", 1), ("M2S_KSPLIT_MAX", "-4", 1), ("M2S_KSPLIT_MAX", "16", 16), ("M2S_KSPLIT_MAX", "", 1),
    ("M2S_KSPLIT_MINST", "0", 1), ("M2S_KSPLIT_MINST", "2", 2),
    ("M2S_IRWS_PARTS", "3", 3), ("M2S_IRWS_PARTS", "0", 0),  # > 0 forces (ir_ws.hip launch_ir_ws)
    # set: atoi, which launch_stem_b0 clamps to 1 .. tiles_y, so a set value below 1 means 1; 0 is "unset"
    ("M2S_STEM_PARTS", "2", 2), ("M2S_STEM_PARTS", "0", 1), ("M2S_STEM_PARTS", "-3", 1), ("M2S_STEM_PARTS", "", 1),
    ("M2S_SEWS_HALF", "1", 1), ("M2S_SEWS_HALF", "2", 0), ("M2S_SEWS_HALF", "0", 0), ("M2S_SEWS_HALF", "", 0),
    ("M2S_SE_WS_CFG", "3", 3), ("M2S_SE_WS_CFG", "", 0),
    ("M2S_SE_SP_WAVES", "4", 4), ("M2S_SE_SP_WAVES", "2", 8), ("M2S_SE_SP_WAVES", "8", 8),
    ("M2S_LSTM_SMALL_B", "8", 8), ("M2S_LSTM_SMALL_B", "7", 4), ("M2S_LSTM_SMALL_B", "4", 4),
    ("M2S_LSTM_MID_CH", "4", 4), ("M2S_LSTM_MID_CH", "8", 8), ("M2S_LSTM_MID_CH", "16", 16), ("M2S_LSTM_MID_CH", "5", 0),
    ("M2S_CG_BN64", "1", 1), ("M2S_CG_BN64", "2", 0), ("M2S_CG_BN64", "", 0),
    ("M2S_CG_STAGES", "3", 3), ("M2S_CG_STAGES", "4", 4), ("M2S_CG_STAGES", "0", 0),
]


@pytest.mark.parametrize("name,text,want", RULES)
def test_value_rule(dump, name, text, want):
    assert dump(**{name: text})["values"] == dict(DEFAULTS, **{VALUES[name][0]: want})


def test_switches_are_independent(dump):
    got = dump(M2S_KSPLIT="1", M2S_IR_WS="0", M2S_MRF_PAIR128="1", M2S_LSTM_SMALL_B="8")["values"]
    assert got == dict(DEFAULTS, **{"conv.ksplit": 1, "ir_ws": 0, "mrf_pair128": 1, "lstm_small_b": 8})
