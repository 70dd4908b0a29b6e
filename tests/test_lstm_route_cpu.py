"""Which recurrence kernel a BiLSTM call runs (csrc/lstm_route.hpp lstm_plan), on the CPU: tests/lstm_route_dump.cpp
prints the plan of a grid of calls and this file holds its own statement of the ladder, so a changed
limit, a reordered rung or a changed record name fails here, at every batch size where the route changes (the GPU
suite reaches B = 2, 5 and 17 only, by kernel name)."""
import json
import os
import subprocess

import pytest

from test_switches_cpu import _compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")

BS = (1, 4, 5, 8, 9, 16, 17, 64, 65)
HS = (640, 512)
F32, BF16, BF16X3, FP8 = 0, 1, 2, 3  # include/m2s.h m2s_dtype
DEFAULTS = dict(persistent=1, mid=1, x3=1, x3g=1, small_b=4, mid_ch=0)
OVERRIDES = [{}, {"persistent": 0}, {"mid": 0}, {"x3": 0}, {"x3g": 0}, {"small_b": 8}, {"mid_ch": 4}, {"mid_ch": 8},
             {"mid_ch": 16}]
# route -> (record name, flops factor, engine-owned hand-off buffer)
RECORD = {"step": ("lstm_step_kernel", 2, 0), "small": ("lstm_small_kernel", 2, 1), "x3g": ("lstm_x3g_kernel", 3, 1),
          "x3": ("lstm_x3_kernel", 3, 0), "mid": ("lstm_mid_kernel", 2, 0),
          "persistent": ("lstm_persistent_kernel", 2, 0)}


def expected(w, dtype, H, B):
    """(route, inst): the table of the ladder, first match wins."""
    split = dtype != F32
    if H != 640 or not w["persistent"]:
        return "step", 0
    if 1 <= B <= w["small_b"]:
        return "small", 8 if B > 4 else 4
    if split and w["x3"] and w["x3g"] and B <= 16:
        return "x3g", 0
    if split and w["x3"]:
        return "x3", 0
    if w["mid"] and w["small_b"] < B <= 16:
        return "mid", w["mid_ch"] if w["mid_ch"] in (4, 8, 16) else (4 if B <= 8 else 8)
    return "persistent", 0


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host compiler and no hipcc: the route dump program cannot be built")
    exe = str(tmp_path_factory.mktemp("lstm_route") / "lstm_route_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "lstm_route_dump.cpp"),
                    "-o", exe], check=True)

    def run(w, dtypes):
        argv = [exe] + [str(w[k]) for k in ("persistent", "mid", "x3", "x3g", "small_b", "mid_ch")]
        argv += [",".join(map(str, v)) for v in (dtypes, HS, BS)]
        out = subprocess.run(argv, check=True, capture_output=True, text=True).stdout
        return [json.loads(line) for line in out.splitlines()]

    return run


@pytest.mark.parametrize("override", OVERRIDES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_route_table(dump, override):
    w = dict(DEFAULTS, **override)
    rows = dump(w, (F32, BF16X3))
    assert len(rows) == 2 * len(HS) * len(BS)
    for r in rows:
        route, inst = expected(w, r["dtype"], r["H"], r["B"])
        name, terms, engine = RECORD[route]
        want = dict(dtype=r["dtype"], H=r["H"], B=r["B"], route=route, inst=inst, name=name, terms=terms,
                    engine_sync=engine)
        assert r == want, (override, r, want)


def test_every_split_dtype_routes_alike(dump):
    by = {d: [dict(r, dtype=0) for r in dump(DEFAULTS, (d,))] for d in (BF16, BF16X3, FP8)}
    assert by[BF16] == by[BF16X3] == by[FP8]


def test_default_routes_by_batch(dump):
    """The default ladder spelled out, H = 640: what tests/golden/launch_plan.json holds at B = 2, 5, 17 and the
    sizes around every limit."""
    got = {(r["dtype"], r["B"]): (r["route"], r["inst"]) for r in dump(DEFAULTS, (F32, BF16X3)) if r["H"] == 640}
    assert [got[F32, B] for B in BS] == [("small", 4), ("small", 4), ("mid", 4), ("mid", 4), ("mid", 8), ("mid", 8),
                                         ("persistent", 0), ("persistent", 0), ("persistent", 0)]
    assert [got[BF16X3, B] for B in BS] == [("small", 4), ("small", 4), ("x3g", 0), ("x3g", 0), ("x3g", 0), ("x3g", 0),
                                            ("x3", 0), ("x3", 0), ("x3", 0)]
