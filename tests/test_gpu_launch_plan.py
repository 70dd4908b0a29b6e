"""The engines' execution plans, pinned: every case of tools/plan_dump.py launches the kernels recorded in
tests/golden/launch_plan.json, in that order, under the same stage, with the same recorded flops, bytes and spill
bytes (to a relative 1e-12: a reassociated double expression, nothing else).

The golden was written by ``python tools/plan_dump.py --plan tests/golden/launch_plan.json`` on an MI355X before the
plan code (csrc/acoustic_cnn.cpp, acoustic_rnn.cpp, vocoder.cpp) was split out of one file.  A pull request that
changes a route on purpose regenerates it and shows the difference; one that only moves host code must not.
"""
import json
import os

import pytest

from tools import plan_dump

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.json")


@pytest.fixture(scope="module")
def ctx():
    return plan_dump.Context()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return plan_dump.decode(json.load(f))


def test_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(c.name for c in plan_dump.CASES)


@pytest.mark.parametrize("case", plan_dump.CASES, ids=[c.name for c in plan_dump.CASES])
def test_launch_plan(ctx, golden, monkeypatch, case):
    got, outs = plan_dump.run_case(case, ctx, monkeypatch.setenv)
    assert outs and got, "the case ran nothing"
    diff = plan_dump.plan_diff(golden[case.name], got)
    assert diff is None, f"{case.name}: {diff}"
