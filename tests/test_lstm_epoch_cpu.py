"""The epoch rule of the engine-owned BiLSTM hand-off buffer (csrc/lstm_route.hpp lstm_epoch_rule), on the CPU.

tests/lstm_epoch_dump.cpp prints the C++ rule as a table and this file walks EVERY sequence of up to five events over
it, against its own model of the buffer: two parity slots and the error word.  What the kernels do with them
(lstm_persistent.hip lstm_small_kernel, lstm_x3g_kernel): a launch (ep, T) publishes tag ep + s + 1 at step s into
slot s & 1 for every s with s + 1 < T, accepts at step s >= 1 a granule of slot (s - 1) & 1 as soon as its tag EQUALS
ep + s, and a timed-out wait writes the error word ep + 1, which a launch takes for its own abort when it equals its
own ep + 1.  Steps 1 and 2 read slots the launch has not rewritten yet, so whatever an earlier launch left is live.

Events: an eager launch of T = 1..6, the same with a timeout, a capture of T = 1..6 (the rule runs, nothing touches
the buffer; the graph keeps the epoch and the memset the rule gave it), a replay of any graph captured so far (its
memset, if it has one, then its launch), with or without a timeout.  Before every launch that does not zero the buffer
itself the invariant must hold: slot 0, slot 1 and the error word are all below ep + 1; in particular
slot0 != ep + 1 (step 1 would accept it), slot1 != ep + 2 (step 2), err != ep + 1 (a false abort).

The rule this replaced set count = T + 1 at capture time although the memset was only recorded, and fails here.  Its
two collisions (eager T = 35, capture T = 31 never replayed, eager; and capture A T = 31, eager, capture B T = 27,
replay A, eager), scaled down, are in the enumeration, under the old rule:
  1. eager T = 5 on a fresh engine: ep 0, tags 1, 3 in slot 0 and 2, 4 in slot 1, count 6.  capture T = 1: count 2.
     eager: ep = 2, step 1 waits for 3 in slot 0 and step 2 for 4 in slot 1: both are the first call's.
  2. capture A T = 5: count 6.  eager T = 1: ep 6, count 8.  capture B T = 1: count 2.  replay A: tags 3 in slot 0 and
     4 in slot 1.  eager: ep = 2 waits for 3 and 4 again.
With the count never lowered by a capture both eager calls run at ep = 6 and ep = 8.  The same walk starts from counts
around the wrap guard, where the rule stops counting and zeroes per launch."""
import json
import os
import subprocess

import pytest

from test_switches_cpu import _compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mri-to-speech_amd", "csrc")
TMAX, DEPTH = 6, 5
WRAP = 0xF0000000


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host compiler and no hipcc: the epoch dump program cannot be built")
    exe = str(tmp_path_factory.mktemp("lstm_epoch") / "lstm_epoch_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "lstm_epoch_dump.cpp"),
                    "-o", exe], check=True)
    table = {}

    def load(lo, hi):
        out = subprocess.run([exe, str(lo), str(hi), str(TMAX)], check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            r = json.loads(line)
            if "wrap" in r:
                assert r["wrap"] == WRAP
            else:
                table[r["count"], r["T"], bool(r["capturing"])] = (r["ep"], r["new"], bool(r["zero"]))

    # every count the walks below can reach: DEPTH launches of at most TMAX + 1 each from 0, and the wrap guard's
    # neighbourhood (a missing entry is a KeyError, not a silent pass)
    load(0, DEPTH * (TMAX + 1) + 1)
    load(WRAP - 64, WRAP + TMAX + 2)
    return table


def _launch(s0, s1, err, ep, T, timeout):
    for s in range(T - 1):
        if s & 1:
            s1 = ep + s + 1
        else:
            s0 = ep + s + 1
    return s0, s1, (ep + 1 if timeout else err)


def _check(path, s0, s1, err, ep):
    what = f"after {path}: launch at ep = {ep} meets slot0 = {s0}, slot1 = {s1}, err = {err}"
    assert s0 != ep + 1, "step 1 accepts a stale granule " + what
    assert s1 != ep + 2, "step 2 accepts a stale granule " + what
    assert err != ep + 1, "a stale timeout mark aborts the launch " + what
    assert s0 < ep + 1 and s1 < ep + 1 and err < ep + 1, "a tag or mark at or above ep + 1 " + what


def walk(rule, start, depth=DEPTH):
    """Every event sequence of `depth` events from the state `start` = (count, slot0, slot1, err); states that agree
    in count, buffer and the set of captured graphs are merged (one witness sequence kept), which loses nothing: what
    follows depends on those alone.  Returns the number of launches checked."""
    layer = {start + (frozenset(),): ()}
    checked = 0
    for d in range(depth):
        nxt = {}
        last = d + 1 == depth
        for (count, s0, s1, err, graphs), path in layer.items():
            for T in range(1, TMAX + 1):
                ep, new, zero = rule[count, T, False]
                for timeout in (False, True)[:2 if T >= 2 else 1]:  # a wait needs a second step
                    p = path + (("eager!" if timeout else "eager", T),)
                    if zero:
                        b = (0, 0, 0)
                    else:
                        _check(p, s0, s1, err, ep)
                        checked += 1
                        b = (s0, s1, err)
                    if not last:
                        nxt.setdefault((new,) + _launch(*b, ep, T, timeout) + (graphs,), p)
                if last:
                    continue
                ep, new, zero = rule[count, T, True]
                nxt.setdefault((new, s0, s1, err, graphs | {(ep, zero, T)}), path + (("capture", T),))
            for ep, zero, T in sorted(graphs):
                for timeout in (False, True)[:2 if T >= 2 else 1]:
                    p = path + (("replay!" if timeout else "replay", T),)
                    if zero:
                        b = (0, 0, 0)
                    else:
                        _check(p, s0, s1, err, ep)
                        checked += 1
                        b = (s0, s1, err)
                    if not last:
                        nxt.setdefault((count,) + _launch(*b, ep, T, timeout) + (graphs,), p)
        layer = nxt
    return checked


def test_rule_shape(rule):
    """What the kernels' launcher relies on besides the invariant: a capture always records its own memset and epoch
    0 (every replay repeats that one epoch) and never lowers the count; an eager launch away from the wrap guard
    continues the count by T + 1 without a memset; no tag reaches past the guard."""
    for (count, T, capturing), (ep, new, zero) in rule.items():
        if capturing:
            assert zero and ep == 0 and new == max(count, T + 1), (count, T)
        elif 0 < count <= WRAP - T:
            assert (ep, new, zero) == (count, count + T + 1, False), (count, T)
        else:
            assert zero and ep == 0, (count, T)
        assert ep + T <= WRAP, (count, T)  # the launch's largest tag is ep + T - 1


def test_every_sequence_from_a_fresh_engine(rule):
    """The two collisions of the docstring are sequences of three and five events of this walk."""
    assert walk(rule, (0, 0, 0, 0)) > 1000


@pytest.mark.parametrize("below", [0, 1, 2, 5, 6, 7, 8, 13, 20, 35])
def test_every_sequence_around_the_wrap_guard(rule, below):
    """The count starts `below` under the guard's threshold, the buffer as the eager launches that got it there can
    have left it: the last tags, count - 2 and count - 3, in either parity."""
    count = WRAP - below
    n = walk(rule, (count, count - 2, count - 3, 0), depth=4) + walk(rule, (count, count - 3, count - 2, count - 7), depth=4)
    assert (n > 0) == (below >= 1)  # at the threshold itself every launch zeroes: nothing left to collide with
