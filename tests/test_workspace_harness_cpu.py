"""The workspace harness (tests/ws_harness.py) can fail: CPU tensors and fake "engine calls" that break the
workspace contract of include/m2s.h one rule at a time.  Each must be flagged; a well-behaved fake passes."""
import numpy as np
import pytest
import torch

import ws_harness as H  # tests/ws_harness.py (pytest puts this directory on sys.path)

WS_BYTES = 4096 + 256


def _arena():
    x = np.arange(37, dtype=np.float32)  # an odd size: the buffer's end is not aligned
    return H.Arena("cpu", [("x", "in", x), ("y", "out", (37,)), ("z", "out", (3, 5)), ("ws", "ws", WS_BYTES)])


def _good(a, ws_bytes=None):
    """y = 2 x through the workspace, z = 1: what a correct call does (every scratch byte written before it is read)."""
    if ws_bytes is not None and ws_bytes < WS_BYTES:
        return H.M2S_E_ARG
    scratch = a.raw("ws")[:37 * 4].view(torch.float32)
    scratch.copy_(a.view("x") * 2)
    a.view("y").copy_(scratch)
    a.view("z").fill_(1.0)
    return H.M2S_OK


def test_layout_alignment_sizes_and_fills():
    a = _arena()
    for n in ("x", "y", "z", "ws"):
        assert a.ptr(n) % 256 == 0
    assert a.ptr(None) is None
    assert a.nbytes("x") == 37 * 4 and a.nbytes("z") == 60 and a.nbytes("ws") == WS_BYTES
    # 1 MiB on both sides of every buffer
    spans = sorted((a.ptr(n), a.ptr(n) + a.nbytes(n)) for n in ("x", "y", "z", "ws"))
    assert spans[0][0] - a.mem.data_ptr() >= H.GUARD
    assert all(lo2 - hi1 >= 2 * H.GUARD for (_, hi1), (lo2, _) in zip(spans, spans[1:]))
    assert a.mem.data_ptr() + a.mem.numel() - spans[-1][1] >= H.GUARD
    a.prepare("nan")
    assert torch.isnan(a.view("y")).all() and torch.isnan(a.view("z")).all()
    assert (a.raw("ws") == 0xFF).all() and torch.equal(a.view("x"), torch.arange(37.0))
    x = a.bufs["x"]
    assert (a._span(x.back, x.back + H.GUARD) == 0xFF).all() and (a._span(x.front, x.off) == 0xA5).all()
    y = a.bufs["y"]
    assert (a._span(y.back, y.back + H.GUARD) == 0xA5).all()
    a.prepare("random", seed=3)
    r1 = a.raw("ws").clone()
    a.prepare("random", seed=3)
    assert torch.equal(r1, a.raw("ws")) and len(torch.unique(r1)) > 100
    a.prepare("stale", stale=torch.full((WS_BYTES + 9,), 7, dtype=torch.uint8))
    assert (a.raw("ws") == 7).all()
    a.prepare("zero")
    assert not a.raw("ws").any()
    assert a.violations() == [s for s in a.violations() if "holds NaN" in s] and len(a.violations()) == 2


def test_well_behaved_call_passes():
    a = _arena()
    rep = H.check_contract(a, _good, stale=torch.full((2 * WS_BYTES,), 0x3C, dtype=torch.uint8), what="good")
    assert rep.deterministic and set(rep.outs) == {"zero", "zero2", "nan", "random", "stale"}
    assert torch.equal(rep.outs["nan"]["y"], 2 * torch.arange(37.0))
    H.check_undersized(a, _good, rep.outs["zero"], what="good")


@pytest.mark.parametrize("where", ["behind y", "in front of z", "behind ws", "last guard byte", "behind input"])
def test_one_byte_in_a_guard_is_flagged(where):
    a = _arena()

    def call(a):
        _good(a)
        b = a.bufs[{"behind y": "y", "in front of z": "z", "behind ws": "ws", "last guard byte": "ws",
                    "behind input": "x"}[where]]
        at = {"behind y": b.back, "in front of z": b.off - 1, "behind ws": b.back,
              "last guard byte": b.back + H.GUARD - 1, "behind input": b.back}[where]
        a._span(at, at + 1).fill_(0)
        return H.M2S_OK

    with pytest.raises(AssertionError, match="guard .* overwritten"):
        H.check_contract(a, call)


def test_unwritten_output_element_is_flagged():
    a = _arena()

    def call(a):
        _good(a)
        a.raw("y")[36 * 4:].fill_(0xFF)  # as if the last element had been left alone: still the pre-run fill
        return H.M2S_OK

    with pytest.raises(AssertionError, match="output 'y' holds NaN.*1 of 37, first at \\+36"):
        H.check_contract(a, call)


def test_workspace_byte_in_the_output_is_flagged():
    a = _arena()

    def call(a):
        _good(a)
        a.raw("z")[0] = a.raw("ws")[4000]  # a byte no kernel wrote: lowest mantissa byte of z[0, 0]
        return H.M2S_OK

    with pytest.raises(AssertionError, match="depends on the workspace contents"):
        H.check_contract(a, call)


def test_nondeterminism_is_reported_not_hidden():
    a = _arena()
    n = [0]

    def call(a):
        _good(a)
        n[0] += 1
        a.view("y")[0] = 1e-6 * n[0]
        return H.M2S_OK

    with pytest.raises(AssertionError, match="nondeterministic"):
        H.check_contract(a, call)
    rep = H.check_contract(a, call, tol={"y": 1e-4})
    assert not rep.deterministic and rep.max_fill_diff
    with pytest.raises(AssertionError, match="nondeterministic"):
        H.check_contract(a, call, tol={"y": 1e-7})


def test_bad_return_status_and_undersized_are_flagged():
    a = _arena()
    with pytest.raises(AssertionError, match="return code 5"):
        H.check_contract(a, lambda a: 5)
    with pytest.raises(AssertionError, match="engine status 5"):
        H.check_contract(a, _good, status=lambda: 5)
    good = H.check_contract(a, _good).outs["zero"]
    with pytest.raises(AssertionError, match="expected M2S_E_ARG"):
        H.check_undersized(a, lambda a, n: _good(a), good)  # accepts a short workspace

    def scribbles(a, n):
        if n < WS_BYTES:
            a.raw("ws")[-1:].fill_(1)  # uses the bytes it was told it does not have... still inside: fine
            b = a.bufs["ws"]
            a._span(b.back, b.back + 1).fill_(1)  # ...and one past them
            return H.M2S_E_ARG
        return _good(a)

    with pytest.raises(AssertionError, match="guard behind 'ws' overwritten"):
        H.check_undersized(a, scribbles, good)

    state = [0.0]

    def sticky(a, n):
        if n < WS_BYTES:
            state[0] = 1.0
            return H.M2S_E_ARG
        _good(a)
        a.view("z")[0, 0] += state[0]
        return H.M2S_OK

    with pytest.raises(AssertionError, match="changed after a refused call"):
        H.check_undersized(a, sticky, good)
