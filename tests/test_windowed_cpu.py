"""Windowed acoustic inference without a GPU: the oracle helper's identities, the fake kernels of the new ops, the
C ABI declarations and AcousticStream's bookkeeping against a stub engine."""
import os

import numpy as np
import pytest
import torch

import windowed_ref as R  # tests/windowed_ref.py
from m2s import _native, ops, synth
from m2s.stream import AcousticStream

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_acoustic_state(2).items()}


@pytest.fixture(scope="module")
def x():
    return torch.randn(9, 208, generator=torch.Generator().manual_seed(0))


def test_mean_with_a_window_past_the_clip_is_the_whole_clip_forward(sd, x):
    y, m = R.M(sd, x)
    for W in (9, 16):
        yw, mw = R.mean(sd, x, W)
        assert torch.equal(yw, y) and torch.equal(mw, m)


def test_latest_last_row_with_a_window_past_the_clip_is_the_whole_clip_last_row(sd, x):
    y, m = R.M(sd, x)
    yw, mw = R.latest(sd, x, 16)
    assert torch.equal(yw[-1], y[-1]) and torch.equal(mw[-1], m[-1])


def test_chunked_calls_with_context_give_the_rows_of_one_call(sd, x):
    W = 4
    _, whole = R.latest(sd, x, W)
    rows, pos = [], 0
    for n in (1, 2, 5, 1):
        ctx = min(W - 1, pos)
        rows.append(R.latest(sd, x[pos - ctx:pos + n], W, ctx)[1])
        pos += n
    assert torch.equal(torch.cat(rows), whole)


def test_the_modes_differ_where_they_should(sd, x):
    """Window inference is not the whole-clip forward, and latest is not mean except on the last frame."""
    _, whole = R.M(sd, x)
    _, lat = R.latest(sd, x, 4)
    _, mean = R.mean(sd, x, 4)
    assert float((lat - whole).abs().amax(1).min()) > 0.05
    assert float((mean - whole).abs().amax(1).min()) > 0.05
    assert float((lat - mean).abs().max()) > 0.1
    assert torch.equal(lat[-1], mean[-1])
    _, lat3 = R.latest(sd, x, 3)
    assert float((lat3[3:] - lat[3:]).abs().amax(1).min()) > 0.05


def test_windowed_ops_are_registered_with_fakes():
    o = ops.load()
    assert ops.WINDOWED_OPS == ("bilstm_windowed", "acoustic_forward_windowed")
    for name in ops.WINDOWED_OPS:
        assert hasattr(o, name)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        feats = torch.empty(12, 208)
        y, m = o.bilstm_windowed(1, feats, [7, 5], [3, 2], 4, 0, 640, 64)
        assert y.shape == (7, 640) and m.shape == (7, 64)
        y, m = o.bilstm_windowed(1, feats, [7, 5], [], 4, 1, 640, 64)
        assert y.shape == (12, 640) and m.shape == (12, 64)
        mn = o.acoustic_forward_windowed(1, torch.empty(12, 96, 80), [7, 5], [0, 1], 4, 0, 64)
        assert mn.shape == (11, 64)


def test_header_declares_the_windowed_calls_and_keeps_the_abi():
    src = open(os.path.join(REPO, "include", "m2s.h")).read()
    for name in ("m2s_acoustic_windowed_workspace_bytes", "m2s_bilstm_windowed", "m2s_acoustic_forward_windowed"):
        assert name + "(" in src and name in _native.exported_symbols()
        assert hasattr(_native.lib(), name)
    assert "#define M2S_ABI_VERSION 6" in src and _native.lib().m2s_abi_version() == 6


class _StubEngine:
    """effnet: frame n of value v -> feature row [v, 0, ...]; bilstm_windowed records its arguments and returns
    one row per output frame holding the sum of the window that ends there."""

    def __init__(self):
        self.calls = []

    def effnet(self, frames):
        return frames.reshape(frames.shape[0], -1)[:, :1].repeat(1, 3)

    def bilstm_windowed(self, feats, lengths, window, merge, context):
        self.calls.append((int(feats.shape[0]), list(lengths), window, merge, list(context)))
        assert merge == "latest" and lengths == [feats.shape[0]] and 0 <= context[0] <= window - 1
        rows = [feats[max(0, t - window + 1):t + 1, :1].sum(0) for t in range(context[0], feats.shape[0])]
        return None, torch.stack(rows)


@pytest.mark.parametrize("window", [1, 2, 4])
def test_stream_holds_the_last_rows_and_returns_the_pushed_frames(window):
    eng = _StubEngine()
    st = AcousticStream(eng, window=window)
    vals = torch.arange(1.0, 12.0)
    frames = vals[:, None, None].repeat(1, 2, 2)
    want = torch.stack([vals[max(0, t - window + 1):t + 1].sum() for t in range(11)])[:, None]
    got, pos = [], 0
    for n in (1, 1, 3, 6):
        out = st.push(frames[pos:pos + n])
        assert out.shape == (n, 1)
        pos += n
        assert st.context == min(window - 1, pos)
        got.append(out)
    assert torch.equal(torch.cat(got), want)
    assert [c[0] - c[4][0] for c in eng.calls] == [1, 1, 3, 6]  # every call: its context plus exactly the new frames
    st.reset()
    assert st.context == 0
    assert torch.equal(st.push(frames[:2]), want[:2])


def test_stream_refuses_bad_arguments():
    with pytest.raises(ValueError):
        AcousticStream(_StubEngine(), window=0)
    with pytest.raises(ValueError):
        AcousticStream(_StubEngine(), window=17)
    with pytest.raises(ValueError):
        AcousticStream(_StubEngine()).push(torch.zeros(0, 2, 2))
