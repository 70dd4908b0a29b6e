"""The streaming vocoder without a GPU: the reach rule against perturbation on the oracle, VocoderStream's bookkeeping
against the chunk contract stated on the oracle (tests/vocoder_stream_ref.py, float64), the proof that this
yardstick notices a wrong reach, and the C ABI / op boundary of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

import vocoder_stream_ref as R  # tests/vocoder_stream_ref.py (pytest puts this directory on sys.path)
from m2s import _native as N
from m2s import ops, synth
from m2s.config import HIFIGAN_H, generator_reach
from m2s.stream import VocoderStream, push_all

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_R2 = dict(HIFIGAN_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])  # tests/test_gpu_ragged.py
# other rates, kernels (k - u = 0, 4 and 2), kernel sizes and dilations; narrow, the reach does not depend on widths
H_ODD = {"resblock": "1", "upsample_rates": [4, 3, 2], "upsample_kernel_sizes": [4, 7, 4],
         "upsample_initial_channel": 32, "resblock_kernel_sizes": [3, 5], "resblock_dilation_sizes": [[1, 2], [2, 6]],
         "num_mels": 8}
H_ODD2 = dict(H_ODD, resblock="2", upsample_rates=[5, 3], upsample_kernel_sizes=[11, 9])
# the shipped rates, kernels and dilations at an eighth of the width: the same rule and so the same reach, cheap
# enough to stream on a CPU
H_NARROW = dict(HIFIGAN_H, upsample_initial_channel=64)
SEED = 2
CHUNKINGS = [[40], [1] * 40, [1, 2, 5, 17, 15], [8, 32]]


# ---- reach ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,want", [("shipped", HIFIGAN_H, (16, 7)), ("r2", H_R2, (6, 7)),
                                         ("odd", H_ODD, None), ("odd2", H_ODD2, None), ("narrow", H_NARROW, (16, 7))])
def test_generator_reach_is_the_measured_reach(name, h, want):
    back, ahead = generator_reach(h)
    if want is not None:
        assert (back, ahead) == want
    # two rows of margin on both sides: a reach larger than the rule says would show as a larger measurement
    sd = R.to64(synth.synth_generator_state(SEED, h))
    got = R.measured_reach(sd, h, rows=back + ahead + 5, row=ahead + 2)
    print(f"reach {name}: rule {(back, ahead)}, perturbation (to first order) {got}")
    assert got == (back, ahead)


def test_latency_of_the_shipped_config():
    _, ahead = generator_reach(HIFIGAN_H)
    assert round(1000 * ahead * HIFIGAN_H["hop_size"] / HIFIGAN_H["sampling_rate"]) == 258


# ---- stream semantics ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    sd = synth.synth_generator_state(SEED, H_NARROW)
    mel = torch.from_numpy(np.ascontiguousarray(synth.synth_mel_log(1, 64, 40, seed=40)[0].T)).double()
    return sd, mel, R.G(R.to64(sd), H_NARROW, mel)


@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "-".join(map(str, c)) if len(c) < 6 else f"{len(c)}x1")
def test_stream_is_the_whole_clip_for_every_chunking(narrow, chunking):
    sd, mel, whole = narrow
    eng = R.OracleEngine(sd, H_NARROW, generator_reach(H_NARROW))
    st, hop = VocoderStream(eng), eng.hop
    assert (st.back, st.ahead) == (16, 7)
    out, seen, done = [], 0, 0
    for n in chunking:
        calls = len(eng.calls)
        w = st.push(mel[seen:seen + n])
        seen += n
        final = max(done, seen - 7)  # empty until 8 rows exist, then one frame per new row
        assert w.shape == ((final - done) * hop,), (seen, w.shape)
        assert st.pending == seen - final and st._rows.shape[0] <= 16 + 7  # the state: the last back + ahead rows
        assert len(eng.calls) == calls + (final > done)
        if final > done:  # the span holds the full look-ahead back, and brings the full history or starts the clip
            (length,), (ctx,), (hold,) = eng.calls[-1]
            assert hold == 7 and (seen - length) + ctx == done and (ctx >= 16 or seen == length)
        done = final
        out.append(w)
    tail = st.flush()
    assert tail.shape == ((40 - done) * hop,) and 40 - done <= 7
    assert st.pending == 0 and st._rows is None  # reset
    assert eng.calls[-1][2] == [0] and eng.calls[-1][0][0] <= 16 + 7  # the flush ends the clip
    wav = torch.cat(out + [tail])
    assert wav.shape == (40 * hop,)
    err = float((wav - whole).abs().max())
    print(f"chunking {chunking[:6]}: max |stream - whole clip| = {err:.2e}")
    assert err <= 1e-6


def test_push_all_runs_streams_at_different_phases_in_one_call(narrow):
    sd, mel, whole = narrow
    eng = R.OracleEngine(sd, H_NARROW, generator_reach(H_NARROW))
    streams = [VocoderStream(eng) for _ in range(3)]
    start = [0, 5, 12]  # stream i has seen `start[i]` rows before the joint pushes begin
    outs = [[], [], []]
    for i, n in enumerate(start):
        if n:
            outs[i].append(streams[i].push(mel[:n]))
    pos = list(start)
    calls = len(eng.calls)
    for step in (3, 6, 10):
        res = push_all(streams, [mel[p:p + step] for p in pos])
        pos = [p + step for p in pos]
        for i in range(3):
            outs[i].append(res[i])
    # one call per joint push; stream 0 has 3 rows at the first one and is left out of it
    assert [c[0] for c in eng.calls[calls:]] == [[8, 15], [9, 14, 21], [19, 24, 31]]
    assert [c[1] for c in eng.calls[calls:]] == [[0, 5], [0, 1, 8], [2, 7, 14]]
    for i in range(3):
        got = torch.cat(outs[i])
        assert got.shape == (max(0, pos[i] - 7) * eng.hop,)
        assert float((got - whole[:got.shape[0]]).abs().max()) <= 1e-6


# ---- the yardstick can fail ------------------------------------------------------------------------------------
def test_a_wrong_reach_misses_the_bar():
    """Rows 24-25 of a 40-row clip, shipped config, float64: the contract with the right reach is exact; one with too
    little history or look-ahead misses the GPU tests' 1e-4 bar against the whole clip (6.4e-3, 5.5e-4, 0.39, 0.77)."""
    h, hop = HIFIGAN_H, 420
    sd = R.to64(synth.synth_generator_state(SEED, h))
    mel = torch.from_numpy(np.ascontiguousarray(synth.synth_mel_log(1, 64, 40, seed=40)[0].T)).double()
    want = R.G(sd, h, mel)[24 * hop:26 * hop]

    def err(context, hold):
        x = mel[24 - context:26 + hold]
        return float((R.chunk(sd, h, x, [x.shape[0]], [context], [hold]) - want).abs().max())

    errs = {"right": err(16, 7), "back 8": err(8, 7), "back 10": err(10, 7), "hold 6": err(16, 6),
            "context 0": err(0, 7)}
    print("rows 24-25 against the whole clip:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert errs.pop("right") <= 1e-9
    for k, v in errs.items():
        assert v > 1e-4, (k, v)


# ---- boundary ----------------------------------------------------------------------------------------------------
NEW = ("m2s_vocoder_reach", "m2s_vocoder_set_chunk_cone", "m2s_vocoder_chunk_workspace_bytes",
       "m2s_vocoder_forward_chunk")


def test_new_header_functions_are_exported_and_bound():
    src = open(os.path.join(REPO, "include", "m2s.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(m2s_[a-z0-9_]+)\s*\(", src))
    L = N.lib()
    for name in NEW:
        assert name in declared and name in N.exported_symbols(), name
        assert getattr(L, name).argtypes is not None, name
    assert sorted(N.exported_symbols()) == sorted(declared)  # test_boundary_cpu's export check
    assert L.m2s_abi_version() == N.ABI_VERSION == 6  # additive
    # null handles: an error code, a zero size
    assert L.m2s_vocoder_reach(None, None, None) == 1
    assert L.m2s_vocoder_chunk_workspace_bytes(None, None, None, None, 1) == 0


def test_stream_op_is_registered_with_its_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    o = ops.load()
    assert ops.STREAM_OPS == ("hifigan_forward_chunk",)
    assert not set(ops.STREAM_OPS) & (set(ops.OPS) | set(ops.RAGGED_OPS) | set(ops.WINDOWED_OPS))
    assert str(o.hifigan_forward_chunk.default._schema) == (
        "m2s::hifigan_forward_chunk(int handle, Tensor mel, int[] lengths, int[] context, int[] hold, int hop) -> Tensor")
    with FakeTensorMode():
        mel = torch.empty(9 + 26 + 18, 64)
        assert o.hifigan_forward_chunk(1, mel, [9, 26, 18], [0, 16, 16], [7, 7, 0], 420).shape == ((2 + 3 + 2) * 420,)


def test_cli_stream_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "m2s_cli_stream_cpu", os.path.join(REPO, "mri-to-speech_amd", "scripts", "run_mri_video_inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--video", "v.mp4", "--mri-checkpoint", "c.pt", "--scaler-json", "s.json", "--hifigan-config", "h.json",
            "--hifigan-checkpoint", "g", "--output-dir", "o"]
    a = cli.parse_args(base)
    assert (a.stream, a.window) == (0, 0)  # without the flag nothing changes
    assert (lambda x: (x.stream, x.window))(cli.parse_args([*base, "--stream", "3"])) == (3, 4)  # implies --window 4
    assert (lambda x: (x.stream, x.window))(cli.parse_args([*base, "--stream", "3", "--window", "8"])) == (3, 8)
    with pytest.raises(SystemExit):
        cli.parse_args([*base, "--stream", "3", "--window-merge", "mean"])
