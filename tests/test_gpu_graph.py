"""HIP graph capture and replay of the engines (include/m2s.h "Graph capture").  GPU box only.

Three places in the library behave differently on a capturing stream, and each has its group here:

1. the dense entry points are captured and replayed on refreshed inputs: every replay must give the bits of the same
   engine's eager call on that input (a host-baked value, a pointer into a freed workspace or scratch shared wrongly
   between launches fails this), and the engine's status must stay clean;
2. eager and captured BiLSTM calls interleaved on ONE engine must each give the bits of a fresh engine's eager call:
   the granule kernels' hand-off tags continue an epoch count across calls (csrc/lstm_route.hpp lstm_epoch_rule;
   tests/test_lstm_epoch_cpu.py pins the rule itself, these pin its wiring);
3. the entry points that stage a table per call refuse a capturing stream with M2S_E_STATE before anything is
   launched;
and the split-K scratch of conv_gemm.hip, process-static, is exercised in a child process (tests/graph_ksplit_child.py).

The capture pattern is tests/test_gpu_frames.py::test_graph_capture_replays_to_the_same_bits: eager calls first,
synchronize, capture, then per replay the input refreshed in place and the outputs filled with NaN.  Every
comparison is bit identity."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ws_harness as H  # tests/ws_harness.py
from graph_ksplit_child import RESULT_TAG  # tests/graph_ksplit_child.py
from m2s import _native, runtime, synth
from m2s.config import HIFIGAN_H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ["fp32", "bf16", "bf16x3", "fp8"]
HW = (96, 80)
NAN = float("nan")
CHILD_TIMEOUT = 300  # seconds; the child creates two vocoder engines and runs a dozen 5-row calls


@pytest.fixture(scope="module")
def states():
    return synth.synth_acoustic_state(4), synth.synth_generator_state(4)


@pytest.fixture(scope="module")
def engines(states):
    """One acoustic engine, one vocoder and the pipeline over them per dtype, created on first use."""
    cache = {}
    mean, std = synth.synth_scaler()

    def get(dtype):
        if dtype not in cache:
            ac = runtime.AcousticEngine(states[0], dtype=dtype, device=DEV)
            voc = runtime.VocoderEngine(states[1], HIFIGAN_H, dtype=dtype, device=DEV)
            cache[dtype] = (ac, voc, runtime.Pipeline(ac, voc, mean, std))
        return cache[dtype]
    return get


def _rand(shape, seed, normal=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g) if normal else torch.rand(shape, device=DEV, generator=g)


def _tensors(out):
    return list(out.values()) if isinstance(out, dict) else list(out) if isinstance(out, (tuple, list)) else [out]


def _capture(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def _replay(graph, x, value, out):
    """One replay on ``value``: the graph's input refreshed in place, every output NaN before it runs."""
    x.copy_(value)
    for t in _tensors(out):
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    return [t.clone() for t in _tensors(out)]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert H.bits_equal(g, w), (what, i, float((g.double() - w.double()).abs().nan_to_num(nan=np.inf).max()))


def _lstm_names(call):
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        call()
        torch.cuda.synchronize()
        return sorted({r["name"] for r in _native.prof_launches() if r["name"].startswith("lstm_")})
    finally:
        _native.prof_enable(False)


# ---- 1. replay equals eager, on refreshed inputs ---------------------------------------------------------------------
# name -> (the call on (acoustic, vocoder, pipeline, x), the input's shape, normal instead of uniform values)
CALLS = {
    "vocoder_1x5": (lambda ac, voc, pipe, x: voc.forward(x), (1, 64, 5), True),
    "vocoder_2x3": (lambda ac, voc, pipe, x: voc.forward(x), (2, 64, 3), True),
    "effnet": (lambda ac, voc, pipe, x: ac.effnet(x), (2,) + HW, False),
    "bilstm_b1": (lambda ac, voc, pipe, x: ac.bilstm(x), (1, 12, 208), True),
    "bilstm_b8": (lambda ac, voc, pipe, x: ac.bilstm(x), (8, 12, 208), True),
    "bilstm_b17": (lambda ac, voc, pipe, x: ac.bilstm(x), (17, 12, 208), True),
    "acoustic": (lambda ac, voc, pipe, x: ac.forward(x), (1, 6) + HW, False),
    "pipeline": (lambda ac, voc, pipe, x: pipe.forward(x), (1, 6) + HW, False),
}
# the recurrence kernel each BiLSTM case captures (csrc/lstm_route.hpp): the first two hand h over in the engine's
# epoch-tagged buffer, the others zero their sync words in the workspace per launch (under capture by a kernel node:
# with a memset node the SECOND replay of lstm_mid, lstm_x3 and lstm_persistent went wrong, lstm_persistent.hip
# lstm_zero; the inputs 0, 1, 0 are what shows it)
LSTM_ROUTE = {"bilstm_b1": {"fp32": "lstm_small_kernel", "split": "lstm_small_kernel"},
              "bilstm_b8": {"fp32": "lstm_mid_kernel", "split": "lstm_x3g_kernel"},
              "bilstm_b17": {"fp32": "lstm_persistent_kernel", "split": "lstm_x3_kernel"}}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CALLS))
def test_replay_equals_eager_on_refreshed_inputs(engines, name, dtype):
    ac, voc, pipe = engines(dtype)
    call, shape, normal = CALLS[name]
    if name.startswith("vocoder"):  # ln-power mels in the range the glue produces
        xs = [torch.from_numpy(synth.synth_mel_log(shape[0], 64, shape[2], seed=50 + k)).to(DEV) for k in (0, 1)]
    else:
        xs = [_rand(shape, 1000 + 17 * k + len(name), normal) for k in (0, 1)]
    assert not H.bits_equal(xs[0], xs[1])
    eager = []
    for v in xs:  # the eager calls are the warm-up of the capture too
        eager.append([t.clone() for t in _tensors(call(ac, voc, pipe, v))])
        ac.check()
    assert not all(H.bits_equal(a, b) for a, b in zip(*eager)), "the two inputs give one output: nothing to tell apart"
    if name in LSTM_ROUTE:
        want = LSTM_ROUTE[name]["fp32" if dtype == "fp32" else "split"]
        assert _lstm_names(lambda: call(ac, voc, pipe, xs[0])) == [want]
    x = xs[0].clone()
    torch.cuda.synchronize()
    graph, out = _capture(lambda: call(ac, voc, pipe, x))
    try:
        for k in (0, 1, 0):
            _same(_replay(graph, x, xs[k], out), eager[k], (name, dtype, "replay on input", k))
            ac.check()
    finally:  # a failure's report is this case's: the shared engine starts the next one clean
        del graph
        try:
            ac.check()
        except _native.M2SError:
            pass


# ---- 2. eager and captured BiLSTM calls interleaved on one engine ----------------------------------------------------
class _Interleaved:
    """One engine under test and, per input, a fresh engine's eager result (computed once per (dtype, B, T, seed))."""
    wanted = {}

    def __init__(self, state, dtype, B):
        self.state, self.dtype, self.B, self.seed = state, dtype, B, 0
        self.eng = runtime.AcousticEngine(state, dtype=dtype, device=DEV)

    def input(self, T):
        self.seed += 1
        return _rand((self.B, T, 208), 7000 + 100 * self.seed + T, normal=True)

    def want(self, x):
        key = (self.dtype, self.B, x.shape[1], self.seed)
        if key not in self.wanted:
            fresh = runtime.AcousticEngine(self.state, dtype=self.dtype, device=DEV)
            self.wanted[key] = [t.clone() for t in fresh.bilstm(x)]
            fresh.check()
        return self.wanted[key]

    def eager(self, T, what):
        x = self.input(T)
        want = self.want(x)  # first: the fresh engine's call also loads the kernels a later capture records
        got = [t.clone() for t in self.eng.bilstm(x)]
        self.eng.check()
        _same(got, want, (what, "eager", T))

    def capture(self, T):
        """Captured WITHOUT an eager call of this engine in front (that call would move the tags the sequences
        below place); the kernels are loaded by a fresh engine's call of the same shape."""
        x = self.input(T)
        self.want(x)
        buf = x.clone()
        torch.cuda.synchronize()
        graph, out = _capture(lambda: self.eng.bilstm(buf))
        torch.cuda.synchronize()
        return graph, buf, out

    def replay(self, cap, what):
        graph, buf, out = cap
        x = self.input(buf.shape[1])
        want = self.want(x)
        got = _replay(graph, buf, x, out)
        self.eng.check()
        _same(got, want, (what, "replay", buf.shape[1]))


def _seq_a(s):
    s.eager(35, "a")
    cap = s.capture(31)  # never replayed
    s.eager(9, "a")
    del cap


def _seq_b(s):
    a = s.capture(31)
    s.eager(20, "b")
    b = s.capture(27)
    s.replay(a, "b")
    s.eager(9, "b")
    s.replay(b, "b")
    s.eager(9, "b")


def _seq_c(s):
    g31, g17 = s.capture(31), s.capture(17)
    s.eager(33, "c")
    s.replay(g31, "c")
    s.eager(40, "c")
    s.replay(g17, "c")


@pytest.mark.parametrize("seq", [_seq_a, _seq_b, _seq_c], ids=["a", "b", "c"])
@pytest.mark.parametrize("dtype,B", [("bf16x3", 1), ("bf16x3", 8), ("fp32", 1)])
def test_interleaved_eager_and_captured_bilstm(states, dtype, B, seq):
    """B = 1 runs lstm_small_kernel, B = 8 in the split engine lstm_x3g_kernel: the two routes whose hand-off tags
    live in the engine's buffer across calls.  In both kernels (csrc/lstm_persistent.hip) a launch (ep, T) publishes
    at step s, while s + 1 < T, the tag ep + s + 1 into parity slot s & 1 (`gd + (step & 1) * ...`), and at step
    s >= 1 sweeps slot (s - 1) & 1 until every tag EQUALS ep + s: the parity is the same in lstm_x3g, so one set of
    lengths serves both.  The error word matches on ep + 1.

    (a) eager T = 35 on the fresh engine runs at ep = 0 and publishes at s = 32 the tag 33 into slot 0 and at s = 33
        the tag 34 into slot 1 (s = 34 publishes nothing).  A capture of T = 31 that restarted the count at 32, with
        its memset only recorded, made the next eager call run at ep = 32: its step 1 sweeps slot 0 for 33 and its
        step 2 slot 1 for 34, the first call's granules, and whichever consumer gets there before the producer has
        overwritten them takes an h of the old clip.
    (b) capture A, T = 31; eager T = 20; capture B, T = 27 (a restarting capture left the count at 28).  A replay of
        A zeroes the buffer and runs at ep = 0: s = 28 leaves tag 29 in slot 0, s = 29 tag 30 in slot 1.  An eager
        call at ep = 28 sweeps for exactly 29 and 30.  Then a replay of B and another eager call.
    (c) eager 33, replay of a T = 31 graph, eager 40, replay of a T = 17 graph: no engineered collision, the plain
        alternation.
    The stale granule is read only if the consumer wins that race, so a wrong count can pass here by luck; the
    arithmetic is pinned on the CPU.  With the count never lowered by a capture, (a)'s last call runs at ep = 36 and
    (b)'s eager calls at 32, 53 and 63."""
    s = _Interleaved(states[0], dtype, B)
    names = _lstm_names(lambda: runtime.AcousticEngine(states[0], dtype=dtype, device=DEV).bilstm(s.input(9)))
    assert names == ["lstm_x3g_kernel" if B == 8 else "lstm_small_kernel"], names
    seq(s)


# ---- 3. refusals launch nothing --------------------------------------------------------------------------------------
M2S_E_STATE = 3
LENS, LENS_P, WIN = [3, 2], [5, 4], 4
BANDS = {"A": list(range(5, 20)), "B": list(range(21, 39))}


def _ints(v):
    return (C.c_int * len(v))(*v)


class _Ctx:
    def __init__(self, states, engines):
        from m2s.gradcam import GradCam
        self.ac, self.voc, _ = engines("bf16x3")
        self.cam = GradCam(states[0], DEV)
        self.mean, self.std = synth.synth_scaler()
        self.L = _native.lib()


def _frames(n, seed):
    return synth.synth_frames(1, n, hw=HW, seed=seed)[0]


def _feats(n, seed):
    return np.random.default_rng(seed).normal(0, 0.5, (n, 208)).astype(np.float32)


def _r_bilstm_ragged(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_acoustic_ragged_workspace_bytes(c.ac._h, cl, len(LENS), *HW)
    specs = [("feats", "in", _feats(n, 1)), ("y", "out", (n, 640)), ("mel_norm", "out", (n, 64)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_bilstm_summerge_ragged(c.ac._h, a.ptr("feats"), cl, len(LENS), n, a.ptr("y"),
                                                              a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_acoustic_ragged(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_acoustic_ragged_workspace_bytes(c.ac._h, cl, len(LENS), *HW)
    specs = [("frames", "in", _frames(n, 2)), ("mel_norm", "out", (n, 64)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_acoustic_forward_ragged(c.ac._h, a.ptr("frames"), cl, len(LENS), n, *HW,
                                                               a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_vocoder_ragged(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_vocoder_ragged_workspace_bytes(c.voc._h, cl, len(LENS))
    mel = np.ascontiguousarray(synth.synth_mel_log(1, 64, n, seed=3)[0].T)
    specs = [("mel", "in", mel), ("wav", "out", (n * c.voc.hop,)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_vocoder_forward_ragged(c.voc._h, a.ptr("mel"), cl, len(LENS), n, a.ptr("wav"),
                                                              a.ptr("ws"), nws, s)


def _r_pipeline_ragged(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_pipeline_ragged_workspace_bytes(c.ac._h, c.voc._h, cl, len(LENS), *HW)
    specs = [("frames", "in", _frames(n, 4)), ("mean", "in", c.mean), ("std", "in", c.std)]
    specs += [(k, "out", (n, 64)) for k in ("mel_norm", "mel_db", "mel_log")]
    specs += [("wav", "out", (n * c.voc.hop,)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_pipeline_forward_ragged(
        c.ac._h, c.voc._h, a.ptr("frames"), cl, len(LENS), n, *HW, a.ptr("mean"), a.ptr("std"), a.ptr("mel_norm"),
        a.ptr("mel_db"), a.ptr("mel_log"), a.ptr("wav"), a.ptr("ws"), nws, s)


def _r_bilstm_windowed(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_acoustic_windowed_workspace_bytes(c.ac._h, cl, None, len(LENS), 0, 0, WIN, 0)
    specs = [("feats", "in", _feats(n, 5)), ("y", "out", (n, 640)), ("mel_norm", "out", (n, 64)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_bilstm_windowed(c.ac._h, a.ptr("feats"), cl, None, len(LENS), n, WIN, 0,
                                                       a.ptr("y"), a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_acoustic_windowed(c):
    n, cl = sum(LENS), _ints(LENS)
    nws = c.L.m2s_acoustic_windowed_workspace_bytes(c.ac._h, cl, None, len(LENS), *HW, WIN, 0)
    specs = [("frames", "in", _frames(n, 6)), ("mel_norm", "out", (n, 64)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_acoustic_forward_windowed(c.ac._h, a.ptr("frames"), cl, None, len(LENS), n, *HW,
                                                                 WIN, 0, a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_bilstm_pairs(c):
    n, cl, P = sum(LENS_P), _ints(LENS_P), sum(v - WIN + 1 for v in LENS_P)
    nws = c.L.m2s_acoustic_pairs_workspace_bytes(c.ac._h, cl, len(LENS_P), 0, 0, WIN)
    specs = [("feats", "in", _feats(n, 7)), ("y", "out", (P, WIN, 640)), ("mel_norm", "out", (P, WIN, 64)),
             ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_bilstm_pairs(c.ac._h, a.ptr("feats"), cl, len(LENS_P), n, WIN, a.ptr("y"),
                                                    a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_acoustic_pairs(c):
    n, cl, P = sum(LENS_P), _ints(LENS_P), sum(v - WIN + 1 for v in LENS_P)
    nws = c.L.m2s_acoustic_pairs_workspace_bytes(c.ac._h, cl, len(LENS_P), *HW, WIN)
    specs = [("frames", "in", _frames(n, 8)), ("mel_norm", "out", (P, WIN, 64)), ("ws", "ws", nws)]
    return specs, lambda a, s: c.L.m2s_acoustic_forward_pairs(c.ac._h, a.ptr("frames"), cl, len(LENS_P), n, *HW, WIN,
                                                              a.ptr("mel_norm"), a.ptr("ws"), nws, s)


def _r_gradcam(c):
    T, nb, fidx = 2, len(BANDS), [1, 0, 1]
    K = nb * (1 + len(fidx))
    nws = c.L.m2s_gradcam_workspace_bytes(c.cam._h, T, *HW, nb, len(fidx))
    mask = np.ascontiguousarray(c.cam.band_mask(BANDS).numpy(), dtype=np.float32)
    cmask, ci = mask.ctypes.data_as(C.POINTER(C.c_float)), _ints(fidx)
    nstat = c.L.m2s_gradcam_bn_stats_floats(c.cam._h)
    specs = [("frames", "in", _frames(T, 9)), ("mean", "in", c.mean), ("std", "in", c.std),
             ("heat_seq", "out", (nb, T) + HW), ("heat_frame", "out", (nb, len(fidx)) + HW), ("pred", "out", (T, 64)),
             ("dpooled", "out", (K, T, 208)), ("bn_stats", "out", (nstat,)), ("ws", "ws", nws)]

    def call(a, s, keep=(mask,)):  # (the host mask stays alive with the closure)
        return c.L.m2s_gradcam_forward(c.cam._h, a.ptr("frames"), T, *HW, a.ptr("mean"), a.ptr("std"), cmask, nb, ci,
                                       len(fidx), 0, a.ptr("heat_seq"), a.ptr("heat_frame"), a.ptr("pred"),
                                       a.ptr("dpooled"), a.ptr("bn_stats"), a.ptr("ws"), nws, s)
    return specs, call


# every entry point include/m2s.h documents as M2S_E_STATE on a capturing stream, but the chunked vocoder call
# (tests/test_gpu_vocoder_stream.py::test_stream_capture_is_refused)
REFUSED = {"bilstm_summerge_ragged": _r_bilstm_ragged, "acoustic_forward_ragged": _r_acoustic_ragged,
           "vocoder_forward_ragged": _r_vocoder_ragged, "pipeline_forward_ragged": _r_pipeline_ragged,
           "bilstm_windowed": _r_bilstm_windowed, "acoustic_forward_windowed": _r_acoustic_windowed,
           "bilstm_pairs": _r_bilstm_pairs, "acoustic_forward_pairs": _r_acoustic_pairs, "gradcam_forward": _r_gradcam}


@pytest.fixture(scope="module")
def refusal_ctx(states, engines):
    return _Ctx(states, engines)


@pytest.mark.parametrize("entry", list(REFUSED))
def test_capturing_stream_is_refused_before_any_launch(refusal_ctx, entry):
    """Inside the capture the call returns M2S_E_STATE and says why.  The captured graph then holds the marker add
    alone: replayed, it leaves every output and the workspace at the sentinel they were filled with (0xFF bytes) and
    the guards around them intact, so no kernel was recorded before the refusal.  The same call outside a capture
    runs and writes every output."""
    c = refusal_ctx
    specs, call = REFUSED[entry](c)
    (nws,) = [what for _, kind, what in specs if kind == "ws"]
    assert nws > 0 and nws % 256 == 0, (entry, nws)
    arena = H.Arena(DEV, specs)
    arena.prepare("nan")
    mark = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(DEV), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            mark.add_(1.0)  # the capture is not empty
            rc = call(arena, side.cuda_stream)
            msg = c.L.m2s_last_error().decode()
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert rc == M2S_E_STATE, (entry, rc, msg)
    assert "captur" in msg, (entry, msg)
    assert float(mark.sum()) == 0.0
    graph.replay()
    torch.cuda.synchronize()
    assert float(mark.sum()) == 8.0  # the replay ran, and it ran the marker
    for name in arena.names("out") + arena.names("ws"):
        assert bool((arena.raw(name) == H.POISON).all()), (entry, name, "written by the replay of a refused call")
    assert not arena.violations(outputs_written=False), entry
    c.ac.check()
    rc = call(arena, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc, c.L.m2s_last_error().decode())
    c.ac.check()
    assert not arena.violations(), entry
    del graph


# ---- 4. split-K scratch under capture, in a process that has none yet ------------------------------------------------
def test_split_k_scratch_under_capture_in_a_fresh_process():
    """conv_gemm.hip ksplit_scratch keeps its buffers per process, and a capturing stream cannot allocate: it borrows
    another stream's buffer or, with none, the launch runs unsplit.  Only a new process has none, so the three steps
    run in a child of their own (started once, never an exec of this process, under a time limit) on a bf16 vocoder
    at B = 1, T = 5, and this test asserts on the JSON line it prints (tests/graph_ksplit_child.py)."""
    env = {k: v for k, v in os.environ.items() if k != "M2S_KSPLIT"}
    p = subprocess.run([sys.executable, os.path.join(HERE, "graph_ksplit_child.py")], env=env, capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (line,) = [ln for ln in p.stdout.splitlines() if ln.startswith(RESULT_TAG)]
    r = json.loads(line[len(RESULT_TAG):])
    print(json.dumps(r))
    # (i) the unsplit engine planned no split launch, (iii) the split one did: the steps test what they are named for
    assert r["ksum_launches_ksplit1"] == 0 and r["ksum_launches_ksplit4"] > 0, r
    # (ii) first call captured with no scratch in the process: the unsplit fall-back, on inputs 0, 1, 0
    if r["same_kernels"]:
        assert r["first_capture_equals_ksplit1_eager"] == [True, True, True], r
    else:  # the engines plan different kernels: the bf16 vocoder bar of tests/test_gpu_parity.py against the oracle
        assert min(r["first_capture_snr_db"]) >= 25.0, r
    # (iii) after an eager call allocated scratch: captured again, the borrowed buffer gives the eager bits
    assert r["eager_ksplit4_snr_db"] >= 25.0, r
    assert r["second_capture_equals_own_eager"] == [True, True, True], r
