"""The streaming vocoder on the GPU (include/m2s.h "streaming vocoder", DESIGN.md "Streaming vocoder"): the stateless
chunk call, the cone, the streams over it and the frames-to-wav stream.

The reference is always the CPU oracle on the WHOLE clip a span was cut from, at the dense and ragged wav bar
(atol = 1e-4; the bf16 and fp8 engines at the bars of their dense vocoder tests, test_gpu_parity.py's 25 dB and
test_gpu_fp8.py's cosine 0.99): a span with too little history or look-ahead, or an edge treated as a clip end where
it is none, misses that bar by one to four orders of magnitude (tests/test_vocoder_stream_cpu.py: 5.5e-4 with 10 of
16 history rows, 0.39 with 6 of 7 look-ahead rows).  Clips are 40 rows, weights from m2s.synth at seed 2.  GPU box only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import windowed_ref as WR  # tests/windowed_ref.py
import ws_harness as H     # tests/ws_harness.py
from m2s import _native, ops, runtime, synth
from m2s.config import HIFIGAN_H, generator_reach
from m2s.stream import SpeechStream, VocoderStream, push_all
from oracle import acoustic, effnet, hifigan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H_R2 = dict(HIFIGAN_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])  # tests/test_gpu_ragged.py
CFG = {"1": HIFIGAN_H, "2": H_R2}
ROWS, HOP = 40, 420
CHUNKINGS = [[40], [1] * 40, [1, 2, 5, 17, 15], [8, 32]]
ERRORS = (_native.M2SError, RuntimeError)
CROP = "crop_rows_kernel"


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.fixture(scope="module")
def gen_sd():
    return {rb: synth.synth_generator_state(2, h) for rb, h in CFG.items()}


@pytest.fixture(scope="module")
def voc(gen_sd):
    cache = {}

    def get(dtype, rb="1"):
        if (dtype, rb) not in cache:
            cache[dtype, rb] = runtime.VocoderEngine(gen_sd[rb], CFG[rb], dtype=dtype, device=DEV)
        eng = cache[dtype, rb]
        eng.set_chunk_cone(True)
        assert eng.reach == generator_reach(CFG[rb])  # C and Python agree for every engine the tests create
        return eng
    return get


@pytest.fixture(scope="module")
def clips(gen_sd):
    """Three 40-row clips (time-major ln-mels) and, per resblock type, the oracle's waveform of each WHOLE clip;
    computed once, never modified."""
    mels = [np.ascontiguousarray(synth.synth_mel_log(1, 64, ROWS, seed=40 + 11 * b)[0].T) for b in range(3)]
    wavs = {}
    for rb, h in CFG.items():
        sd = _t(gen_sd[rb])
        with torch.no_grad():
            wavs[rb] = hifigan.generator(sd, h, torch.from_numpy(np.stack([m.T for m in mels])))[:, 0].numpy()
    return mels, wavs


def _spans(back, which):
    """(clip, first row, length, context, hold) of the named spans, all cut from 40-row clips."""
    table = {"start": (0, 0, 9, 0, 7),                                  # a stream's first emitting push
             "middle": (1, 5, back + 3 + 7, back, 7),                    # steady state
             "flush": (2, ROWS - back - 2, back + 2, back, 0),           # the clip's end
             "middle2": (2, 3, back + 4 + 5 + 7, back + 4, 7)}           # more history than needed, another length
    return [table[w] for w in which]


def _run_chunk(eng, mels, spans):
    x = torch.from_numpy(np.concatenate([mels[c][s:s + n] for c, s, n, _, _ in spans])).to(DEV)
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        wav = eng.forward_chunk(x, [n for _, _, n, _, _ in spans], [c for *_, c, _ in spans], [k for *_, k in spans])
        torch.cuda.synchronize()
        rec = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    return wav.cpu().numpy(), rec


def _against_whole_clips(what, wav, spans, ref, atol=1e-4):
    assert wav.shape == (sum(n - c - k for _, _, n, c, k in spans) * HOP,), (what, wav.shape)
    off = 0
    for clip, s, n, c, k in spans:
        m = (n - c - k) * HOP
        want = ref[clip][(s + c) * HOP:(s + n - k) * HOP]
        err = float(np.abs(wav[off:off + m] - want).max())
        print(f"{what}: rows {s + c}..{s + n - k - 1} of clip {clip}: max|d| vs the whole clip = {err:.2e}")
        assert err <= atol, (what, clip, err)
        off += m


# ---- 1. the chunk call against the oracle's whole clips ------------------------------------------------------------
# mixed: a start, a middle and a flush in one call, so neither side may be cropped; left / right: one side may;
# full: every clip has full context and hold
MIXES = {"mixed": ("start", "middle", "flush"), "left": ("middle", "flush"), "right": ("start", "middle"),
         "full": ("middle", "middle2")}


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("rb", ["1", "2"])
@pytest.mark.parametrize("mix", list(MIXES))
def test_chunk_call_vs_oracle_whole_clips(voc, clips, mix, rb, dtype):
    mels, ref = clips
    eng = voc(dtype, rb)
    spans = _spans(eng.reach[0], MIXES[mix])
    wav, rec = _run_chunk(eng, mels, spans)
    names = [r["name"] for r in rec]
    assert "chunk_wav_pack_kernel" in names and "ragged_wav_pack_kernel" not in names
    assert (CROP in names) == (mix != "mixed"), (mix, names)
    assert all(r["stage"] == "glue" for r in rec if r["name"] == CROP)
    assert {r["stage"].split("_")[0] for r in rec} <= {"glue", "voc", "ups", "mrf"}, rec
    _against_whole_clips(f"chunk {mix} rb{rb} {dtype}", wav, spans, ref[rb])


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("rb", ["1", "2"])
@pytest.mark.parametrize("mix", ["mixed", "left", "full"])
def test_chunk_call_with_the_cone_switched_off(voc, clips, mix, rb, dtype):
    mels, ref = clips
    eng = voc(dtype, rb)
    spans = _spans(eng.reach[0], MIXES[mix])
    on, _ = _run_chunk(eng, mels, spans)
    eng.set_chunk_cone(False)
    try:
        wav, rec = _run_chunk(eng, mels, spans)
    finally:
        eng.set_chunk_cone(True)
    assert CROP not in [r["name"] for r in rec]
    _against_whole_clips(f"chunk {mix} rb{rb} {dtype}, cone off", wav, spans, ref[rb])
    print(f"cone on vs off, {mix} rb{rb} {dtype}: max|d| = {float(np.abs(on - wav).max()):.2e}, "
          f"bit-equal {np.array_equal(on, wav)}")


def test_cone_shortens_the_stages(voc, clips):
    """Full context and hold, 3 new rows of 26: every MRF stage after the first runs on fewer rows than the span."""
    mels, _ = clips
    eng = voc("bf16x3")
    spans = _spans(16, ["middle"])
    _, rec = _run_chunk(eng, mels, spans)
    eng.set_chunk_cone(False)
    try:
        _, rec_off = _run_chunk(eng, mels, spans)
    finally:
        eng.set_chunk_cone(True)

    def flops(r, stage):
        return sum(x["flops"] for x in r if x["stage"] == stage)
    for stage, most in (("mrf_c256", 20 / 26), ("mrf_c128", 7 / 26), ("mrf_c64", 5 / 26), ("mrf_c32", 5 / 26)):
        ratio = flops(rec, stage) / flops(rec_off, stage)
        print(f"{stage}: cone / full algorithmic FLOPs = {ratio:.3f} (rows kept / 26 <= {most:.3f})")
        assert ratio <= most + 1e-9, (stage, ratio)


# ---- 2. streams ------------------------------------------------------------------------------------------------------
def _stream_clip(eng, mel, chunking):
    st, out, pos = VocoderStream(eng), [], 0
    for n in chunking:
        w = st.push(mel[pos:pos + n])
        pos += n
        assert w.shape == ((max(0, pos - st.ahead) - max(0, pos - n - st.ahead)) * eng.hop,)
        out.append(w)
    out.append(st.flush())
    return torch.cat(out)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "-".join(map(str, c)) if len(c) < 6 else f"{len(c)}x1")
def test_vocoder_stream_is_the_whole_clip(voc, clips, chunking, dtype):
    mels, ref = clips
    eng = voc(dtype)
    mel = torch.from_numpy(mels[0]).to(DEV)
    wav = _stream_clip(eng, mel, chunking)
    dense = eng.forward(mel[None], layout=1).view(-1)
    torch.cuda.synchronize()
    assert wav.shape == (ROWS * HOP,)
    e_or = float(np.abs(wav.cpu().numpy() - ref["1"][0]).max())
    e_dev = float((wav - dense).abs().max())
    print(f"stream {dtype} {chunking[:6]}: max|d| vs oracle {e_or:.2e}, vs the device's forward {e_dev:.2e}, "
          f"bit-equal to it: {torch.equal(wav, dense)}")
    assert e_or <= 1e-4
    assert e_dev <= 2e-4  # the two 1e-4 bars added


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_push_all_gives_each_stream_its_solo_result(voc, clips, dtype):
    mels, ref = clips
    eng = voc(dtype)
    dev = [torch.from_numpy(m).to(DEV) for m in mels]
    start, steps = [0, 5, 12], [3, 6, 10, 9]  # three phases: not emitting yet, just started, steady state
    streams = [VocoderStream(eng) for _ in range(3)]
    solo = [VocoderStream(eng) for _ in range(3)]
    got, want = [[] for _ in range(3)], [[] for _ in range(3)]
    for i, n in enumerate(start):
        if n:
            got[i].append(streams[i].push(dev[i][:n]))
            want[i].append(solo[i].push(dev[i][:n]))
    pos = list(start)
    for step in steps:
        _native.prof_enable(True)
        try:
            _native.prof_launches()
            res = push_all(streams, [dev[i][pos[i]:pos[i] + step] for i in range(3)])
            torch.cuda.synchronize()
            packs = sum(r["name"] == "chunk_wav_pack_kernel" for r in _native.prof_launches())
        finally:
            _native.prof_enable(False)
        assert packs == 1  # ONE engine call
        for i in range(3):
            got[i].append(res[i])
            want[i].append(solo[i].push(dev[i][pos[i]:pos[i] + step]))
        pos = [p + step for p in pos]
    for i in range(3):
        g, w = torch.cat(got[i]), torch.cat(want[i])
        assert g.shape == w.shape == ((pos[i] - 7) * HOP,)
        e_or = float(np.abs(g.cpu().numpy() - ref["1"][i][:g.shape[0]]).max())
        e_solo = float((g - w).abs().max())
        print(f"push_all {dtype} stream {i}: max|d| vs oracle {e_or:.2e}, vs solo {e_solo:.2e}")
        assert e_or <= 1e-4 and e_solo <= 2e-4


def _snr_db(ref, x):
    ref, x = np.asarray(ref, np.float64), np.asarray(x, np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / max(np.sum((ref - x) ** 2), 1e-30))


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_vocoder_stream_other_engines(voc, clips, dtype):
    """One chunking at the bar of the dtype's dense vocoder test against the same oracle: test_gpu_parity.py's
    test_vocoder_bf16_snr (25 dB), test_gpu_fp8.py's COS_MIN (0.99)."""
    mels, ref = clips
    eng = voc(dtype)
    wav = _stream_clip(eng, torch.from_numpy(mels[0]).to(DEV), [1, 2, 5, 17, 15]).cpu().numpy()
    assert wav.shape == (ROWS * HOP,) and np.isfinite(wav).all()
    snr, c = _snr_db(ref["1"][0], wav), _cos(wav, ref["1"][0])
    print(f"stream {dtype}: SNR {snr:.1f} dB, cos {c:.5f}")
    if dtype == "bf16":
        assert snr >= 25.0
    else:
        assert c >= 0.99


# ---- 3. frames to wav ------------------------------------------------------------------------------------------------
def test_speech_stream_frames_to_wav(voc):
    hw, T, pushes = (96, 80), 12, [1, 4, 7]
    ac_sd = synth.synth_acoustic_state(2)
    mean, std = synth.synth_scaler()
    pipe = runtime.Pipeline(runtime.AcousticEngine(ac_sd, dtype="bf16x3", device=DEV), voc("bf16x3"), mean, std)
    frames = synth.synth_frames(1, T, hw=hw, seed=100)[0]
    fr = torch.from_numpy(frames).to(DEV)
    st = SpeechStream(pipe, window=4)
    outs, pos = [], 0
    for n in pushes:
        o = st.push(fr[pos:pos + n])
        pos += n
        assert o["mel_norm"].shape == o["mel_db"].shape == o["mel_log"].shape == (n, 64)
        assert o["wav"].shape == ((max(0, pos - 7) - max(0, pos - n - 7)) * HOP,)
        outs.append(o)
    tail = st.flush()
    pipe.ac.check()
    mel_norm = torch.cat([o["mel_norm"] for o in outs])
    wav = torch.cat([o["wav"] for o in outs] + [tail])
    whole = pipe.forward_windowed(fr, [T], 4)
    assert torch.equal(mel_norm, whole["mel_norm"])
    assert wav.shape == (T * HOP,)
    sd = _t(ac_sd)
    with torch.no_grad():
        feats = effnet.effnet_gap(sd, torch.from_numpy(frames))
        _, mn = WR.latest(sd, feats, 4)
        ln = acoustic.mel_db_to_log(acoustic.denormalize_mel(mn, mean, std))
        ref = hifigan.generator(_t(synth.synth_generator_state(2, HIFIGAN_H)), HIFIGAN_H, ln.T[None])[0, 0].numpy()
    e_or = float(np.abs(wav.cpu().numpy() - ref).max())
    print(f"speech stream: max|d wav| vs oracle {e_or:.2e}, vs forward_windowed "
          f"{float((wav - whole['wav']).abs().max()):.2e}")
    assert e_or <= 1e-4


# ---- 4. contract -----------------------------------------------------------------------------------------------------
def _ints(v):
    return None if v is None else (C.c_int * len(v))(*v)


BAD = {"no_clip": dict(B=0), "zero_length": dict(lens=[9, 0, 17]), "negative_context": dict(ctx=[0, -1]),
       "negative_hold": dict(hold=[7, -1]), "nothing_to_emit": dict(ctx=[2, 16]),
       "context_is_len": dict(lens=[9, 16], ctx=[0, 16], hold=[7, 0]), "short": dict(rows=34), "long": dict(rows=36),
       "null_context": dict(ctx=None), "null_hold": dict(hold=None)}


@pytest.mark.parametrize("bad", list(BAD))
def test_argument_errors_before_any_launch(voc, bad):
    eng, L = voc("bf16x3"), _native.lib()
    a = dict(lens=[9, 26], ctx=[0, 16], hold=[7, 7], rows=None, B=None)
    a.update(BAD[bad])
    B = len(a["lens"]) if a["B"] is None else a["B"]
    rows = sum(a["lens"]) if a["rows"] is None else a["rows"]
    mel = torch.zeros(max(rows, 40), 64, device=DEV)
    wav = torch.zeros(40 * HOP, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)  # never reached: the call is refused first
    lens, ctx, hold = _ints(a["lens"]), _ints(a["ctx"]), _ints(a["hold"])
    if a["rows"] is None:  # the query takes no row count: sum(lengths) != rows is the call's own error
        assert L.m2s_vocoder_chunk_workspace_bytes(eng._h, lens, ctx, hold, B) == 0
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        rc = L.m2s_vocoder_forward_chunk(eng._h, mel.data_ptr(), lens, ctx, hold, B, rows, wav.data_ptr(), ws.data_ptr(),
                                         ws.numel(), torch.cuda.current_stream(DEV).cuda_stream)
        assert rc == 1, (bad, rc)  # M2S_E_ARG
        assert _native.prof_launches() == []
    finally:
        _native.prof_enable(False)
    if a["ctx"] is not None and a["hold"] is not None and B:
        with pytest.raises(ERRORS):
            eng.forward_chunk(mel[:rows], a["lens"], a["ctx"], a["hold"])
    assert float(wav.abs().max()) == 0.0
    good = eng.forward_chunk(mel[:35], [9, 26], [0, 16], [7, 7])  # the engine is usable afterwards
    assert good.shape == (5 * HOP,) and bool(torch.isfinite(good).all())


def test_stream_capture_is_refused(voc):
    eng, L = voc("bf16x3"), _native.lib()
    lens, ctx, hold = _ints([26]), _ints([16]), _ints([7])
    mel = torch.zeros(26, 64, device=DEV)
    wav = torch.zeros(3 * HOP, device=DEV)
    ws = torch.zeros(L.m2s_vocoder_chunk_workspace_bytes(eng._h, lens, ctx, hold, 1), dtype=torch.uint8, device=DEV)
    mark = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(DEV), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            mark.add_(1.0)  # the capture is not empty
            rc = L.m2s_vocoder_forward_chunk(eng._h, mel.data_ptr(), lens, ctx, hold, 1, 26, wav.data_ptr(),
                                             ws.data_ptr(), ws.numel(), side.cuda_stream)
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert rc == 3, rc  # M2S_E_STATE
    assert "captur" in L.m2s_last_error().decode()
    assert eng.forward_chunk(mel, [26], [16], [7]).shape == (3 * HOP,)  # the same call outside a capture runs


def test_opcheck_the_stream_op(voc, clips):
    mels, _ = clips
    v, o = voc("bf16x3"), ops.load()
    x = torch.from_numpy(np.concatenate([mels[0][:9], mels[1][5:31], mels[2][22:]])).to(DEV)
    assert ops.STREAM_OPS == ("hifigan_forward_chunk",)
    for args in [(v.handle, x, [9, 26, 18], [0, 16, 16], [7, 7, 0], v.hop),
                 (v.handle, x[9:35], [26], [16], [7], v.hop)]:
        torch.library.opcheck(o.hifigan_forward_chunk.default, args,
                              test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))


@pytest.mark.parametrize("cone", [True, False], ids=["cone", "cone_off"])
@pytest.mark.parametrize("mix", ["mixed", "left", "full"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3", "fp8"])
def test_workspace_contract(voc, clips, dtype, mix, cone):
    """include/m2s.h "Workspace contract" through tests/ws_harness.py: exact sizes, guards on every side, the same
    bits under every workspace fill, 256 bytes less refused, the engine usable afterwards."""
    mels, ref = clips
    eng, L = voc(dtype), _native.lib()
    spans = _spans(16, MIXES[mix])
    x = np.concatenate([mels[c][s:s + n] for c, s, n, _, _ in spans])
    lens, ctx, hold = ([v[i] for v in spans] for i in (2, 3, 4))
    cl, cc, ch = _ints(lens), _ints(ctx), _ints(hold)
    out_rows = sum(lens) - sum(ctx) - sum(hold)
    eng.set_chunk_cone(cone)
    try:
        nws = L.m2s_vocoder_chunk_workspace_bytes(eng._h, cl, cc, ch, len(lens))
        assert nws > 0 and nws % 256 == 0
        arena = H.Arena(DEV, [("mel", "in", x), ("wav", "out", (out_rows * HOP,)), ("ws", "ws", nws)])

        def call(a, n):
            return L.m2s_vocoder_forward_chunk(eng._h, a.ptr("mel"), cl, cc, ch, len(lens), x.shape[0], a.ptr("wav"),
                                               a.ptr("ws"), n, torch.cuda.current_stream(DEV).cuda_stream)

        what = f"vocoder_forward_chunk {dtype} {mix} cone {cone}"
        sync = lambda: torch.cuda.synchronize(DEV)  # noqa: E731
        rep = H.check_contract(arena, lambda a: call(a, nws), sync=sync, what=what)
        assert rep.deterministic, what
        H.check_undersized(arena, call, rep.outs["zero"], sync=sync, what=what)
        if dtype in ("fp32", "bf16x3"):
            _against_whole_clips(what, rep.outs["nan"]["wav"].cpu().numpy(), spans, ref["1"])
    finally:
        eng.set_chunk_cone(True)


# ---- 5. command line -------------------------------------------------------------------------------------------------
def test_cli_stream_writes_the_windowed_run(tmp_path):
    """run_mri_video_inference.py --stream 4: the files of the --window 4 run; the mel rows bit for bit (AcousticStream
    and the elementwise glue), the audio within the two 1e-4 bars added."""
    import importlib.util
    import json
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "m2s_cli_stream", os.path.join(repo, "mri-to-speech_amd", "scripts", "run_mri_video_inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    T = 11
    mean, std = synth.synth_scaler()
    ckdir = tmp_path / "ck" / "mri"
    ckdir.mkdir(parents=True)
    torch.save({"model_state_dict": _t(synth.synth_acoustic_state(4))}, ckdir / "best.pt")
    torch.save({"generator": _t(synth.synth_generator_state(4))}, tmp_path / "g_00000001")
    (tmp_path / "config.json").write_text(json.dumps(dict(HIFIGAN_H)))
    (tmp_path / "scaler.json").write_text(json.dumps({"mean": mean.tolist(), "std": std.tolist()}))
    np.save(tmp_path / "clip.npy", np.random.default_rng(0).integers(0, 256, size=(T, 256, 256), dtype=np.uint8))
    common = ["--video", str(tmp_path / "clip.npy"), "--mri-checkpoint", str(ckdir / "best.pt"), "--scaler-json",
              str(tmp_path / "scaler.json"), "--hifigan-config", str(tmp_path / "config.json"), "--hifigan-checkpoint",
              str(tmp_path / "g_00000001"), "--mri-code-dir", os.path.join(repo, "mri-to-speech_amd", "mri2speech_code")]
    got = cli.main([*common, "--output-dir", str(tmp_path / "stream"), "--stream", "4"])
    want = cli.main([*common, "--output-dir", str(tmp_path / "window"), "--window", "4"])
    assert sorted(p.name for p in (tmp_path / "stream").iterdir()) == sorted(p.name for p in (tmp_path / "window").iterdir())
    assert got["audio"].shape == want["audio"].shape == (T * HOP,)
    for k in ("mel_db", "mel_log"):
        assert np.array_equal(got[k], want[k]), k
    err = float(np.abs(got["audio"] - want["audio"]).max())
    print(f"--stream 4 vs --window 4: max|d audio| = {err:.2e}")
    assert err <= 2e-4
