"""The execution plans of the engines as data: for a fixed list of small cases, the launches each call records
(m2s._native.prof_launches: name, stage, flops, bytes, spill_bytes; not ms) and the sha256 of every output tensor.

  python tools/plan_dump.py --plan launch_plan.json [--hashes output_hashes.json]

The launch lists are what tests/test_gpu_launch_plan.py replays against tests/golden/launch_plan.json: a change to the
host code that plans the launches (csrc/acoustic_cnn.cpp, acoustic_rnn.cpp, vocoder.cpp) shows there as a changed
kernel, order or recorded cost.  The output hashes are for comparing two builds on one machine by hand (a refactor
of the plans must leave every one identical); they are not committed.

The plan file keeps the kernel and stage names in two tables and, per case, rows of
[kernel, stage, flops, bytes, spill_bytes, repeats]: consecutive equal records are run-length encoded (the fp32
BiLSTM's per-step launches), numbers are written by repr so they read back exactly.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from collections import namedtuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "mri-to-speech_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS = ("name", "stage", "flops", "bytes", "spill_bytes")
REL_TOL = 1e-12  # a reassociated double expression, nothing else

# name: unique; env: M2S_* switches set before the case's engines are created; make(ctx) creates the engines and
# inputs and returns the call to record, which returns the list of output tensors
Case = namedtuple("Case", "name env make")


class Context:
    """Weights, inputs and engines shared by the cases.  An engine is created once per (kind, dtype, chunk,
    switches): the switches are read when an engine is created, so ``env`` (what the running case has set) is part of
    the key."""

    def __init__(self, device=None):
        import torch
        from m2s import runtime, synth
        from m2s.config import HIFIGAN_H
        self.torch, self.rt, self.synth, self.h = torch, runtime, synth, HIFIGAN_H
        self.dev = torch.device("cuda", 0) if device is None else device
        self.ac_sd, self.gen_sd = synth.synth_acoustic_state(11), synth.synth_generator_state(12)
        self.mean, self.std = synth.synth_scaler()
        self.env = ()
        self._engines = {}

    def _engine(self, key, create):
        key = key + (self.env,)
        if key not in self._engines:
            self._engines[key] = create()
        return self._engines[key]

    def acoustic(self, dtype, chunk=None):
        kw = {} if chunk is None else {"chunk": chunk}
        return self._engine(("ac", dtype, chunk),
                            lambda: self.rt.AcousticEngine(self.ac_sd, dtype=dtype, device=self.dev, **kw))

    def vocoder(self, dtype, h=None):  # h: another generator config than HIFIGAN_H, with weights of its own
        if h is None:
            return self._engine(("voc", dtype), lambda: self.rt.VocoderEngine(self.gen_sd, self.h, dtype=dtype,
                                                                              device=self.dev))
        return self._engine(("voc", dtype, json.dumps(h, sort_keys=True)), lambda: self.rt.VocoderEngine(
            self.synth.synth_generator_state(12, h), h, dtype=dtype, device=self.dev))

    def pipeline(self, dtype):
        return self.rt.Pipeline(self.acoustic(dtype), self.vocoder(dtype), self.mean, self.std)

    def frames(self, clips, n, seed=5):  # (clips, n, 256, 256)
        return self.torch.from_numpy(self.synth.synth_frames(clips, n, seed=seed)).to(self.dev)

    def feats(self, *shape, seed=21):
        import numpy as np
        x = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
        return self.torch.from_numpy(x).to(self.dev)

    def mel(self, B, T, seed=3):  # (B, num_mels, T) ln-power mel
        return self.torch.from_numpy(self.synth.synth_mel_log(B, self.h["num_mels"], T, seed=seed)).to(self.dev)

    def mel_rows(self, n, seed=3):  # packed (n, num_mels)
        return self.mel(1, n, seed)[0].t().contiguous()


def _ac(method, dtype, *args, chunk=None, frames=None, feats=None, **kw):
    def make(ctx):
        eng = ctx.acoustic(dtype, chunk)
        x = ctx.frames(*frames) if frames else ctx.feats(*feats)
        if frames and method != "forward":
            x = x[0]  # packed frame rows (N, H, W)
        return lambda: _as_list(getattr(eng, method)(x, *args, **kw))
    return make


def _voc(method, dtype, mel, *args, h=None, **kw):
    def make(ctx):
        eng = ctx.vocoder(dtype, h)
        x = ctx.mel(*mel) if isinstance(mel, tuple) else ctx.mel_rows(mel)
        return lambda: _as_list(getattr(eng, method)(x, *args, **kw))
    return make


def _voc_chunk_cone(dtype):
    """Two spans that bring the generator's whole reach as context and hold: the cone crops between the stages."""
    def make(ctx):
        eng = ctx.vocoder(dtype)
        back, ahead = eng.reach
        lengths = [back + ahead + 3, back + ahead + 2]
        x = ctx.mel_rows(sum(lengths))
        return lambda: [eng.forward_chunk(x, lengths, [back, back], [ahead, ahead])]
    return make


def _pipe(method, dtype, frames, *args):
    def make(ctx):
        pipe = ctx.pipeline(dtype)
        x = ctx.frames(*frames)
        if method != "forward":
            x = x[0]
        return lambda: _as_list(getattr(pipe, method)(x, *args))
    return make


def _as_list(out):
    if isinstance(out, dict):
        return [out[k] for k in sorted(out)]
    return list(out) if isinstance(out, (list, tuple)) else [out]


DTYPES = ("fp32", "bf16", "bf16x3", "fp8")
PERSISTENT = {"M2S_IRWS_MIN": "0", "M2S_SEWS_MIN": "0"}  # ir_ws / se_ws at any pass size

# MRF routes of the generator (csrc/voc_route.hpp) that the voc_forward_* cases below do not take, each one forward of
# 1 x 8 frames: (case suffix, dtype, switches, config or None for HIFIGAN_H).  tests/test_gpu_voc_route.py runs the same
VOC_ROUTE_CASES = (
    ("bf16_nofused", "bf16", {"M2S_MRF_FUSED": "0"}, None),
    ("fp8_nofused", "fp8", {"M2S_MRF_FUSED": "0"}, None),
    ("bf16x3_nobatch", "bf16x3", {"M2S_MRF_BATCH": "0"}, None),
    ("bf16x3_nohalo_pair128", "bf16x3", {"M2S_MRF_HALO": "0", "M2S_MRF_PAIR128": "1"}, None),
    ("fp8_mrf32", "fp8", {"M2S_F8_MRF32": "1"}, None),
    ("fp8_mrf64_nofused", "fp8", {"M2S_F8_MRF64": "1", "M2S_MRF_FUSED": "0"}, None),
    ("bf16x3_r2", "bf16x3", {}, "r2"),
)


def _h_r2():  # resblock "2": one conv per dilation (tests/test_pack_cpu.py H_R2)
    from m2s.config import HIFIGAN_H
    return dict(HIFIGAN_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])


CASES = (
    # ---- acoustic
    [Case(f"ac_forward_1x3_{d}", {}, _ac("forward", d, frames=(1, 3))) for d in DTYPES]
    + [Case("ac_forward_1x3_bf16x3_persistent", PERSISTENT, _ac("forward", "bf16x3", frames=(1, 3))),
       # ... and no split K (read, like every switch, when the case's engine is created): blocks.2.0 on
       # launch_conv_gemm_er
       Case("ac_forward_1x3_bf16x3_persistent_ksplit1", dict(PERSISTENT, M2S_KSPLIT="1"),
            _ac("forward", "bf16x3", frames=(1, 3)))]
    + [Case(f"ac_forward_1x9_chunk4_{d}", {}, _ac("forward", d, frames=(1, 9), chunk=4)) for d in ("bf16x3", "fp32")]
    + [Case(f"ac_probe_{n}_bf16x3", {}, _ac("probe", "bf16x3", n, frames=(1, 3))) for n in (1, 3)]
    + [Case(f"ac_bilstm_{B}x3_{d}", {}, _ac("bilstm", d, feats=(B, 3, 208))) for d in ("fp32", "bf16x3")
       for B in (2, 5, 17)]
    + [Case("ac_bilstm_ragged_3_1_2", {}, _ac("bilstm_ragged", "bf16x3", [3, 1, 2], feats=(6, 208))),
       Case("ac_bilstm_windowed4_latest", {}, _ac("bilstm_windowed", "bf16x3", [5, 2], 4, "latest", feats=(7, 208))),
       Case("ac_bilstm_windowed4_latest_fp32", {}, _ac("bilstm_windowed", "fp32", [5, 2], 4, "latest", feats=(7, 208))),
       Case("ac_bilstm_windowed4_latest_context", {},
            _ac("bilstm_windowed", "bf16x3", [5, 2], 4, "latest", [1, 0], feats=(7, 208))),
       Case("ac_bilstm_windowed4_mean", {}, _ac("bilstm_windowed", "bf16x3", [5, 2], 4, "mean", feats=(7, 208))),
       Case("ac_bilstm_windowed1", {}, _ac("bilstm_windowed", "bf16x3", [5, 2], 1, "latest", feats=(7, 208))),
       Case("ac_bilstm_pairs4", {}, _ac("bilstm_pairs", "bf16x3", [5, 4], 4, feats=(9, 208))),
       Case("ac_forward_ragged_3_2", {}, _ac("forward_ragged", "bf16x3", [3, 2], frames=(1, 5))),
       Case("ac_forward_windowed4_5_2", {}, _ac("forward_windowed", "bf16x3", [5, 2], 4, "latest", frames=(1, 7))),
       Case("ac_forward_pairs4_5_4", {}, _ac("forward_pairs", "bf16x3", [5, 4], 4, frames=(1, 9)))]
    # ---- vocoder
    + [Case(f"voc_forward_1x8_{d}", {}, _voc("forward", d, (1, 8))) for d in DTYPES]
    + [Case("voc_forward_2x40_bf16x3", {}, _voc("forward", "bf16x3", (2, 40))),
       Case("voc_forward_1x8_bf16x3_pair128", {"M2S_MRF_PAIR128": "1"}, _voc("forward", "bf16x3", (1, 8))),
       Case("voc_forward_1x8_bf16x3_nopair", {"M2S_MRF_PAIR": "0"}, _voc("forward", "bf16x3", (1, 8))),
       Case("voc_forward_1x8_bf16x3_nohalo", {"M2S_MRF_HALO": "0"}, _voc("forward", "bf16x3", (1, 8))),
       Case("voc_forward_1x8_fp8_mrf64", {"M2S_F8_MRF64": "1"}, _voc("forward", "fp8", (1, 8))),
       Case("voc_forward_ragged_8_5", {}, _voc("forward_ragged", "bf16x3", 13, [8, 5])),
       Case("voc_forward_chunk_cone", {}, _voc_chunk_cone("bf16x3")),
       Case("voc_forward_chunk_zeros", {}, _voc("forward_chunk", "bf16x3", 13, [8, 5], [0, 0], [0, 0]))]
    # ---- pipeline
    + [Case(f"pipe_forward_1x3_{d}", {}, _pipe("forward", d, (1, 3))) for d in ("bf16x3", "fp32")]
    + [Case("pipe_forward_ragged_3_2", {}, _pipe("forward_ragged", "bf16x3", (1, 5), [3, 2]))]
    # ---- vocoder, the other MRF routes (last: the golden's kernel and stage tables keep their order)
    + [Case("voc_forward_1x8_" + name, env, _voc("forward", d, (1, 8), h=_h_r2() if h == "r2" else None))
       for name, d, env, h in VOC_ROUTE_CASES]
)


def run_case(case, ctx, setenv):
    """(launch records, output tensors) of one case.  ``setenv(name, value)`` sets the case's switches; undoing
    them afterwards is the caller's (pytest's monkeypatch.setenv, or ``main`` below)."""
    from m2s import _native
    for k, v in case.env.items():
        setenv(k, v)
    ctx.env = tuple(sorted(case.env.items()))
    call = case.make(ctx)
    ctx.torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        outs = call()
        ctx.torch.cuda.synchronize()
        launches = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    return [{f: r[f] for f in FIELDS} for r in launches], outs


def tensor_sha256(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def encode(plans: dict) -> dict:
    """{case: [record]} -> the plan file's tables and run-length-encoded rows."""
    kernels, stages, cases = [], [], {}

    def idx(table, v):
        if v not in table:
            table.append(v)
        return table.index(v)

    for name, recs in plans.items():
        rows = []
        for r in recs:
            row = [idx(kernels, r["name"]), idx(stages, r["stage"]), r["flops"], r["bytes"], r["spill_bytes"]]
            if rows and rows[-1][:5] == row:
                rows[-1][5] += 1
            else:
                rows.append(row + [1])
        cases[name] = rows
    return {"kernels": kernels, "stages": stages, "cases": cases}


def decode(doc: dict) -> dict:
    out = {}
    for name, rows in doc["cases"].items():
        out[name] = [dict(name=doc["kernels"][k], stage=doc["stages"][st], flops=fl, bytes=by, spill_bytes=sp)
                     for k, st, fl, by, sp, n in rows for _ in range(n)]
    return out


def _close(a: float, b: float) -> bool:
    return abs(a - b) <= REL_TOL * max(abs(a), abs(b))


def plan_diff(want, got):
    """The first difference between two launch lists as a message, or None: names and stages exactly, the recorded
    costs to a relative REL_TOL."""
    for i, (w, g) in enumerate(zip(want, got)):
        for f in ("name", "stage"):
            if w[f] != g[f]:
                return f"launch {i}: {f} {g[f]!r}, recorded {w[f]!r}"
        for f in ("flops", "bytes", "spill_bytes"):
            if not _close(w[f], g[f]):
                return f"launch {i} ({w['name']}): {f} {g[f]!r}, recorded {w[f]!r}"
    if len(want) != len(got):
        return f"{len(got)} launches, recorded {len(want)}"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--plan", required=True, help="write the launch lists here (tests/golden/launch_plan.json)")
    ap.add_argument("--hashes", help="write the sha256 of every case's output tensors here")
    args = ap.parse_args()
    ctx = Context()
    plans, hashes = {}, {}
    for case in CASES:
        saved = {k: os.environ.get(k) for k in case.env}
        try:
            recs, outs = run_case(case, ctx, os.environ.__setitem__)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        plans[case.name] = recs
        hashes[case.name] = [tensor_sha256(t) for t in outs]
        print(f"{case.name}: {len(recs)} launches, {len(outs)} outputs", flush=True)
    with open(args.plan, "w") as f:
        json.dump(encode(plans), f, separators=(",", ":"))
        f.write("\n")
    if args.hashes:
        with open(args.hashes, "w") as f:
            json.dump(hashes, f, indent=1)
            f.write("\n")
    print(f"{len(CASES)} cases, {sum(len(r) for r in plans.values())} launches")


if __name__ == "__main__":
    main()
