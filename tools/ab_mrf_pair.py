"""Same-process A/B of the split-fp32 MRF stages between engine switch settings: VocoderEngine.forward on the
64 x 30 mel (AB_SHAPE=CxF), one engine per setting, alternating for AB_ROUNDS rounds (default 4) of 5 calls
each; prints, per round and setting, the ms per call of every mrf_c* stage from the engine's event profiler,
then per stage the median and the spread (max - min over rounds) of each setting.  A gain counts where it is
larger than the largest spread.  argv: settings as NAME=VALUE[,NAME=VALUE...] (default M2S_MRF_PAIR=1
M2S_MRF_PAIR=0); AB_OUT=<file> also writes the per-round values as JSON.  GPU box only."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))

import torch  # noqa: E402

from m2s import _native, runtime as rt, synth  # noqa: E402
from m2s.config import HIFIGAN_H  # noqa: E402

settings = sys.argv[1:] or ["M2S_MRF_PAIR=1", "M2S_MRF_PAIR=0"]
dev = torch.device("cuda", 0)
nc, nf = (int(v) for v in os.environ.get("AB_SHAPE", "64x30").split("x"))
rounds, calls = int(os.environ.get("AB_ROUNDS", "4")), 5
mel = torch.from_numpy(synth.synth_mel_log(nc, 64, nf, seed=0)).to(dev)
sd = synth.synth_generator_state(0)
engines = {}
for st in settings:  # the switches are read once, at engine creation
    kv = dict(p.split("=") for p in st.split(","))
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    engines[st] = rt.VocoderEngine(sd, HIFIGAN_H, dtype="bf16x3", device=dev)
    for k, v in old.items():
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v
wavs = {st: e.forward(mel) for st, e in engines.items()}
for _ in range(2):
    for e in engines.values():
        e.forward(mel)
torch.cuda.synchronize()
print("bit-equal outputs:", all(torch.equal(w, wavs[settings[0]]) for w in wavs.values()))
rec = {st: [] for st in settings}
for rnd in range(rounds):
    for st, e in engines.items():
        _native.prof_enable(True)
        _native.prof_launches()
        for _ in range(calls):
            e.forward(mel)
        torch.cuda.synchronize()
        agg = {s["name"]: s for s in _native.aggregate(_native.prof_launches(), "stage")}
        _native.prof_enable(False)
        row = {k: dict(ms=v["ms"] / calls, launches=v["launches"] // calls) for k, v in sorted(agg.items())
               if k.startswith("mrf_c")}
        row["total"] = dict(ms=sum(v["ms"] for v in agg.values()) / calls, launches=sum(v["launches"] for v in agg.values()) // calls)
        rec[st].append(row)
        print(f"round {rnd} {st:32s} " + "  ".join(f"{k} {v['ms']:6.3f} ms ({v['launches']})" for k, v in row.items()), flush=True)
for stage in rec[settings[0]][0]:
    for st in settings:
        ms = [r[stage]["ms"] for r in rec[st]]
        print(f"{stage:8s} {st:32s} median {statistics.median(ms):6.3f} ms  spread {max(ms) - min(ms):5.3f}")
if os.environ.get("AB_OUT"):
    with open(os.environ["AB_OUT"], "w") as fh:
        json.dump(dict(shape=[nc, nf], calls_per_round=calls, rounds=rec), fh, indent=1)
