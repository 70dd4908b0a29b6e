"""Same-process A/B of CNN kernels between engine switch settings: AcousticEngine.effnet on 1920 frames of
256 x 256 (AB_FRAMES=n), bf16x3, one engine per setting, alternating for AB_ROUNDS rounds (default 4) of 5
passes each; prints, per round and setting, the ms per pass of every kernel group from the engine's event
profiler, then per group the median and the spread (max - min over rounds) of each setting.  A gain counts
where one setting's slowest round is below the other's fastest.
argv: settings as NAME=VALUE[,NAME=VALUE...] (default M2S_ER_S2_FUSED=0 M2S_ER_S2_FUSED=1).
AB_GROUPS: `label:prefix[|prefix...]` groups separated by `;`, a launch counted in the first group one of whose
prefixes starts its name (default: blocks.2.0's launches, and se_ws by tile); AB_OUT=<file> also writes the
per-round values as JSON.  GPU box only."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mri-to-speech_amd"))

import torch  # noqa: E402

from m2s import _native, runtime as rt, synth  # noqa: E402

settings = sys.argv[1:] or ["M2S_ER_S2_FUSED=0", "M2S_ER_S2_FUSED=1"]
groups = [(g.split(":")[0], tuple(g.split(":")[1].split("|"))) for g in os.environ.get(
    "AB_GROUPS",
    "blocks.2.0:conv_gemm_kernel<128, 128, 4, 4, 2, 0, 0, 1|conv_gemm_kernel<128, 64, 4, 2, 3, 3, 0, 1>;"
    "se_ws 16x16:se_ws_kernel<4, 1, 8,;se_ws 8x8:se_ws_kernel<2, 2, 7,").split(";")]
dev = torch.device("cuda", 0)
rounds, calls = int(os.environ.get("AB_ROUNDS", "4")), 5
x = torch.rand(int(os.environ.get("AB_FRAMES", "1920")), 256, 256, device=dev)
sd = synth.synth_acoustic_state(1)
engines = {}
for st in settings:  # the switches are read once, at engine creation
    kv = dict(p.split("=") for p in st.split(","))
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    engines[st] = rt.AcousticEngine(sd, dtype="bf16x3", device=dev)
    for k, v in old.items():
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v
outs = {st: e.effnet(x) for st, e in engines.items()}
for e in engines.values():
    e.effnet(x)
torch.cuda.synchronize()
print("bit-equal outputs:", all(torch.equal(o, outs[settings[0]]) for o in outs.values()))
rec = {st: [] for st in settings}
for rnd in range(rounds):
    for st, e in engines.items():
        _native.prof_enable(True)
        _native.prof_launches()
        for _ in range(calls):
            e.effnet(x)
        torch.cuda.synchronize()
        launches = _native.prof_launches()
        _native.prof_enable(False)
        row = {label: dict(ms=0.0, launches=0) for label, _ in groups}
        for r in launches:
            for label, prefixes in groups:
                if r["name"].startswith(prefixes):
                    row[label]["ms"] += r["ms"] / calls
                    row[label]["launches"] += 1
                    break
        row["cnn"] = dict(ms=sum(r["ms"] for r in launches) / calls, launches=len(launches))
        for v in row.values():
            v["launches"] //= calls
        rec[st].append(row)
        print(f"round {rnd} {st:36s} " + "  ".join(f"{k} {v['ms']:6.3f} ms ({v['launches']})" for k, v in row.items()), flush=True)
for label in rec[settings[0]][0]:
    for st in settings:
        ms = [r[label]["ms"] for r in rec[st]]
        print(f"{label:12s} {st:36s} median {statistics.median(ms):6.3f} ms  min {min(ms):6.3f}  max {max(ms):6.3f}  spread {max(ms) - min(ms):5.3f}")
if os.environ.get("AB_OUT"):
    with open(os.environ["AB_OUT"], "w") as fh:
        json.dump(dict(frames=x.shape[0], calls_per_round=calls, rounds=rec), fh, indent=1)
