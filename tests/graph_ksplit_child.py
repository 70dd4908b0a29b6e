"""The split-K scratch of conv_gemm.hip under graph capture, in a process of its own.

``ksplit_scratch`` keeps one buffer per (device, stream) for the life of the process, and a capturing stream cannot
allocate: it borrows the device's largest buffer, or, if there is none, the launch runs unsplit.  Only a fresh
process has no buffer, so tests/test_gpu_graph.py starts this file once and asserts on the one JSON line it prints.
A bf16 vocoder, B = 1, T = 5, two different mels:

  (i)   an engine created under M2S_KSPLIT=1 runs both mels eagerly: the code objects are loaded, no split launch is
        planned and so no scratch is allocated;
  (ii)  an engine created under M2S_KSPLIT=4 has its FIRST call captured: nothing can be borrowed, every launch falls
        back to one K range, and the replays (inputs 0, 1, 0) are compared with (i)'s eager outputs;
  (iii) the same engine called eagerly plans its split launches and allocates scratch on its stream; captured again,
        the graph borrows that buffer and the replays are compared with this engine's own eager outputs.

Whether (i) and (iii) ran the same kernels apart from the partial-sum reduction is reported from the launch log; the
SNR of every result against the CPU oracle is reported too (the bf16 vocoder bar of tests/test_gpu_parity.py).

Helper program, not a test and not a conftest."""
import json
import os
import sys

RESULT_TAG = "GRAPH_KSPLIT_RESULT "
KSUM = "conv_gemm_ksum_kernel"


def _snr_db(ref, x):
    import numpy as np
    ref, x = np.asarray(ref, np.float64), np.asarray(x, np.float64)
    return float(10 * np.log10(np.sum(ref ** 2) / max(np.sum((ref - x) ** 2), 1e-30)))


def main():
    import numpy as np
    import torch

    import ws_harness as H
    from m2s import _native, runtime, synth
    from m2s.config import HIFIGAN_H
    from oracle import hifigan

    dev = torch.device("cuda", 0)
    sd = synth.synth_generator_state(6)
    mels = [synth.synth_mel_log(1, 64, 5, seed=70 + k) for k in (0, 1)]
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    with torch.no_grad():
        oracle = [hifigan.generator(tsd, HIFIGAN_H, torch.from_numpy(m)).numpy() for m in mels]
    xs = [torch.from_numpy(m).to(dev) for m in mels]

    def engine(ksplit):
        os.environ["M2S_KSPLIT"] = ksplit  # read once, when the engine is created (csrc/switches.hpp)
        try:
            return runtime.VocoderEngine(sd, HIFIGAN_H, dtype="bf16", device=dev)
        finally:
            del os.environ["M2S_KSPLIT"]

    def eager_logged(eng):
        torch.cuda.synchronize()
        _native.prof_enable(True)
        try:
            _native.prof_launches()
            out = [eng.forward(x).clone() for x in xs]
            torch.cuda.synchronize()
            names = [r["name"] for r in _native.prof_launches()]
        finally:
            _native.prof_enable(False)
        return out, names

    def captured(eng):
        """The call captured on a buffer holding input 0, then replayed on inputs 0, 1, 0."""
        buf = xs[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = eng.forward(buf)
        got = []
        for k in (0, 1, 0):
            buf.copy_(xs[k])
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            got.append(out.clone())
        return got

    e1 = engine("1")
    eager1, names1 = eager_logged(e1)                      # (i)
    e4 = engine("4")
    first = captured(e4)                                   # (ii)
    eager4, names4 = eager_logged(e4)                      # (iii)
    second = captured(e4)
    res = {
        "ksum_launches_ksplit1": sum(n.startswith(KSUM) for n in names1),
        "ksum_launches_ksplit4": sum(n.startswith(KSUM) for n in names4),
        "same_kernels": names1 == [n for n in names4 if not n.startswith(KSUM)],
        "first_capture_equals_ksplit1_eager": [H.bits_equal(first[i], eager1[k]) for i, k in enumerate((0, 1, 0))],
        "first_capture_snr_db": [_snr_db(oracle[k], first[i].cpu().numpy()) for i, k in enumerate((0, 1, 0))],
        "eager_ksplit4_snr_db": min(_snr_db(oracle[k], eager4[k].cpu().numpy()) for k in (0, 1)),
        "second_capture_equals_own_eager": [H.bits_equal(second[i], eager4[k]) for i, k in enumerate((0, 1, 0))],
    }
    print(RESULT_TAG + json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":  # the paths tests/conftest.py sets for the suite
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_repo, "mri-to-speech_amd"), _repo):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    sys.exit(main())
