"""One dense BiLSTM call on the hard weights, measured against the float64 reference (tests/lstm_hard.py).

``measure`` is what test_gpu_lstm_hard.py runs per case.  Run as a program, this file measures a list of cases in a
process of its own and prints them as one JSON line: ``M2S_LSTM_SMALL_B`` and ``M2S_LSTM_MID_CH`` are read at their
first use in a process and frozen (csrc/switches.hpp), so the cases that set them need a fresh process each; the
test starts it with the variable in its environment and a time limit.

    python tests/lstm_hard_child.py '[["hard", "fp32", 5, 40], ...]'

Helper module, not a test and not a conftest.
"""
import json
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":  # the paths tests/conftest.py sets for the suite
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_repo, "mri-to-speech_amd"), _repo):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import lstm_hard as LH  # noqa: E402

RESULT_TAG = "LSTM_HARD_RESULT "


def recorded(eng, call):
    """(what ``call()`` returned, the launch records of it), the engine checked in between."""
    from m2s import _native
    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()  # start from an empty record
        out = call()
        eng.check()
        rec = _native.prof_launches()
    finally:
        _native.prof_enable(False)
    return out, rec


def worst(got, want) -> float:
    """max |got - want| in float64; inf when ``got`` holds a non-finite value."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) if np.isfinite(got).all() else float("inf")


def measure(eng, kind, B, T):
    """``eng.bilstm`` on ``LH.reference(kind, B, T)``: worst |d y|, worst |d mel_norm| and the names of the ``lstm_``
    launches the call recorded."""
    x, y_ref, m_ref = LH.reference(kind, B, T)
    (y, m), rec = recorded(eng, lambda: eng.bilstm(x.to(eng.device)))
    assert y.shape == (B, T, 640) and m.shape == (B, T, 64)
    return {"y": worst(y, y_ref), "mel": worst(m, m_ref),
            "kernels": sorted({r["name"] for r in rec if r["name"].startswith("lstm_")})}


def main(argv):
    from m2s import runtime
    dev = torch.device("cuda", 0)
    engines, out = {}, []
    for kind, dtype, B, T in json.loads(argv[1]):
        if (kind, dtype) not in engines:
            st = {"hard": LH.hard_acoustic_state, "sat": LH.saturating_acoustic_state}[kind](LH.SEED)
            engines[kind, dtype] = runtime.AcousticEngine(st, dtype=dtype, device=dev)
        out.append(measure(engines[kind, dtype], kind, B, T))
    print(RESULT_TAG + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
