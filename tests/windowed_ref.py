"""CPU restatement of windowed acoustic inference (include/m2s.h "windowed inference") on the oracle.

``M(x)`` is the oracle's per-clip forward on ``k`` feature rows: ``acoustic.head(acoustic.bilstm_summerge(x))``,
both directions from zero state.  The three definitions are written as they read, one oracle call per window:

    latest   out[t] = M(x[max(0, t - W + 1) .. t])[last]
    mean     len <= W: M(x); otherwise the mean over the full windows w = 0 .. len - W containing t of
             M(x[w .. w + W - 1])[t - w]
    context  (latest) the first context rows are history: windows reach into them, no output row for them

Every function takes one clip of (len, 208) features and returns (y (rows, 640), mel_norm (rows, 64)) fp32, y
being the sum-merged hidden rows (averaged like mel_norm under ``mean``).
"""
import torch

from oracle import acoustic


def M(sd, x):
    """(k, 208) -> (y (k, 640), mel_norm (k, 64)): the whole-clip forward on these rows alone."""
    with torch.no_grad():
        y = acoustic.bilstm_summerge(sd, x[None])
        return y[0], acoustic.head(sd, y)[0]


def latest(sd, x, W, context=0):
    ys, ms = [], []
    for t in range(context, x.shape[0]):
        y, m = M(sd, x[max(0, t - W + 1):t + 1])
        ys.append(y[-1])
        ms.append(m[-1])
    return torch.stack(ys), torch.stack(ms)


def mean(sd, x, W):
    n = x.shape[0]
    if n <= W:
        return M(sd, x)
    ys = [[] for _ in range(n)]
    ms = [[] for _ in range(n)]
    for w in range(n - W + 1):
        y, m = M(sd, x[w:w + W])
        for s in range(W):
            ys[w + s].append(y[s])
            ms[w + s].append(m[s])
    return (torch.stack([torch.stack(v).mean(0) for v in ys]), torch.stack([torch.stack(v).mean(0) for v in ms]))


def windowed(sd, clips, W, merge="latest", context=None):
    """Packed result of a batch: ``clips`` a list of (len_b, 208) tensors -> (y, mel_norm) concatenated in clip
    order, as the engine returns them."""
    context = [0] * len(clips) if context is None else context
    assert merge in ("latest", "mean") and (merge == "latest" or not any(context))
    outs = [latest(sd, x, W, c) if merge == "latest" else mean(sd, x, W) for x, c in zip(clips, context)]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
