"""CPU restatement of the streaming vocoder (include/m2s.h "streaming vocoder") on the oracle, in float64.

    G(x)            oracle/hifigan.generator on the rows x as a whole clip: both ends of x are clip ends
    chunk           the chunk call's contract, as it reads: G(x_b)[context_b * hop : (len_b - hold_b) * hop], packed
    measured_reach  which output frames one mel row touches, by perturbing it (to first order): row r changes frames
                    r - ahead .. r + back, so (back, ahead) = (last - r, r - first)
    OracleEngine    what m2s.stream.VocoderStream needs of an engine (reach, hop, forward_chunk), over ``chunk``;
                    ``reach`` may be set wrong on purpose, to show that the yardstick notices

Everything takes time-major (T, num_mels) mels, as the engine's packed calls do.
"""
import numpy as np
import torch

from oracle import hifigan


def hop_of(h):
    return int(np.prod(h["upsample_rates"]))


def to64(sd):
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}


def G(sd64, h, x):
    """x (T, num_mels) -> (T * hop,) float64."""
    with torch.no_grad():
        return hifigan.generator(sd64, h, torch.as_tensor(x).double().T[None])[0, 0]


def chunk(sd64, h, mel, lengths, context, hold):
    hop, out, off = hop_of(h), [], 0
    for n, c, k in zip(lengths, context, hold):
        assert n >= 1 and c >= 0 and k >= 0 and c + k < n, (n, c, k)
        out.append(G(sd64, h, mel[off:off + n])[c * hop:(n - k) * hop])
        off += n
    assert off == mel.shape[0]
    return torch.cat(out)


def _touched(d, rows, hop, row):
    hit = (d != 0).view(rows, hop).any(dim=1).nonzero().view(-1)
    return int(hit[-1]) - row, row - int(hit[0])


def measured_reach(sd64, h, rows, row, seed=0):
    """(back, ahead) seen from mel row ``row`` of a ``rows``-row clip: that row is perturbed and the output frames that
    change are counted.  The perturbation is taken to first order, as the tangent of the oracle along the row
    (forward-mode differentiation of the very same function), because a finite difference of two float64 waveforms
    is not a reliable yardstick here, in either direction: the farthest frame hangs on a chain of single edge taps,
    2.5e-20 per unit of the row in the shipped config, below an ulp of the O(0.1) waveform; and a CPU's convolution
    may round the same position differently in two runs or batch entries, which shows as changed frames where no path
    exists (both seen, on different machines).  A tangent is a sum of products, not a difference of waveforms: it is
    zero exactly where no path exists, and LeakyReLU's and tanh's slopes are never zero."""
    hop = hop_of(h)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, h["num_mels"], generator=g, dtype=torch.float64)
    t = torch.zeros_like(x)
    t[row] = 1.0
    with torch.no_grad():
        _, tan = torch.func.jvp(lambda m: hifigan.generator(sd64, h, m.T[None])[0, 0], (x,), (t,))
    return _touched(tan, rows, hop, row)


class OracleEngine:
    """The engine interface of VocoderStream on the oracle; ``calls`` records (lengths, context, hold) per call."""

    def __init__(self, sd, h, reach):
        self.sd64, self.h, self.reach, self.hop = to64(sd), h, tuple(reach), hop_of(h)
        self.calls = []

    def forward_chunk(self, mel, lengths=None, context=None, hold=None):
        if isinstance(mel, (list, tuple)):
            lengths = [int(m.shape[0]) for m in mel]
            mel = torch.cat(list(mel))
        self.calls.append((list(lengths), list(context), list(hold)))
        return chunk(self.sd64, self.h, mel, lengths, context, hold)
