"""Guarded buffers for calling libm2s the way a C integrator does (include/m2s.h "Workspace contract").

Every input, output and workspace buffer of one call is carved out of ONE ``torch.uint8`` tensor.  Each buffer
starts 256-byte aligned, has exactly its documented size, and has a guard band of 1 MiB in front of it and
another one right behind its last byte:

    [front guard 0xA5][buffer][back guard: 0xA5, or 0xFF behind an input] ... next buffer

Before a run the guards are refilled, the outputs are set to 0xFF (NaN as fp32) and the workspace to one of

    "zero"    0x00
    "nan"     0xFF: NaN as fp32, as bf16 and as e4m3
    "random"  seeded random bytes
    "stale"   what an earlier, larger call of the same engine left in its workspace (``Arena.prepare(stale=...)``)

After the run ``Arena.violations()`` lists every guard byte that changed (a write outside a buffer; behind an
input the guard is NaN, so an over-read shows up in the result instead) and every output that still holds a
NaN (an element never written, or one computed from workspace or from bytes past an input).
``check_contract`` runs a call under every fill and asserts the contract; ``check_undersized`` is the
too-small-workspace case.  Nothing here needs a GPU: tests/test_workspace_harness_cpu.py drives the same code
with CPU tensors and fake calls that break each rule.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

GUARD = 1 << 20
ALIGN = 256
GUARD_BYTE = 0xA5
POISON = 0xFF
M2S_OK, M2S_E_ARG = 0, 1  # include/m2s.h m2s_status
FILLS = ("zero", "nan", "random", "stale")


def _up(n: int, a: int = ALIGN) -> int:
    return (n + a - 1) // a * a


class _Buf:
    def __init__(self, name, kind, nbytes, shape, dtype, front, off):
        self.name, self.kind, self.nbytes, self.shape, self.dtype = name, kind, nbytes, shape, dtype
        self.front, self.off = front, off  # front guard = [front, off), back guard = [off + nbytes, + GUARD)

    @property
    def back(self):
        return self.off + self.nbytes


class Arena:
    """``specs``: (name, "in", array) | (name, "out", shape) fp32 | (name, "ws", nbytes), in memory order."""

    def __init__(self, device, specs: Sequence[tuple]):
        self.device = torch.device(device)
        self.bufs: Dict[str, _Buf] = {}
        inputs = {}
        pos = 0
        for name, kind, what in specs:
            assert name not in self.bufs, name
            if kind == "in":
                t = torch.as_tensor(np.ascontiguousarray(what) if isinstance(what, np.ndarray) else what).contiguous()
                inputs[name] = t
                nbytes, shape, dtype = t.numel() * t.element_size(), tuple(t.shape), t.dtype
            elif kind == "out":
                shape = tuple(int(d) for d in what)
                nbytes, dtype = 4 * int(np.prod(shape, dtype=np.int64)), torch.float32
            else:
                assert kind == "ws", kind
                nbytes, shape, dtype = int(what), (int(what),), torch.uint8
            assert nbytes > 0, (name, nbytes)
            off = _up(pos + GUARD)
            self.bufs[name] = _Buf(name, kind, nbytes, shape, dtype, pos, off)
            pos = off + nbytes + GUARD
        self.mem = torch.empty(pos + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.mem.data_ptr()) % ALIGN  # buffer starts are 256-byte aligned addresses
        self.mem.fill_(GUARD_BYTE)
        for name, t in inputs.items():
            self.raw(name).copy_(t.view(-1).view(torch.uint8).to(self.device))

    # ---- views -------------------------------------------------------------------------------------------
    def _span(self, lo: int, hi: int) -> torch.Tensor:
        return self.mem[self.base + lo:self.base + hi]

    def raw(self, name: str) -> torch.Tensor:
        b = self.bufs[name]
        return self._span(b.off, b.back)

    def view(self, name: str) -> torch.Tensor:
        b = self.bufs[name]
        return self.raw(name).view(b.dtype).view(b.shape)

    def ptr(self, name: Optional[str]) -> Optional[int]:
        """Device address for ctypes (None -> NULL)."""
        if name is None:
            return None
        p = self.mem.data_ptr() + self.base + self.bufs[name].off
        assert p % ALIGN == 0
        return p

    def nbytes(self, name: str) -> int:
        return self.bufs[name].nbytes

    def names(self, kind: str) -> List[str]:
        return [n for n, b in self.bufs.items() if b.kind == kind]

    # ---- fills -------------------------------------------------------------------------------------------
    def prepare(self, fill: str, seed: int = 0, stale: Optional[torch.Tensor] = None) -> None:
        for b in self.bufs.values():
            self._span(b.front, b.off).fill_(GUARD_BYTE)
            self._span(b.back, b.back + GUARD).fill_(POISON if b.kind == "in" else GUARD_BYTE)
            if b.kind == "out":
                self.raw(b.name).fill_(POISON)
            elif b.kind == "ws":
                w = self.raw(b.name)
                if fill == "zero":
                    w.zero_()
                elif fill == "nan":
                    w.fill_(POISON)
                elif fill == "random":
                    g = torch.Generator(device=self.device).manual_seed(seed)
                    w.copy_(torch.randint(0, 256, (b.nbytes,), dtype=torch.uint8, generator=g, device=self.device))
                elif fill == "stale":
                    assert stale is not None and stale.numel() >= b.nbytes, "stale fill needs a larger workspace image"
                    w.copy_(stale[:b.nbytes].to(self.device))
                else:
                    raise ValueError(fill)

    # ---- checks ------------------------------------------------------------------------------------------
    def violations(self, outputs_written: bool = True) -> List[str]:
        regions, labels = [], []
        for b in self.bufs.values():
            regions.append(self._span(b.front, b.off) != GUARD_BYTE)
            labels.append(f"guard in front of {b.name!r} overwritten")
            want = POISON if b.kind == "in" else GUARD_BYTE
            regions.append(self._span(b.back, b.back + GUARD) != want)
            labels.append(f"guard behind {b.name!r} overwritten")
            if b.kind == "out" and outputs_written:
                regions.append(torch.isnan(self.view(b.name)).reshape(-1))
                labels.append(f"output {b.name!r} holds NaN (unwritten or contaminated elements)")
        counts = torch.stack([r.sum() for r in regions]).cpu().tolist()
        found = []
        for r, label, n in zip(regions, labels, counts):
            if n:
                first = int(torch.nonzero(r)[0, 0])
                found.append(f"{label}: {n} of {r.numel()}, first at +{first}")
        return found

    def outputs(self) -> Dict[str, torch.Tensor]:
        return {n: self.view(n).clone() for n in self.names("out")}

    def workspace_image(self) -> torch.Tensor:
        (ws,) = self.names("ws")
        return self.raw(ws).clone()


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _noop():
    return None


class Report:
    """``outs[fill]``: the outputs of the run under that fill ("zero2" = the repeated zero run)."""

    def __init__(self):
        self.outs: Dict[str, Dict[str, torch.Tensor]] = {}
        self.deterministic = True
        self.max_fill_diff: Dict[str, float] = {}


def check_contract(arena: Arena, call: Callable[[Arena], int], *, sync: Callable[[], None] = _noop,
                   status: Callable[[], int] = lambda: M2S_OK, stale: Optional[torch.Tensor] = None,
                   tol: Optional[Dict[str, float]] = None, what: str = "") -> Report:
    """Run ``call`` under fills zero, zero again, nan, random and (with ``stale``) stale; assert for each run:
    M2S_OK, a clean engine status, intact guards, no NaN in an output; and across the runs: bit-identical
    outputs.  If the two zero runs differ the call is nondeterministic (``Report.deterministic`` = False, a
    finding of its own); the fills are then compared at ``tol`` (name -> max |d|), or fail without one."""
    rep = Report()
    runs = [("zero", "zero"), ("zero2", "zero"), ("nan", "nan"), ("random", "random")]
    if stale is not None:
        runs.append(("stale", "stale"))
    for key, fill in runs:
        arena.prepare(fill, seed=1234, stale=stale)
        sync()
        rc = call(arena)
        sync()
        assert rc == M2S_OK, f"{what} [{key}]: return code {rc}"
        st = status()
        assert st == M2S_OK, f"{what} [{key}]: engine status {st}"
        bad = arena.violations()
        assert not bad, f"{what} [workspace fill {key}]: " + "; ".join(bad)
        rep.outs[key] = arena.outputs()
    base = rep.outs["zero"]
    rep.deterministic = all(bits_equal(base[n], rep.outs["zero2"][n]) for n in base)
    for key, _ in runs[1:]:
        for n in base:
            if bits_equal(base[n], rep.outs[key][n]):
                continue
            d = float((base[n].double() - rep.outs[key][n].double()).abs().max())
            rep.max_fill_diff[f"{key}:{n}"] = d
            if key == "zero2":
                continue  # the control itself: recorded in rep.deterministic
            if rep.deterministic:
                raise AssertionError(f"{what}: output {n!r} depends on the workspace contents "
                                     f"(fill {key} vs zero: max |d| = {d:.3e})")
            else:
                assert tol is not None and n in tol and d <= tol[n], (
                    f"{what}: nondeterministic call, and output {n!r} differs between fills zero and {key} by "
                    f"{d:.3e} (allowed {None if tol is None else tol.get(n)})")
    return rep


def check_undersized(arena: Arena, call: Callable[[Arena, int], int], good: Dict[str, torch.Tensor], *,
                     sync: Callable[[], None] = _noop, status: Callable[[], int] = lambda: M2S_OK,
                     exact: bool = True, what: str = "") -> None:
    """``call(arena, ws_bytes)``: 256 bytes less than reported -> M2S_E_ARG and intact guards; then the right size
    on the same engine -> the bits of ``good`` (the zero-fill outputs).  ``exact`` False: the second half only
    compares NaN-free outputs at the call's own repeatability (for calls found nondeterministic)."""
    (ws,) = arena.names("ws")
    arena.prepare("nan")
    sync()
    rc = call(arena, arena.nbytes(ws) - 256)
    sync()
    assert rc == M2S_E_ARG, f"{what}: workspace 256 bytes short returned {rc}, expected M2S_E_ARG"
    bad = arena.violations(outputs_written=False)
    assert not bad, f"{what} [undersized]: " + "; ".join(bad)
    status()  # an engine that reports the refused call here is clean afterwards
    arena.prepare("zero")
    sync()
    rc = call(arena, arena.nbytes(ws))
    sync()
    assert rc == M2S_OK and status() == M2S_OK, f"{what}: call after the refused one returned {rc}"
    bad = arena.violations()
    assert not bad, f"{what} [after undersized]: " + "; ".join(bad)
    if exact:
        for n, t in arena.outputs().items():
            assert bits_equal(t, good[n]), f"{what}: output {n!r} changed after a refused call"
