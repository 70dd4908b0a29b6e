"""Fused validation metrics on the GPU (include/m2s.h "fused mel metrics") against the float64
restatement tests/metrics_ref.py, which tests/test_metrics_cpu.py holds against the reference's own classes.

Tolerances come from the kernel's documented reduction geometry, not from its results.  Every loss numerator and
denominator is a sum of non-negative terms: a lane adds ceil(T M / 256) terms, the 256 lanes are added in a tree of
depth 8, and a term carries 4 roundings (the difference, its square, the two weight products), so the relative
error is at most (terms + 8 + 4) 2^-24; the bar is twice that.  The MCD-like bar is the worst case of an M-term fp32
dot product per coefficient: (10 / ln 10) sqrt(2) sqrt(n_mfcc) 2 M 2^-24 max|x'|, from the case's data.  GPU box only.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR  # tests/metrics_ref.py
import ws_harness as H    # tests/ws_harness.py
from m2s import _native, metrics, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ERRORS = (_native.M2SError, RuntimeError)
NS = len(metrics.SLOTS)
LOSS_SLOTS = [s for s in metrics.SLOTS if s not in ("groups", "mcd_sum", "mcd_count")]
U = 2.0 ** -24
LANES, DEPTH = 256, 8  # mel_metrics_seq_kernel's geometry


def loss_bar(T, M):
    return 2.0 * (math.ceil(T * M / LANES) + DEPTH + 4) * U


def mcd_bar(pred, target, mask, mean, std, n_mfcc=13):
    """Per sequence: the worst-case bar from the largest |x'| of its masked rows (0 where it has none)."""
    bars = []
    for b in range(pred.shape[0]):
        rows = np.ones(pred.shape[1], bool) if mask is None else mask[b] != 0
        if not rows.any():
            bars.append(0.0)
            continue
        xm = max(np.abs(MR.power_to_db_of_db(v[b][rows].astype(np.float64) * std + mean)).max() for v in (pred, target))
        bars.append((10 / math.log(10)) * math.sqrt(2) * math.sqrt(n_mfcc) * 2 * pred.shape[2] * U * xm)
    return np.array(bars)


def _mean_std(M, seed=1):
    g = np.random.default_rng(seed)
    return g.uniform(-45, -35, M).astype(np.float32), g.uniform(8, 12, M).astype(np.float32)


def _case(name):
    g = np.random.default_rng(sum(map(ord, name)))
    rn = lambda *s: g.standard_normal(s).astype(np.float32)
    c = dict(group=0, ramp=1.0, mask=None, M=64)
    if name == "b3_masks":  # the all-masked sequence: no MCD value, its latest row and band terms still count
        c.update(pred=rn(3, 4, 64), target=rn(3, 4, 64), mask=np.array([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]], np.float32))
    elif name in ("t1", "t2"):
        T = int(name[1])
        c.update(pred=rn(2, T, 64), target=rn(2, T, 64), mask=np.ones((2, T), np.float32))
    elif name == "group2":  # a short last group
        c.update(pred=rn(5, 4, 64), target=rn(5, 4, 64), group=2,
                 mask=np.array([[1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 0], [0, 1, 1, 1], [1, 1, 1, 1]], np.float32))
    elif name == "half_mask":  # the mask multiplies: 0.5 halves a row's weight, and quarters it in eval's squares
        c.update(pred=rn(2, 4, 64), target=rn(2, 4, 64), mask=np.array([[0.5, 0.5, 1, 1], [1, 0.5, 0.5, 0.5]], np.float32),
                 ramp=0.5)
    elif name == "m16":  # f2 empty after clipping, high = (0, 16) overlapping f0 and f1
        c.update(pred=rn(3, 4, 16), target=rn(3, 4, 16), M=16, mask=np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]], np.float32))
    elif name == "t300":  # 75 terms per lane
        c.update(pred=rn(2, 300, 64), target=rn(2, 300, 64), mask=(g.random((2, 300)) > 0.2).astype(np.float32))
    elif name == "t130":  # past the reference's max_frames
        c.update(pred=rn(2, 130, 64), target=rn(2, 130, 64))
    elif name == "top_db":  # the target spans more than 80 dB (mean ~ -40, std ~ 10): its floor engages, pred's does not
        tgt = rn(2, 4, 64)
        tgt[:, :, 0], tgt[:, :, 5:9] = 3.5, -5.8
        c.update(pred=0.5 * rn(2, 4, 64), target=tgt)
    elif name == "below_100db":  # values under -100 dB are clamped (amin = 1e-10) before the floor
        p, t = rn(2, 4, 64), rn(2, 4, 64)
        p[:, 1, 10:20], t[:, 2, 30:40] = -8.0, -9.0
        c.update(pred=p, target=t)
    else:
        raise KeyError(name)
    return c


CASES = ["b3_masks", "t1", "t2", "group2", "half_mask", "m16", "t300", "t130", "top_db", "below_100db"]


def _run(c, acc=None, with_mcd=True, sl=slice(None), group=None):
    """One op call -> (out float64 array, per_seq array, acc tensor)."""
    M, T = c["M"], c["pred"].shape[1]
    fw, tw, coeffs, bands = metrics.train_weights(M, T, c["ramp"])
    mean, std = _mean_std(M)
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    acc = torch.zeros(NS, dtype=torch.float64, device=DEV) if acc is None else acc
    out, per_seq = metrics.mel_metrics(d(c["pred"][sl]), d(c["target"][sl]), d(None if c["mask"] is None else c["mask"][sl]),
                                       c["group"] if group is None else group, d(fw), d(tw), coeffs,
                                       [v for k in metrics.BAND_NAMES for v in bands[k]],
                                       d(mean) if with_mcd else None, d(std) if with_mcd else None, 13, acc)
    return out.cpu().numpy().astype(np.float64), per_seq.cpu().numpy().astype(np.float64), acc


def _ref(c, with_mcd=True):
    M, T = c["M"], c["pred"].shape[1]
    fw, tw, coeffs, bands = metrics.train_weights(M, T, c["ramp"])
    mean, std = _mean_std(M)
    return MR.metrics(c["pred"], c["target"], c["mask"], c["group"], fw, tw, coeffs,
                      [bands[k] for k in metrics.BAND_NAMES], mean.astype(np.float64) if with_mcd else None,
                      std.astype(np.float64) if with_mcd else None, 13)


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            c = _case(name)
            cache[name] = (c, *_ref(c))
        return cache[name]
    return get


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_restatement(refs, name):
    c, want, want_seq = refs(name)
    out, per_seq, acc = _run(c)
    got = dict(zip(metrics.SLOTS, out))
    B, T, M = c["pred"].shape
    bar = loss_bar(T, M)
    worst = 0.0
    for k in LOSS_SLOTS:
        if want[k] == 0.0:
            assert got[k] == 0.0, (k, got[k])  # T = 1 / T <= 2 terms, empty bands, unused band slots
            continue
        rel = abs(got[k] - want[k]) / abs(want[k])
        worst = max(worst, rel)
        assert rel <= bar, f"{name} {k}: got {got[k]!r} want {want[k]!r} rel {rel:.2e} > bar {bar:.2e}"
    print(f"{name}: worst loss-slot relative error {worst:.2e} (bar {bar:.2e})")
    assert got["groups"] == want["groups"] and got["mcd_count"] == want["mcd_count"]
    mbar = mcd_bar(c["pred"], c["target"], c["mask"], *[v.astype(np.float64) for v in _mean_std(M)])
    assert np.array_equal(np.isnan(per_seq[:, 2]), np.isnan(want_seq[:, 2])), (per_seq[:, 2], want_seq[:, 2])
    ok = ~np.isnan(want_seq[:, 2])
    merr = np.abs(per_seq[ok, 2] - want_seq[ok, 2])
    print(f"{name}: MCD-like {want_seq[ok, 2]} max err {merr.max() if ok.any() else 0:.2e} (bar {mbar[ok].max() if ok.any() else 0:.2e})")
    assert (merr <= mbar[ok]).all(), (merr, mbar)
    assert abs(got["mcd_sum"] - want["mcd_sum"]) <= mbar.sum()
    for j in (0, 1):  # the per-sequence masked sums
        np.testing.assert_allclose(per_seq[:, j], want_seq[:, j], rtol=bar, atol=0)
    np.testing.assert_allclose(acc.cpu().numpy(), out, rtol=2 * U, atol=0)  # out is acc's fp32 rounding


def test_case_data_exercises_what_it_claims(refs):
    """The two MCD cases, checked on the restatement's side: the floor moves the target and not pred; the clamp binds."""
    mean, std = [v.astype(np.float64) for v in _mean_std(64)]
    c = _case("top_db")
    for b in range(2):
        dbp, dbt = c["pred"][b] * std + mean, c["target"][b] * std + mean
        assert dbt.max() - dbt.min() > 80 and dbp.max() - dbp.min() < 80
        assert np.abs(MR.power_to_db_of_db(dbt) - np.maximum(dbt, -100)).max() > 1.0  # the floor lifts target bins
        assert np.abs(MR.power_to_db_of_db(dbp) - np.maximum(dbp, -100)).max() < 1e-9  # and leaves pred alone
    c = _case("below_100db")
    assert ((c["pred"][0] * std + mean) < -100).any() and ((c["target"][0] * std + mean) < -100).any()
    c, want, want_seq = refs("b3_masks")
    assert np.isnan(want_seq[2, 2]) and want["mcd_count"] == 2 and want_seq[2, 0] == 0.0
    sub = dict(c, pred=c["pred"][:2], target=c["target"][:2], mask=c["mask"][:2])
    assert _ref(sub)[0]["latest"] != want["latest"] and _ref(sub)[0]["band0"] != want["band0"]


def test_without_a_scaler_there_is_no_mcd(refs):
    c, want, _ = refs("b3_masks")
    out, per_seq, _ = _run(c, with_mcd=False)
    got = dict(zip(metrics.SLOTS, out))
    assert got["mcd_sum"] == 0 and got["mcd_count"] == 0 and np.isnan(per_seq[:, 2]).all()
    assert abs(got["loss"] - want["loss"]) <= loss_bar(4, 64) * want["loss"]


# ---- 2. groups and accumulation ------------------------------------------------------------------------------------
def test_groups_equal_separate_calls_accumulated(refs):
    c, _, _ = refs("group2")
    out, _, acc = _run(c)
    acc3 = torch.zeros(NS, dtype=torch.float64, device=DEV)
    outs = [_run(c, acc=acc3, sl=s, group=0)[0] for s in (slice(0, 2), slice(2, 4), slice(4, 5))]
    a, a3 = acc.cpu().numpy(), acc3.cpu().numpy()
    np.testing.assert_allclose(a3, a, rtol=1e-12, atol=0)  # the same per-group doubles, added in another order
    np.testing.assert_allclose(np.sum(outs, 0), out, rtol=4 * U, atol=0)
    assert a[metrics.SLOTS.index("groups")] == 3


def test_melmetrics_update_compute_reset(refs):
    c, want, _ = refs("group2")
    mean, std = _mean_std(64)
    mm = metrics.MelMetrics(64, mean, std, device=DEV)
    d = lambda a: torch.from_numpy(a).to(DEV)
    mm.update(d(c["pred"]), d(c["target"]), d(c["mask"]), group=2)
    mm.update(d(c["pred"]), d(c["target"]), d(c["mask"]), group=2)  # twice: the averages stay
    r = mm.compute()
    bar = loss_bar(4, 64)
    assert r["batches"] == 6 and r["mcd_sequences"] == 10 and set(r["band"]) == {"f0", "f1", "f2", "high"}
    for k in ("loss", "mse", "mae", "delta", "accel", "latest"):
        assert abs(r[k] - want[k] / 3) <= bar * want[k] / 3, k
    for i, k in enumerate(metrics.BAND_NAMES):
        assert abs(r["band"][k] - want[f"band{i}"] / 3) <= bar * want[f"band{i}"] / 3, k
    for k in ("loss", "mse", "mae"):
        assert abs(r["eval"][k] - want[f"eval_{k}"] / 3) <= bar * want[f"eval_{k}"] / 3, k
    assert abs(r["mcd_like"] - want["mcd_sum"] / 5) <= mcd_bar(c["pred"], c["target"], c["mask"], mean.astype(np.float64),
                                                               std.astype(np.float64)).max()
    mm.reset()
    with pytest.raises(_native.M2SError):
        mm.compute()
    with pytest.raises(_native.M2SError):
        mm.update(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64))  # CPU tensors


# ---- 3. reproducibility --------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(refs):
    c, _, _ = refs("t300")
    a, pa, _ = _run(c)
    b, pb, _ = _run(c)
    assert np.array_equal(a, b) and np.array_equal(pa, pb, equal_nan=True)


def test_a_sequence_alone_and_in_a_batch(refs):
    c, _, _ = refs("group2")
    _, whole, _ = _run(c)
    for b in (0, 3, 4):
        _, one, _ = _run(c, sl=slice(b, b + 1), group=0)
        assert np.array_equal(one[0].view(np.int64), whole[b].view(np.int64)), b


# ---- 4. workspace contract through the C ABI ------------------------------------------------------------------------
def test_workspace_contract(refs):
    c, want, _ = refs("group2")
    L = _native.lib()
    B, T, M = c["pred"].shape
    fw, tw, coeffs, bands = metrics.train_weights(M, T, 1.0)
    mean, std = _mean_std(M)
    nws = L.m2s_mel_metrics_workspace_bytes(B)
    assert nws == 768  # 5 x 32 floats to the granule
    arena = H.Arena(DEV, [("pred", "in", c["pred"]), ("target", "in", c["target"]), ("mask", "in", c["mask"]),
                          ("fw", "in", fw), ("tw", "in", tw), ("mean", "in", mean), ("std", "in", std),
                          ("acc", "in", np.zeros(NS, np.float64)), ("out", "out", (NS,)), ("per_seq", "out", (B, 3)),
                          ("ws", "ws", nws)])
    bd = (C.c_int * 8)(*[v for k in metrics.BAND_NAMES for v in bands[k]])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(a, n):
        a.view("acc").zero_()  # acc is added to: every run starts from zero
        return L.m2s_mel_metrics(a.ptr("pred"), a.ptr("target"), a.ptr("mask"), B, T, M, 2, a.ptr("fw"), a.ptr("tw"),
                                 coeffs[0], coeffs[1], coeffs[2], bd, 4, a.ptr("mean"), a.ptr("std"), 13, a.ptr("acc"),
                                 a.ptr("out"), a.ptr("per_seq"), a.ptr("ws"), n, stream)

    sync = lambda: torch.cuda.synchronize(DEV)
    rep = H.check_contract(arena, lambda a: call(a, nws), sync=sync, what="mel_metrics")
    assert rep.deterministic
    H.check_undersized(arena, call, rep.outs["zero"], sync=sync, what="mel_metrics")
    got = rep.outs["nan"]["out"].cpu().numpy().astype(np.float64)
    assert abs(got[0] - want["loss"]) <= loss_bar(T, M) * want["loss"]
    acc = arena.view("acc").cpu().numpy()
    np.testing.assert_allclose(acc, got, rtol=2 * U, atol=0)


# ---- 5. argument errors --------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    L = _native.lib()
    x = torch.zeros(2, 4, 16, device=DEV)
    one, acc = torch.ones(16, device=DEV), torch.zeros(NS, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    tw = torch.ones(4, device=DEV)
    bd = (C.c_int * 4)(0, 6, 6, 16)
    p = lambda t: C.c_void_p(t.data_ptr())

    def raw(B=2, T=4, M=16, n_bands=2, bands=bd, mean=one, std=one, n_mfcc=13, nws=1024, group=0):
        return L.m2s_mel_metrics(p(x), p(x), None, B, T, M, group, p(one), p(tw), 0.3, 0.1, 0.2, bands, n_bands,
                                 None if mean is None else p(mean), None if std is None else p(std), n_mfcc, p(acc), None,
                                 None, p(ws), nws, None)

    torch.cuda.synchronize()
    _native.prof_enable(True)
    try:
        _native.prof_launches()
        for kw in (dict(B=0), dict(T=0), dict(M=0), dict(M=257), dict(n_bands=9), dict(n_bands=-1), dict(bands=None),
                   dict(std=None), dict(n_mfcc=17), dict(n_mfcc=0), dict(nws=0), dict(group=-1)):
            assert raw(**kw) == 1, kw  # M2S_E_ARG
        o = ops.load()
        with pytest.raises(ERRORS):  # n_mfcc > M through the op
            o.mel_metrics(x, x, None, 0, one, tw, [0.3, 0.1, 0.2], [], one, one, 17, acc)
        with pytest.raises(ERRORS):
            o.mel_metrics(x, x[:1], None, 0, one, tw, [0.3, 0.1, 0.2], [], None, None, 13, acc)
        assert _native.prof_launches() == []
        assert raw() == 0  # and the good call is recorded: two launches
        torch.cuda.synchronize()
        assert [r["name"] for r in _native.prof_launches()] == ["mel_metrics_seq_kernel", "mel_metrics_group_kernel"]
    finally:
        _native.prof_enable(False)
    a = acc.cpu().numpy()  # only the good call added anything: one group, every loss 0
    assert a[metrics.SLOTS.index("groups")] == 1 and a[metrics.SLOTS.index("mcd_count")] == 2 and a[:17].sum() == 0


# ---- 6. opcheck -----------------------------------------------------------------------------------------------------
def test_opcheck_mel_metrics(refs):
    c, _, _ = refs("group2")
    o = ops.load()
    fw, tw, coeffs, bands = metrics.train_weights(64, 4, 1.0)
    mean, std = _mean_std(64)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    flat = [v for k in metrics.BAND_NAMES for v in bands[k]]
    for args in ((d(c["pred"]), d(c["target"]), d(c["mask"]), 2, d(fw), d(tw), list(coeffs), flat, d(mean), d(std), 13,
                  torch.zeros(NS, dtype=torch.float64, device=DEV)),
                 # no mask, no bands; the scaler stays: without it per_seq's third column is NaN by contract, which
                 # opcheck's eager-against-traced comparison cannot tell from a wrong value
                 (d(c["pred"]), d(c["target"]), None, 0, d(fw), d(tw), list(coeffs), [], d(mean), d(std), 5,
                  torch.zeros(NS, dtype=torch.float64, device=DEV))):
        torch.library.opcheck(o.mel_metrics.default, args,
                              test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
