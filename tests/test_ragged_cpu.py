"""Ragged batches without a GPU: the planner's properties, split_packed, the command lines' flags, the
exported symbols, and run_sharded(ragged=True) over gloo with a stand-in device call."""
import importlib.util
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from m2s import _native as N
from m2s import drivers, ops, runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTH_LISTS = [[7, 1, 4, 7, 3], [5] * 9, [1], list(range(1, 41)), [300, 50, 299, 51, 120, 120, 7],
                [int(n) for n in np.random.default_rng(3).integers(20, 61, size=64)]]


def _jobs(lens, feat=(4,)):
    """Mels (feat, T): time on the last axis."""
    return [drivers.Job(None, f"j{i}", array=np.full(tuple(feat) + (n,), float(i), np.float32), length=n)
            for i, n in enumerate(lens)]


def _pad_frac(batch):
    lens = [j.array.shape[-1] for j in batch]
    return 1.0 - sum(lens) / (len(lens) * max(lens))


@pytest.mark.parametrize("lens", LENGTH_LISTS)
@pytest.mark.parametrize("max_batch,frac", [(64, 0.25), (3, 0.25), (16, 0.1), (64, 0.6)])
def test_plan_covers_every_job_once_within_both_bounds(lens, max_batch, frac):
    jobs = _jobs(lens)
    plan = drivers.plan_ragged_batches(jobs, max_batch, frac)
    assert sorted(id(j) for b in plan for j in b) == sorted(id(j) for j in jobs)
    for b in plan:
        assert 1 <= len(b) <= max_batch
        assert _pad_frac(b) <= frac + 1e-12
        assert [j.array.shape[-1] for j in b] == sorted((j.array.shape[-1] for j in b), reverse=True)
    # longest first, stable: equal lengths keep their input order
    flat = [j for b in plan for j in b]
    assert [j.stem for j in flat] == [j.stem for j in sorted(jobs, key=lambda j: -j.array.shape[-1])]


@pytest.mark.parametrize("lens", LENGTH_LISTS)
def test_zero_pad_bound_is_grouping_by_equal_length(lens):
    jobs = _jobs(lens)
    plan = drivers.plan_ragged_batches(jobs, max_batch=4, max_pad_frac=0.0)
    for b in plan:
        assert len({j.array.shape[-1] for j in b}) == 1
    want = sorted(sorted(j.stem for j in b) for b in drivers.plan_batches(jobs, max_batch=4))
    assert sorted(sorted(j.stem for j in b) for b in plan) == want


def test_pad_bound_buys_fewer_batches():
    lens = LENGTH_LISTS[-1]
    n = [len(drivers.plan_ragged_batches(_jobs(lens), 64, f)) for f in (0.0, 0.1, 0.25, 0.5)]
    assert n == sorted(n, reverse=True) and n[-1] < n[0]
    assert len(drivers.plan_ragged_batches(_jobs(lens), 64, 0.0)) == len(set(lens))


def test_failed_jobs_are_skipped_and_shapes_never_mix():
    jobs = _jobs([5, 4, 3]) + _jobs([5, 4], feat=(6,)) + _jobs([4, 4], feat=(2, 2))
    jobs[1].error = "OSError: unreadable"
    jobs.append(drivers.Job(None, "empty"))  # no array
    plan = drivers.plan_ragged_batches(jobs, 64, 0.9)
    assert sum(len(b) for b in plan) == 6
    assert all(j.ok for b in plan for j in b)
    for b in plan:
        assert len({j.array.shape[:-1] for j in b}) == 1
    assert len(plan) == 3
    # time on another axis: frames (T, H, W)
    fr = [drivers.Job(None, f"f{i}", array=np.zeros((n, 3, 2), np.float32)) for i, n in enumerate([2, 9, 8])]
    assert [[j.stem for j in b] for b in drivers.plan_ragged_batches(fr, 64, 0.25, time_axis=0)] == [["f1", "f2"], ["f0"]]
    with pytest.raises(ValueError):
        drivers.plan_ragged_batches(jobs, 0)
    with pytest.raises(ValueError):
        drivers.plan_ragged_batches(jobs, 4, 1.0)


def test_run_ragged_batches_one_call_per_batch_and_per_job_errors():
    lens = [6, 2, 5, 1]
    jobs = _jobs(lens, feat=(3,))
    calls = []

    def fn(x, lengths):  # packed (N, 3) -> packed (2 N,): two entries per time step
        calls.append(list(lengths))
        assert x.shape == (sum(lengths), 3)
        if 1 in lengths:
            raise RuntimeError("device call failed")
        return x.sum(dim=1).repeat_interleave(2) + torch.arange(2.0).repeat(x.shape[0])

    drivers.run_ragged_batches([[jobs[0], jobs[2]], [jobs[1], jobs[3]]], fn, torch.device("cpu"))
    assert calls == [[6, 5], [2, 1]]
    for i in (0, 2):
        assert jobs[i].error is None
        assert np.array_equal(jobs[i].result, np.repeat(np.full(lens[i], 3.0 * i), 2) + np.tile([0.0, 1.0], lens[i]))
    for i in (1, 3):
        assert jobs[i].result is None and "device call failed" in jobs[i].error


def test_split_packed_round_trips():
    lens = [7, 1, 4]
    clips = [torch.randn(n, 5) for n in lens]
    packed = torch.cat(clips)
    got = runtime.split_packed(packed, lens)
    assert all(torch.equal(a, b) for a, b in zip(got, clips))
    assert got[1].data_ptr() == packed[7:].data_ptr()  # views, not copies
    wav = torch.arange(12 * 3.0)
    parts = runtime.split_packed(wav, lens, per_step=3)
    assert [p.numel() for p in parts] == [21, 3, 12] and torch.equal(torch.cat(parts), wav)
    with pytest.raises(ValueError):
        runtime.split_packed(packed, [7, 1, 5])


def _script(rel):
    spec = importlib.util.spec_from_file_location("m2s_ragged_cli_" + os.path.basename(rel)[:-3],
                                                  os.path.join(REPO, "mri-to-speech_amd", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rel,argv", [
    ("scripts/export_predicted_mels.py", ["--processed_dir", "p", "--mri_checkpoint", "c", "--scaler_json", "s",
                                          "--output_dir", "o"]),
    ("mel_to_audio_synthesis.py", ["--input", "i", "--checkpoint_file", "c"]),
    ("inference_e2e.py", ["--checkpoint_file", "c"]),
])
def test_scripts_take_ragged_flags_default_off(rel, argv):
    mod = _script(rel)
    a = mod.parse_args(argv)
    assert a.ragged is False and a.max_pad_frac == 0.25
    a = mod.parse_args(argv + ["--ragged", "--max-pad-frac", "0.1"])
    assert a.ragged is True and a.max_pad_frac == pytest.approx(0.1)


def test_ragged_symbols_and_ops_are_declared():
    want = {"m2s_bilstm_summerge_ragged", "m2s_acoustic_forward_ragged", "m2s_vocoder_forward_ragged",
            "m2s_pipeline_forward_ragged", "m2s_acoustic_ragged_workspace_bytes", "m2s_vocoder_ragged_workspace_bytes",
            "m2s_pipeline_ragged_workspace_bytes"}
    assert want <= set(N.exported_symbols())
    L = N.lib()
    for name in want:
        assert getattr(L, name).argtypes is not None, name
    assert set(ops.RAGGED_OPS) == {"bilstm_summerge_ragged", "acoustic_forward_ragged", "hifigan_forward_ragged",
                                   "pipeline_forward_ragged"}
    assert not set(ops.RAGGED_OPS) & set(ops.OPS)
    o = ops.load()
    for name in ops.RAGGED_OPS:
        assert str(getattr(o, name).default._schema).startswith(f"m2s::{name}(")
        assert "int[] lengths" in str(getattr(o, name).default._schema)


def test_ragged_fake_shapes():
    o = ops.load()
    meta = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    lens = [7, 1, 4]
    y, m = o.bilstm_summerge_ragged(1, meta(12, 208), lens, 640, 64)
    assert y.shape == (12, 640) and m.shape == (12, 64)
    assert o.acoustic_forward_ragged(1, meta(12, 96, 80), lens, 64).shape == (12, 64)
    assert o.hifigan_forward_ragged(2, meta(12, 64), lens, 420).shape == (12 * 420,)
    outs = o.pipeline_forward_ragged(1, 2, meta(12, 96, 80), lens, meta(64), meta(64), 64, 420)
    assert [tuple(t.shape) for t in outs] == [(12, 64)] * 3 + [(12 * 420,)]


# ---- run_sharded(ragged=True) over gloo, in the manner of test_dist_export_gloo.py
LENS = [5, 9, 2, 7, 7, 1, 4, 3, 9, 6]
BAD = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sh_jobs():
    return [drivers.Job(None, f"utt{i}", length=t) for i, t in enumerate(LENS)]


def _sh_load(job):
    i = int(job.stem[3:])
    if i == BAD:
        job.error = "OSError: unreadable"
        return job
    job.array = np.random.default_rng(i).random((LENS[i], 4, 4), dtype=np.float32)  # frames: time first
    return job


def _sh_fn(x, lengths):  # packed (N,4,4) -> packed (N,3): a per-clip running mean, so a neighbour's rows would show
    m = x.mean(dim=(1, 2))
    out = torch.cat([torch.cumsum(c, dim=0) for c in torch.split(m, list(lengths))])
    return out[:, None] * torch.tensor([1.0, 2.0, 3.0])[None, :]


def _sh_want(i):
    m = torch.from_numpy(np.random.default_rng(i).random((LENS[i], 4, 4), dtype=np.float32)).mean(dim=(1, 2))
    return (torch.cumsum(m, dim=0)[:, None] * torch.tensor([1.0, 2.0, 3.0])[None, :]).numpy()


def _sh_run():
    jobs = _sh_jobs()
    drivers.run_sharded(jobs, _sh_fn, torch.device("cpu"), LENS, (3,), max_batch=3, load=_sh_load, time_axis=0,
                        ragged=True, max_pad_frac=0.5, in_time_axis=0)
    return jobs


def _sh_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        jobs = _sh_run()
        if rank == 0:
            q.put([(j.result, j.error) for j in jobs])
    finally:
        dist.destroy_process_group()


def _check(got):
    for i, (res, err) in enumerate(got):
        if i == BAD:
            assert res is None and "unreadable" in err
            continue
        assert err is None, (i, err)
        want = _sh_want(i)
        assert res.shape == want.shape == (LENS[i], 3)
        np.testing.assert_allclose(res, want, rtol=0, atol=1e-6, err_msg=str(i))


def test_run_sharded_ragged_single_process():
    _check([(j.result, j.error) for j in _sh_run()])


def test_run_sharded_ragged_gloo_world2_returns_every_jobs_rows():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sh_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    _check(got)
