"""bench.py --dump-outputs: what is written and that it is the same from run to run.

The snapshot is host logic around device tensors (bench.snapshot_outputs / write_outputs), checked
here on CPU tensors: every stats entry and the two flat buffers come out as float32 .npy files; a
flat buffer of more than DUMP_SAMPLE elements is cut to the same seeded sample in every call (so two
builds can be compared element for element); and the snapshot is a copy (a later step that
overwrites the graph's static outputs does not change it)."""
import types

import numpy as np
import torch

import bench


def fake(n):
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(n, generator=g)
    model = types.SimpleNamespace(flat=types.SimpleNamespace(flat=flat))
    opt = types.SimpleNamespace(exp_avg=torch.randn(n, generator=g))
    stats = {"loss": torch.tensor(7.5, dtype=torch.float64), "acc": None, "grad_norm": torch.tensor([2.0])}
    return stats, model, opt


def test_small_buffers_are_written_whole_as_float32(tmp_path):
    stats, model, opt = fake(1000)
    snap = bench.snapshot_outputs(stats, model, opt)
    params = model.flat.flat.clone()
    stats["grad_norm"].fill_(-1.0)  # a later step overwrites the static outputs
    model.flat.flat.add_(1.0)
    bench.write_outputs(snap, str(tmp_path / "d"))
    got = {p.name: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["adam_exp_avg.npy", "grad_norm.npy", "loss.npy", "params.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss.npy"].tolist() == [7.5] and got["grad_norm.npy"].tolist() == [2.0]
    assert np.array_equal(got["params.npy"], params.numpy())
    assert np.array_equal(got["adam_exp_avg.npy"], opt.exp_avg.numpy())


def test_large_buffers_are_cut_to_one_fixed_sample(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 257)
    stats, model, opt = fake(5000)
    a = bench.snapshot_outputs(stats, model, opt)
    b = bench.snapshot_outputs(stats, model, opt)
    assert a["params"].shape == (257,) and a["adam_exp_avg"].shape == (257,)
    assert torch.equal(a["params"], b["params"]) and torch.equal(a["adam_exp_avg"], b["adam_exp_avg"])
    # the same elements of both buffers, in index order, each drawn from the buffer itself
    idx = torch.nonzero(torch.isin(model.flat.flat, a["params"])).view(-1)
    assert idx.numel() == 257 and torch.equal(model.flat.flat[idx], a["params"])
    assert torch.equal(opt.exp_avg[idx], a["adam_exp_avg"])


def test_dump_stays_under_64_mb():
    assert 2 * 4 * bench.DUMP_SAMPLE + 4096 <= 64 * 10 ** 6
