"""bench.py --dump-outputs / --full on the CPU: the dump writer on host tensors (names, dtypes, the fixed env
sample, the byte budget) and the option parsing. The GPU run itself is bench.py's."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _fake(B=100, N=16, dtype=torch.complex128):
    g = torch.Generator().manual_seed(3)
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    psi = torch.complex(torch.randn(B, N, generator=g, dtype=real), torch.randn(B, N, generator=g, dtype=real))
    out = {"fail_step": torch.arange(B, dtype=torch.int32) % 3, "obs": torch.randn(B, 5, generator=g, dtype=torch.float64)}
    return out, psi


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_and_the_whole_state_when_it_fits(tmp_path):
    out, psi = _fake()
    bench.dump_outputs(str(tmp_path / "a"), out, psi)
    got = _load(tmp_path / "a")
    assert set(got) == {"fail_step", "obs", "psi", "psi_envs"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["obs"], out["obs"].numpy())
    assert np.array_equal(got["fail_step"], out["fail_step"].numpy().astype(np.float64))
    assert np.array_equal(got["psi_envs"], np.arange(100.0))
    assert got["psi"].shape == (100, 16, 2)
    assert np.array_equal(got["psi"][..., 0] + 1j * got["psi"][..., 1], psi.numpy())


def test_dump_samples_the_same_envs_every_time_within_the_budget(tmp_path, monkeypatch):
    out, psi = _fake(dtype=torch.complex64)
    small = sum(t.numel() * 8 for t in out.values())
    monkeypatch.setattr(bench, "DUMP_BUDGET", small + 10 * (16 * 8 + 8))
    bench.dump_outputs(str(tmp_path / "a"), out, psi)
    bench.dump_outputs(str(tmp_path / "b"), out, psi, suffix="_rank1")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(b) == {k + "_rank1" for k in a}
    assert a["psi"].dtype == np.float32 and a["psi"].shape == (10, 16, 2)
    idx = a["psi_envs"].astype(np.int64)
    assert len(set(idx)) == 10 and np.all(np.diff(idx) > 0) and idx.max() < 100
    assert np.array_equal(a["psi_envs"], b["psi_envs_rank1"]) and np.array_equal(a["psi"], b["psi_rank1"])
    assert np.array_equal(a["psi"], torch.view_as_real(psi[idx]).numpy())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET


def test_shipped_budget_is_under_64_mb():
    assert bench.DUMP_BUDGET <= 64 * 10 ** 6


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_cpu_baseline


def test_zero_steps_is_refused(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.main()
