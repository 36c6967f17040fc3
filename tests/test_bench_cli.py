"""bench.py's host-side parts on the CPU: the command line (--full off by default, --steps and --per-launch checked), the
--dump-outputs writer (float32, the 64 MB cap by a fixed seeded sample) and the snapshot / restore round trip that puts
the seeded starting state back IN PLACE before the written step (a captured graph keeps reading the same storage)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_bad_arguments_are_refused(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = parse(monkeypatch, "--full", "--per-launch", "t.txt", "--dump-outputs", "d")
    assert a.full and a.per_launch == "t.txt" and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--per-launch", "t.txt"]):
        with pytest.raises(SystemExit):
            parse(monkeypatch, *bad)


def test_write_outputs_float32_and_seeded_sample_under_the_cap(tmp_path, monkeypatch):
    arrays = {"a": torch.arange(1000, dtype=torch.float64), "b": torch.ones(3, 5)}
    bench.write_outputs(str(tmp_path / "full"), arrays)
    a = np.load(tmp_path / "full" / "a.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(1000, dtype=np.float32))
    assert np.load(tmp_path / "full" / "b.npy").shape == (3, 5)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2000)         # 4060 bytes in all: about half of every array is kept
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), arrays)
    s1, s2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert np.array_equal(s1, s2) and 0 < s1.size < 1000 and np.all(np.diff(s1) > 0)     # same sample, sorted indices
    assert sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in ("a.npy", "b.npy")) <= 2000


def test_restore_puts_the_seeded_state_back_in_place():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Linear(8, 1))
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.5, 0.999), eps=1e-6)
    x = torch.randn(16, 4, generator=torch.Generator().manual_seed(1))

    def step():
        opt.zero_grad()
        loss = model(x).pow(2).mean()
        loss.backward()
        opt.step()
        return bench.step_outputs(model, opt, loss.detach())

    start = bench.snapshot(model, opt)
    storage = [t.data_ptr() for t in list(model.parameters()) + list(model.buffers())]
    first = step()
    for _ in range(5):
        step()
    bench.restore(model, opt, start)
    assert storage == [t.data_ptr() for t in list(model.parameters()) + list(model.buffers())]
    again = step()
    assert set(first) == {"loss", "grads", "buffers", "exp_avg", "exp_avg_sq"}
    for k in first:
        assert torch.equal(first[k], again[k]), k
