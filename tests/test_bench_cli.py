"""bench.py's command line and --dump-outputs writer (no GPU: main() stops at its argument checks, and
dump_outputs takes any tensors)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_float32_sampled_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)          # 512 elements for each of the two arrays
    big = torch.arange(10000, dtype=torch.float64).to(torch.bfloat16).reshape(100, 100)
    arrays = {"loss": torch.tensor(1.25, dtype=torch.bfloat16), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "loss.npy"]
    loss, a, b = (np.load(tmp_path / p) for p in ("a/loss.npy", "a/big.npy", "b/big.npy"))
    assert loss.dtype == np.float32 and loss.shape == () and loss == 1.25
    assert a.dtype == np.float32 and a.shape == (512,) and np.array_equal(a, b)
    assert loss.nbytes + a.nbytes <= 4096
    # a sample of the array's own elements at ascending positions
    assert np.all(np.diff(a) >= 0) and np.isin(a, big.float().numpy()).all()


def test_dump_outputs_keeps_small_arrays_whole(tmp_path):
    x = torch.randn(3, 4, 5, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(str(tmp_path), {"x": x})
    assert np.array_equal(np.load(tmp_path / "x.npy"), x.numpy())


@pytest.mark.parametrize("argv", [["--timer-dump", "t.json"], ["--steps", "0"]])
def test_rejected_arguments(argv, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err or argv[0] == "--steps"
