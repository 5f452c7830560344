"""bench.py's command line and output dump, without a GPU."""
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(args))
    return bench.parse()


def test_plain_run_times_one_region_and_full_keeps_five(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.repeats, a.steps, a.warmup, a.dump_outputs) == (False, 1, 7, 3, None)
    a = _parse(monkeypatch, "--full")
    assert a.full and a.repeats == 5
    a = _parse(monkeypatch, "--full", "--repeats", "2", "--dump-outputs", "out")
    assert a.repeats == 2 and a.dump_outputs == "out"


def test_dump_outputs_whole_arrays_as_float32(tmp_path):
    outs = {"flow": torch.arange(24, dtype=torch.float32).view(3, 4, 2),
            "target_cls": torch.tensor([[1, 0, -1, 0]] * 3, dtype=torch.int64),
            "wide": torch.ones(3, 2, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "d"), outs)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(got) == {"flow", "target_cls", "wide"}
    assert got["flow"].dtype == np.float32 and np.array_equal(got["flow"], outs["flow"].numpy())
    assert got["target_cls"].dtype == np.float32 and np.array_equal(got["target_cls"], outs["target_cls"].numpy())
    assert got["wide"].dtype == np.float64


def test_dump_outputs_samples_the_same_rows_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    B = 100
    outs = {"flow": torch.arange(B * 8, dtype=torch.float32).view(B, 4, 2),
            "mask": torch.arange(B * 4, dtype=torch.float32).view(B, 4)}      # 4800 bytes in all
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), outs)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert sum(v.nbytes for v in got.values()) <= 4000
    rows = got["sample_rows"].astype(np.int64)
    assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["flow"], outs["flow"].numpy()[rows])
    assert np.array_equal(got["mask"], outs["mask"].numpy()[rows])
    for p in (tmp_path / "b").glob("*.npy"):                               # fixed seed: the same sample each run
        assert np.array_equal(np.load(p), got[p.stem])
