"""bench.py's command line (no GPU): a plain run carries none of the legs beside the timed
steps, --full switches them on (each still droppable), and --dump-outputs writes float64 .npy
files of a fixed sample under the size cap."""
import os
import types

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extra_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.config) == (7, 3, "c4")
    assert not (a.full or a.cpu or a.check or a.dropin) and a.dump_outputs is None


def test_full_switches_the_legs_on(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.cpu and a.check and a.dropin
    a = _parse(monkeypatch, "--full", "--no-cpu", "--no-dropin")
    assert not a.cpu and a.check and not a.dropin
    # the --no-* switches alone do not make a run full
    a = _parse(monkeypatch, "--no-cpu")
    assert not (a.cpu or a.check or a.dropin)


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_sample_index_is_fixed_and_sorted():
    assert np.array_equal(bench.sample_index(5, 10), np.arange(5))
    i, j = bench.sample_index(1_000_000, 1000), bench.sample_index(1_000_000, 1000)
    assert np.array_equal(i, j) and i.size == 1000 and np.all(np.diff(i) > 0)
    assert i.max() < 1_000_000


def test_dump_outputs_writes_float64_npy(tmp_path):
    a = types.SimpleNamespace(dump_outputs=str(tmp_path / "d"))
    bench.dump_outputs(a, {"coef": np.arange(6, dtype=np.float32).reshape(2, 3), "rows": [1, 2]})
    assert sorted(os.listdir(a.dump_outputs)) == ["coef.npy", "rows.npy"]
    c = np.load(os.path.join(a.dump_outputs, "coef.npy"))
    assert c.dtype == np.float64 and c.shape == (2, 3) and c[1, 2] == 5.0
    # nothing is written without the option, and the cap holds for the run's files together
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=None), {"x": np.zeros(3)})
    big = types.SimpleNamespace(dump_outputs=str(tmp_path / "big"))
    with pytest.raises(SystemExit):
        bench.dump_outputs(big, {"x": np.zeros(bench.DUMP_CAP_BYTES // 8 + 1)})
    assert not os.path.exists(big.dump_outputs)
