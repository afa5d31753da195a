"""bench.py's run modes: a plain run times the headline workload and nothing
else, --full adds every other leg, and --dump-outputs writes what the last
timed step computed as float .npy files within a fixed size."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_plain_run_is_the_default():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.workload, a.steps, a.warmup) == (False, None, None, 7, 3)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_riding_workloads_take_bounded_steps():
    """--steps is the headline's: the workloads behind it (half a second per
    step) take at most 20 timed and 5 warm-up steps however many it asks."""
    bench = _bench()
    a = bench.parse(["--full", "--steps", "5000", "--warmup", "300"])
    r = bench.rider_args(a)
    assert (r.steps, r.warmup, r.full) == (20, 5, True) and (a.steps, a.warmup) == (5000, 300)
    r = bench.rider_args(bench.parse(["--steps", "3", "--warmup", "1"]))
    assert (r.steps, r.warmup) == (3, 1)


def test_dump_outputs_formats_and_size_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "_dumped_bytes", 0)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    big = np.arange(1 << 18, dtype=np.float64).reshape(512, 512)      # 2 MiB: over the limit
    arrays = {"flag": np.array([1], dtype=np.int32), "half": np.ones(5, dtype=np.float32),
              "scalar": 2.5, "big": big}
    bench.dump_outputs(str(tmp_path / "a"), "w", arrays)
    monkeypatch.setattr(bench, "_dumped_bytes", 0)
    bench.dump_outputs(str(tmp_path / "b"), "w", arrays)
    got = {n: np.load(tmp_path / "a" / f"w_{n}.npy") for n in arrays}
    assert got["flag"].dtype == np.float64 and got["flag"].tolist() == [1.0]
    assert got["half"].dtype == np.float32
    assert got["scalar"].dtype == np.float64 and got["scalar"].item() == 2.5
    # the sample: distinct elements of the array in index order, the same every run
    s = got["big"]
    assert s.dtype == np.float64 and s.ndim == 1 and 0 < s.size < big.size
    assert np.all(np.diff(s) > 0) and np.all(s == np.floor(s)) and s.max() < big.size
    assert np.array_equal(s, np.load(tmp_path / "b" / "w_big.npy"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 1 << 20


@pytest.mark.gpu
def test_plain_kmeans_run_dumps_its_last_step(cuda, tmp_path):
    """A plain KMeans run at 8192 rows: the line carries the headline fields
    and none of --full's legs; the dumped arrays are the last step's (every
    row weighed once, each live center = its sum / weight) and a second run
    with the same arguments writes the same centers."""
    import torch
    bench = _bench()
    from cycloneml_amd import _native as N
    N.load()
    outs = []
    for tag in ("a", "b"):
        args = bench.parse(["--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", "8192",
                            "--dump-outputs", str(tmp_path / tag)])
        line = bench.run_workload("kmeans", args, cuda, 0, 1, 0.0)
        torch.cuda.synchronize()
        outs.append({f[len("kmeans_"):-4]: np.load(tmp_path / tag / f)
                     for f in os.listdir(tmp_path / tag)})
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "rows/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["cpu_baseline"] is None and "fit" not in line
    assert line["roofline"]["diag_kernels_ms_per_step"] == {}
    o = outs[0]
    assert set(o) == {"centers", "center_norms", "sums", "weights", "cost", "converged"}
    assert all(v.dtype == np.float64 for v in o.values())
    assert o["centers"].shape == (1024, 256) and o["sums"].shape == (1024, 256)
    assert o["weights"].sum() == 8192 and np.isfinite(o["cost"]).all() and o["cost"][0] > 0
    live = o["weights"] > 0
    np.testing.assert_allclose(o["centers"][live], o["sums"][live] / o["weights"][live, None],
                               rtol=1e-14)
    np.testing.assert_allclose(o["center_norms"], np.sqrt((o["centers"] ** 2).sum(1)), rtol=1e-13)
    np.testing.assert_allclose(outs[1]["centers"], o["centers"], rtol=1e-12, atol=0)
