"""
bench.py's own plumbing: --dump-outputs writes the last timed step's arrays (a fixed sample of the large
ones), a plain run leaves out what --full measures, and the result line keeps its meaning.  the GPU cases
run bench.main() in this process on config 1 (100 k points, one scale).
"""

import json
import os

import numpy as np
import pytest
import torch

import bench
from nimrud_amd import synth


def test_dump_outputs_samples_the_same_rows_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_PER_ARRAY", 8 * 4 * 100)        # room for 100 rows of 4 doubles
    big = torch.arange(1000 * 4, dtype=torch.float64).reshape(1000, 4)
    small = torch.arange(50, dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"features": big, "labels": small})
    a, b = np.load(tmp_path / "a" / "features.npy"), np.load(tmp_path / "b" / "features.npy")
    assert a.dtype == np.float64 and a.shape == (100, 4)
    assert np.array_equal(a, b)
    rows = (a[:, 0] / 4).astype(np.int64)
    assert np.array_equal(a, big.numpy()[rows])             # whole rows of the input ...
    assert (np.diff(rows) > 0).all()                        # ... in ascending order, none twice
    labels = np.load(tmp_path / "a" / "labels.npy")
    assert labels.dtype == np.float64 and np.array_equal(labels, np.arange(50))   # small arrays: whole
    # ranks of a multi-GPU run write files of their own
    bench.dump_outputs(str(tmp_path / "c"), {"features": big}, rank=1, world=2)
    assert os.listdir(tmp_path / "c") == ["features_rank1.npy"]


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setenv("NIMRUD_BENCH_RUN_IN_S", "0")
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--workload", "c1_uniform_100k"] + list(argv))
    bench.main()
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, "one JSON result line"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_path_computes(tmp_path, monkeypatch, capsys):
    from nimrud_amd.minimal import multiscale
    recs = [_run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
            for d in ("a", "b")]
    rec = recs[0]
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["metric"] == "point-scale feature ops/sec" and rec["unit"] == "point-scales/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["value"] == pytest.approx(100_000 * 1 / (rec["ms_per_step"] * 1e-3))
    # nothing that takes a run of its own
    for key in ("roofline", "cpu_baseline", "voxels_per_scale", "extra_search_passes_per_scale"):
        assert rec[key] is None
    a, b = np.load(tmp_path / "a" / "features.npy"), np.load(tmp_path / "b" / "features.npy")
    assert a.dtype == np.float64 and a.shape == (100_000, 4)
    assert np.array_equal(a, b)
    points, _, edges, radii = synth.make_config("c1_uniform_100k")
    want = multiscale.process_single_core(points, points, edges, radii)
    assert np.array_equal(a, want)


@pytest.mark.gpu
def test_full_run_keeps_the_extra_figures(monkeypatch, capsys):
    # (the multi-process CPU leg forks, which this process must not do once HIP is up: one worker = skipped)
    monkeypatch.setenv("NIMRUD_BENCH_CPU_WORKERS", "1")
    rec = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full", "--cpu-sample", "2000")
    assert rec["roofline"]["achieved"] > 0 and rec["roofline"]["measured_copy_GBps"] > 0
    assert len(rec["voxels_per_scale"]) == 1 and rec["voxels_per_scale"][0] > 0
    assert len(rec["extra_search_passes_per_scale"]) == 1
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_lattice_c"]["value"] > 0
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
