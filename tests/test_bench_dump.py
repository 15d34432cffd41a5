"""bench.py's ``--dump-outputs`` and ``--full``: the dump holds the last timed batch's sink rows as float64 vectors,
two runs with the same arguments give the same files, and ``--steps`` sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_flattens_rows_and_samples_large_outputs(tmp_path):
    small = [json.dumps({"a": {"b": k, "s": "x" if k % 2 else "y"}, "flag": k > 1, "none": None, "v": k / 4})
             for k in range(4)]
    big = [json.dumps({"k": k}) for k in range(bench.DUMP_MAX_ROWS + 100)]
    written = bench.dump_outputs(str(tmp_path), [("Small", small), ("Big", big), ("Empty", [])])
    assert written["Small.rows.npy"] == 4 and written["Big.rows.npy"] == bench.DUMP_MAX_ROWS
    assert written["Empty.rows.npy"] == 0
    ld = lambda n: np.load(os.path.join(tmp_path, n))            # noqa: E731
    assert ld("Small.a.b.npy").dtype == np.float64
    assert ld("Small.a.b.npy").tolist() == [0.0, 1.0, 2.0, 3.0]
    assert ld("Small.v.npy").tolist() == [0.0, 0.25, 0.5, 0.75]
    assert ld("Small.flag.npy").tolist() == [0.0, 0.0, 1.0, 1.0]
    assert np.isnan(ld("Small.none.npy")).all()
    s = ld("Small.a.s.npy")
    assert s[0] == s[2] and s[1] == s[3] and s[0] != s[1]        # equal text, equal number
    rows = ld("Big.rows.npy")
    assert (np.diff(rows) > 0).all() and rows.max() < len(big)
    assert np.array_equal(ld("Big.k.npy"), rows)                  # the sample keeps row order
    again = bench.dump_outputs(str(tmp_path / "again"), [("Big", big)])
    assert again["Big.rows.npy"] == bench.DUMP_MAX_ROWS
    assert np.array_equal(np.load(os.path.join(tmp_path, "again", "Big.rows.npy")), rows)   # a fixed sample
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in written)
    assert total <= bench.DUMP_MAX_BYTES <= 64_000_000


def _run_bench(tmp_path, *extra, gpu=False):
    env = dict(os.environ, PYTHONPATH=ROOT)
    if not gpu:
        env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--events-per-batch", "300", *extra], capture_output=True, text=True, env=env, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("flow", ["groupby", "window"])
def test_bench_dumps_the_same_outputs_in_every_run(flow, tmp_path):
    outs = [_run_bench(tmp_path, "--flow", flow, "--full", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in outs:
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["value"] == pytest.approx(300 * 3 / (out["ms_per_step"] * 3 / 1e3), rel=1e-9)
    fa, fb = (sorted(os.listdir(tmp_path / d)) for d in ("a", "b"))
    assert fa == fb and fa and all(f.endswith(".npy") for f in fa)
    summary = {"groupby": "DeviceSummary", "window": "DeviceWindow"}[flow]
    n = int(outs[0]["last_batch_outputs"][f"Output_{summary}_Sink_InputEvents"])
    assert n > 0 and np.load(tmp_path / "a" / f"{summary}.rows.npy").shape == (n,)
    for f in fa:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and a.ndim == 1
        assert np.array_equal(a, b, equal_nan=True), f
    counts = np.load(tmp_path / "a" / f"{summary}.EventCount.npy")
    # groupby: every event of the last batch is in exactly one group; window: the groups hold several batches' events
    assert counts.sum() == 300 if flow == "groupby" else counts.sum() >= 300


@pytest.mark.gpu
def test_bench_dumps_what_the_device_serializer_rendered(gpu, tmp_path):
    """On the GPU the sinks get the device serializer's lines: the dump holds the last batch's rows, every event in
    exactly one group."""
    out = _run_bench(tmp_path, "--dump-outputs", str(tmp_path / "d"), gpu=True)
    assert out["steps"] == 3 and "h2d_gb_s" not in out            # a plain run does not probe the link
    n = int(out["last_batch_outputs"]["Output_DeviceSummary_Sink_InputEvents"])
    alerts = int(out["last_batch_outputs"]["Output_HotDeviceAlerts_Sink_InputEvents"])
    files = sorted(os.listdir(tmp_path / "d"))
    assert out["dumped_outputs"]["files"] == len(files)
    assert np.load(tmp_path / "d" / "DeviceSummary.rows.npy").tolist() == list(range(n))
    assert np.load(tmp_path / "d" / "HotDeviceAlerts.rows.npy").shape == (alerts,)
    counts = np.load(tmp_path / "d" / "DeviceSummary.EventCount.npy")
    assert counts.dtype == np.float64 and counts.shape == (n,) and counts.sum() == 300
    hot = np.load(tmp_path / "d" / "DeviceSummary.MaxTemperature.npy")
    assert int((hot > 44.99).sum()) == alerts
