"""bench.py's plain / --full split and --dump-outputs: the option parsing and
the sampled env ids (CPU), and a small plain run on the GPU whose dump must
not depend on the runner or on how long the clock ramp ran."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MOVED = ("trajectory_digest", "single_stream", "single_stream_full_outputs", "scan_check", "scan_l2_vs_cpu",
         "roofline", "secondary", "cpu_baseline")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default_and_dump_takes_a_directory(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _parse(monkeypatch, "--full", "--dump-outputs", "some/dir")
    assert a.full is True and a.dump_outputs == "some/dir"
    with pytest.raises(SystemExit) as e:  # the ddpg loop's outputs are not reproducible run to run
        _parse(monkeypatch, "--workload", "ddpg", "--dump-outputs", "d")
    assert e.value.code == 2


def test_dump_env_ids_fixed_sorted_sample_within_the_size_limit():
    import bench
    ids = bench.dump_env_ids(65536, 1084, 12345)
    assert ids.shape == (bench.DUMP_ENVS,) and ids.dtype == np.int64
    assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < 65536
    assert np.array_equal(ids, bench.dump_env_ids(65536, 1084, 12345))
    assert not np.array_equal(ids, bench.dump_env_ids(65536, 1084, 12346))
    assert np.array_equal(bench.dump_env_ids(100, 1084, 12345), np.arange(100))  # everything when it fits
    wide = bench.dump_env_ids(65536, 100000, 12345)  # rows of 400 kB: fewer of them
    assert 1 <= wide.size and wide.size * 100000 * 4 <= bench.DUMP_MAX_BYTES < 64 << 20
    assert bench.DUMP_ENVS * (1084 + 8) * 4 <= bench.DUMP_MAX_BYTES


def _run(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(gpu, tmp_path, monkeypatch, capsys):
    """Two plain runs of 1000 envs, 3 timed steps after 2 warm-up: stream
    sub-shards with no clock ramp, and one context after a short ramp (a
    wall-time-dependent number of untimed steps before the reset).  Both
    lines carry the headline fields and nothing of --full; the dumps are
    float32 / float64 arrays of every env and equal bit for bit (the
    sub-shards are bit-identical to one context)."""
    common = ["--gpus", "1", "--global-envs", "1000", "--steps", "3", "--warmup", "2"]
    a = _run(monkeypatch, capsys, *common, "--ramp-s", "0", "--dump-outputs", str(tmp_path / "a"))
    b = _run(monkeypatch, capsys, *common, "--ramp-s", "0.05", "--runner", "one", "--dump-outputs", str(tmp_path / "b"))
    assert a["config"]["runner_kind"] == "streams" and b["config"]["runner_kind"] == "one"
    assert b["config"]["ramp"]["steps"] > 0 == a["config"]["ramp"]["steps"]
    for line in (a, b):
        assert line["full"] is False and not [k for k in MOVED if k in line]
        assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "env-steps/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(1000 * 3 / (line["ms_per_step"] * 3e-3), rel=1e-9)
    shapes = {"obs": (1000, 1084), "collisions": (1000, 1), "terminated": (1000,), "env_ids": (1000,)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.shape == shape and x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert np.isfinite(obs).all() and obs[:, :1080].max() > 0.0  # stepped scans, not the zero-filled buffer
    assert np.array_equal(np.load(tmp_path / "a" / "env_ids.npy"), np.arange(1000))
