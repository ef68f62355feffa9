"""bench.py's options (CPU): a plain run switches off every pass behind --full, and
--dump-outputs writes float arrays within its size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_switches_off_the_full_passes():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.check_samples == a.phase_steps == a.exact_steps == 0
    assert not a.replay_audit and not a.energy and a.p_audit == "off"
    # their options do nothing without --full
    a = bench.parse(["--exact-steps", "4", "--check-samples", "64", "--p-audit", "on"])
    assert a.exact_steps == a.check_samples == 0 and a.p_audit == "off"


def test_full_run_keeps_every_pass_and_its_options():
    import bench

    a = bench.parse(["--full"])
    assert (a.check_samples, a.phase_steps, a.exact_steps) == (256, 4, 10)
    assert a.replay_audit and a.energy and a.p_audit == "auto"
    a = bench.parse(["--full", "--exact-steps", "0", "--no-energy", "--dump-outputs", "d"])
    assert a.exact_steps == 0 and not a.energy and a.replay_audit and a.dump_outputs == "d"


def test_dump_outputs_precision_and_size_limit(tmp_path, monkeypatch):
    import bench

    rng = np.random.default_rng(3)
    pos, vel = rng.standard_normal((1000, 3)), rng.standard_normal((1000, 3))
    bench.dump_outputs(str(tmp_path / "a"), pos, vel, fp64=True)
    assert np.array_equal(np.load(tmp_path / "a" / "pos.npy"), pos)
    assert np.array_equal(np.load(tmp_path / "a" / "vel.npy"), vel)
    bench.dump_outputs(str(tmp_path / "b"), pos, vel, fp64=False)
    got = np.load(tmp_path / "b" / "pos.npy")
    assert got.dtype == np.float32 and np.array_equal(got, pos.astype(np.float32))
    # past the limit: the same seeded sample of rows in every run, rows kept together
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * 2 * 3 * 8)
    for d in ("c", "d"):
        bench.dump_outputs(str(tmp_path / d), pos, vel, fp64=True)
    p, v = np.load(tmp_path / "c" / "pos.npy"), np.load(tmp_path / "c" / "vel.npy")
    assert p.shape == v.shape == (100, 3) and p.nbytes + v.nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(p, np.load(tmp_path / "d" / "pos.npy"))
    rows = [int(np.flatnonzero((pos == r).all(axis=1))[0]) for r in p]
    assert rows == sorted(set(rows)) and np.array_equal(v, vel[rows])
