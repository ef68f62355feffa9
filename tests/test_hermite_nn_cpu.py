"""Nearest neighbours, overlaps and mergers on the CPU: gs_cpu_nn_* (csrc/cpu/cpu_engine.cpp) and
the records of HermiteCpuEngine against oracle.nearest_neighbours, the merge rule of
oracle.merge_overlaps, and the driver (config, CLI, metrics, checkpoints) end to end.

Pair measure, tie rule, reference and bounds: tests/test_hermite_nn_gpu.py (B = 8 u (r^2 + s^2)).
Excused share (bodies whose best and second-best oracle q are within 2 B of each other) of the
inputs of both files, measured here by test_excused_share_of_the_inputs: 0 of every size, for
fp32, mixed and fp64, solar+random and Plummer (the 1 % cap is never approached).
"""
import functools
import json
import os

import numpy as np
import pytest

from gravsim.cli import main
from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.runtime.hermite import HermiteCpuEngine
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ck
from hermite_nn_helpers import (DTYPES, SIZES, SOFT, U, chain_and_bystander, check_against_oracle,
                                head_on, lattice, merger_with_bystander, pair_q, run_driver, seen,
                                with_radii)

def _engine(n, dtype, **kw):
    kw.setdefault("integrator", "hermite")
    kw.setdefault("collisions", "detect")
    return HermiteCpuEngine(SimConfig(n=n, dtype=dtype, device="cpu", **kw).validate())


def _nn(b, dtype, rows=None, **kw):
    eng = _engine(b.n, dtype, **kw)
    eng.load(b)
    return eng.derivs_nn(rows)[2:]


@functools.lru_cache(maxsize=None)
def _bodies(family, n):
    b = ic.solar_random(n, 7 + n) if family == "solar" else ic.make("plummer", n, 7 + n, G_SI)
    return with_radii(b, 100 + n)


# ---- 1. the CPU functions against the oracle -------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 257, 2049])
def test_cpu_nn_matches_oracle(n, dtype):
    b = _bodies("solar", n)
    q, nn = _nn(b, dtype)
    check_against_oracle(q, nn, b, dtype)
    rows = np.random.default_rng(1).permutation(n)[: max(1, n // 3)].astype(np.int32)
    qi, ni = _nn(b, dtype, rows)
    assert np.array_equal(qi, q[rows]) and np.array_equal(ni, nn[rows])  # (the _idx form)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_nn_plummer_softened(dtype):
    b = _bodies("plummer", 2049)
    for kw in (dict(softening=SOFT), dict(softening=SOFT, cutoff=0.0)):
        q, nn = _nn(b, dtype, **kw)
        check_against_oracle(q, nn, b, dtype, kw["softening"], kw.get("cutoff", 1e-10))


def test_excused_share_of_the_inputs():
    """The oracle alone: how many bodies have a second-best q within 2 B of the best."""
    worst = 0.0
    for family, sizes in (("solar", SIZES), ("plummer", [2049])):
        for n in sizes:
            b = _bodies(family, n)
            for dtype in DTYPES:
                pos, rad = seen(b.pos, b.radius, dtype)
                oq, onn, oq2 = oracle.nearest_neighbours(pos, rad, second=True)
                ok = onn >= 0
                _, scale = pair_q(pos, rad, np.arange(n)[ok], onn[ok])
                share = float(((oq2[ok] - oq[ok]) <= 16.0 * U[dtype] * scale).mean()) \
                    if ok.any() else 0.0
                worst = max(worst, share)
    print(f"largest excused share: {worst}")
    assert worst == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_exact_ties_and_planted_cases(dtype):
    b = lattice(2049)
    oq, onn = oracle.nearest_neighbours(b.pos, b.radius)
    q, nn = _nn(b, dtype)
    assert np.array_equal(nn, onn) and np.array_equal(q, oq)
    one = BodySet(np.array([[1e11, 2e10, 0.0]]), np.zeros((1, 3)), np.array([1e24]),
                  np.array([1e7]))
    q, nn = _nn(one, dtype)
    assert q[0] == np.inf and nn[0] == -1
    pos = np.array([[1e11, 0, 0], [1e11, 0, 0], [-1e11, 2e10, 0]], dtype=float)
    c = BodySet(pos, np.zeros((3, 3)), np.array([1e25, 2e25, 3e25]), np.array([1e6, 1e6, 3e6]))
    q, nn = _nn(c, dtype)
    assert list(nn) == [2, 2, 0]
    big = BodySet(np.array([[0, 0, 0], [5e8, 0, 0], [0, 8e8, 0], [3e11, 1e11, 0]], dtype=float),
                  np.zeros((4, 3)), np.array([1e24, 1e23, 2e30, 1e24]),
                  np.array([0.0, 0.0, 7e8, 0.0]))
    q, nn = _nn(big, dtype)
    assert nn[0] == 2 and q[0] > 0


def test_oracle_rows_and_zero_radii():
    b = _bodies("solar", 257)
    q, nn = oracle.nearest_neighbours(b.pos, None)
    d2 = ((b.pos[None] - b.pos[:, None]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    assert np.array_equal(nn, d2.argmin(1)) and np.allclose(q, d2.min(1), rtol=1e-15)
    rows = [5, 200, 0]
    qr, nr = oracle.nearest_neighbours(b.pos, b.radius, rows=rows)
    qa, na = oracle.nearest_neighbours(b.pos, b.radius)
    assert np.array_equal(qr, qa[rows]) and np.array_equal(nr, na[rows])


# ---- 2. the engine's records and the overlap stop ------------------------------------------------
@pytest.mark.parametrize("dtype,centre", [("fp64", (1.5e11, 0.7e11, -0.3e11)),
                                          ("mixed", (1.5e11, 0.7e11, -0.3e11)),
                                          ("fp32", (0.0, 0.0, 0.0))])
def test_cpu_shared_step_stops_at_the_oracles_step(dtype, centre):
    b = head_on(centre)
    rec = {}
    taken = oracle.simulate_hermite(b.pos, b.vel, b.mass, 1000.0, 200, radius=b.radius,
                                    collisions="merge", record=rec)[4]
    assert 50 < len(taken) < 120 and rec["overlaps"] == 2 and rec["ca_q"].max() < -1e13
    free = oracle.simulate_hermite(b.pos, b.vel, b.mass, 1000.0, len(taken) + 3,
                                   radius=b.radius, collisions="detect")[4]
    assert len(free) == len(taken) + 3  # (detect never stops)
    eng = _engine(2, dtype, collisions="merge", dt=1000.0)
    eng.load(b)
    eng.step(150)
    eng.step(50)
    st = eng.status()
    assert st.steps == len(taken) and st.overlaps == 2 and st.time == sum(taken)
    assert list(eng.closest()[1]) == [1, 0] and (eng.closest()[0] < 0).all()
    eng.clear_overlap()
    eng.step(1)
    assert eng.status().steps == len(taken) + 1


@pytest.mark.parametrize("block", [False, True])
def test_detect_changes_no_state_bit(block):
    n = 300
    b = _bodies("solar", n)
    kw = dict(dt=3600.0, block_steps=True, eta=0.02, max_level=6) if block else dict(dt=3600.0)
    out = {}
    for mode in ("off", "detect"):
        eng = _engine(n, "fp64", collisions=mode, **kw)
        eng.load(b)
        eng.step(2)
        s = eng.state()
        out[mode] = (s.pos, s.vel, *eng.carried())
    assert all(np.array_equal(x, y) for x, y in zip(out["off"], out["detect"]))


def test_block_run_records_on_the_cpu():
    # (1e23 kg: the pull between the bodies is felt, Aarseth steps of a few 1000 s, yet they are
    # still 2e7 m apart at the end of the macro step, far from the point-mass singularity)
    b = head_on((1.5e11, 0.7e11, -0.3e11), mass=1e23)
    kw = dict(dt=88000.0, eta=0.02, max_level=10)
    rec = {}
    oracle.simulate_hermite_block(b.pos, b.vel, b.mass, kw["dt"], kw["dt"], kw["eta"],
                                  kw["max_level"], radius=b.radius, collisions="detect",
                                  record=rec)
    eng = _engine(2, "fp64", collisions="merge", block_steps=True, **kw)
    eng.load(b)
    eng.step(1)
    assert eng.status().steps == 1 and eng.status().overlaps == rec["overlaps"] >= 2
    assert eng.status().block_steps > 4
    assert np.allclose(eng.closest()[0], rec["ca_q"], rtol=1e-9, atol=0)
    assert list(eng.closest()[1]) == [1, 0]


# ---- 3. the merge rule ------------------------------------------------------------------------
def test_merge_conserves_mass_and_momentum_and_keeps_the_lowest_id():
    rng = np.random.default_rng(4)
    n = 9
    pos, vel = rng.normal(size=(n, 3)) * 1e9, rng.normal(size=(n, 3)) * 1e3
    mass, rad = rng.uniform(1e22, 1e25, n), rng.uniform(1e5, 1e7, n)
    ids = np.arange(100, 100 + n)
    ca_q, ca_nn = np.full(n, 1.0), np.full(n, -1)
    ca_q[6], ca_nn[6] = -5.0, 2          # 6 overlaps 2
    ca_q[4], ca_nn[4] = -1.0, 7          # the chain 4 - 7 - 1: one body
    ca_q[7], ca_nn[7] = -2.0, 1
    p, v, m, R, I, k = oracle.merge_overlaps(pos, vel, mass, rad, ids, ca_q, ca_nn)
    assert k == 3 and list(I) == [100, 101, 102, 103, 105, 108]  # (order stable, lowest id kept)
    assert abs(m.sum() - mass.sum()) <= 4 * np.finfo(float).eps * mass.sum()
    mom0, mom1 = (mass[:, None] * vel).sum(0), (m[:, None] * v).sum(0)
    assert np.abs(mom1 - mom0).max() <= 16 * np.finfo(float).eps * np.abs(mass[:, None] * vel).sum()
    g = [1, 4, 7]
    assert m[1] == mass[g].sum()
    assert np.allclose(p[1], (mass[g, None] * pos[g]).sum(0) / mass[g].sum(), rtol=1e-14)
    assert np.isclose(R[1], np.cbrt((rad[g] ** 3).sum()), rtol=1e-15)
    assert np.isclose(R[2], np.cbrt(rad[2] ** 3 + rad[6] ** 3), rtol=1e-15)
    for i, j in ((0, 0), (3, 3), (4, 5), (5, 8)):  # (bodies that overlap nobody: untouched)
        assert np.array_equal(p[i], pos[j]) and m[i] == mass[j] and R[i] == rad[j]
    # q >= eps^2 is no overlap; massless components merge at their mean position
    same = oracle.merge_overlaps(pos, vel, mass, rad, ids, np.full(n, 4.0), ca_nn, softening=2.0)
    assert same[5] == 0 and np.array_equal(same[0], pos)
    z = oracle.merge_overlaps(pos[:2], vel[:2], np.zeros(2), rad[:2], ids[:2],
                              np.array([-1.0, 1.0]), np.array([1, -1]))
    assert z[5] == 1 and np.allclose(z[0][0], pos[:2].mean(0)) and z[2][0] == 0.0


# ---- 4. the driver: merge runs, metrics, CLI, checkpoints ---------------------------------------
@pytest.mark.parametrize("block", [False, True])
def test_three_body_chain_becomes_one_body(block):
    b = chain_and_bystander()
    kw = dict(block_steps=True, eta=0.02, max_level=6) if block else {}
    s, ids, m, _ = run_driver(b, steps=3, collisions="merge", **kw)
    assert list(ids) == [0, 3] and m.mergers == 2 and m.bodies_left == 2 and m.steps_taken == 3
    assert m.overlaps_seen == 3 and m.closest_q_min < 0
    assert s.n == 2 and np.isclose(s.mass[0], 6e24, rtol=1e-15) and s.mass[1] == 1e23
    assert np.isclose(s.radius[0], np.cbrt(3 * 2e7 ** 3), rtol=1e-15) and s.radius[1] == 1e6
    # momentum: the merger conserves it to rounding, the integrator over three steps as well
    p0, p1 = (b.mass[:, None] * b.vel).sum(0), (s.mass[:, None] * s.vel).sum(0)
    assert np.abs(p1 - p0).max() <= 1e-12 * np.abs(b.mass[:, None] * b.vel).sum()
    off = run_driver(b, steps=3, collisions="off", **kw)
    assert off[0].n == 4 and off[2].mergers is None


@pytest.mark.parametrize("block", [False, True])
def test_detect_reports_and_changes_no_bit(block):
    b = head_on((1.5e11, 0.7e11, -0.3e11), mass=1e23)
    kw = dict(dt=8000.0, block_steps=True, eta=0.02, max_level=6) if block else {}
    steps = 11 if block else 85
    off, _, m0, _ = run_driver(b, steps=steps, collisions="off", **kw)
    det, ids, m1, _ = run_driver(b, steps=steps, collisions="detect", **kw)
    assert np.array_equal(off.pos, det.pos) and np.array_equal(off.vel, det.vel)
    assert m1.mergers == 0 and m1.bodies_left == 2 and list(ids) == [0, 1]
    assert m1.overlaps_seen >= 2 and m1.closest_q_min < 0 and m1.steps_taken == steps
    assert m0.overlaps_seen is None and "mergers" not in json.loads(m0.to_json())


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_resume_is_bit_exact_across_a_merger(tmp_path, dtype):
    """Two bodies merge at step 71; checkpoints at 50 (before) and 100 (after)."""
    h = head_on((1.5e11, 0.7e11, -0.3e11))
    b = BodySet(np.vstack([h.pos, [[2e11, 0, 0]]]), np.vstack([h.vel, [[0, 2e4, 0]]]),
                np.append(h.mass, 1e22), np.append(h.radius, 1e6))
    kw = dict(collisions="merge", checkpoint_dir=str(tmp_path), dtype=dtype)
    full, ids, m, step = run_driver(b, steps=120, checkpoint_every=50, **kw)
    assert m.mergers == 1 and list(ids) == [0, 2] and step == 120 and m.steps_taken == 120
    assert np.isclose(full.radius[0], np.cbrt(2.0) * 2.05e7, rtol=1e-15)
    for at, left in ((50, 3), (100, 2)):
        c = ck.load(ck.path_for(str(tmp_path), at))
        assert c.bodies.n == left and c.meta["collide_columns"] == ["radius", "id"]
        got, gids, gm, gstep = run_driver(b, steps=120, resume=ck.path_for(str(tmp_path), at),
                                          run_steps=120 - at, **kw)
        assert gstep == 120 and list(gids) == [0, 2] and gm.mergers == 1
        assert np.array_equal(got.pos, full.pos) and np.array_equal(got.vel, full.vel)
        assert np.array_equal(got.radius, full.radius)
    # a checkpoint without the columns loads as before
    plain = run_driver(b, steps=4, collisions="off", checkpoint_dir=str(tmp_path / "p"),
                       checkpoint_every=4)
    c = ck.load(ck.path_for(str(tmp_path / "p"), 4))
    assert "collide" not in c.extra
    again = run_driver(b, steps=4, collisions="off", resume=ck.path_for(str(tmp_path / "p"), 4),
                       run_steps=0)
    assert np.array_equal(again[0].pos, plain[0].pos)


def test_cli_merge_end_to_end(tmp_path):
    out = tmp_path / "m.json"
    rc = main(["--n", "64", "--steps", "20", "--dt", "3600", "--device", "cpu", "--init", "cold",
               "--integrator", "hermite", "--collisions", "merge", "--body-density", "1e-3",
               "--quiet", "--log-format", "none", "--metrics-json", str(out)])
    d = json.loads(out.read_text().strip().splitlines()[-1])
    assert rc == 0 and d["mergers"] >= 1 and d["bodies_left"] == 64 - d["mergers"]
    assert d["steps_taken"] == 20 and d["overlaps_seen"] >= d["mergers"] and d["closest_q_min"] < 0


def test_config_and_radius_rules():
    with pytest.raises(ValueError):
        SimConfig(n=8, collisions="merge").validate()  # (integrator kd)
    with pytest.raises(ValueError):
        SimConfig(n=8, integrator="leapfrog", body_density=1.0).validate()
    with pytest.raises(ValueError):
        SimConfig(n=8, integrator="hermite", collisions="maybe").validate()
    with pytest.raises(ValueError):
        SimConfig(n=8, integrator="hermite", collisions="detect", body_density=0.0).validate()
    b = BodySet(np.zeros((3, 3)), np.zeros((3, 3)), np.array([0.0, 1e24, 8e24]))
    r = b.radii(1000.0)
    assert r[0] == 0 and np.isclose(r[1], np.cbrt(3e24 / (4e3 * np.pi))) and np.isclose(r[2], 2 * r[1])
    assert not b.radii().any() and b.copy().radius is None


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_block_run_merges_at_the_macro_boundary(tmp_path, dtype):
    """Block steps, macro step 44,000 s: the two bodies of 1e23 kg touch at about 7.9e4 s, inside
    the second macro step, and are merged at its boundary (88,000 s), not before and not later.
    The driver's figures carry across the engine restart, and a resume is bit-exact from the
    checkpoint before the merger (step 1) and from the one after it (step 2)."""
    b = merger_with_bystander(mass=1e23)
    kw = dict(dtype=dtype, dt=44000.0, block_steps=True, eta=0.02, max_level=10)
    first, ids1, m1, _ = run_driver(b, steps=1, collisions="merge", **kw)
    assert m1.mergers == 0 and list(ids1) == [0, 1, 2] and first.n == 3 and m1.overlaps_seen == 0
    two, ids2, m2, _ = run_driver(b, steps=2, collisions="merge", **kw)
    assert m2.mergers == 1 and list(ids2) == [0, 2] and m2.bodies_left == 2 and two.n == 2
    assert m2.steps_taken == 2 and m2.time_reached == 88000.0 and m2.overlaps_seen >= 2
    # the same two macro steps without the merger: what the merged body is made of
    det, _, md, _ = run_driver(b, steps=2, collisions="detect", **kw)
    assert det.n == 3 and np.array_equal(det.pos[2], two.pos[1]) and two.mass[1] == 1e22
    mt = det.mass[0] + det.mass[1]
    assert two.mass[0] == mt and two.radius[0] == np.cbrt(2 * 2.05e7 ** 3)
    com = (det.mass[:2, None] * det.pos[:2]).sum(0) / mt
    assert np.abs(two.pos[0] - com).max() <= 4 * np.finfo(float).eps * np.abs(com).max()
    p0, p1 = (det.mass[:, None] * det.vel).sum(0), (two.mass[:, None] * two.vel).sum(0)
    assert np.abs(p1 - p0).max() <= 8 * np.finfo(float).eps * np.abs(det.mass[:, None] * det.vel).sum()
    # up to the merger the engine did what the detect run did; pairs are counted against 3 bodies
    assert (m2.block_steps, m2.body_steps, m2.level_max, m2.level_clamped) == \
        (md.block_steps, md.body_steps, md.level_max, md.level_clamped)
    assert m2.block_steps > 2 and m2.pair_evals == 3 * m2.body_steps
    # four macro steps: the counters of the engine before and of the engine after add up
    ckdir = str(tmp_path)
    full, ids, m, step = run_driver(b, steps=4, collisions="merge", checkpoint_dir=ckdir,
                                    checkpoint_every=1, **kw)
    tail, _, mtail, _ = run_driver(two, steps=2, collisions="merge", **kw)
    assert m.mergers == 1 and list(ids) == [0, 2] and step == 4 and m.steps_taken == 4
    assert m.time_reached == 176000.0
    assert m.block_steps == m2.block_steps + mtail.block_steps
    assert m.body_steps == m2.body_steps + mtail.body_steps
    assert m.pair_evals == 3 * m2.body_steps + 2 * mtail.body_steps
    assert m.level_max == max(m2.level_max, mtail.level_max)
    assert m.level_clamped == m2.level_clamped + mtail.level_clamped
    assert np.array_equal(full.pos, tail.pos) and np.array_equal(full.vel, tail.vel)
    for at, left in ((1, 3), (2, 2)):
        c = ck.load(ck.path_for(ckdir, at))
        assert c.bodies.n == left and c.meta["block_steps"] and "level" in c.extra
        got, gids, gm, gstep = run_driver(b, steps=4, collisions="merge",
                                          resume=ck.path_for(ckdir, at), run_steps=4 - at, **kw)
        assert gstep == 4 and list(gids) == [0, 2] and gm.mergers == 1
        assert np.array_equal(got.pos, full.pos) and np.array_equal(got.vel, full.vel)


def test_periodic_work_never_runs_ahead_of_a_stopped_engine(tmp_path):
    """Shared step, merger at step 71 of 120, a frame every 10 steps: 12 frames, each taken at its
    own step (3 bodies up to step 70, 2 from step 80), and one checkpoint per period."""
    b = merger_with_bystander()
    sim = Simulation(SimConfig(n=3, device="cpu", integrator="hermite", dt=1000.0, steps=120,
                               collisions="merge", record_every=10, checkpoint_every=40,
                               checkpoint_dir=str(tmp_path)))
    try:
        sim.engine.load(b)
        m = sim.run()
        frames = sim.trajectory
    finally:
        sim.close()
    assert m.mergers == 1 and m.steps_taken == 120
    assert [len(f) for f in frames] == [3] * 7 + [2] * 5
    for a, c in zip(frames[7:], frames[8:]):
        assert not np.array_equal(a, c)
    assert sorted(p.name for p in tmp_path.iterdir()) == \
        sorted(os.path.basename(ck.path_for(str(tmp_path), k)) for k in (40, 80, 120))
