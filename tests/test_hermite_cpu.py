"""4th-order Hermite integrator on the CPU: the NumPy oracle's scheme, the native C++
acceleration+jerk sum and step against it, adaptive steps, checkpoints, validation and the CLI.

Accuracy gates: |err| <= 128 eps sum_j |term_ij| (the gate of tests/test_gpu_kernels.py
assert_close_sum); the jerk's scale is, per component c,
sum_j mu_j r^-3 (|w_c| + 3 (sum_k |d_k w_k|) |d_c| / r^2) (oracle.acc_jerk with_abs).
"""
import json
import math
import subprocess
import sys

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.ops import _native, oracle
from gravsim.ops.force import acc_jerk
from gravsim.parallel import comm
from gravsim.parallel.partition import layout
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ckpt

EPS = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}


def quantized_acc_jerk(b, dtype, **kw):
    """Oracle on the inputs as the native code sees them (positions, velocities and mu = G m
    rounded to dtype): ref acc, jerk, phi and the two rounding scales."""
    T = np.float32 if dtype == "fp32" else np.float64
    p = b.pos.astype(T).astype(np.float64)
    v = b.vel.astype(T).astype(np.float64)
    mu = (G_SI * b.mass).astype(T).astype(np.float64)
    return oracle.acc_jerk(p, v, mu, G=1.0, with_potential=True, with_abs=True, **kw)


def worst_ratio(got, ref, scale, dtype):
    return float((np.abs(got - ref) / (EPS[dtype] * scale + 1e-300)).max())


def eccentric_pair():
    """ic.kepler() with both velocities scaled by 0.6: eccentricity 0.64, period 173.9 days
    (the pair starts at apocentre). Returns (bodies, period, separation)."""
    b = ic.kepler()
    b.vel = b.vel * 0.6
    mt = b.mass.sum()
    r = np.linalg.norm(b.pos[1] - b.pos[0])
    v = np.linalg.norm(b.vel[1] - b.vel[0])
    sma = -G_SI * mt / (2.0 * (0.5 * v * v - G_SI * mt / r))
    return b, 2.0 * math.pi * math.sqrt(sma ** 3 / (G_SI * mt)), r


def energy(b):
    _, phi = oracle.accelerations(b.pos, b.mass, with_potential=True)
    return 0.5 * (b.mass * (b.vel ** 2).sum(1)).sum() + 0.5 * (b.mass * phi).sum()


def rel_energy_error(b0, pos, vel):
    e0 = energy(b0)
    return abs(energy(ic.BodySet(pos, vel, b0.mass)) - e0) / abs(e0)


@pytest.fixture(scope="module")
def pair():
    return eccentric_pair()


@pytest.fixture(scope="module")
def adaptive_ref(pair):
    """The oracle's adaptive orbit: eta 0.02, dt_max T/50, t_end T."""
    b, T, _ = pair
    return oracle.simulate(b.pos, b.vel, b.mass, T / 50, 100000, integrator="hermite", eta=0.02,
                           t_end=T)


# ---- 1. jerk against a central difference ------------------------------------------------
def test_oracle_jerk_is_the_time_derivative_of_acc():
    b = ic.solar_random(300, 5)
    a, j, phi = oracle.acc_jerk(b.pos, b.vel, b.mass, with_potential=True)
    h = 10.0
    cd = (oracle.accelerations(b.pos + b.vel * h, b.mass) -
          oracle.accelerations(b.pos - b.vel * h, b.mass)) / (2 * h)
    rel = np.linalg.norm(j - cd, axis=1) / np.linalg.norm(j, axis=1)
    print(f"jerk vs central difference: {rel.max():.3g}")
    assert rel.max() < 1e-7
    a0, phi0 = oracle.accelerations(b.pos, b.mass, with_potential=True)
    assert np.abs(a - a0).max() <= 1e-15 * np.abs(a0).max()
    assert np.abs(phi - phi0).max() <= 1e-15 * np.abs(phi0).max()


# ---- 2. native CPU against the oracle ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 65, 1000, 2049])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_native_accjerk_matches_oracle(n, dtype):
    b = ic.solar_random(n, seed=7 + n)
    ra, rj, rphi, sa, sj = quantized_acc_jerk(b, dtype)
    ga, gj, gphi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype=dtype)
    r = (worst_ratio(ga, ra, sa, dtype), worst_ratio(gj, rj, sj, dtype),
         worst_ratio(gphi, rphi, np.abs(rphi), dtype))
    print(f"n={n} {dtype}: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f} (x eps x scale)")
    assert r[0] <= 128.0 and r[1] <= 128.0 and r[2] <= 128.0
    if n == 1:
        assert not ga.any() and not gj.any() and not gphi.any()


def test_native_accjerk_range_and_chunk_order():
    """A sub-range of i equals the same rows of the full call; the canonical chunk (2048) is
    what the one-shot entry uses, and another chunk length changes only rounding."""
    lib = _native.cpu_lib()
    n = 2500
    b = ic.solar_random(n, 3)
    X = np.zeros((n, 4))
    V = np.zeros((n, 4))
    X[:, :3], X[:, 3], V[:, :3] = b.pos, G_SI * b.mass, b.vel
    full = [np.zeros((n, 4)), np.zeros((n, 4))]
    part = [np.zeros((100, 4)), np.zeros((100, 4))]
    other = [np.zeros((n, 4)), np.zeros((n, 4))]
    d = _native.dptr
    assert lib.gs_cpu_accjerk_f64(d(X), d(V), n, 0, n, 2048, 1e-20, 0.0, d(full[0]),
                                  d(full[1])) == 0
    assert lib.gs_cpu_accjerk_f64(d(X), d(V), n, 2000, 2100, 2048, 1e-20, 0.0, d(part[0]),
                                  d(part[1])) == 0
    assert lib.gs_cpu_accjerk_f64(d(X), d(V), n, 0, n, 1024, 1e-20, 0.0, d(other[0]),
                                  d(other[1])) == 0
    assert np.array_equal(part[0], full[0][2000:2100])
    assert np.array_equal(part[1], full[1][2000:2100])
    assert layout(n).chunk == 2048
    ga, gj, _ = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="fp64")
    assert np.array_equal(ga, full[0][:, :3]) and np.array_equal(gj, full[1][:, :3])
    assert not np.array_equal(other[1], full[1])
    assert np.allclose(other[1], full[1], rtol=1e-9, atol=0)
    assert lib.gs_cpu_accjerk_f64(d(X), d(V), n, 0, n + 1, 2048, 1e-20, 0.0, d(full[0]),
                                  d(full[1])) != 0  # rows past n_real are refused


# ---- 3. order of accuracy ----------------------------------------------------------------
def closure_errors(run, pair):
    """Relative orbit-closure error after one period at T/500, T/1000, T/2000."""
    b, T, r = pair
    return [np.linalg.norm(run(b, T / m, m) - b.pos) / r for m in (500, 1000, 2000)]


def assert_fourth_order(errs):
    print("closure errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    assert 12.0 <= errs[0] / errs[1] <= 22.0
    assert 12.0 <= errs[1] / errs[2] <= 22.0
    assert errs[1] < 1e-6


def test_oracle_is_fourth_order(pair):
    def run(b, dt, m):
        x, _, _, t, taken = oracle.simulate(b.pos, b.vel, b.mass, dt, m, integrator="hermite")
        assert len(taken) == m and all(h == dt for h in taken)
        return x

    assert_fourth_order(closure_errors(run, pair))


def test_circular_orbit_energy_beats_leapfrog():
    b = ic.kepler()
    r = np.linalg.norm(b.pos[1] - b.pos[0])
    T = 2.0 * math.pi * math.sqrt(r ** 3 / (G_SI * b.mass.sum()))
    m = int(round(T / 4 / 86400.0))
    x, v, _, _, _ = oracle.simulate(b.pos, b.vel, b.mass, 86400.0, m, integrator="hermite")
    xl, vl, _ = oracle.simulate(b.pos, b.vel, b.mass, 86400.0, m, integrator="leapfrog")
    eh, el = rel_energy_error(b, x, v), rel_energy_error(b, xl, vl)
    print(f"quarter period, dt 86400: hermite {eh:.3g} leapfrog {el:.3g}")
    assert eh < 1e-9 and eh < el


# ---- 4. adaptive steps -------------------------------------------------------------------
def test_oracle_adaptive_orbit(pair, adaptive_ref):
    b, T, _ = pair
    x, v, _, t, taken = adaptive_ref
    assert t == T
    assert 90 <= len(taken) <= 140
    assert abs(sum(taken) - T) <= 1e-9 * T and max(taken) <= T / 50
    xf, vf, _, _, _ = oracle.simulate(b.pos, b.vel, b.mass, T / len(taken), len(taken),
                                      integrator="hermite")
    ea, ef = rel_energy_error(b, x, v), rel_energy_error(b, xf, vf)
    print(f"{len(taken)} steps: adaptive {ea:.3g}, fixed {ef:.3g}, "
          f"dt_min/dt_max {min(taken[:-1]) / (T / 50):.3f}")
    assert ea * 50 <= ef
    assert min(taken[:-1]) / (T / 50) < 0.2
    # the cap on the step count holds, and a run past t_end takes no further step
    assert len(oracle.simulate(b.pos, b.vel, b.mass, T / 50, 7, integrator="hermite", eta=0.02,
                               t_end=T)[4]) == 7


def test_native_first_step_rule():
    """(eta / 2) min |a| / |j| on hand-made rows: |a|/|j| = 5/5, 1/0 (skipped: |j| = 0), 2/8;
    and the CPU engine's first dt_next against the formula written out here on its own a, j."""
    lib = _native.cpu_lib()
    A = np.array([[3, 4, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0]], dtype=np.float64)
    J = np.array([[0, 0, 5, 0], [0, 0, 0, 0], [0, 0, 8, 0]], dtype=np.float64)
    d = _native.dptr
    assert lib.gs_cpu_hermite_first_dt_f64(d(A), d(J), 3, 0.02) == 0.01 * 0.25
    assert lib.gs_cpu_hermite_first_dt_f64(d(A), d(J), 2, 0.02) == 0.01
    assert lib.gs_cpu_hermite_first_dt_f64(d(A[1:]), d(J[1:]), 1, 0.02) == math.inf
    Af, Jf = A.astype(np.float32), J.astype(np.float32)
    assert lib.gs_cpu_hermite_first_dt_f32(_native.fptr(Af), _native.fptr(Jf), 3, 0.02) == 0.0025
    from gravsim.runtime.hermite import HermiteCpuEngine

    eng = HermiteCpuEngine(SimConfig(n=300, dt=1e9, eta=0.02, device="cpu",
                                     integrator="hermite"))
    eng.init_ics("solar+random", 9)
    a, j = eng.carried()
    want = (0.01 * np.sqrt((a * a).sum(1)) / np.sqrt((j * j).sum(1))).min()
    assert abs(eng.status().dt_next / want - 1.0) < 1e-14 and want < 1e9


# ---- 5. CPU engine against the oracle ----------------------------------------------------
def test_cpu_engine_matches_oracle_fixed():
    cfg = SimConfig(n=400, steps=12, dtype="fp64", device="cpu", integrator="hermite")
    sim = Simulation(cfg)
    b0 = ic.solar_random(400, cfg.seed)
    m = sim.run()
    got = sim.global_state()
    x, v, _, t, taken = oracle.simulate(b0.pos, b0.vel, b0.mass, cfg.dt, 12, integrator="hermite")
    assert np.abs(got.pos - x).max() / np.abs(x).max() < 1e-12
    assert np.abs(got.vel - v).max() / np.abs(v).max() < 1e-10
    st = sim.engine.status()
    assert st.time == t == 12 * cfg.dt and st.steps == 12 and not st.finished
    assert m.time_reached == t and m.steps_taken == 12 and m.dt_min == cfg.dt


def test_cpu_engine_matches_oracle_adaptive(pair, adaptive_ref):
    b, T, _ = pair
    x, v, _, t, taken = adaptive_ref
    cfg = SimConfig(n=2, steps=1000, dt=T / 50, dtype="fp64", device="cpu", init="kepler",
                    integrator="hermite", eta=0.02, t_end=T)
    sim = Simulation(cfg)
    sim.engine.load(b)
    got_dt = []
    while not sim.engine.status().finished:
        sim.engine.step(1)
        got_dt.append(sim.engine.status().dt_last)
    assert len(got_dt) == len(taken)
    assert np.abs(np.array(got_dt) / np.array(taken) - 1.0).max() < 1e-9
    st = sim.engine.status()
    assert st.time == T and st.finished
    assert st.dt_min == min(got_dt[:-1])
    got = sim.engine.state()
    assert np.abs(got.pos - x).max() / np.abs(x).max() < 1e-12
    assert np.abs(got.vel - v).max() / np.abs(v).max() < 1e-10
    sim.engine.step(5)  # past t_end: no-ops, not counted
    after = sim.engine.state()
    assert np.array_equal(after.pos, got.pos) and sim.engine.status().steps == len(taken)


def test_cpu_driver_stops_at_t_end(pair, adaptive_ref):
    b, T, _ = pair
    cfg = SimConfig(n=2, steps=1000, dt=T / 50, dtype="fp64", device="cpu", init="kepler",
                    integrator="hermite", eta=0.02, t_end=T, diagnostics=True)
    sim = Simulation(cfg)
    sim.engine.load(b)
    m = sim.run()
    assert m.time_reached == T and m.steps_taken == m.steps == len(adaptive_ref[4])
    assert m.dt_min / cfg.dt < 0.2
    assert m.extra["conservation"]["energy_rel_drift"] < 1e-4
    d = json.loads(m.to_json())
    assert d["time_reached"] == T and d["steps_taken"] == m.steps and d["dt_min"] == m.dt_min


def test_cpu_engine_fp32_tracks_fp64():
    out = {}
    for dtype in ("fp32", "fp64"):
        sim = Simulation(SimConfig(n=300, steps=8, dtype=dtype, device="cpu",
                                   integrator="hermite"))
        sim.run()
        out[dtype] = sim.global_state()
    assert np.abs(out["fp32"].pos - out["fp64"].pos).max() / np.abs(out["fp64"].pos).max() < 1e-5
    assert np.abs(out["fp32"].vel - out["fp64"].vel).max() / np.abs(out["fp64"].vel).max() < 1e-4


# ---- 6. resume and validation ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("eta", [0.0, 0.02])
def test_resume_is_bit_exact(tmp_path, dtype, eta):
    cfg = SimConfig(n=200, steps=5, dt=4e5, dtype=dtype, device="cpu", integrator="hermite",
                    eta=eta)
    sim = Simulation(cfg)
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    sim.run(3)
    ref, ref_st = sim.global_state(), sim.engine.status()
    c = ckpt.load(path)
    assert c.meta["extra"] == ["acc", "jerk"] and c.meta["integrator"] == "hermite"
    assert c.extra["acc"].shape == (200, 3) and c.step == 5
    sim2 = Simulation(cfg.replace(resume=path))
    assert sim2.engine.status().time == c.meta["time"] and sim2.step == 5
    sim2.run(3)
    got, got_st = sim2.global_state(), sim2.engine.status()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert got_st.time == ref_st.time and got_st.dt_next == ref_st.dt_next
    assert sim2.step == 8
    if eta:
        assert ref_st.dt_last < cfg.dt  # the criterion, not the ceiling, chose the steps


def test_old_checkpoints_and_other_integrators(tmp_path):
    b = ic.solar_random(50, 1)
    # the format before this integrator: no "extra" in the header, nothing after mass
    old = str(tmp_path / "old.gsck")
    ckpt.save(old, b, 4, dict(dt=3600.0, time=4 * 3600.0, integrator="kd",
                              velocity="synchronized"))
    c = ckpt.load(old)
    assert c.extra == {} and "extra" not in c.meta and np.array_equal(c.bodies.pos, b.pos)
    # a reader that stops after mass still gets the same bodies from a Hermite checkpoint
    new = str(tmp_path / "new.gsck")
    ckpt.save(new, b, 4, dict(dt=3600.0),
              extra={"acc": np.ones((50, 3)), "jerk": np.zeros((50, 3))})
    c2 = ckpt.load(new)
    assert np.array_equal(c2.bodies.mass, b.mass)
    assert np.array_equal(c2.extra["acc"], np.ones((50, 3)))
    assert open(new, "rb").read()[: -2 * 50 * 24].endswith(b.mass.astype("<f8").tobytes())
    # a KD checkpoint resumed under hermite: a, j evaluated afresh, time carried on
    sim = Simulation(SimConfig(n=50, steps=3, device="cpu", integrator="hermite", seed=1,
                               resume=old))
    m = sim.run()
    assert sim.step == 7 and m.time_reached == 7 * 3600.0 and sim.engine.nonfinite() == 0
    x, v, _, _, _ = oracle.simulate(b.pos, b.vel, b.mass, 3600.0, 3, integrator="hermite")
    assert np.abs(sim.global_state().pos - x).max() / np.abs(x).max() < 1e-12
    # a leapfrog checkpoint (half-step velocities) is synchronised first
    lf = Simulation(SimConfig(n=50, steps=2, device="cpu", integrator="leapfrog", seed=1))
    lf.run()
    path = str(tmp_path / "lf.gsck")
    lf.save_checkpoint(path)
    want = lf.global_state()
    sim = Simulation(SimConfig(n=50, steps=0, device="cpu", integrator="hermite", seed=1,
                               resume=path))
    got = sim.global_state()
    assert np.abs(got.vel - want.vel).max() <= 1e-12 * np.abs(want.vel).max()
    assert sim.engine.status().time == 2 * 3600.0


def test_validation():
    for kw in (dict(integrator="kd", eta=0.02), dict(integrator="leapfrog", t_end=10.0),
               dict(integrator="hermite", cutoff=0.0, softening=0.0),
               dict(integrator="hermite", eta=-0.1), dict(integrator="hermite", t_end=-1.0),
               dict(integrator="hermite", ipl=8, dtype="fp32"), dict(integrator="rk4")):
        with pytest.raises(ValueError):
            SimConfig(**kw).validate()
    SimConfig(integrator="hermite", cutoff=0.0, softening=1e6).validate()
    assert SimConfig().integrator == "kd" and SimConfig().eta == 0.0 and SimConfig().t_end is None
    with pytest.raises(ValueError):
        oracle.simulate(np.zeros((1, 3)), np.zeros((1, 3)), np.ones(1), 1.0, 1, eta=0.1)


def test_two_ranks_are_refused_before_any_engine(monkeypatch):
    import gravsim.runtime.simulation as simulation

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    for name in ("HermiteCpuEngine", "HermiteHipEngine", "CpuEngine", "HipEngine"):
        monkeypatch.setattr(simulation, name, no_engine)
    cfg = SimConfig(n=64, device="cpu", integrator="hermite")
    with pytest.raises(ValueError, match="hermite runs on one rank"):
        Simulation(cfg, comm.DistInfo(rank=1, world=2))
    from gravsim.runtime.hermite import HermiteCpuEngine

    with pytest.raises(ValueError, match="hermite runs on one rank"):
        HermiteCpuEngine(cfg, 0, 2)


# ---- 7. CLI ------------------------------------------------------------------------------
def test_cli_hermite_metrics(tmp_path):
    out = tmp_path / "m.jsonl"
    t_end = 40 * 3600.0
    r = subprocess.run([sys.executable, "-m", "gravsim", "--n", "64", "--integrator", "hermite",
                        "--eta", "0.02", "--t-end", str(t_end), "--steps", "500", "--device",
                        "cpu", "--metrics-json", str(out), "--quiet", "--log-format", "none"],
                       capture_output=True, text=True, timeout=300,
                       cwd=str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.loads(out.read_text().splitlines()[-1])
    assert m["time_reached"] == t_end
    assert 40 <= m["steps_taken"] < 500 and m["steps"] == m["steps_taken"]
    assert 0 < m["dt_min"] <= 3600.0
    r = subprocess.run([sys.executable, "-m", "gravsim", "--n", "64", "--eta", "0.02", "--device",
                        "cpu", "--steps", "1"], capture_output=True, text=True, timeout=300,
                       cwd=str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    assert r.returncode != 0 and "hermite" in r.stderr
