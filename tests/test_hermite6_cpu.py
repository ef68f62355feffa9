"""The 6th-order Hermite scheme (Nitadori & Makino 2008) without a GPU: the oracle's snap and
higher derivatives against their definitions, the order of accuracy of the oracle and of the
native CPU engine, the adaptive step, the CPU engine against the oracle, and the command line
(checkpoints, resume, refusals, metrics)."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from gravsim import cli
from gravsim.config import SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.ops import oracle
from gravsim.ops.force import acc_jerk_snap
from gravsim.runtime.hermite import HermiteCpuEngine
from gravsim.utils import checkpoint as ckpt

import hermite6_helpers as h6

ROOT = str(pathlib.Path(__file__).resolve().parent.parent)


def test_snap_is_the_second_derivative_of_the_acceleration():
    """50 random bodies: the snap against (a(x+) - 2 a(x) + a(x-)) / delta^2 along
    x+- = x +- v delta + a delta^2 / 2, at two deltas: the difference falls as delta^2 (the
    second difference's own truncation error), so it is the formula's, not the snap's."""
    b = ic.random_cube(50, 3)
    a, j, s, _ = acc_jerk_snap(b.pos, b.vel, b.mass, device="oracle")
    a4, j4 = oracle.acc_jerk(b.pos, b.vel, b.mass)
    assert np.array_equal(a, a4) or np.abs(a - a4).max() <= 4e-16 * np.abs(a4).max()
    assert np.abs(j - j4).max() <= 1e-14 * np.abs(j4).max()
    scale = np.abs(s).max()
    err = []
    for delta in (2e3, 1e3):
        xp = b.pos + b.vel * delta + a * (delta * delta / 2)
        xm = b.pos - b.vel * delta + a * (delta * delta / 2)
        fd = (oracle.accelerations(xp, b.mass) - 2.0 * a + oracle.accelerations(xm, b.mass)) \
            / delta ** 2
        err.append(float(np.abs(fd - s).max() / scale))
    print(f"snap against the second difference: {err[0]:.2e}, {err[1]:.2e} of max |s|")
    assert err[1] < 1e-4                       # the formula is the second derivative ...
    assert 3.0 < err[0] / err[1] < 5.0         # ... and what is left is the O(delta^2) term


def test_higher_derivatives_match_a_polynomial_solve():
    rng = np.random.default_rng(11)
    a0, j0, s0, a1, j1, s1 = (rng.standard_normal((40, 3)) for _ in range(6))
    for h in (0.37, 2.5, 1e3):
        c1, p1, a5 = oracle.hermite6_high(a0, j0 / h, s0 / h ** 2, a1, j1 / h, s1 / h ** 2, h)
        r3, r4, r5 = h6.poly_high(a0, j0 / h, s0 / h ** 2, a1, j1 / h, s1 / h ** 2, h)
        for got, ref in ((c1, r3), (p1, r4), (a5, r5)):
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # a quintic's own derivatives come back
    c = rng.standard_normal((6, 5, 3))
    h = 0.8
    f = lambda k, t: sum(c[m] * np.prod(np.arange(m, m - k, -1)) * t ** (m - k)  # noqa: E731
                         for m in range(k, 6))
    c1, p1, a5 = oracle.hermite6_high(f(0, 0.0), f(1, 0.0), f(2, 0.0), f(0, h), f(1, h), f(2, h), h)
    for got, k in ((c1, 3), (p1, 4), (a5, 5)):
        assert np.abs(got - f(k, h)).max() <= 1e-11 * np.abs(f(k, h)).max()


def test_order_of_the_oracle():
    o6 = h6.orders(lambda b, dt, k: oracle.simulate_hermite6(b.pos, b.vel, b.mass, dt, k)[0])
    o4 = h6.orders(lambda b, dt, k: oracle.simulate_hermite(b.pos, b.vel, b.mass, dt, k)[0])
    print(f"orders: 6th {o6[0]:.2f} {o6[1]:.2f}, 4th {o4[0]:.2f} {o4[1]:.2f}")
    assert 5.7 <= o6[0] <= 6.3 and 5.7 <= o6[1] <= 6.3
    assert o4[0] < 4.5 and o4[1] < 4.5


def test_order_of_the_cpu_engine():
    o = h6.orders(h6.engine_positions(HermiteCpuEngine, "cpu"))
    print(f"orders: {o[0]:.2f} {o[1]:.2f}")
    assert 5.7 <= o[0] <= 6.3 and 5.7 <= o[1] <= 6.3


def test_adaptive_step_takes_fewer_steps_for_less_error():
    b, period = h6.two_body(0.9)
    e0 = h6.energy(b)
    out = {}
    for name, fn, eta in (("6", oracle.simulate_hermite6, 0.18), ("4", oracle.simulate_hermite,
                                                                  0.005)):
        x, v, _, t, taken = fn(b.pos, b.vel, b.mass, period, 100000, eta=eta, t_end=period)
        assert t == period
        out[name] = (len(taken), abs(h6.energy(h6.BodySet(x, v, b.mass)) - e0) / abs(e0))
    print(f"order 6: {out['6'][0]} steps, dE/E {out['6'][1]:.2e}; "
          f"order 4: {out['4'][0]} steps, dE/E {out['4'][1]:.2e}")
    assert out["6"][0] < 0.7 * out["4"][0]
    assert out["6"][1] < out["4"][1]


def test_cpu_engine_matches_the_oracle():
    cfg = SimConfig(n=h6.CASE_N, dt=h6.CASE_DT, eta=h6.CASE_ETA, t_end=h6.adaptive_case()[1],
                    dtype="fp64", device="cpu", integrator="hermite", hermite_order=6).validate()
    h6.check_against_oracle(HermiteCpuEngine(cfg))


def test_cpu_engine_fp32_runs_and_carries_four_rows():
    cfg = SimConfig(n=100, dt=3600.0, eta=0.25, dtype="fp32", device="cpu", integrator="hermite",
                    hermite_order=6).validate()
    eng = HermiteCpuEngine(cfg)
    eng.init_ics("solar+random", 2)
    eng.step(5)
    rows = eng.carried()
    assert len(rows) == 4 and all(r.shape == (100, 3) and np.isfinite(r).all() for r in rows)
    assert rows[3].any() and eng.nonfinite() == 0 and eng.status().steps == 5
    a4, j4, s4 = eng.derivs()
    ref = acc_jerk_snap(*(y.astype(np.float32).astype(float)
                          for y in (eng.state().pos, eng.state().vel)), eng.state().mass,
                        device="oracle")
    assert np.abs(s4[:, :3] - ref[2]).max() <= 1e-4 * np.abs(ref[2]).max()


@pytest.mark.parametrize("kw, word", [
    (dict(block_steps=True, eta=0.25), "--block-steps"),
    (dict(dtype="mixed"), "--dtype mixed"),
    (dict(collisions="detect", softening=1e6), "--collisions"),
    (dict(gpus=2), "--gpus"),
])
def test_simconfig_refusals_name_the_option(kw, word):
    with pytest.raises(ValueError, match=word):
        SimConfig(n=64, integrator="hermite", hermite_order=6, **kw).validate()
    with pytest.raises(ValueError, match="hermite_order"):
        SimConfig(n=64, integrator="hermite", hermite_order=5).validate()
    with pytest.raises(ValueError, match="hermite"):
        SimConfig(n=64, integrator="kd", hermite_order=6).validate()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gravsim", "--n", "120", "--integrator",
                           "hermite", "--hermite-order", "6", "--eta", "0.25", "--dt", "4e5",
                           "--device", "cpu", "--seed", "3", "--quiet", "--log-format", "none",
                           *args], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_cli_checkpoint_resume_refusals_and_metrics(tmp_path):
    """Through python -m gravsim: 8 steps in one go against 5 + a resumed 3 (bit for bit), the
    checkpoint's four arrays, hermite_order in the metrics, and a refusal at the command line."""
    out = tmp_path / "m.jsonl"
    whole, part = str(tmp_path / "whole.gsck"), str(tmp_path / "part.gsck")
    r = _cli("--steps", "8", "--checkpoint-dir", str(tmp_path / "ck"), "--checkpoint-every", "5",
             "--dump", whole, "--metrics-json", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.loads(out.read_text().splitlines()[-1])
    assert m["hermite_order"] == 6 and m["steps_taken"] == 8
    c5 = ckpt.load(ckpt.latest(str(tmp_path / "ck")))
    assert c5.step == 5 and c5.meta["hermite_order"] == 6
    assert c5.meta["extra"] == ["acc", "jerk", "snap", "crackle"]
    assert all(c5.extra[k].shape == (120, 3) for k in ("acc", "jerk", "snap", "crackle"))
    assert c5.extra["crackle"].any() and c5.extra["snap"].any()
    r = _cli("--steps", "3", "--resume", str(tmp_path / "ck"), "--dump", part)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = ckpt.load(whole), ckpt.load(part)
    assert a.step == b.step == 8 and a.meta["time"] == b.meta["time"]
    assert np.array_equal(a.bodies.pos, b.bodies.pos) and np.array_equal(a.bodies.vel, b.bodies.vel)
    for k in ("acc", "jerk", "snap", "crackle"):
        assert np.array_equal(a.extra[k], b.extra[k])
    assert a.meta["dt_next"] == b.meta["dt_next"]
    # the command line refuses what order 6 leaves out, naming the option (no process needed)
    p = cli.build_parser()
    for extra, word in ((["--block-steps"], "--block-steps"), (["--dtype", "mixed"], "--dtype mixed"),
                        (["--collisions", "detect", "--softening", "1e6"], "--collisions"),
                        (["--gpus", "2"], "--gpus")):
        with pytest.raises(ValueError, match=word):
            cli.config_from_args(p.parse_args(["--integrator", "hermite", "--hermite-order", "6",
                                               "--eta", "0.25", *extra]))


def test_checkpoint_of_the_other_order_restarts_the_derivatives(tmp_path):
    from gravsim.runtime.simulation import Simulation

    base = SimConfig(n=80, dt=4e5, eta=0.02, steps=4, device="cpu", integrator="hermite", seed=2)
    sim = Simulation(base)
    sim.run()
    path = sim.save_checkpoint(str(tmp_path / "o4.gsck"))
    t4 = sim.engine.status().time
    with pytest.warns(UserWarning, match="order"):
        sim6 = Simulation(base.replace(hermite_order=6, eta=0.25, resume=path))
    assert sim6.order_restart and sim6.engine.status().time == t4 and sim6.step == 4
    rows = sim6.engine.carried()
    assert len(rows) == 4 and not rows[3].any()  # (afresh: the crackle starts at 0)
    s = sim6.engine.state()
    ref = acc_jerk_snap(s.pos, s.vel, s.mass, device="oracle")
    assert np.abs(rows[2] - ref[2]).max() <= 1e-9 * np.abs(ref[2]).max()
    sim6.run(2)
    assert sim6.step == 6 and sim6.engine.nonfinite() == 0
