"""Shared pieces of the 6th-order Hermite tests (tests/test_hermite6_cpu.py, _gpu.py): the
two-body orbits, the engines' step-by-step record, the oracle run both are judged against, and
the 6x6 polynomial solve the higher derivatives are checked with."""
import functools
import math

import numpy as np

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle


def two_body(e, m_total=2e30, sma=1.5e11):
    """Two equal masses at the pericentre of a Kepler orbit of eccentricity e in SI
    units, centre of mass at rest at the origin: (BodySet, period)."""
    mu = G_SI * m_total
    r = sma * (1.0 - e)
    v = math.sqrt(mu * (1.0 + e) / (sma * (1.0 - e)))
    pos = np.array([[r / 2, 0, 0], [-r / 2, 0, 0]], dtype=float)
    vel = np.array([[0, v / 2, 0], [0, -v / 2, 0]], dtype=float)
    period = 2.0 * math.pi * math.sqrt(sma ** 3 / mu)
    return BodySet(pos, vel, np.array([m_total / 2, m_total / 2])), period


def energy(b):
    ke = 0.5 * (b.mass * (b.vel ** 2).sum(1)).sum()
    d = np.linalg.norm(b.pos[0] - b.pos[1])
    return ke - G_SI * b.mass[0] * b.mass[1] / d


def orders(run):
    """The two observed position-error orders 200 -> 400 -> 800 fixed steps over one period of the
    e = 0.5 orbit; run(b, dt, steps) returns the final positions."""
    b, period = two_body(0.5)
    err = [float(np.abs(run(b, period / k, k) - b.pos).max()) for k in (200, 400, 800)]
    return math.log2(err[0] / err[1]), math.log2(err[1] / err[2]), err


def engine_positions(engine_cls, device, dtype="fp64"):
    """run() of orders() on an engine: `steps` fixed steps of dt."""
    def run(b, dt, steps):
        cfg = SimConfig(n=2, dt=dt, dtype=dtype, device=device, integrator="hermite",
                        hermite_order=6).validate()
        eng = engine_cls(cfg)
        try:
            eng.load(b)
            eng.step(steps)
            return eng.state().pos
        finally:
            eng.close()
    return run


# The adaptive case both engines are run on: 300 solar+random bodies, eta 0.25 under a ceiling
# of 4e5 s, 40 steps asked for and a t_end that cuts step 38 short.
CASE_N, CASE_ETA, CASE_DT, CASE_STEPS = 300, 0.25, 4e5, 40


@functools.lru_cache(maxsize=None)
def adaptive_case():
    """(bodies, t_end, oracle positions, oracle velocities, oracle step list)."""
    b = ic.solar_random(CASE_N, 5)
    free = oracle.simulate_hermite6(b.pos, b.vel, b.mass, CASE_DT, CASE_STEPS, eta=CASE_ETA)[4]
    t_end = float(sum(free[:37]) + 0.4 * free[37])
    x, v, _, t, taken = oracle.simulate_hermite6(b.pos, b.vel, b.mass, CASE_DT, CASE_STEPS,
                                                 eta=CASE_ETA, t_end=t_end)
    assert t == t_end and len(taken) == 38
    for y in (x, v):
        y.setflags(write=False)
    return b, t_end, x, v, tuple(taken)


def run_stepwise(eng, b, steps):
    """Load b, take `steps` single steps; (list of step sizes taken, final status)."""
    eng.load(b)
    taken = []
    for _ in range(steps):
        before = eng.status().steps
        eng.step(1)
        st = eng.status()
        if st.steps > before:
            taken.append(st.dt_last)
    return taken, eng.status()


def check_against_oracle(eng, rtol_x=1e-10, rtol_h=1e-9):
    """The adaptive case on `eng` against simulate_hermite6: the gates of both engines."""
    b, t_end, x, v, ref = adaptive_case()
    taken, st = run_stepwise(eng, b, CASE_STEPS)
    assert len(taken) == len(ref) == 38
    worst_h = max(abs(g - r) / r for g, r in zip(taken, ref))
    s = eng.state()
    worst_x = float(np.abs(s.pos - x).max() / np.abs(x).max())
    print(f"step sizes within {worst_h:.2e} relative, positions within {worst_x:.2e} of max |x|")
    assert worst_h <= rtol_h
    assert worst_x <= rtol_x
    assert st.time == t_end and st.finished and st.steps == 38
    # later steps are no-ops
    eng.step(3)
    st2, s2 = eng.status(), eng.state()
    assert st2.steps == 38 and st2.time == t_end
    assert np.array_equal(s2.pos, s.pos) and np.array_equal(s2.vel, s.vel)


def poly_high(a0, j0, s0, a1, j1, s1, h):
    """3rd, 4th and 5th derivatives at t = h of the quintic through (a0, j0, s0) at 0 and
    (a1, j1, s1) at h, from a 6x6 solve per component in the scaled variable u = t / h."""
    M = np.zeros((6, 6))
    for k in range(6):
        M[0, k] = 0.0 ** k if k else 1.0
        M[3, k] = 1.0
        M[1, k] = 1.0 if k == 1 else 0.0
        M[4, k] = k
        M[2, k] = 2.0 if k == 2 else 0.0
        M[5, k] = k * (k - 1)
    out = []
    rhs = np.stack([a0, j0 * h, s0 * h * h, a1, j1 * h, s1 * h * h])     # (6, n, 3)
    coef = np.linalg.solve(M, rhs.reshape(6, -1)).reshape(rhs.shape)     # a(u) = sum c_k u^k
    for order in (3, 4, 5):
        d = np.zeros_like(a0)
        for k in range(order, 6):
            d = d + coef[k] * math.factorial(k) / math.factorial(k - order)
        out.append(d / h ** order)
    return out
