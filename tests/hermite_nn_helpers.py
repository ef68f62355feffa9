"""Helpers shared by tests/test_hermite_nn_cpu.py and tests/test_hermite_nn_gpu.py: the inputs as a
pair kernel sees them, the three assertions against oracle.nearest_neighbours with the bound
B = 8 u (r^2 + s^2), the planted body sets and a driver run."""
import numpy as np

from gravsim.config import SimConfig
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.runtime.simulation import Simulation

F32, F64 = np.float32, np.float64
U = {"fp32": 2.0 ** -24, "mixed": 2.0 ** -24, "fp64": 2.0 ** -53}
DTYPES = ["fp32", "fp64", "mixed"]
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]
SOFT = 2.0 ** 20  # a softening whose square is exact in fp32


def seen(pos, radius, dtype):
    """Positions and radii as the pair kernel of `dtype` sees them, in fp64."""
    pos, radius = np.asarray(pos, F64), np.asarray(radius, F64)
    if dtype == "fp64":
        return pos, radius
    if dtype == "fp32":
        return pos.astype(F32).astype(F64), radius.astype(F32).astype(F64)
    hi = pos.astype(F32)
    lo = (pos - hi).astype(F32)
    return hi.astype(F64) + lo.astype(F64), radius.astype(F32).astype(F64)


def with_radii(b, seed, scale=1e8):
    """Radii up to a few `scale` metres, a quarter of the bodies with none."""
    rng = np.random.default_rng(seed)
    r = np.abs(rng.normal(size=b.n)) * scale
    r[rng.random(b.n) < 0.25] = 0.0
    return BodySet(b.pos, b.vel, b.mass, r)


def pair_q(pos, radius, i, j, softening=0.0):
    d = pos[j] - pos[i]
    s = radius[i] + radius[j]
    r2 = (d * d).sum(-1) + softening * softening
    return r2 - s * s, r2 + s * s


def check_against_oracle(q, nn, b, dtype, softening=0.0, cutoff=1e-10, rows=None, cap=0.01):
    """The three assertions of the module docstring; returns the excused share (cap: the share
    allowed; a planted exact tie, whose index the caller asserts itself, lifts it)."""
    pos, rad = seen(b.pos, b.radii(), dtype)
    oq, onn, oq2 = oracle.nearest_neighbours(pos, rad, cutoff, softening, rows=rows, second=True)
    idx = np.arange(b.n) if rows is None else np.asarray(rows)
    none = onn < 0
    assert np.array_equal(nn[none], onn[none]) and np.all(np.isinf(q[none]))
    ok = ~none
    assert (nn[ok] >= 0).all() and (nn[ok] < b.n).all() and (nn[ok] != idx[ok]).all()
    qr, scale = pair_q(pos, rad, idx[ok], nn[ok], softening)
    B = 8.0 * U[dtype] * scale
    assert (np.abs(q[ok] - qr) <= B).all(), float((np.abs(q[ok] - qr) / B).max())
    assert (qr - oq[ok] <= 2.0 * B).all()
    _, sbest = pair_q(pos, rad, idx[ok], onn[ok], softening)
    clear = (oq2[ok] - oq[ok]) > 2.0 * 8.0 * U[dtype] * sbest
    assert np.array_equal(nn[ok][clear], onn[ok][clear])
    excused = 1.0 - clear.mean() if ok.any() else 0.0
    assert excused <= cap, excused
    return excused


def lattice(n, seed=3, spacing=2.0 ** 30, radius=2.0 ** 27):
    """n bodies on distinct points of a 13^3 lattice of power-of-two spacing in a shuffled order,
    all of the same power-of-two radius: every r^2 and every q is exact in fp32, and interior
    bodies have up to six equally near neighbours."""
    g = np.arange(13) - 6
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F64)
    pts = pts[np.random.default_rng(seed).permutation(len(pts))[:n]] * spacing
    rng = np.random.default_rng(seed + 1)
    return BodySet(pts, rng.normal(size=(n, 3)) * 1e3, rng.uniform(1e23, 1e25, n),
                   np.full(n, radius))


def head_on(centre, mass=1e24):
    """Two bodies of `mass` kg and radius 2.05e7 m, 2e8 m apart, closing at 2 km/s: they touch
    (separation 4.1e7 m) after 7.95e4 s less what their pull gains them (1e24 kg: step 71 of
    1000 s); a step changes the separation by 2e6 m or more, q by 1.6e14 or more, and the tests
    assert that the oracle's deciding q is far from 0."""
    c = np.asarray(centre, dtype=float)
    pos = np.array([c - [1e8, 0, 0], c + [1e8, 0, 0]])
    vel = np.array([[1e3, 0, 0], [-1e3, 0, 0]], dtype=float)
    return BodySet(pos, vel, np.array([mass, mass]), np.array([2.05e7, 2.05e7]))


def chain_and_bystander():
    """A touches B and B touches C (A and C do not): one body. A fourth body far away."""
    pos = np.array([[0, 0, 0], [3e7, 0, 0], [6e7, 0, 0], [5e10, 1e10, 0]], dtype=float)
    vel = np.array([[0, 10, 0], [0, -20, 5], [3, 0, 0], [0, 1e3, 0]], dtype=float)
    return BodySet(pos, vel, np.array([1e24, 2e24, 3e24, 1e23]), np.array([2e7, 2e7, 2e7, 1e6]))


def run_driver(b, device="cpu", dtype="fp64", resume=None, run_steps=None, **kw):
    kw.setdefault("dt", 1000.0)
    sim = Simulation(SimConfig(n=b.n, dtype=dtype, device=device, integrator="hermite",
                               resume=resume, **kw))
    try:
        if resume is None:
            sim.engine.load(b)
        m = sim.run(run_steps)
        return sim.global_state(), sim.ids.copy(), m, sim.step
    finally:
        sim.close()




def merger_with_bystander(mass=1e24):
    """head_on() at 1 AU plus a third, light body far away: bodies 0 and 1 merge, ids [0, 2]."""
    h = head_on((1.5e11, 0.7e11, -0.3e11), mass)
    return BodySet(np.vstack([h.pos, [[2e11, 0, 0]]]), np.vstack([h.vel, [[0, 2e4, 0]]]),
                   np.append(h.mass, 1e22), np.append(h.radius, 1e6))
