"""k nearest neighbours, local density and cluster structure without a GPU: the native CPU
entry points (gs_cpu_knn_*) and the driver's --structure against the NumPy oracle.

The neighbours of body i are the first k of the ascending lexicographic order on (r^2_ij, j),
j != i by index. The lattice pins the tie and the self-by-index rules exactly; the random cube
pins fp64 against the oracle up to rounding; the far cube shows what dtype mixed is for."""
import json

import numpy as np
import pytest

import gravsim
from gravsim.cli import main
from gravsim.config import G_SI, SimConfig
from gravsim.models.initial_conditions import make, plummer
from gravsim.ops import neighbours, oracle

from knn_helpers import DTYPES, cube, far_cube, lattice, oracle_lattice


@pytest.mark.parametrize("shift", [0.0, 2.0 ** 20])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_ties_exact(dtype, shift):
    """Every r^2 is a small integer in every type, so all three dtypes equal the oracle exactly,
    r^2 and index: most bodies have 6 neighbours at r^2 = 1 (the lower j first), and the two
    bodies of the duplicated site are each other's first neighbour at r^2 = 0."""
    pos = lattice(shift)
    n = len(pos)
    assert n == 4097
    r2o, idxo = oracle_lattice(shift)
    dup = int(np.flatnonzero((pos[: n - 1] == pos[n - 1]).all(1))[0])
    assert idxo[dup, 0] == n - 1 and idxo[n - 1, 0] == dup and r2o[dup, 0] == r2o[n - 1, 0] == 0
    assert (r2o[:, :6] == 1).all(1).sum() > n // 2
    for k in (1, 6, 8):
        r2, idx = neighbours.k_nearest(pos, k, device="cpu", dtype=dtype)
        assert r2.shape == idx.shape == (n, k) and idx.dtype == np.int32
        assert np.array_equal(idx, idxo[:, :k])
        assert np.array_equal(r2, r2o[:, :k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 7])
def test_small_n_pads_with_inf(dtype, n):
    pos = cube(n, seed=n)
    r2, idx = neighbours.k_nearest(pos, 8, device="cpu", dtype=dtype)
    r2o, idxo = oracle.k_nearest(pos, 8)
    assert np.array_equal(idx, idxo)  # (7 bodies in the unit cube: no near tie)
    assert (idx[:, n - 1:] == -1).all() and np.isinf(r2[:, n - 1:]).all()
    assert (idx[:, : n - 1] >= 0).all() and np.isfinite(r2[:, : n - 1]).all()
    assert (np.diff(r2[:, : n - 1], axis=1) >= 0).all()


# fp64 against the oracle: each component of d is one rounding of an exact difference, and the
# three-term sum (fma or not) adds three more, so two evaluations of one r^2 differ relatively
# by at most 8 * 2^-53; the orders can differ only where two of the oracle's consecutive r^2
# are closer than that.
MARGIN = 8 * 2.0 ** -53


def test_random_cube_fp64_matches_oracle():
    pos = cube(1000)
    for k in (1, 6, 8):
        r2o, idxo = oracle.k_nearest(pos, k + 1)  # (one more: the gap behind the list's end)
        gap = np.diff(r2o, axis=1) / r2o[:, 1:]
        close = gap <= MARGIN
        excused = close[:, :k].copy()
        excused[:, 1:] |= close[:, : k - 1]
        # at this seed and n no position of any list is excused, so every index is compared
        assert not excused.any()
        r2, idx = neighbours.k_nearest(pos, k, device="cpu", dtype="fp64")
        assert np.array_equal(idx[~excused], idxo[:, :k][~excused])
        assert (np.abs(r2 - r2o[:, :k]) <= MARGIN * r2o[:, :k]).all()


def test_mixed_resolves_what_fp32_cannot():
    """4e7 m wide at 1.5e11 m: the double-single separation orders the neighbours as fp64 does,
    for every body; fp32 positions (ulp 16384 m) do not."""
    pos = far_cube()
    _, idxo = oracle.k_nearest(pos, 6)
    assert np.array_equal(neighbours.k_nearest(pos, 6, device="cpu", dtype="mixed")[1], idxo)
    assert np.array_equal(neighbours.k_nearest(pos, 6, device="cpu", dtype="fp64")[1], idxo)
    idx32 = neighbours.k_nearest(pos, 6, device="cpu", dtype="fp32")[1]
    assert (idx32 != idxo).any(1).sum() >= 1


def test_local_density_definition():
    """rho_i = (mass of the k - 1 nearest) / (4/3 pi r_k^3), by hand on 5 collinear bodies."""
    pos = np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0], [15, 0, 0]])
    mass = np.array([1.0, 2, 4, 8, 16])
    rho = oracle.local_density(pos, mass, k=3)
    # body 0: neighbours 1, 2, 3 at 1, 3, 7 -> (2 + 4) / (4/3 pi 7^3)
    assert rho[0] == pytest.approx(6.0 / (4 / 3 * np.pi * 343.0), rel=1e-15)
    # body 4: neighbours 3, 2, 1 at 8, 12, 14
    assert rho[4] == pytest.approx(12.0 / (4 / 3 * np.pi * 14.0 ** 3), rel=1e-15)
    dup = np.concatenate([pos, pos[:1], pos[:1]])  # three bodies on one site: r_2 = 0
    s = oracle.cluster_structure(dup, np.ones(7), k=2)
    assert s["degenerate"] == 3 and np.isfinite(s["core_radius"])
    assert oracle.cluster_structure(pos[:2], mass[:2], k=6)["degenerate"] == 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_structure_of_a_plummer_sphere(seed):
    """4,096 bodies: the half-mass radius is 1.305 a in theory (NumPy measured 1.299 to 1.317 at
    these seeds), the density centre sits within 0.1 a of the origin (0.045 to 0.065) and the
    Casertano & Hut core radius is 0.53 to 0.55 a."""
    a = 1.5e11
    b = plummer(4096, seed, scale=a)
    s = oracle.cluster_structure(b.pos, b.mass)
    print(seed, s)
    assert s["degenerate"] == 0
    assert 1.25 <= s["lagrangian_radii"][1] / a <= 1.36
    assert np.linalg.norm(s["density_centre"]) < 0.1 * a
    assert 0.45 < s["core_radius"] / a < 0.65
    assert s["lagrangian_radii"][0] < s["lagrangian_radii"][1] < s["lagrangian_radii"][2]
    assert s["density_max"] > 0


def _close(a, b, rel=1e-12):
    for key in ("core_radius", "density_max"):
        assert abs(a[key] - b[key]) <= rel * abs(b[key]), key
    assert np.allclose(a["lagrangian_radii"], b["lagrangian_radii"], rtol=rel, atol=0)
    xa, xb = np.array(a["density_centre"]), np.array(b["density_centre"])
    assert np.linalg.norm(xa - xb) <= rel * np.linalg.norm(xb)
    assert a["degenerate"] == b["degenerate"]


def test_cli_structure_samples(tmp_path):
    """--structure-every 2 --steps 4: the start, step 2 and the end (step 4) - a periodic sample
    that would fall on the last step is the end sample and is not taken twice: 3 samples."""
    mj = tmp_path / "m.json"
    assert main(["--device", "cpu", "--init", "plummer", "--n", "1024", "--structure",
                 "--structure-every", "2", "--steps", "4", "--metrics-json", str(mj),
                 "--quiet"]) == 0
    m = json.loads(mj.read_text().splitlines()[-1])
    st = m["structure"]
    assert st["k"] == 6
    assert [s["step"] for s in st["samples"]] == [0, 2, 4]
    assert [s["time"] for s in st["samples"]] == [0.0, 7200.0, 14400.0]
    for s in st["samples"]:
        assert set(s) == {"step", "time", "density_centre", "core_radius", "density_max",
                          "lagrangian_radii", "degenerate"}
    cfg = SimConfig()
    b = make("plummer", 1024, cfg.seed, G_SI)
    _close(st["samples"][0], oracle.cluster_structure(b.pos, b.mass))
    # off by default: the key is absent
    assert main(["--device", "cpu", "--n", "64", "--steps", "1", "--metrics-json", str(mj),
                 "--quiet"]) == 0
    assert "structure" not in json.loads(mj.read_text().splitlines()[-1])


def test_structure_works_with_hermite_and_after_mergers():
    """Every integrator; after mergers the samples are of the bodies left."""
    from gravsim.runtime.simulation import Simulation

    sim = Simulation(SimConfig(n=64, device="cpu", integrator="hermite", eta=0.02, dt=3600.0,
                               steps=2, init="plummer", structure=True, structure_k=4,
                               block_steps=True))
    try:
        m = sim.run()
    finally:
        sim.close()
    assert m.structure["k"] == 4 and [s["step"] for s in m.structure["samples"]] == [0, 2]
    assert m.structure["samples"][1]["time"] == 7200.0


def test_refusals():
    pos = cube(16)
    for dev in ("cpu", "oracle"):
        with pytest.raises(ValueError):
            neighbours.k_nearest(pos, 9, device=dev)
        with pytest.raises(ValueError):
            neighbours.k_nearest(pos, 0, device=dev)
    with pytest.raises(ValueError):
        neighbours.k_nearest(pos, 6, device="tpu")
    with pytest.raises(ValueError):
        neighbours.cluster_structure(pos, np.ones(16), k=1)
    for k in (1, 9):
        with pytest.raises(ValueError):
            SimConfig(structure=True, structure_k=k).validate()
    with pytest.raises(ValueError):
        SimConfig(structure_every=-1).validate()
    SimConfig(structure=True, structure_k=2).validate()
    SimConfig(structure=True, structure_k=8).validate()
    # the native entry refuses on its own, with the project's error code and message
    from gravsim.ops import _native

    lib = _native.cpu_lib()
    X = np.zeros((16, 4))
    X[:, :3] = pos
    r2, idx = np.zeros((16, 9)), np.zeros((16, 9), np.int32)
    assert lib.gs_cpu_knn_f64(_native.dptr(X), 16, 0, 16, 9, _native.dptr(r2),
                              idx.ctypes.data_as(_native.PI32)) != 0
    assert b"k in 1..8" in lib.gs_last_error()


def test_exports():
    assert gravsim.k_nearest is neighbours.k_nearest
    assert gravsim.cluster_structure is neighbours.cluster_structure
