"""The gfx950 k-nearest-neighbour kernel (csrc/hip/nbody_knn.hip) against the native CPU engine,
bit for bit: the order on (r^2, j) is total and both form r^2 with the same operations, so the
lists are equal in every bit at every size, dtype and launch shape. What the CPU lists are
worth against the oracle is tests/test_knn_cpu.py's business."""
import importlib.util
import json
import os

import numpy as np
import pytest

from gravsim.cli import main
from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.ops import _native, neighbours, oracle
from gravsim.runtime.hermite import HermiteHipEngine

from knn_helpers import DTYPES, approaching, cube, late_pair, lattice, receding

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one tile (256 fp32 / 128 fp64 bodies), the tile edge, ghost rows, a partial last chunk
SIZES = [1, 2, 7, 255, 257, 1000, 4097]


def _same(pos, dtype, k=8, **kw):
    r2c, idxc = neighbours.k_nearest(pos, k, device="cpu", dtype=dtype)
    r2g, idxg = neighbours.k_nearest(pos, k, device="gpu", dtype=dtype, **kw)
    assert idxg.dtype == np.int32 and r2g.shape == idxg.shape == (len(pos), k)
    assert np.array_equal(idxg, idxc), (dtype, kw, np.argwhere(idxg != idxc)[:4])
    assert np.array_equal(r2g, r2c)  # (+inf == +inf; no nan in a list)
    return r2g, idxg


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_equals_cpu_random_cube(hip, dtype, n):
    r2, idx = _same(cube(n, seed=n), dtype)
    m = min(8, n - 1)
    assert (idx[:, m:] == -1).all() and np.isinf(r2[:, m:]).all()
    assert (idx[:, :m] >= 0).all() and (idx[:, :m] < n).all()
    assert (idx[:, :m] != np.arange(n)[:, None]).all()
    for k in (1, 6):  # (the first k of the 8)
        r2k, idxk = neighbours.k_nearest(cube(n, seed=n), k, device="gpu", dtype=dtype)
        assert np.array_equal(idxk, idx[:, :k]) and np.array_equal(r2k, r2[:, :k])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_equals_cpu_lattice(hip, dtype, n):
    """The first n bodies of the shuffled lattice with the duplicate of a site moved to the end
    of the slice: ties on r^2 at nearly every body, a neighbour at r^2 = 0."""
    pos = lattice()[:n].copy()
    if n > 7:
        pos[n - 1] = pos[5]
    r2, idx = _same(pos, dtype)
    if n > 7:
        assert idx[5, 0] == n - 1 and idx[n - 1, 0] == 5 and r2[5, 0] == 0


def test_full_lattice_equals_oracle(hip):
    from knn_helpers import oracle_lattice

    r2o, idxo = oracle_lattice(0.0)
    for dtype in DTYPES:
        r2, idx = neighbours.k_nearest(lattice(), 8, device="gpu", dtype=dtype)
        assert np.array_equal(idx, idxo) and np.array_equal(r2, r2o)


@pytest.mark.parametrize("dtype", DTYPES)
def test_launch_shape_independence(hip, dtype):
    """n = 20,000 (10 chunks of 2,048; 20 groups resolve to one chunk each): every compiled ipl x
    groups gives the bits of the CPU, hence of one another."""
    pos = cube(20000, seed=5)
    ipls = [i for i in (1, 2) if hip.gs_knn_ipl_ok(_native.DTYPE_IDS[dtype], i)]
    assert 1 in ipls and (dtype == "fp64" or 2 in ipls)
    r2c, idxc = neighbours.k_nearest(pos, 8, device="cpu", dtype=dtype)
    for ipl in ipls:
        for groups in (1, 3, 7, 20):
            r2, idx = neighbours.k_nearest(pos, 8, device="gpu", dtype=dtype, ipl=ipl,
                                           groups=groups)
            assert np.array_equal(idx, idxc) and np.array_equal(r2, r2c), (ipl, groups)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("make", [approaching, receding, late_pair])
def test_early_out_path(hip, dtype, make):
    """Body 0 inserting at every j (the test never lets the chain rest), only in its first 8
    steps, and one lane of the last wave inserting at the very end; groups 1 keeps each list one
    sweep, the auto shape merges."""
    pos = make(4097)
    for ipl in (1, 2):
        _, idx = _same(pos, dtype, ipl=ipl, groups=1)
    _, idx = _same(pos, dtype)
    if make is approaching:
        assert list(idx[0]) == [4096 - s for s in range(8)]
    if make is receding:
        assert list(idx[0]) == [1 + s for s in range(8)]
    if make is late_pair:
        assert idx[4095, 0] == 4096 and idx[4096, 0] == 4095


def test_refusals(hip):
    pos = cube(16)
    with pytest.raises(ValueError):
        neighbours.k_nearest(pos, 9, device="gpu")
    r2, idx = np.zeros((16, 9)), np.zeros((16, 9), np.int32)
    pi = idx.ctypes.data_as(_native.PI32)
    assert hip.gs_hip_knn(_native.dptr(pos), 16, 1, 9, 0, 0, 0, _native.dptr(r2), pi) != 0
    assert hip.gs_hip_knn(_native.dptr(pos), 0, 1, 6, 0, 0, 0, _native.dptr(r2), pi) != 0
    assert hip.gs_hip_knn(_native.dptr(pos), 16, 1, 6, 4, 0, 0, _native.dptr(r2), pi) != 0
    assert b"k in 1..8" in hip.gs_last_error()


def test_beside_a_live_engine(hip):
    """k_nearest on the state of a running HermiteHipEngine between its steps: the run ends in
    the bits of the same run without the calls."""
    b = ic.solar_random(4097, seed=9)
    finals = []
    for calls in (False, True):
        eng = HermiteHipEngine(SimConfig(n=b.n, dtype="fp64", device="gpu", integrator="hermite",
                                         eta=0.02).validate())
        try:
            eng.load(b)
            for _ in range(3):
                eng.step(1)
                if calls:
                    st = eng.state()
                    _same(st.pos, "fp64", k=6)
                    _same(st.pos, "mixed", k=6)
            st = eng.state()
            finals.append((st.pos.copy(), st.vel.copy(), eng.status().time))
        finally:
            eng.close()
    assert np.array_equal(finals[0][0], finals[1][0])
    assert np.array_equal(finals[0][1], finals[1][1])
    assert finals[0][2] == finals[1][2]


def _close(a, b, rel=1e-12):
    for key in ("core_radius", "density_max"):
        assert abs(a[key] - b[key]) <= rel * abs(b[key]), key
    assert np.allclose(a["lagrangian_radii"], b["lagrangian_radii"], rtol=rel, atol=0)
    xa, xb = np.array(a["density_centre"]), np.array(b["density_centre"])
    assert np.linalg.norm(xa - xb) <= rel * np.linalg.norm(xb)
    assert a["degenerate"] == b["degenerate"]


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_driver_structure_on_the_gpu(hip, tmp_path, dtype):
    mj = tmp_path / "m.json"
    assert main(["--device", "gpu", "--integrator", "hermite", "--init", "plummer", "--n", "4096",
                 "--structure", "--steps", "2", "--dtype", dtype, "--metrics-json", str(mj),
                 "--quiet"]) == 0
    st = json.loads(mj.read_text().splitlines()[-1])["structure"]
    assert [s["step"] for s in st["samples"]] == [0, 2]  # the start and the end
    b = ic.make("plummer", 4096, SimConfig().seed, G_SI)
    ref = oracle.cluster_structure(b.pos, b.mass)
    if dtype == "fp64":
        _close(st["samples"][0], ref)
    else:
        # the double-single lists order the neighbours as fp64 does; the sample is the oracle's
        # code on exactly those lists
        lists = neighbours.k_nearest(b.pos, 6, device="gpu", dtype="mixed")
        assert np.array_equal(lists[1], oracle.k_nearest(b.pos, 6)[1])
        mine = oracle.cluster_structure(b.pos, b.mass, lists=lists)
        assert {k: v for k, v in st["samples"][0].items() if k not in ("step", "time")} == mine
        _close(st["samples"][0], ref, rel=1e-5)  # (r_k in fp32: 2^-24 relative, cubed)


def test_bench_counts(hip):
    """bench/knn_rate.py reports the pair evaluations of a pass, n x n_pad; no times asserted."""
    spec = importlib.util.spec_from_file_location("knn_rate",
                                                  os.path.join(ROOT, "bench", "knn_rate.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    row = kr.knn_pass(cube(4097, seed=1), "fp32", reps=2)
    assert row["n"] == 4097 and row["n_pad"] == 6144 and row["pair_evals"] == 4097 * 6144
    assert len(row["ms_runs"]) == 2 and row["k"] == 6
    assert row["early_out"] == hip.gs_knn_early_out()
