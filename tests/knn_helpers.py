"""Body sets of the k-nearest-neighbour tests (tests/test_knn_cpu.py, test_knn_gpu.py), all from
fixed seeds, and the fp64 oracle lists of the larger ones, computed once per process."""
import functools

import numpy as np

from gravsim.ops import oracle

DTYPES = ("fp32", "fp64", "mixed")
SHIFT = np.array([1.5e11, 0.7e11, -0.3e11])  # where one fp32 ulp of x is 16384 m


def lattice(shift: float = 0.0) -> np.ndarray:
    """4,097 bodies on the 16^3 integer lattice (spacing 1) in a shuffled order, one site used
    twice with the duplicate at the highest index; every coordinate shifted by `shift` (2^20 is
    still exact in fp32). Every r^2 is a small integer, exact in any type with or without fma."""
    g = np.arange(16, dtype=np.float64)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sites = sites[np.random.default_rng(16).permutation(len(sites))]
    return np.concatenate([sites, sites[5:6]]) + shift


def cube(n: int, seed: int = 7) -> np.ndarray:
    return np.random.default_rng(seed).random((n, 3))


def far_cube(n: int = 1000, seed: int = 3) -> np.ndarray:
    """A cube 4e7 m wide at 1.5e11 m from the origin: fp32 positions there move by up to 8 km."""
    return SHIFT + 4e7 * (np.random.default_rng(seed).random((n, 3)) - 0.5)


def _directions(n: int) -> np.ndarray:
    u = np.random.default_rng(11).normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def approaching(n: int = 4097) -> np.ndarray:
    """Body 0 at the origin, body j at distance n - j: body 0 inserts at the front of its list at
    every j of an ascending sweep."""
    d = (n - np.arange(n, dtype=np.float64))[:, None] * _directions(n)
    d[0] = 0.0
    return d


def receding(n: int = 4097) -> np.ndarray:
    """Body j at distance j from body 0: body 0 inserts only in the first 8 steps."""
    return np.arange(n, dtype=np.float64)[:, None] * _directions(n)


def late_pair(n: int = 4097) -> np.ndarray:
    """receding(), but the two highest indices are one close pair: a single lane of the last wave
    inserts at the very end of its sweep."""
    p = receding(n)
    p[n - 1] = p[n - 2] + np.array([1e-3, 0.0, 0.0])
    return p


@functools.lru_cache(maxsize=None)
def oracle_lattice(shift: float):
    """oracle.k_nearest(lattice(shift), 8): the first k columns are the lists of any k <= 8."""
    r2, idx = oracle.k_nearest(lattice(shift), 8)
    r2.setflags(write=False)
    idx.setflags(write=False)
    return r2, idx
