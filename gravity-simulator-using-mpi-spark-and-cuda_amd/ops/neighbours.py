"""k nearest neighbours and the cluster-structure read-outs that rest on them.

The k nearest neighbours of body i are the first k entries of the ascending lexicographic order
on (r^2_ij, j) over the real bodies j != i (the body itself left out by index, no softening, no
cutoff; (+inf, -1) past the n - 1 neighbours there are). The order is total, so the lists are a
property of the body set and of the pair type alone: the gfx950 kernel (csrc/hip/nbody_knn.hip,
any launch shape) and the native CPU engine return the same bits, and in fp64 they differ from
the NumPy oracle only where two distances agree to rounding.

cluster_structure: density centre, core radius, central density and Lagrangian radii by
Casertano & Hut (1985), the O(N^2) lists from the chosen device and the O(N) remainder on the
host in fp64 with the oracle's code.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native, oracle

K_MAX = 8
DEVICES = ("cpu", "gpu", "oracle")


def _cpu_k_nearest(pos, n: int, k: int, dtype: str):
    lib = _native.cpu_lib()
    T = np.float32 if dtype == "fp32" else np.float64
    X = np.zeros((n, 4), T)
    X[:, :3] = pos  # (fp32: rounded as the engines round; mixed: split natively)
    r2 = np.empty((n, k), T)
    idx = np.empty((n, k), np.int32)
    fn, ptr = _native.cpu_entry(lib, "knn", dtype)
    _native.check(lib, fn(ptr(X), n, 0, n, k, ptr(r2), idx.ctypes.data_as(_native.PI32)),
                  "cpu k_nearest")
    return r2.astype(np.float64), idx


def _gpu_k_nearest(pos, n: int, k: int, dtype: str, ipl: int, groups: int, device: int):
    lib = _native.hip_lib()
    r2 = np.empty((n, k), np.float64)
    idx = np.empty((n, k), np.int32)
    _native.check(lib, lib.gs_hip_knn(_native.dptr(pos), n, _native.DTYPE_IDS[dtype], k, ipl,
                                      groups, device, _native.dptr(r2),
                                      idx.ctypes.data_as(_native.PI32)), "gpu k_nearest")
    return r2, idx


def k_nearest(pos, k: int = 6, device: str = "cpu", dtype: str = "fp64", ipl: int = 0,
              groups: int = 0, gpu: int = 0):
    """(r2 (n, k) float64 ascending, idx (n, k) int32) of every body.

    device "oracle": NumPy fp64; "cpu": the native C++ engine; "gpu": the gfx950 kernel on HIP
    device `gpu` (raises if the HIP path is unavailable; stateless, safe beside a live engine).
    dtype "fp32", "fp64" or "mixed" (fp64 positions seen as double-single fp32 pairs, fp32 pair
    arithmetic) is the type r^2 is formed in; ipl (0 auto, 1, 2) and groups (0 auto) shape the
    GPU launch and never change a bit of the result."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] < 1:
        raise ValueError("pos must be (n, 3) with n >= 1")
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"k must be in 1..{K_MAX}")
    if device not in DEVICES:
        raise ValueError(f"unknown device {device!r}")
    if dtype not in _native.DTYPE_IDS:
        raise ValueError(f"unknown dtype {dtype!r}")
    n = pos.shape[0]
    if device == "oracle":
        return oracle.k_nearest(pos, k)
    if device == "cpu":
        return _cpu_k_nearest(pos, n, k, dtype)
    return _gpu_k_nearest(pos, n, k, dtype, int(ipl), int(groups), int(gpu))


def gpu_pass_ms(pos, k: int = 6, dtype: str = "fp32", ipl: int = 0, groups: int = 0,
                reps: int = 5, gpu: int = 0):
    """Milliseconds of `reps` k-nearest passes (kernel + merge between two device events, no
    upload or download) and the launch shape: (ms list, {n_pad, ipl, groups, chunk, pair_evals})."""
    lib = _native.hip_lib()
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = pos.shape[0]
    ms = np.zeros(reps)
    info = (ctypes.c_int64 * 4)()
    _native.check(lib, lib.gs_hip_knn_time(_native.dptr(pos), n, _native.DTYPE_IDS[dtype], int(k),
                                           int(ipl), int(groups), int(gpu), int(reps),
                                           _native.dptr(ms), info), "gpu k_nearest timing")
    return list(ms), {"n_pad": info[0], "ipl": info[1], "groups": info[2], "chunk": info[3],
                      "pair_evals": n * info[0]}


def cluster_structure(pos, mass, k: int = 6, device: str = "cpu", dtype: str = "fp64",
                      fractions=(0.1, 0.5, 0.9), **kw):
    """oracle.cluster_structure with the k-nearest lists of the chosen device and dtype."""
    if not 2 <= int(k) <= K_MAX:
        raise ValueError(f"k must be in 2..{K_MAX}")
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    lists = k_nearest(pos, k, device, dtype, **kw)
    return oracle.cluster_structure(pos, mass, k, fractions, lists=lists)
