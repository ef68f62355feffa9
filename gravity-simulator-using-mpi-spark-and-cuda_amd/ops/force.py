"""Stateless force entry points (one-shot accelerations of a body set).

The reference computes forces three ways: a racy upper-triangle CUDA kernel with Newton-3
scatter (cuda.cu:32-60), a full-row C loop (mpi.c:196-205), and a Spark pair map with a
driver-side reduction (pyspark.py:59-86). All three are replaced by i-owned full-row sums.
"""
from __future__ import annotations

import numpy as np

from ..config import G_SI, SimConfig
from ..models.initial_conditions import BodySet
from ..parallel.partition import layout
from . import _native, oracle


def cpu_accelerations(pos, mass, dtype: str = "fp64", G: float = G_SI, cutoff: float = 1e-10,
                      softening: float = 0.0, chunk: int = 0):
    """Native C++ engine: returns (acc (n,3), phi (n,)) as float64 arrays."""
    lib = _native.cpu_lib()
    n = int(np.asarray(mass).shape[0])
    L = layout(n, 0, 1, chunk)
    T = np.float64 if dtype == "fp64" else np.float32
    X = np.zeros((L.n_pad, 4), T)
    X[:n, :3] = pos
    X[:n, 3] = G * np.asarray(mass, dtype=np.float64)
    out = np.zeros((n, 4), T)
    fn, ptr = _native.cpu_entry(lib, "accel", dtype)
    _native.check(lib, fn(ptr(X), n, 0, n, L.chunk, T(cutoff * cutoff), T(softening ** 2),
                          ptr(out)), "cpu accel")
    out = out.astype(np.float64)
    return out[:, :3], out[:, 3]


def hip_accelerations(pos, mass, dtype: str = "fp32", G: float = G_SI, cutoff: float = 1e-10,
                      softening: float = 0.0, kernel: str = "auto", ipl: int = 0,
                      chunk: int = 0, mode: str = "auto"):
    """gfx950 kernels: returns (acc (n,3), phi (n,)). Raises if the HIP path is unavailable."""
    from ..runtime.engines import HipEngine

    n = int(np.asarray(mass).shape[0])
    cfg = SimConfig(n=n, dtype=dtype, G=G, cutoff=cutoff, softening=softening, kernel=kernel,
                    ipl=ipl, chunk=chunk, mode=mode, device="gpu")
    eng = HipEngine(cfg)
    try:
        eng.load(BodySet(np.asarray(pos, np.float64), np.zeros((n, 3)),
                         np.asarray(mass, np.float64)))
        a = eng.accel()[:n]
    finally:
        eng.close()
    return a[:, :3], a[:, 3]


def accelerations(pos, mass, device: str = "cpu", **kw):
    """Dispatch: device in {"oracle", "cpu", "gpu"}."""
    if device == "oracle":
        kw.pop("dtype", None)
        return oracle.accelerations(pos, mass, with_potential=True, **kw)
    if device == "cpu":
        return cpu_accelerations(pos, mass, **kw)
    if device == "gpu":
        return hip_accelerations(pos, mass, **kw)
    raise ValueError(f"unknown device {device!r}")


def acc_jerk(pos, vel, mass, device: str = "cpu", dtype: str = "fp64", G: float = G_SI,
             cutoff: float = 1e-10, softening: float = 0.0, chunk: int = 0, ipl: int = 0,
             split_groups: int = 0):
    """One-shot Hermite derivatives: (acc (n,3), jerk (n,3), phi (n,)) as float64 arrays.

    device "oracle": NumPy fp64; "cpu": the native C++ engine; "gpu": the gfx950
    acceleration+jerk kernel (raises if the HIP path is unavailable). dtype "fp32", "fp64" or
    "mixed" (fp64 inputs seen as double-single fp32 positions, fp32 pair arithmetic)."""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    mass = np.asarray(mass, np.float64)
    n = int(mass.shape[0])
    if device == "oracle":
        return oracle.acc_jerk(pos, vel, mass, G, cutoff, softening, with_potential=True)
    if device not in ("cpu", "gpu"):
        raise ValueError(f"unknown device {device!r}")
    from ..runtime.hermite import HermiteCpuEngine, HermiteHipEngine

    cfg = SimConfig(n=n, dtype=dtype, G=G, cutoff=cutoff, softening=softening, chunk=chunk,
                    ipl=ipl, split_groups=split_groups, device=device,
                    integrator="hermite").validate()
    eng = HermiteCpuEngine(cfg) if device == "cpu" else HermiteHipEngine(cfg)
    try:
        eng.load(BodySet(pos, vel, mass))
        a4, j4 = eng.derivs()
    finally:
        eng.close()
    return a4[:, :3], j4[:, :3], a4[:, 3]


def acc_jerk_snap(pos, vel, mass, device: str = "cpu", dtype: str = "fp64", G: float = G_SI,
                  cutoff: float = 1e-10, softening: float = 0.0, chunk: int = 0, ipl: int = 0,
                  split_groups: int = 0):
    """One-shot 6th-order Hermite derivatives of a state: (acc, jerk, snap (n,3), phi (n,)) as
    float64 arrays, the snap at the acceleration of the state itself (two passes: a, then s).

    device "oracle": NumPy fp64; "cpu": the native C++ engine; "gpu": the gfx950
    acceleration+jerk+snap kernel (raises if the HIP path is unavailable). dtype "fp32" or
    "fp64"."""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    mass = np.asarray(mass, np.float64)
    n = int(mass.shape[0])
    if device == "oracle":
        a = oracle.acc_jerk_snap(pos, vel, np.zeros_like(pos), mass, G, cutoff, softening)[0]
        return oracle.acc_jerk_snap(pos, vel, a, mass, G, cutoff, softening, with_potential=True)
    if device not in ("cpu", "gpu"):
        raise ValueError(f"unknown device {device!r}")
    from ..runtime.hermite import HermiteCpuEngine, HermiteHipEngine

    cfg = SimConfig(n=n, dtype=dtype, G=G, cutoff=cutoff, softening=softening, chunk=chunk,
                    ipl=ipl, split_groups=split_groups, device=device, integrator="hermite",
                    hermite_order=6).validate()
    eng = HermiteCpuEngine(cfg) if device == "cpu" else HermiteHipEngine(cfg)
    try:
        eng.load(BodySet(pos, vel, mass))
        a4, j4, s4 = eng.derivs()
    finally:
        eng.close()
    return a4[:, :3], j4[:, :3], s4[:, :3], a4[:, 3]
