"""Step rate of the Hermite integrator against the one-sided kick-drift step, on one GPU.

For every (N, dtype) of the grid: ms/step and pair evaluations/s (N^2 per step, both are
one-sided sums) of
  * `--integrator hermite` (fixed step: control, predict, acceleration+jerk, reduce + correct);
  * the KD step of the one-sided schedule mode=auto picks when the Newton-3 schedule is left
    out (fused from 2048 i-blocks up, else split; csrc/common/layout.cpp), same N, dtype and box;
and their ratio. The windows alternate (hermite, kd, hermite, kd, ...) and the median window
counts; each window ends in a device synchronise. Prints one JSON line.

    python bench/hermite_rate.py [--sizes 65536,262144] [--dtypes fp32,fp64] [--repeat 3]

--drift also runs 65,536 solar+random bodies for 24 simulated hours under kd, leapfrog (dt 3600)
and hermite --eta 0.02 and reports each run's relative energy drift.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _window(eng, steps: int) -> float:
    t0 = time.perf_counter()
    eng.step(steps)
    eng.sync()
    return (time.perf_counter() - t0) / steps


def _kd_mode(n: int, dtype: str) -> str:
    """The one-sided schedule of mode=auto (sym left out): fused needs >= 2048 i-blocks."""
    from gravsim.parallel.partition import layout

    L = layout(n)
    ipl = (8 if L.n_local >= 262144 else 4) if dtype == "fp32" else 2
    while ipl > 1 and L.n_local % (256 * ipl):
        ipl //= 2
    return "fused" if L.n_local // (256 * ipl) >= 2048 else "split"


def rate(n: int, dtype: str, seed: int, repeat: int, min_s: float) -> dict:
    from gravsim.config import SimConfig
    from gravsim.runtime.engines import HipEngine
    from gravsim.runtime.hermite import HermiteHipEngine

    mode = _kd_mode(n, dtype)
    herm = HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite"))
    kd = HipEngine(SimConfig(n=n, dtype=dtype, device="gpu", mode=mode))
    try:
        engines = {"hermite": herm, "kd": kd}
        steps = {}
        for name, eng in engines.items():
            eng.init_ics("solar+random", seed)
            eng.sync()
            _window(eng, 2)  # warm-up: code objects, the KD step graph
            per = _window(eng, 4)
            steps[name] = max(4, 2 * int(min_s / per / 2 + 1))  # (even: whole graph periods)
        times = {name: [] for name in engines}
        for _ in range(repeat):
            for name, eng in engines.items():
                times[name].append(_window(eng, steps[name]))
        out = {"n": n, "dtype": dtype, "kd_mode": mode,
               "nonfinite": sum(eng.nonfinite() for eng in engines.values()),
               "hermite_ipl": herm.native_layout["ipl"],
               "hermite_groups": herm.native_layout["split_groups"],
               "kd_ipl": kd.native_layout["ipl"], "kd_kernel": kd.native_layout["kernel"]}
        for name in engines:
            t = statistics.median(times[name])
            out[f"{name}_ms_per_step"] = 1e3 * t
            out[f"{name}_ms_windows"] = [round(1e3 * x, 4) for x in times[name]]
            out[f"{name}_steps_per_window"] = steps[name]
            out[f"{name}_pair_evals_per_s"] = float(n) * n / t
        out["hermite_over_kd"] = out["hermite_ms_per_step"] / out["kd_ms_per_step"]
        return out
    finally:
        herm.close()
        kd.close()


def drift(n: int, hours: float, seed: int) -> list:
    from gravsim.config import SimConfig
    from gravsim.runtime.simulation import Simulation

    t_end = hours * 3600.0
    out = []
    for name, kw in (("kd", dict(integrator="kd", steps=int(hours))),
                     ("leapfrog", dict(integrator="leapfrog", steps=int(hours))),
                     ("hermite eta 0.02", dict(integrator="hermite", eta=0.02, t_end=t_end,
                                               steps=20000))):
        sim = Simulation(SimConfig(n=n, dtype="fp32", device="gpu", dt=3600.0, seed=seed,
                                   diagnostics=True, **kw))
        try:
            m = sim.run()
        finally:
            sim.close()
        out.append({"integrator": name, "steps": m.steps, "wall_s": m.wall_s,
                    "time_reached": m.time_reached if m.time_reached is not None else t_end,
                    "dt_min": m.dt_min,
                    "energy_rel_drift": m.extra["conservation"]["energy_rel_drift"]})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--dtypes", default="fp32,fp64")
    ap.add_argument("--repeat", type=int, default=3, help="alternating windows per engine")
    ap.add_argument("--min-window-s", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=20250307)
    ap.add_argument("--drift", action="store_true",
                    help="also the 24-hour energy drift of kd, leapfrog and hermite at 65,536")
    ap.add_argument("--drift-n", type=int, default=65536)
    a = ap.parse_args()
    import torch

    import gravsim  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("hermite_rate: needs a HIP device")
    res = {"bench": "hermite_rate", "device": torch.cuda.get_device_name(0),
           "engine_clock_ghz": None,  # (the Hermite kernel does not record the engine clock)
           "rates": [rate(int(n), d, a.seed, a.repeat, a.min_window_s)
                     for n in a.sizes.split(",") for d in a.dtypes.split(",")]}
    if a.drift:
        res["drift_24h"] = drift(a.drift_n, 24.0, a.seed)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
