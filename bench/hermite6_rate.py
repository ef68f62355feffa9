"""Step rate and accuracy-per-cost of the 6th-order Hermite scheme against the 4th-order one, on
one GPU.

For every (N, dtype) of the grid: ms/step of `--hermite-order 6` (control, predict to x, v, a,
acceleration+jerk+snap, reduce + correct) and of order 4 at a fixed step, same N, dtype, bodies
and box, and their ratio. The windows alternate (order 4, order 6, order 4, ...), each ends in a
device synchronise, and the median window counts. Prints one JSON line.

    python bench/hermite6_rate.py [--sizes 65536,262144] [--dtypes fp32,fp64] [--repeat 3]

--drift also runs 65,536 solar+random bodies for 24 simulated hours under order 4 at eta 0.02
and order 6 at eta 0.25 (each criterion's own convention) in every --drift-dtypes: steps, wall
time, smallest step and relative energy drift.
--against PATH times the order-4 step of this checkout and of another built checkout of the
project at PATH (bench/hermite_rate.py of each, --sizes 65536 --dtypes fp32) in alternating child
processes, one at a time: each run's median, and whether the two medians differ by more than the
other checkout's own runs do from each other.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(eng, steps: int) -> float:
    t0 = time.perf_counter()
    eng.step(steps)
    eng.sync()
    return (time.perf_counter() - t0) / steps


def rate(n: int, dtype: str, seed: int, repeat: int, min_s: float) -> dict:
    """The fixed step of both orders at one size and dtype, windows alternating."""
    from gravsim.config import SimConfig
    from gravsim.models.initial_conditions import make
    from gravsim.runtime.hermite import HermiteHipEngine

    engines = {o: HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite",
                                             hermite_order=o)) for o in (4, 6)}
    try:
        b = make("solar+random", n, seed)
        steps = {}
        for o, eng in engines.items():
            eng.load(b)  # (the same bodies through the same path)
            eng.sync()
            _window(eng, 2)  # warm-up: code objects
            steps[o] = max(4, int(min_s / _window(eng, 4) + 1))
        times = {o: [] for o in engines}
        for _ in range(repeat):
            for o, eng in engines.items():
                times[o].append(_window(eng, steps[o]))
        out = {"n": n, "dtype": dtype,
               "nonfinite": sum(eng.nonfinite() for eng in engines.values())}
        for o, eng in engines.items():
            t = statistics.median(times[o])
            out[f"order{o}"] = {"ms_per_step": 1e3 * t,
                                "ms_windows": [round(1e3 * x, 4) for x in times[o]],
                                "spread": (max(times[o]) - min(times[o])) / t,
                                "steps_per_window": steps[o], "ipl": eng.native_layout["ipl"],
                                "groups": eng.native_layout["split_groups"],
                                "pair_evals_per_s": float(n) * n / t}
        out["order6_over_order4"] = out["order6"]["ms_per_step"] / out["order4"]["ms_per_step"]
        return out
    finally:
        for eng in engines.values():
            eng.close()


def drift(n: int, hours: float, seed: int, dtype: str) -> list:
    from gravsim.config import SimConfig
    from gravsim.runtime.simulation import Simulation

    out = []
    for order, eta in ((4, 0.02), (6, 0.25)):
        sim = Simulation(SimConfig(n=n, dtype=dtype, device="gpu", dt=3600.0, seed=seed,
                                   integrator="hermite", hermite_order=order, eta=eta,
                                   t_end=hours * 3600.0, steps=20000, diagnostics=True))
        try:
            m = sim.run()
        finally:
            sim.close()
        out.append({"order": order, "eta": eta, "dtype": dtype, "steps": m.steps,
                    "wall_s": m.wall_s, "time_reached": m.time_reached, "dt_min": m.dt_min,
                    "energy_rel_drift": m.extra["conservation"]["energy_rel_drift"]})
    return out


def against(other: str, rounds: int, seed: int) -> dict:
    """Order-4 step of this checkout and of the checkout at `other`, alternating processes."""
    def one(tree: str) -> dict:
        env = {k: v for k, v in os.environ.items() if k != "GRAVSIM_NATIVE_DIR"}
        r = subprocess.run([sys.executable, os.path.join(tree, "bench", "hermite_rate.py"),
                            "--sizes", "65536", "--dtypes", "fp32", "--repeat", "3", "--seed",
                            str(seed)], capture_output=True, text=True, cwd=tree, env=env)
        if r.returncode != 0:
            raise RuntimeError(f"hermite_rate.py of {tree} failed:\n{r.stderr[-2000:]}")
        row = json.loads(r.stdout.strip().splitlines()[-1])["rates"][0]
        return {"ms_per_step": row["hermite_ms_per_step"], "ms_windows": row["hermite_ms_windows"]}

    runs = {"this": [], "other": []}
    for _ in range(rounds):
        runs["other"].append(one(os.path.abspath(other)))
        runs["this"].append(one(ROOT))
    med = {k: statistics.median(r["ms_per_step"] for r in v) for k, v in runs.items()}
    own = [r["ms_per_step"] for r in runs["other"]]
    return {"n": 65536, "dtype": "fp32", "rounds": rounds, "runs": runs,
            "this_ms_per_step": med["this"], "other_ms_per_step": med["other"],
            "difference_ms": abs(med["this"] - med["other"]),
            "other_own_spread_ms": max(own) - min(own),
            "within_other_own_spread": abs(med["this"] - med["other"]) <= max(own) - min(own)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--dtypes", default="fp32,fp64")
    ap.add_argument("--repeat", type=int, default=3, help="alternating windows per engine")
    ap.add_argument("--min-window-s", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=20250307)
    ap.add_argument("--no-rates", action="store_true", help="skip the step rates")
    ap.add_argument("--drift", action="store_true", help="also the 24-hour energy-drift runs")
    ap.add_argument("--drift-n", type=int, default=65536)
    ap.add_argument("--drift-hours", type=float, default=24.0)
    ap.add_argument("--drift-dtypes", default="fp32")
    ap.add_argument("--against", default="", help="another built checkout: order-4 A/B")
    ap.add_argument("--against-rounds", type=int, default=3)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("hermite6_rate: no GPU visible (a rate is measured on the device or not at all)",
              file=sys.stderr)
        return 2
    res = {"bench": "hermite6_rate", "device": torch.cuda.get_device_name(0)}
    if not a.no_rates:
        res["rates"] = [rate(int(n), d, a.seed, a.repeat, a.min_window_s)
                        for n in a.sizes.split(",") for d in a.dtypes.split(",")]
    if a.drift:
        res["drift"] = [row for d in a.drift_dtypes.split(",")
                        for row in drift(a.drift_n, a.drift_hours, a.seed, d)]
    if a.against:
        res["order4_against"] = against(a.against, a.against_rounds, a.seed)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
