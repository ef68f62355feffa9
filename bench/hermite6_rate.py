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
--block runs the same 24 hours in fp64 with block steps at order 6 (eta 0.25), with one shared
step at order 6 (eta 0.25) and with block steps at order 4 (eta 0.02), one after the other in this
process: block steps, body-steps, deepest level, clamps, wall time, energy drift, and for the block
runs the wall time per block step (the per-launch cost of the seven-launch chain dominates it
while the active sets are small).
--active-sweep times one evaluate + reduce of the order-6 block step on both paths against the
number of active bodies (fp64, every --sizes): the crossover is the default narrow_max.
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


def block_table(n: int, hours: float, seed: int) -> list:
    """The 24-hour runs in fp64: order 6 block, order 6 shared, order 4 block."""
    from gravsim.config import SimConfig
    from gravsim.runtime.simulation import Simulation

    out = []
    for order, eta, block in ((6, 0.25, True), (6, 0.25, False), (4, 0.02, True)):
        steps = int(round(hours)) if block else 20000  # (block: macro steps of dt)
        sim = Simulation(SimConfig(n=n, dtype="fp64", device="gpu", dt=3600.0, seed=seed,
                                   integrator="hermite", hermite_order=order, eta=eta,
                                   block_steps=block and order == 4,
                                   block_steps6=block and order == 6, t_end=hours * 3600.0,
                                   steps=steps,
                                   diagnostics=True))
        try:
            m = sim.run()
        finally:
            sim.close()
        row = {"order": order, "eta": eta, "block_steps_on": block, "dtype": "fp64", "n": n,
               "steps": m.steps, "wall_s": m.wall_s, "time_reached": m.time_reached,
               "dt_min": m.dt_min,
               "energy_rel_drift": m.extra["conservation"]["energy_rel_drift"]}
        if block:
            row.update(block_steps=m.block_steps, body_steps=m.body_steps,
                       level_max=m.level_max, level_clamped=m.level_clamped,
                       ms_per_block_step=1e3 * m.wall_s / max(1, m.block_steps))
        else:
            row.update(body_steps=m.steps * n)
        out.append(row)
    return out


def active_sweep(n: int, seed: int, repeat: int, narrow_cap: int) -> dict:
    """Milliseconds per evaluate + reduce of the order-6 block step against n_act, both paths."""
    import numpy as np

    from gravsim.config import SimConfig
    from gravsim.runtime.hermite import HermiteHipEngine

    eng = HermiteHipEngine(SimConfig(n=n, dtype="fp64", device="gpu", integrator="hermite",
                                     hermite_order=6, eta=0.25, block_steps6=True))
    try:
        eng.init_ics("solar+random", seed)
        cap = min(n, narrow_cap)
        default = eng.status_narrow_max()
        eng.set_block_tuning(narrow_max=cap)
        perm = np.random.default_rng(seed).permutation(n)
        sizes = sorted({min(n, 4 ** k) for k in range(0, 12)} | {n} |
                       {2 ** k for k in range(8, 17) if 2 ** k <= n})
        rows = []
        for m in sizes:
            idx = np.sort(perm[:m]).astype(np.int32)
            paths = ["wide"] + (["narrow"] if m <= cap else [])
            t = {p: [] for p in paths}
            for p in paths:
                eng.time_active(idx, p, 2)  # warm-up
            for _ in range(repeat):
                for p in paths:
                    once = eng.time_active(idx, p, 1)
                    t[p].append(eng.time_active(idx, p,
                                                max(1, min(50, int(20.0 / max(once, 1e-3))))))
            row = {"n_act": m}
            for p in paths:
                row[f"{p}_ms"] = statistics.median(t[p])
            rows.append(row)
        both = [r for r in rows if "narrow_ms" in r]
        faster = [r["n_act"] for r in both if r["narrow_ms"] <= r["wide_ms"]]
        return {"n": n, "dtype": "fp64", "order": 6, "narrow_cap": cap, "rows": rows,
                "narrow_faster_up_to": max(faster) if faster else 0,
                "default_narrow_max": default}
    finally:
        eng.close()


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
    ap.add_argument("--block", action="store_true",
                    help="the 24-hour fp64 table: order 6 block, order 6 shared, order 4 block")
    ap.add_argument("--active-sweep", action="store_true",
                    help="order-6 block step: evaluate + reduce time against n_act, both paths")
    ap.add_argument("--narrow-cap", type=int, default=65536,
                    help="--active-sweep: largest n_act timed on the narrow path")
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
    if a.block:
        res["block"] = block_table(a.drift_n, a.drift_hours, a.seed)
    if a.active_sweep:
        res["active_sweep"] = [active_sweep(int(n), a.seed, a.repeat, a.narrow_cap)
                               for n in a.sizes.split(",")]
    if a.against:
        res["order4_against"] = against(a.against, a.against_rounds, a.seed)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
