"""Cost of one k-nearest-neighbour pass (k = 6) beside the Hermite evaluate, on one GPU.

For every (N, dtype) of the grid: milliseconds per pass of the kernel of csrc/hip/nbody_knn.hip
plus its merge, between two device events (no upload, no download), the median of --reps passes
after a warm-up pass; the Hermite acceleration+jerk evaluate of the same N and dtype from the
same process (the gathered i-owned kernel with every body active plus its reduce, the block
path's `wide` form: the same j sweep as the shared step's evaluate), windows alternating with the
passes; and their ratio. A pass does a third of the evaluate's arithmetic per pair. Prints one
JSON line; `pair_evals` is n x n_pad per pass.

    python bench/knn_rate.py [--sizes 65536,262144] [--dtypes fp32,mixed,fp64] [--reps 5]

--ab DIR: the early-out A/B. DIR holds a second native build (csrc/build.py with
GRAVSIM_NATIVE_DIR=DIR and GRAVSIM_HIP_EXTRA=-DGS_KNN_EARLY=0: the insertion chain runs for every
candidate); --rounds times, a fresh child process per arm times the passes with the in-tree build
(A) and with DIR (B), alternating A, B, A, B, ..., and the medians over the rounds are reported
with B / A. The lists are the same bits either way (tests/test_knn_gpu.py holds for both builds).
--shapes: instead of the rates, ms per pass for ipl 1, 2 x 1 to 32 chunk groups at every size and
dtype (the sweep behind the auto shape of gs_hip_knn; profiles/knn_shapes.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bodies(n: int, seed: int):
    """A Plummer sphere: what the read-outs are for (and a density contrast for the lists)."""
    import gravsim  # noqa: F401
    from gravsim.models.initial_conditions import plummer

    return plummer(n, seed)


def knn_pass(pos, dtype: str, reps: int = 5, k: int = 6, ipl: int = 0, groups: int = 0) -> dict:
    import gravsim  # noqa: F401
    from gravsim.ops import _native, neighbours

    ms, info = neighbours.gpu_pass_ms(pos, k, dtype, ipl, groups, reps + 1)  # (first: warm-up)
    runs = ms[1:]
    t = statistics.median(runs)
    return {"n": len(pos), "dtype": dtype, "k": k, "ms_per_pass": t,
            "ms_runs": [round(x, 4) for x in runs], "spread": (max(runs) - min(runs)) / t,
            "early_out": _native.hip_lib().gs_knn_early_out(),
            "pair_evals_per_s": info["pair_evals"] / (1e-3 * t), **info}


def rate(n: int, dtype: str, seed: int, reps: int, evaluate: bool) -> dict:
    import numpy as np

    from gravsim.config import SimConfig
    from gravsim.runtime.hermite import HermiteHipEngine

    b = bodies(n, seed)
    if not evaluate:
        return knn_pass(b.pos, dtype, reps)
    eng = HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite",
                                     eta=0.02, block_steps=True))
    try:
        eng.load(b)
        every = np.arange(n, dtype=np.int32)
        eng.time_active(every, "wide", 2)  # warm-up
        knn_pass(b.pos, dtype, 1)
        ev, passes = [], []
        for _ in range(reps):  # alternating: evaluate, pass, evaluate, pass, ...
            ev.append(eng.time_active(every, "wide", 3))
            passes.append(knn_pass(b.pos, dtype, 1))
        out = dict(passes[-1])
        runs = [p["ms_per_pass"] for p in passes]
        t, e = statistics.median(runs), statistics.median(ev)
        out.update(ms_per_pass=t, ms_runs=[round(x, 4) for x in runs],
                   spread=(max(runs) - min(runs)) / t,
                   pair_evals_per_s=out["pair_evals"] / (1e-3 * t),
                   evaluate_ms=e, evaluate_ms_runs=[round(x, 4) for x in ev],
                   evaluate_ipl=eng.native_layout["ipl"], pass_over_evaluate=t / e)
        return out
    finally:
        eng.close()


def shapes(n: int, dtypes: list, seed: int, reps: int) -> list:
    import gravsim  # noqa: F401
    from gravsim.ops import neighbours

    pos, rows = bodies(n, seed).pos, []
    for dtype in dtypes:
        for ipl in (1, 2):
            for groups in (1, 2, 4, 8, 16, 32):
                ms, info = neighbours.gpu_pass_ms(pos, 6, dtype, ipl, groups, reps + 1)
                rows.append({"n": n, "dtype": dtype, "ipl": ipl, "groups_asked": groups,
                             "groups": info["groups"],
                             "ms": round(statistics.median(ms[1:]), 4)})
    return rows


def early_out_ab(args, other: str) -> list:
    """Alternating child runs of the in-tree build (A) and the build in `other` (B)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--no-evaluate", "--sizes", args.sizes,
           "--dtypes", args.dtypes, "--reps", str(args.reps), "--seed", str(args.seed)]
    rows: dict = {}
    for _ in range(args.rounds):
        for arm in ("A", "B"):
            env = dict(os.environ)
            if arm == "B":
                env["GRAVSIM_NATIVE_DIR"] = os.path.abspath(other)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode:
                raise SystemExit(f"knn_rate: arm {arm} failed:\n{r.stdout}\n{r.stderr}")
            line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
            for row in json.loads(line)["rates"]:
                d = rows.setdefault((row["n"], row["dtype"]), {"A": [], "B": [], "early": {}})
                d[arm].append(row["ms_per_pass"])
                d["early"][arm] = row["early_out"]
    out = []
    for (n, dtype), d in rows.items():
        a, b = statistics.median(d["A"]), statistics.median(d["B"])
        out.append({"n": n, "dtype": dtype, "early_out": d["early"],
                    "A_ms": a, "B_ms": b, "A_ms_rounds": [round(x, 4) for x in d["A"]],
                    "B_ms_rounds": [round(x, 4) for x in d["B"]], "B_over_A": b / a})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--dtypes", default="fp32,mixed,fp64")
    ap.add_argument("--reps", type=int, default=5, help="timed passes (median), at least 5")
    ap.add_argument("--seed", type=int, default=20250307)
    ap.add_argument("--no-evaluate", action="store_true", help="the passes only")
    ap.add_argument("--ab", default="", help="a second native build directory: early-out A/B")
    ap.add_argument("--rounds", type=int, default=3, help="--ab: alternating rounds")
    ap.add_argument("--shapes", action="store_true", help="the launch-shape sweep only")
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("knn_rate: --reps must be at least 5")
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("knn_rate: needs a HIP device")
    if a.shapes:
        print(json.dumps({"bench": "knn_rate", "device": torch.cuda.get_device_name(0),
                          "shapes": [r for n in a.sizes.split(",")
                                     for r in shapes(int(n), a.dtypes.split(","), a.seed,
                                                     a.reps)]}), flush=True)
        return 0
    res = {"bench": "knn_rate", "device": torch.cuda.get_device_name(0),
           "rates": [rate(int(n), d, a.seed, a.reps, not a.no_evaluate)
                     for n in a.sizes.split(",") for d in a.dtypes.split(",")]}
    if a.ab:
        res["early_out_ab"] = early_out_ab(a, a.ab)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
