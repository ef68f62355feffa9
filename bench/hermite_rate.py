"""Step rate of the Hermite integrator against the one-sided kick-drift step, on one GPU.

For every (N, dtype) of the grid: ms/step and pair evaluations/s (N^2 per step, both are
one-sided sums) of
  * `--integrator hermite` (fixed step: control, predict, acceleration+jerk, reduce + correct);
  * the KD step of the one-sided schedule mode=auto picks when the Newton-3 schedule is left
    out (fused from 2048 i-blocks up, else split; csrc/common/layout.cpp), same N, dtype and box;
and their ratio. The windows alternate (hermite, kd, hermite, kd, ...) and the median window
counts; each window ends in a device synchronise. Prints one JSON line.

    python bench/hermite_rate.py [--sizes 65536,262144] [--dtypes fp32,fp64] [--repeat 3]

dtype mixed (fp64 state, fp32 pair kernels on double-single positions) has no KD step: its rate
is reported alone. --compare-dtypes alternates the Hermite step of every --dtypes at each size
(fp32, mixed, fp64, fp32, ...) and reports each median, the spread of its windows and the ratio
to the first dtype.

--drift also runs 65,536 solar+random bodies for 24 simulated hours under kd, leapfrog (dt 3600)
and hermite --eta 0.02 (in --drift-dtype) and reports each run's relative energy drift.
--block runs the same workload (and the same at the other --sizes) with the shared adaptive step
and with individual block time steps: wall time, steps, body-steps, energy drift and the ratio,
for every --block-dtypes; --tight-pairs K moves body 4 + 2k next to body 3 + 2k (k < K) as a
circular binary of 1e6 m, the encounters far from the origin that fp32 positions cannot resolve.
--active-sweep times one evaluate + reduce of a block step at n_act = 1, 4, 16, ..., N on both
paths (narrow: parallel over j, up to --narrow-cap active bodies; wide: the gathered i-owned
kernel): alternating windows of back-to-back launches between device events, median.
--collisions times the fixed Hermite step with collisions off and on (detect: nearest neighbours,
closest approaches and the overlap count from the force kernel) at every --sizes and --dtypes, in
alternating windows (off, on, off, on, ...): each median, the spread of its windows and on / off.
--ranks P[,P...] runs the shared step on P virtual ranks (HermiteVirtualGroup: the shards of a
multi-rank run in one process on this device, the gathers as device copies) at every --sizes and
--dtypes: each shard's evaluate launch alone on the device (events), the whole group step (the
shards take turns on the one device, so it is about their sum) in windows alternating with the
one-rank step, and the bytes a rank gathers per step.
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

    mode = _kd_mode(n, dtype) if dtype != "mixed" else None
    herm = HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite"))
    kd = HipEngine(SimConfig(n=n, dtype=dtype, device="gpu", mode=mode)) if mode else None
    try:
        engines = {"hermite": herm, "kd": kd} if kd else {"hermite": herm}
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
               "hermite_groups": herm.native_layout["split_groups"]}
        if kd:
            out.update(kd_ipl=kd.native_layout["ipl"], kd_kernel=kd.native_layout["kernel"])
        for name in engines:
            t = statistics.median(times[name])
            out[f"{name}_ms_per_step"] = 1e3 * t
            out[f"{name}_ms_windows"] = [round(1e3 * x, 4) for x in times[name]]
            out[f"{name}_steps_per_window"] = steps[name]
            out[f"{name}_pair_evals_per_s"] = float(n) * n / t
        if kd:
            out["hermite_over_kd"] = out["hermite_ms_per_step"] / out["kd_ms_per_step"]
        return out
    finally:
        herm.close()
        if kd:
            kd.close()


def compare_dtypes(n: int, dtypes: list, seed: int, repeat: int, min_s: float) -> dict:
    """The fixed Hermite step of every dtype at one size, windows alternating over the dtypes."""
    from gravsim.config import SimConfig
    from gravsim.runtime.hermite import HermiteHipEngine

    engines = {d: HermiteHipEngine(SimConfig(n=n, dtype=d, device="gpu", integrator="hermite"))
               for d in dtypes}
    try:
        steps = {}
        for d, eng in engines.items():
            eng.init_ics("solar+random", seed)
            eng.sync()
            _window(eng, 2)
            steps[d] = max(4, int(min_s / _window(eng, 4) + 1))
        times = {d: [] for d in engines}
        for _ in range(repeat):
            for d, eng in engines.items():
                times[d].append(_window(eng, steps[d]))
        out = {"n": n, "nonfinite": sum(eng.nonfinite() for eng in engines.values())}
        for d, eng in engines.items():
            t = statistics.median(times[d])
            out[d] = {"ms_per_step": 1e3 * t, "ms_windows": [round(1e3 * x, 4) for x in times[d]],
                      "spread": (max(times[d]) - min(times[d])) / t,
                      "steps_per_window": steps[d], "ipl": eng.native_layout["ipl"],
                      "groups": eng.native_layout["split_groups"],
                      "pair_evals_per_s": float(n) * n / t}
        for d in dtypes[1:]:
            out[f"{d}_over_{dtypes[0]}"] = out[d]["ms_per_step"] / out[dtypes[0]]["ms_per_step"]
        return out
    finally:
        for eng in engines.values():
            eng.close()


def collisions(n: int, dtype: str, seed: int, repeat: int, min_s: float) -> dict:
    """The fixed Hermite step without and with the nearest-neighbour work, windows alternating."""
    from gravsim.config import SimConfig
    from gravsim.models.initial_conditions import make
    from gravsim.runtime.hermite import HermiteHipEngine

    engines = {m: HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite",
                                             collisions=m)) for m in ("off", "detect")}
    try:
        b = make("solar+random", n, seed)
        steps = {}
        for m, eng in engines.items():
            eng.load(b)  # (the same bodies through the same path; every radius 0)
            eng.sync()
            _window(eng, 2)
            steps[m] = max(4, int(min_s / _window(eng, 4) + 1))
        times = {m: [] for m in engines}
        for _ in range(repeat):
            for m, eng in engines.items():
                times[m].append(_window(eng, steps[m]))
        out = {"n": n, "dtype": dtype,
               "nonfinite": sum(eng.nonfinite() for eng in engines.values()),
               "overlaps": engines["detect"].status().overlaps}
        for m in engines:
            t = statistics.median(times[m])
            out[m] = {"ms_per_step": 1e3 * t, "ms_windows": [round(1e3 * x, 4) for x in times[m]],
                      "spread": (max(times[m]) - min(times[m])) / t, "steps_per_window": steps[m],
                      "ipl": engines[m].native_layout["ipl"],
                      "groups": engines[m].native_layout["split_groups"]}
        out["on_over_off"] = out["detect"]["ms_per_step"] / out["off"]["ms_per_step"]
        return out
    finally:
        for eng in engines.values():
            eng.close()


def ranks(n: int, dtype: str, P: int, seed: int, repeat: int, min_s: float) -> dict:
    """P virtual ranks beside one rank: per-shard evaluate, group step, gathered bytes."""
    from gravsim.config import SimConfig
    from gravsim.runtime.hermite import HermiteHipEngine, HermiteVirtualGroup

    cfg = SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite")
    engines = {"one": HermiteHipEngine(cfg), "group": HermiteVirtualGroup(cfg, P)}
    try:
        steps = {}
        for name, eng in engines.items():
            eng.init_ics("solar+random", seed)
            eng.sync()
            _window(eng, 2)
            steps[name] = max(4, int(min_s / _window(eng, 4) + 1))
        times = {name: [] for name in engines}
        for _ in range(repeat):
            for name, eng in engines.items():
                times[name].append(_window(eng, steps[name]))
        grp = engines["group"]
        ev = grp.time_eval(max(2, steps["one"] // 2))
        lay = [e.native_layout for e in grp.shards]
        n_pad, psz = lay[0]["n_pad"], 8 if dtype == "fp64" else 4
        rows = (3 if dtype == "mixed" else 2) * n_pad * 4 * psz + n_pad // 256 * 8
        one, group = (statistics.median(times[k]) for k in ("one", "group"))
        out = {"n": n, "dtype": dtype, "ranks": P, "n_pad": n_pad,
               "rows": [x["n_local"] for x in lay], "ipl": [x["ipl"] for x in lay],
               "groups": [x["split_groups"] for x in lay],
               "workgroups": [x["n_local"] // (256 * x["ipl"]) * x["split_groups"] for x in lay],
               "shard_eval_ms": [round(x, 4) for x in ev],
               "one_rank_ms_per_step": 1e3 * one,
               "one_rank_ms_windows": [round(1e3 * x, 4) for x in times["one"]],
               "group_ms_per_step": 1e3 * group,
               "group_ms_windows": [round(1e3 * x, 4) for x in times["group"]],
               "max_shard_eval_over_one_rank_step": max(ev) / (1e3 * one),
               "gathered_bytes_per_step": rows,  # (what every rank holds after the gathers)
               "received_bytes_per_step_rank0": rows - rows * lay[0]["n_local"] // n_pad}
        return out
    finally:
        for eng in engines.values():
            eng.close()


def tight_pairs(b, pairs: int, sep: float = 1e6):
    """Body 4 + 2k next to body 3 + 2k (k < pairs) on a circular orbit of separation sep."""
    import math

    import numpy as np

    from gravsim.config import G_SI

    rng = np.random.default_rng(pairs)
    for k in range(pairs):
        i = 3 + 2 * k
        if i + 1 >= b.n:
            break
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        t = np.cross(u, (0.3, 0.5, 0.8))
        t /= np.linalg.norm(t)
        b.pos[i + 1] = b.pos[i] + sep * u
        b.vel[i + 1] = b.vel[i] + math.sqrt(G_SI * (b.mass[i] + b.mass[i + 1]) / sep) * t
    return b


def drift(n: int, hours: float, seed: int, dtype: str = "fp32") -> list:
    from gravsim.config import SimConfig
    from gravsim.runtime.simulation import Simulation

    t_end = hours * 3600.0
    out = []
    for name, kw in (("kd", dict(integrator="kd", steps=int(hours))),
                     ("leapfrog", dict(integrator="leapfrog", steps=int(hours))),
                     ("hermite eta 0.02", dict(integrator="hermite", eta=0.02, t_end=t_end,
                                               steps=20000))):
        # (kd and leapfrog have no mixed precision: they run in fp32 beside a mixed hermite)
        d = dtype if kw["integrator"] == "hermite" or dtype != "mixed" else "fp32"
        sim = Simulation(SimConfig(n=n, dtype=d, device="gpu", dt=3600.0, seed=seed,
                                   diagnostics=True, **kw))
        try:
            m = sim.run()
        finally:
            sim.close()
        out.append({"integrator": name, "dtype": d, "steps": m.steps, "wall_s": m.wall_s,
                    "time_reached": m.time_reached if m.time_reached is not None else t_end,
                    "dt_min": m.dt_min,
                    "energy_rel_drift": m.extra["conservation"]["energy_rel_drift"]})
    return out


def block(n: int, hours: float, seed: int, dtype: str = "fp32", pairs: int = 0,
          shared: bool = True) -> dict:
    """Shared adaptive step against block steps, same build, same workload."""
    from gravsim.config import SimConfig
    from gravsim.models.initial_conditions import make
    from gravsim.runtime.simulation import Simulation

    out = {"n": n, "dtype": dtype, "hours": hours, "tight_pairs": pairs}
    for name, kw in (("shared", dict(steps=10 ** 6)),
                     ("block", dict(block_steps=True, steps=int(hours)))):
        if name == "shared" and not shared:
            continue
        sim = Simulation(SimConfig(n=n, dtype=dtype, device="gpu", dt=3600.0, seed=seed,
                                   integrator="hermite", eta=0.02, t_end=hours * 3600.0,
                                   diagnostics=True, **kw))
        try:
            if pairs:
                sim.engine.load(tight_pairs(make("solar+random", n, seed, sim.cfg.G), pairs))
            m = sim.run()
        finally:
            sim.close()
        r = {"wall_s": m.wall_s, "steps": m.steps, "time_reached": m.time_reached,
             "dt_min": m.dt_min,
             "energy_rel_drift": m.extra["conservation"]["energy_rel_drift"]}
        if name == "block":
            r.update(block_steps=m.block_steps, body_steps=m.body_steps, level_max=m.level_max,
                     level_clamped=m.level_clamped,
                     mean_n_act=m.body_steps / max(1, m.block_steps),
                     us_per_block_step=1e6 * m.wall_s / max(1, m.block_steps))
        else:
            r.update(body_steps=m.steps * n)
        out[name] = r
    if shared:
        out["shared_over_block_wall"] = out["shared"]["wall_s"] / out["block"]["wall_s"]
        out["shared_over_block_body_steps"] = \
            out["shared"]["body_steps"] / out["block"]["body_steps"]
    return out


def active_sweep(n: int, dtype: str, seed: int, repeat: int, narrow_cap: int) -> dict:
    import numpy as np

    from gravsim.config import SimConfig
    from gravsim.runtime.hermite import HermiteHipEngine

    eng = HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite",
                                     eta=0.02, block_steps=True))
    try:
        eng.init_ics("solar+random", seed)
        cap = min(n, narrow_cap)
        default = eng.status_narrow_max()
        eng.set_block_tuning(narrow_max=cap)
        perm = np.random.default_rng(seed).permutation(n)
        sizes = sorted({min(n, 4 ** k) for k in range(0, 12)} | {n} |
                       {2 ** k for k in range(10, 17) if 2 ** k <= n})
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
                    t[p].append(eng.time_active(idx, p, max(1, min(50, int(20.0 / max(once,
                                                                                     1e-3))))))
            row = {"n_act": m}
            for p in paths:
                row[f"{p}_ms"] = statistics.median(t[p])
            rows.append(row)
        both = [r for r in rows if "narrow_ms" in r]
        faster = [r["n_act"] for r in both if r["narrow_ms"] <= r["wide_ms"]]
        return {"n": n, "dtype": dtype, "narrow_cap": cap, "rows": rows,
                "narrow_faster_up_to": max(faster) if faster else 0,
                "default_narrow_max": default}
    finally:
        eng.close()


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
    ap.add_argument("--drift-dtype", default="fp32", help="dtype of the --drift hermite run")
    ap.add_argument("--compare-dtypes", action="store_true",
                    help="the Hermite step of every --dtypes in alternating windows, per size")
    ap.add_argument("--block-dtypes", default="fp32", help="dtypes of the --block runs")
    ap.add_argument("--no-shared", action="store_true",
                    help="--block: the block-step runs only")
    ap.add_argument("--tight-pairs", type=int, default=0,
                    help="--block: binaries of 1e6 m added to the workload")
    ap.add_argument("--block", action="store_true",
                    help="the 24-hour workload at every --sizes: shared adaptive step against "
                         "block steps (fp32, eta 0.02)")
    ap.add_argument("--active-sweep", action="store_true",
                    help="ms per evaluate of a block step at n_act = 1, 4, 16, ..., N, both paths")
    ap.add_argument("--narrow-cap", type=int, default=65536,
                    help="--active-sweep: largest n_act timed on the narrow path")
    ap.add_argument("--collisions", action="store_true",
                    help="the Hermite step with collisions off and on in alternating windows")
    ap.add_argument("--ranks", default="",
                    help="P[,P...]: the shared step on P virtual ranks of this device beside one "
                         "rank (per-shard evaluate, group step, gathered bytes)")
    ap.add_argument("--no-rates", action="store_true", help="skip the hermite / kd step rates")
    a = ap.parse_args()
    import torch

    import gravsim  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("hermite_rate: needs a HIP device")
    res = {"bench": "hermite_rate", "device": torch.cuda.get_device_name(0),
           "engine_clock_ghz": None,  # (the Hermite kernel does not record the engine clock)
           "rates": [] if a.no_rates else
                    [rate(int(n), d, a.seed, a.repeat, a.min_window_s)
                     for n in a.sizes.split(",") for d in a.dtypes.split(",")]}
    if a.compare_dtypes:
        res["compare_dtypes"] = [compare_dtypes(int(n), a.dtypes.split(","), a.seed, a.repeat,
                                                a.min_window_s) for n in a.sizes.split(",")]
    if a.drift:
        res["drift_24h"] = drift(a.drift_n, 24.0, a.seed, a.drift_dtype)
    if a.block:
        res["block_24h"] = [block(int(n), 24.0, a.seed, d, a.tight_pairs, not a.no_shared)
                            for n in a.sizes.split(",") for d in a.block_dtypes.split(",")]
    if a.collisions:
        res["collisions"] = [collisions(int(n), d, a.seed, a.repeat, a.min_window_s)
                             for n in a.sizes.split(",") for d in a.dtypes.split(",")]
    if a.ranks:
        res["ranks"] = [ranks(int(n), d, int(P), a.seed, a.repeat, a.min_window_s)
                        for n in a.sizes.split(",") for d in a.dtypes.split(",")
                        for P in a.ranks.split(",")]
    if a.active_sweep:
        res["active_sweep"] = [active_sweep(int(n), d, a.seed, a.repeat, a.narrow_cap)
                               for n in a.sizes.split(",") for d in a.dtypes.split(",")]
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
