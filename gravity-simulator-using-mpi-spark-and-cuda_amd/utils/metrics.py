"""Machine-readable run metrics (one JSON line per run) and timing helpers.

The reference reports only wall time: "Total execution time" / "Average time per step"
(mpi.c:245-247, pyspark.py:191-193) and "Simulation took" (cuda.cu:171). The headline
metric of this project (BASELINE.json) is body-updates/s = N * steps / wall, plus
effective_interactions_per_s = N^2 * steps / wall (the ordered pair terms a one-sided direct
sum evaluates) and pair_evals_per_s, the pair evaluations actually performed: N(N-1)/2 per
step for the Newton-3 sym schedule, N^2 otherwise. `extra` carries the comm/compute split of
multi-rank GPU runs (comm_ms, exposed_comm_ms; --phase-timing).
"""
from __future__ import annotations

import json
import time
from dataclasses import asdict, dataclass, field


@dataclass
class RunMetrics:
    n: int
    steps: int
    dt: float
    dtype: str
    device: str
    nranks: int
    wall_s: float
    kernel: str = ""
    mode: str = ""
    extra: dict = field(default_factory=dict)
    # integrator hermite (None otherwise, and then left out of the JSON line): the simulated
    # time reached, the steps taken (steps past t_end are not taken) and the smallest step
    time_reached: float | None = None
    steps_taken: int | None = None
    dt_min: float | None = None
    # ... with block steps (`steps` then counts macro steps of dt): block steps taken, the sum
    # of their active bodies, the pair evaluations (body_steps * n), the deepest level and the
    # times a body wanted a step below dt 2^-max_level
    block_steps: int | None = None
    body_steps: int | None = None
    pair_evals: int | None = None
    level_max: int | None = None
    level_clamped: int | None = None
    # ... with collisions detect | merge: bodies absorbed by mergers, bodies left, the smallest
    # pair measure q = r^2 - (R_i + R_j)^2 any evaluation has seen (< softening^2: an overlap;
    # None when no pair was seen) and the overlaps the evaluations counted
    mergers: int | None = None
    bodies_left: int | None = None
    closest_q_min: float | None = None
    overlaps_seen: int | None = None
    # --structure: {"k", "samples": [{"step", "time", "density_centre", "core_radius",
    # "density_max", "lagrangian_radii", "degenerate"}]} (None, and left out, otherwise)
    structure: dict | None = None
    # integrator hermite: the order of the scheme, 4 or 6 (None, and left out, otherwise)
    hermite_order: int | None = None

    @property
    def ms_per_step(self) -> float:
        return 1e3 * self.wall_s / self.steps if self.steps else 0.0

    @property
    def body_updates_per_s(self) -> float:
        return self.n * self.steps / self.wall_s if self.wall_s > 0 else 0.0

    @property
    def effective_interactions_per_s(self) -> float:
        return float(self.n) * self.n * self.steps / self.wall_s if self.wall_s > 0 else 0.0

    @property
    def pair_evals_per_s(self) -> float:
        if self.wall_s <= 0:
            return 0.0
        pairs = self.n * (self.n - 1) / 2 if self.mode == "sym" else float(self.n) * self.n
        return pairs * self.steps / self.wall_s

    def to_json(self) -> str:
        d = asdict(self)
        for k in ("time_reached", "steps_taken", "dt_min", "block_steps", "body_steps",
                  "pair_evals", "level_max", "level_clamped", "mergers", "bodies_left",
                  "closest_q_min", "overlaps_seen", "structure", "hermite_order"):
            if d[k] is None:
                del d[k]
        d.update(ms_per_step=self.ms_per_step, body_updates_per_s=self.body_updates_per_s,
                 effective_interactions_per_s=self.effective_interactions_per_s,
                 pair_evals_per_s=self.pair_evals_per_s)
        return json.dumps(d, sort_keys=True)


class Stopwatch:
    def __init__(self):
        self.t0 = time.perf_counter()

    def elapsed(self) -> float:
        return time.perf_counter() - self.t0
