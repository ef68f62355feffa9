"""Simulation driver: ICs or resume -> step loop -> stats, dumps, checkpoints.

Reference step loops: cuda.cu:154-167, mpi.c:189-237, pyspark.py:104-121. Differences by
design:
* the whole loop is enqueued on the device; the host only wakes up at "events" (progress
  lines, checkpoints, trajectory frames, NaN guard) instead of crossing the host/device
  boundary twice per step (cuda.cu:157,160);
* timing brackets the step loop like the reference ("Total execution time", mpi.c:239-247)
  but ends with a device sync so the number is real;
* NaN/Inf guard (the reference silently produced non-finite output, D1-D3) and RCCL health
  checks run at a configurable period;
* optional conserved-quantity diagnostics (--diagnostics / --diag-every): total energy with
  the exact-cutoff potential, linear and angular momentum, and their relative drift;
* optional cluster-structure read-outs (--structure / --structure-every): density centre, core
  radius, central density and Lagrangian radii from the k-nearest-neighbour lists of the state
  (ops/neighbours.py), on the engine's device in the run's dtype, outside the timed wall;
* checkpoints are rank-agnostic and a resumed run continues bit-exactly;
* integrator "kd" is the reference's kick-drift update (cuda.cu:73-76, mpi.c:207-215);
  "leapfrog" runs the very same per-step kernel on velocities staggered by half a step
  (v_{k-1/2}): a backward half-kick at the start, synchronized velocities
  v_k = v_{k-1/2} + a(x_k) dt/2 on output — second-order (KDK) accuracy at no extra cost per
  step. Checkpoints keep the staggered velocities (meta "velocity": "half-step") so resume
  stays bit-exact;
* integrator "hermite" is the 4th-order predictor-corrector of runtime/hermite.py with
  its own acceleration+jerk kernel, a fixed step or a shared adaptive one (eta) and an optional
  end time (t_end); the engine carries the time, so metrics and checkpoints report its t, and a
  checkpoint keeps the carried a, j and the next step size so that resume stays bit-exact.
  Shared steps run on P GPU ranks (runtime/hermite.py): every rank holds the same time and step
  size and returns all rows from state() / carried() / derivs(), so checkpoints, dumps and the
  conserved quantities are formed from the gathered rows in the one-rank order and are the
  one-rank values bit for bit; a checkpoint resumes at any P. Block steps, collisions and the
  CPU engine stay on one rank.
  hermite_order 6 (Nitadori & Makino 2008) carries the snap and the crackle too: a checkpoint
  keeps all four of a, j, s, c and the order, and a checkpoint of the other order restarts its
  derivatives from x, v, t (the log says so).
  With block_steps every body has its own step dt 2^-k and `steps` counts macro steps of dt, at
  which all bodies stand at the same time: all periodic work lands on synchronised states, and a
  checkpoint also keeps the levels.
  collisions "detect" reports the nearest-neighbour records of the engine; "merge" also replaces
  overlapping bodies by one (ops/oracle.py merge_overlaps) at synchronised states: the step at
  which a shared-step run stopped itself, or each macro boundary of a block-step run. The engine
  is rebuilt on the survivors at the same time (a, j evaluated afresh, levels re-initialised);
  `ids` keeps their original indices, and checkpoints carry radius and id.
"""
from __future__ import annotations

import os
import time
import warnings
from typing import Optional

import numpy as np

from ..config import SimConfig
from ..models.initial_conditions import BodySet
from ..parallel import comm
from ..utils import checkpoint as ckpt
from ..utils.logs import RunLog
from ..utils.metrics import RunMetrics
from .engines import CpuEngine, HipEngine, gpu_available
from .hermite import HermiteCpuEngine, HermiteHipEngine


class NonFiniteError(RuntimeError):
    pass


def engine_conserved(engine, dist, step: int = 0, staggered: bool = False,
                     dt: float = 0.0) -> dict:
    """Total energy, linear and angular momentum of an engine's current state (collective).

    Each rank sums over its own bodies: kinetic 1/2 m v^2, potential 1/2 m phi with phi the
    exact-cutoff potential of the engine's diagnostic force path (the same pass returns the
    accelerations that synchronise leapfrog's half-step velocities v_{k-1/2} + a dt/2),
    p = sum m v and L = sum m x cross v; the sums are all-reduced. The reference has no such
    check (it only prints positions); it is the standard correctness gauge of an N-body
    integrator (bench.py reports the drift over its timed steps)."""
    # An engine whose reads return every rank's rows (multi-rank hermite): each rank forms the
    # sums over all bodies in the one-rank order, and nothing is reduced.
    whole = dist.world > 1 and getattr(engine, "gathers_all", False)
    rows = range(engine.cfg.n) if whole else engine.layout.real_local
    b = engine.state()
    sl = slice(rows.start, rows.stop)
    m, x, v = b.mass[sl], b.pos[sl], b.vel[sl]
    if whole:
        a4 = engine.derivs()[0]
    else:
        a4 = engine.accel()[: len(rows)] if len(rows) else np.zeros((0, 4))
    if staggered:
        v = v + 0.5 * dt * a4[:, :3]
    xv = np.cross(x, v) if len(rows) else np.zeros((0, 3))
    red = float if whole else lambda y: comm.allreduce_sum(dist, float(y))  # noqa: E731
    ke = red(0.5 * (m * (v * v).sum(1)).sum())
    pe = red(0.5 * (m * a4[:, 3]).sum())
    return {"step": int(step), "kinetic": ke, "potential": pe, "energy": ke + pe,
            "momentum": [red(c) for c in (m[:, None] * v).sum(0)],
            "angular_momentum": [red(c) for c in (m[:, None] * xv).sum(0)],
            "momentum_scale": red((m * np.linalg.norm(v, axis=1)).sum()),
            "angular_momentum_scale": red((m * np.linalg.norm(xv, axis=1)).sum())}


def conservation_summary(c0: dict, c1: dict, samples: list = ()) -> dict:
    """Relative drifts of the conserved quantities between two engine_conserved() records."""
    def rel(a, b, scale):
        d = float(np.linalg.norm(np.asarray(b, dtype=float) - np.asarray(a, dtype=float)))
        return d / scale if scale > 0 else (0.0 if d == 0 else float("inf"))

    return {"energy_start": c0["energy"], "energy_end": c1["energy"],
            "energy_rel_drift": rel(c0["energy"], c1["energy"], abs(c0["energy"])),
            "momentum_rel_drift": rel(c0["momentum"], c1["momentum"], c0["momentum_scale"]),
            "angular_momentum_rel_drift": rel(c0["angular_momentum"], c1["angular_momentum"],
                                              c0["angular_momentum_scale"]),
            "samples": [{"step": c["step"], "energy": c["energy"]} for c in samples]}


class Simulation:
    def __init__(self, cfg: SimConfig, dist: Optional[comm.DistInfo] = None, guard=None):
        self.cfg = cfg.validate()
        self.dist = dist or comm.env_info()
        self.hermite = cfg.integrator == "hermite"
        self.overlap_check: Optional[str] = None
        use_gpu = cfg.device == "gpu" or (cfg.device == "auto" and gpu_available())
        if self.hermite and self.dist.world > 1:
            # shared steps on GPU ranks; the refusals before any engine or collective
            from ..parallel.partition import hermite_layout

            cfg.replace(gpus=self.dist.world, device="gpu" if use_gpu else "cpu").validate()
            hermite_layout(cfg.n, self.dist.rank, self.dist.world, cfg.chunk)
        if cfg.device == "gpu" and not gpu_available():
            raise RuntimeError("device=gpu requested but no HIP device / native library")
        d = self.dist
        stage = guard.stage if guard else (lambda *_a, **_k: None)
        ecfg = self._engine_cfg()
        if use_gpu:
            import torch

            from ..parallel.guard import INIT_TIMEOUT_S

            dev = d.local_rank % max(1, torch.cuda.device_count())
            stage("engine", INIT_TIMEOUT_S)
            self._hermite_engine = lambda c: HermiteHipEngine(c, device=dev)
            self.engine = (HermiteHipEngine(ecfg, d.rank, d.world, device=dev, dist=d)
                           if self.hermite else
                           HipEngine(cfg, d.rank, d.world, device=dev, dist=d))
            if guard:
                guard.on_abort(self.engine.abort)
                guard.probe(lambda: {"comm_stage": self.engine.comm_stage()})
            if d.world > 1:
                stage("comm_init", INIT_TIMEOUT_S)
                uid = HipEngine.unique_id() if d.is_root else None
                uid = comm.broadcast_bytes(d, uid)
                self.engine.comm_init(uid)
                if self.hermite:
                    # (no start-up probe: a shared adaptive step has no fixed cost; the bound is
                    # the configured one, or the floor of the derived one)
                    from ..parallel.guard import step_timeout

                    self.engine.set_step_timeout(step_timeout(0.0) if cfg.step_timeout_s is None
                                                 else cfg.step_timeout_s)
                else:
                    stage("self_check", INIT_TIMEOUT_S)
                    per_step = self._self_check()
                    if cfg.step_timeout_s is None:
                        from ..parallel.guard import step_timeout

                        self.engine.set_step_timeout(step_timeout(per_step))
            stage("ics", INIT_TIMEOUT_S)
        else:
            # CPU engine (gloo for P > 1): no RCCL to hang on, and set-up includes O(N^2) work
            # (a leapfrog half-kick), so the start-up deadline of gloo_init is cleared here
            # instead of killing a slow but healthy start; gloo's own timeouts
            # bound its collectives.
            stage("cpu_setup", None)
            self._hermite_engine = HermiteCpuEngine
            self.engine = (HermiteCpuEngine(ecfg) if self.hermite else
                           CpuEngine(cfg, d.rank, d.world, dist=d))
        self.step0 = 0
        self.trajectory: list[np.ndarray] = []
        self.staggered = False  # velocities held as v_{k-1/2} (leapfrog)
        self.order_restart = False  # a hermite checkpoint of the other order was resumed
        if cfg.resume:
            c = self._resume
            if c.bodies.n != ecfg.n:
                raise ValueError(f"checkpoint has n={c.bodies.n}, config n={cfg.n}")
            same_order = int(c.meta.get("hermite_order", 4)) == cfg.hermite_order
            self.order_restart = self.hermite and c.meta.get("integrator") == "hermite" and \
                not same_order
            if self.order_restart:
                warnings.warn(f"resuming a hermite checkpoint of order "
                              f"{int(c.meta.get('hermite_order', 4))} under order "
                              f"{cfg.hermite_order}: the derivatives restart from x, v, t",
                              stacklevel=2)
            if self.hermite and cfg.hermite_order == 6 and same_order and \
                    c.meta.get("integrator") == "hermite" and \
                    all(k in c.extra for k in ("acc", "jerk", "snap", "crackle")):
                self.engine.load(c.bodies, c.extra["acc"], c.extra["jerk"],
                                 t=float(c.meta.get("time", 0.0)), dt_next=c.meta.get("dt_next"),
                                 dt_min=c.meta.get("dt_min"), snap=c.extra["snap"],
                                 crackle=c.extra["crackle"], **self._resumed_levels(c))
            elif self.hermite and same_order and cfg.hermite_order == 4 and \
                    c.meta.get("integrator") == "hermite" and \
                    "acc" in c.extra and "jerk" in c.extra:
                # the carried a, j (evaluated at the last predicted state) and the step size
                # the criterion chose: the run continues bit for bit
                self.engine.load(c.bodies, c.extra["acc"], c.extra["jerk"],
                                 t=float(c.meta.get("time", 0.0)), dt_next=c.meta.get("dt_next"),
                                 dt_min=c.meta.get("dt_min"), **self._resumed_levels(c))
            elif self.hermite:
                self.engine.load(c.bodies, t=float(c.meta.get("time", 0.0)))  # a, j afresh
            else:
                self.engine.load(c.bodies)
            self.step0 = c.step
            self.staggered = c.meta.get("velocity") == "half-step"
            stored_dt = float(c.meta.get("dt", cfg.dt))
            if self.staggered and stored_dt != cfg.dt:
                # Half-step velocities v_{k-1/2} belong to the checkpoint's dt: synchronise
                # them with THAT dt first; the new stagger (below) then uses cfg.dt.
                self._half_kick(+1.0, stored_dt)
                self.staggered = False
            for key in ("G", "cutoff", "softening"):
                if key in c.meta and float(c.meta[key]) != float(getattr(cfg, key)):
                    warnings.warn(f"resuming a checkpoint written with {key}={c.meta[key]} "
                                  f"under {key}={getattr(cfg, key)}", stacklevel=2)
        else:
            self.engine.init_ics(cfg.init, cfg.seed)
        if cfg.integrator == "leapfrog" and not self.staggered:
            self._half_kick(-1.0)
            self.staggered = True
        elif cfg.integrator in ("kd", "hermite") and self.staggered:
            self._half_kick(+1.0)
            self.staggered = False

    def _resumed_levels(self, c) -> dict:
        """load()'s levels of a block-step run resumed from a block-step checkpoint of the same
        max_level (a shared-step checkpoint resumed with block steps starts the levels afresh)."""
        cfg = self.cfg
        if cfg.block_mode and c.meta.get("block_steps") and "level" in c.extra and \
                int(c.meta.get("max_level", -1)) == cfg.max_level:
            return {"levels": c.extra["level"][:, int(c.meta.get("level_column", 0))]}
        return {}

    def _engine_cfg(self) -> SimConfig:
        """The engine's configuration: cfg, but for the bodies a resumed merge run has left.
        Reads the checkpoint (self._resume) and the collision bookkeeping it carries."""
        cfg = self.cfg
        self.ids = np.arange(cfg.n, dtype=np.int64)  # original index of every body left
        self.mergers = self.overlaps_seen = 0
        self.closest_q_min = float("inf")
        self._resume = ckpt.load(cfg.resume) if cfg.resume else None
        c = self._resume
        if c is None or not self.hermite or "collide" not in c.extra:
            return cfg
        cols = list(c.meta.get("collide_columns", ["radius", "id"]))
        c.bodies.radius = c.extra["collide"][:, cols.index("radius")].copy()
        if cfg.collisions == "off":
            return cfg
        ids = c.extra["collide"][:, cols.index("id")].astype(np.int64)
        if c.bodies.n > cfg.n or (ids >= cfg.n).any():
            raise ValueError(f"checkpoint has n={c.bodies.n}, config n={cfg.n}")
        self.ids = ids
        self.mergers = int(c.meta.get("mergers", cfg.n - c.bodies.n))
        return cfg.replace(n=c.bodies.n, resume=None)

    def _eps2(self) -> float:
        """softening^2 as the engine's pair type holds it (the overlap threshold)."""
        e = self.cfg.softening * self.cfg.softening
        return float(e) if self.cfg.dtype == "fp64" else float(np.float32(e))

    def _note_collisions(self) -> None:
        """Fold the engine's records into the run's figures (before the engine goes)."""
        q = self.engine.closest()[0]
        if len(q):
            self.closest_q_min = min(self.closest_q_min, float(q.min()))

    def _merge(self, st) -> int:
        """Replace every set of overlapping bodies by one body and restart the engine on the
        survivors at the time reached. Returns the number of bodies absorbed."""
        from ..ops import oracle

        eng = self.engine
        b = eng.state()
        ca_q, ca_nn = eng.closest()
        self._note_collisions()
        self.overlaps_seen += st.overlaps
        pos, vel, mass, rad, ids, k = oracle.merge_overlaps(
            b.pos, b.vel, b.mass, b.radii(), self.ids, ca_q, ca_nn, eps2=self._eps2())
        if k == 0:  # (an overlap of the predicted state that the record does not hold)
            eng.clear_overlap()
            return 0
        self._steps_gone += eng.steps_done
        for key in ("block_steps", "body_steps", "level_clamped"):
            self._counts_gone[key] += getattr(st, key)
        # (pair evaluations: each engine's body-steps against the bodies it had)
        self._counts_gone["pair_evals"] += (st.body_steps - self._body_base) * eng.cfg.n
        self._body_base = 0
        self._counts_gone["level_max"] = max(self._counts_gone["level_max"], st.level_max)
        eng.close()
        self.ids, self.mergers = ids, self.mergers + k
        self.engine = self._hermite_engine(eng.cfg.replace(n=len(ids), resume=None))
        self.engine.load(BodySet(pos, vel, mass, rad), t=st.time)
        return k

    def _self_check(self) -> float:
        """Multi-rank GPU start-up (collective): the gated launch's bitwise self-check
        against the ungated schedule (runtime/selfcheck.py; the CLI's default picks overlap 3
        only if it passes, as bench.py does), or a one-step probe; both from the run's IC
        family, which the caller then (re)loads. Returns seconds per step."""
        from ..ops._native import MODE_IDS
        from .selfcheck import gated_self_check

        eng, cfg = self.engine, self.cfg

        def reload():
            eng.init_ics(cfg.init, cfg.seed)

        if eng.native_layout["mode"] == MODE_IDS["sym"] and cfg.overlap == -1 and \
                eng.overlap == 3:
            _, self.overlap_check, per_step = gated_self_check(eng, self.dist, comm, reload)
            return per_step
        reload()
        eng.sync()
        comm.barrier(self.dist)
        t0 = time.perf_counter()
        eng.step(1)
        eng.sync()
        return comm.allreduce_max(self.dist, time.perf_counter() - t0)

    @property
    def device(self) -> str:
        return self.engine.kind

    _steps_gone = 0  # steps of the engines a merger has replaced

    @property
    def step(self) -> int:
        return self.step0 + self._steps_gone + self.engine.steps_done

    def _own_accel(self) -> np.ndarray:
        """(n, 3) accelerations with this rank's rows filled (others zero)."""
        if self.hermite and self.dist.world > 1:  # (its reads return every rank's rows)
            return self.engine.derivs()[0][:, :3].copy()
        L = self.engine.layout
        acc = np.zeros((self.cfg.n, 3))
        rows = L.real_local
        if len(rows):
            acc[rows.start:rows.stop] = self.engine.accel()[: len(rows), :3]
        return acc

    def _half_kick(self, sign: float, dt: Optional[float] = None) -> None:
        """v += sign * a(x) dt/2 on every body (collective): the leapfrog stagger."""
        b = self.engine.state()
        acc = self._own_accel()
        b.vel = b.vel + sign * 0.5 * (self.cfg.dt if dt is None else dt) * acc
        if self.hermite:  # (a leapfrog checkpoint resumed under hermite: its time carries on)
            self.engine.load(b, t=self.engine.status().time)
        else:
            self.engine.load(b)

    def raw_state(self) -> BodySet:
        """Full (pos, vel as stored, mass) on every rank (collective when P > 1)."""
        b = self.engine.state()
        if self.dist.world > 1 and not self.hermite:  # (hermite: state() gathered all rows)
            rows = self.engine.layout.real_local
            comm.gather_rows_to_root(self.dist, b.vel, slice(rows.start, rows.stop))
        return b

    def global_state(self) -> BodySet:
        """Full (pos, synchronized vel, mass) on every rank (collective when P > 1)."""
        b = self.raw_state()
        if self.staggered:
            acc = self._own_accel()
            if self.dist.world > 1 and not self.hermite:
                comm.gather_rows_to_root(self.dist, acc, slice(self.engine.layout.real_local.start,
                                                               self.engine.layout.real_local.stop))
            b.vel = b.vel + 0.5 * self.cfg.dt * acc
        return b

    def conserved(self) -> dict:
        """Total energy, linear and angular momentum of the current state (collective);
        see engine_conserved."""
        return engine_conserved(self.engine, self.dist, self.step, self.staggered, self.cfg.dt)

    def structure(self, step: Optional[int] = None) -> Optional[dict]:
        """One cluster-structure sample of the current state (the bodies left after mergers):
        the k-nearest lists from the engine's device in the run's dtype, the rest on the host
        (ops/neighbours.py). Every rank reads the state as it does for a dump; rank 0 alone
        computes and returns the sample (the others None)."""
        from ..ops import neighbours

        b = self.engine.state()
        if not self.dist.is_root:
            return None
        t = self.engine.status().time if self.hermite else self.step * self.cfg.dt
        kw = {"gpu": self.engine.device} if self.engine.kind == "gpu" else {}
        out = neighbours.cluster_structure(b.pos, b.mass, self.cfg.structure_k,
                                           device=self.engine.kind, dtype=self.cfg.dtype, **kw)
        return {"step": int(self.step if step is None else step), "time": float(t), **out}

    def check_finite(self) -> None:
        bad = comm.allreduce_sum(self.dist, self.engine.nonfinite())
        if bad:
            raise NonFiniteError(f"{int(bad)} non-finite position/velocity components at step "
                                 f"{self.step}")
        if isinstance(self.engine, (HipEngine, HermiteHipEngine)) and self.dist.world > 1:
            self.engine.comm_check()

    def save_checkpoint(self, path: Optional[str] = None) -> Optional[str]:
        b = self.raw_state()
        # (hermite on P ranks: the carried a, j are gathered by every rank, the root writes)
        carried = self.engine.carried() if self.hermite else None
        if not self.dist.is_root:
            return None
        cfg = self.cfg
        path = path or ckpt.path_for(cfg.checkpoint_dir or ".", self.step)
        meta = dict(dt=cfg.dt, dtype=cfg.dtype, G=cfg.G, cutoff=cfg.cutoff,
                    softening=cfg.softening, init=cfg.init, seed=cfg.seed,
                    time=self.step * cfg.dt, integrator=cfg.integrator,
                    velocity="half-step" if self.staggered else "synchronized")
        extra = None
        if self.hermite:
            st = self.engine.status()
            extra = dict(zip(("acc", "jerk", "snap", "crackle"), carried))
            fin = lambda y: y if np.isfinite(y) else None  # noqa: E731
            meta.update(time=st.time, dt_next=fin(st.dt_next), dt_min=fin(st.dt_min),
                        eta=cfg.eta, hermite_order=cfg.hermite_order)
            if cfg.collisions != "off":
                col = np.zeros((b.n, 3))
                col[:, 0], col[:, 1] = b.radii(), self.ids
                extra["collide"] = col
                meta.update(collide_columns=["radius", "id"], mergers=self.mergers)
            if cfg.block_mode:  # (a synchronised state: every body time is st.time)
                lev = np.zeros((b.n, 3))
                lev[:, 0] = self.engine.levels()
                extra["level"] = lev
                meta.update(block_steps=True, max_level=cfg.max_level, level_column=0)
        return ckpt.save(path, b, self.step, meta, extra)

    def run(self, steps: Optional[int] = None, log: Optional[RunLog] = None) -> RunMetrics:
        cfg = self.cfg
        steps = cfg.steps if steps is None else int(steps)
        periods = [p for p in (cfg.progress_every if log else 0, cfg.checkpoint_every,
                               cfg.record_every, cfg.nan_check_every, cfg.dump_every,
                               cfg.diag_every, cfg.structure_every if cfg.structure else 0)
                   if p and p > 0]
        gpu = isinstance(self.engine, HipEngine)
        c0 = self.conserved() if cfg.diagnostics else None
        samples, diag_s = [], 0.0
        # structure samples: the start, every structure_every steps (macro steps of a block-step
        # run) short of the last, and the end; none inside the timed wall
        struct = [self.structure()] if cfg.structure else []
        timing = cfg.phase_timing and gpu
        if timing:
            self.engine.set_timing(True)
        if gpu:
            self.engine.audit_reset()
            self.engine.clock()  # (reset: the engine-clock record of this run's steps)
        # Hermite with an end time: the engine stops by itself (steps past t_end are no-ops), so
        # the host asks whether it has finished once per 32 enqueued steps and then stops
        # enqueueing; `steps` caps the count.
        ends = self.hermite and cfg.t_end is not None
        merging = self.hermite and cfg.collisions == "merge"
        self._counts_gone = dict(block_steps=0, body_steps=0, level_clamped=0, level_max=0,
                                 pair_evals=0)
        steps_gone0 = self._steps_gone
        st0 = self.engine.status() if self.hermite else None
        self._body_base = st0.body_steps if self.hermite else 0  # (of the engine now running)
        if merging and st0.overlaps:  # (bodies that overlap as the run starts: merged at once)
            self._merge(st0)
        polled = 0
        poll = 1 if cfg.block_mode else 32  # (a macro step waits for its block steps anyway)
        comm.barrier(self.dist)
        t0 = time.perf_counter()
        s = 0
        finished = False
        while s < steps and not finished:
            if log and cfg.progress_every and s % cfg.progress_every == 0 and self.dist.is_root:
                log.progress(s, steps)
            nxt = min([steps] + [(s // p + 1) * p for p in periods])
            if ends or merging:
                nxt = min(nxt, polled + poll)
            self.engine.step(nxt - s)
            s = nxt
            # (a merge run reads the status after every chunk, so that no periodic work below
            # ever sees a loop counter ahead of an engine that has stopped at an overlap)
            if merging or (ends and s - polled == poll):
                polled = s
                st = self.engine.status()
                finished = ends and st.finished
                if merging and st.overlaps:
                    # the engine stopped at the step that saw the overlap (shared step; further
                    # steps were no-ops) or stands at a macro boundary: merge there
                    # (st0.steps: what the first engine had taken before this run)
                    s = polled = self._steps_gone - steps_gone0 + st.steps - st0.steps
                    self._merge(st)
            if cfg.nan_check_every and s % cfg.nan_check_every == 0:
                self.check_finite()
            if cfg.record_every and s % cfg.record_every == 0:
                self.trajectory.append(self.raw_state().pos.copy())
            if cfg.checkpoint_every and s % cfg.checkpoint_every == 0 and cfg.checkpoint_dir:
                self.save_checkpoint()
            if cfg.dump_every and s % cfg.dump_every == 0:
                self.dump_positions()
            if cfg.diag_every and s % cfg.diag_every == 0 and s < steps:
                self.engine.sync()  # the steps so far stay inside the wall ...
                td = time.perf_counter()
                samples.append(self.conserved())
                diag_s += time.perf_counter() - td  # ... the O(N^2) sample does not
            if cfg.structure and cfg.structure_every and s % cfg.structure_every == 0 and \
                    s < steps and not finished:
                self.engine.sync()
                td = time.perf_counter()
                struct.append(self.structure())
                diag_s += time.perf_counter() - td
        self.engine.sync()
        wall = time.perf_counter() - t0 - diag_s
        wall = comm.allreduce_max(self.dist, wall)
        extra = {}
        if timing:  # the comm/compute split, max over ranks
            ph = self.engine.phase_stats()
            self.engine.set_timing(False)
            for k in ("step_ms", "comm_ms", "exposed_comm_ms", "gather_ms", "exchange_ms"):
                ph[k] = comm.allreduce_max(self.dist, ph[k])
            extra = {"phase": ph, "comm_ms": ph["comm_ms"],
                     "exposed_comm_ms": ph["exposed_comm_ms"]}
        self.check_finite()
        if gpu:
            # Work audit (as bench.py's): every sym force unit ran once per step on every rank.
            done, per = self.engine.audit()
            short = comm.allreduce_sum(self.dist, 0.0 if done == per * steps else 1.0)
            if short:
                raise RuntimeError(f"work audit: {int(short)} rank(s) ran the wrong number of "
                                   f"force units (rank {self.dist.rank}: {done} of {per * steps})")
            gi = self.engine.graph_info()
            # engine clock of the run's force launches (sym schedule; mean over ranks): the
            # clock-normalised cost next to the wall time (bench.py clock_summary)
            ghz = comm.allreduce_sum(self.dist, self.engine.clock()["ghz"]) / self.dist.world
            extra.update(engine_clock_ghz=ghz or None)
            extra.update(work_audit="ok" if per else "n/a (one-sided schedule)",
                         overlap=self.engine.overlap, graph=gi["mode"],
                         graph_segments=gi["segments"] or None,
                         overlap_check=self.overlap_check,
                         step_timeout_s=self.engine.step_timeout_s or None)
        if c0 is not None:
            extra["conservation"] = conservation_summary(c0, self.conserved(), samples)
        if cfg.structure:
            struct.append(self.structure())
        lay = getattr(self.engine, "native_layout", {})
        from ..ops._native import KERNEL_NAMES, MODE_NAMES

        herm = {}
        if self.hermite:
            st = self.engine.status()
            gone = self._counts_gone  # (of the engines that mergers have replaced)
            # the steps this run took (none past t_end or past an overlap)
            steps = self._steps_gone - steps_gone0 + st.steps - st0.steps
            herm = dict(time_reached=st.time, steps_taken=steps, hermite_order=cfg.hermite_order,
                        dt_min=st.dt_min if np.isfinite(st.dt_min) else None)
            if cfg.block_mode:
                body = gone["body_steps"] + st.body_steps - st0.body_steps
                herm.update(block_steps=gone["block_steps"] + st.block_steps - st0.block_steps,
                            body_steps=body,
                            pair_evals=gone["pair_evals"] +
                            (st.body_steps - self._body_base) * self.engine.cfg.n,
                            level_max=max(gone["level_max"], st.level_max),
                            level_clamped=gone["level_clamped"] + st.level_clamped -
                            st0.level_clamped)
            if cfg.collisions != "off":
                self._note_collisions()
                herm.update(mergers=self.mergers, bodies_left=len(self.ids),
                            closest_q_min=self.closest_q_min
                            if np.isfinite(self.closest_q_min) else None,
                            overlaps_seen=self.overlaps_seen + st.overlaps)
        return RunMetrics(n=cfg.n, steps=steps, dt=cfg.dt, dtype=cfg.dtype, device=self.device,
                          nranks=self.dist.world, wall_s=wall,
                          kernel=KERNEL_NAMES.get(lay.get("kernel", 0), "cpu"),
                          mode=MODE_NAMES.get(lay.get("mode", 0), "cpu"), extra=extra,
                          structure={"k": cfg.structure_k, "samples": struct}
                          if cfg.structure and self.dist.is_root else None, **herm)

    def dump_path_for(self, step: int) -> str:
        cfg = self.cfg
        if cfg.dump_path and not cfg.dump_path.endswith(".gsck"):
            stem, ext = os.path.splitext(cfg.dump_path)
            return f"{stem}_step{step:08d}{ext or '.txt'}"
        return os.path.join(cfg.log_dir or ".", f"positions_step{step:08d}.txt")

    def dump_positions(self, path: Optional[str] = None) -> Optional[str]:
        """Periodic text dump of all positions in the mpi.c format (mpi.c:249-257);
        collective, rank 0 writes."""
        from ..utils.logs import format_positions_mpi

        b = self.raw_state()
        if not self.dist.is_root:
            return None
        path = path or self.dump_path_for(self.step)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(format_positions_mpi(b.pos[: self.cfg.n]))
        return path

    def save_trajectory(self, path: str) -> None:
        if self.dist.is_root and self.trajectory:
            np.save(path, np.stack(self.trajectory))

    def close(self) -> None:
        self.engine.close()
