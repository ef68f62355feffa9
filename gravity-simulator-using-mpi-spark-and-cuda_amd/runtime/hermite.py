"""Engines of the Hermite integrators: 4th order (Makino & Aarseth 1992) and 6th order.

The same interface as the engines of runtime/engines.py (load / init_ics / step / sync / state /
accel / nonfinite / steps_done / close) plus status(): the integrator carries x, v, a, j, t and
the next step size, so the time reached is the engine's, not step * dt.

* HermiteHipEngine: the native gs_hermite object (csrc/hip/hermite.hip): device-resident state,
  the acceleration+jerk kernel of csrc/hip/nbody_hermite.hip, the step size chosen on the device.
  With nranks > 1 (shared steps only) a rank owns whole units of 1024 rows
  (parallel/partition.py hermite_partition), predicts, evaluates and corrects them against all j
  and gathers the predicted rows and the step minima over RCCL every step (comm_init); every
  rank then holds the same time and step size, state() / carried() / derivs() return all n rows
  on every rank (collectives), and the run equals the one-rank run bit for bit.
* HermiteVirtualGroup: the P shards of such a run in one process on one device, the gathers done
  by device copies (gs_hermite_group_*): the same kernels and schedule without RCCL.
* HermiteCpuEngine: the native C++/OpenMP step (csrc/cpu/cpu_engine.cpp gs_cpu_hermite_step_*).

dtype "mixed": both engines hold x, v, a, j in fp64 and predict, correct and choose steps in fp64;
only the pair sums are fp32, on positions handed over as double-single (hi, lo) pairs, so that
the separation of two close bodies far from the origin keeps its digits.

One step of size h: predict xp = x + v h + a h^2/2 + j h^3/6, vp = v + a h + j h^2/2; evaluate
a1, j1 at (xp, vp); correct v1 = v + (a + a1) h/2 + (j - j1) h^2/12,
x1 = x + (v + v1) h/2 + (a - a1) h^2/12; a1, j1 become the next step's a, j. With eta > 0 every
step takes h = min(dt, min_i dt_i) of Aarseth's criterion; with t_end set the last step is cut
to reach it exactly and further steps are no-ops.

Order 6 (cfg.hermite_order; Nitadori & Makino 2008): the state also carries the snap s and the
crackle c, the predictor runs to h^5 in x and also predicts a, the one evaluation returns a1, j1
and s1 at (xp, vp, ap), and the corrector is v1 = v + (a + a1) h/2 - (j1 - j) h^2/10 +
(s + s1) h^3/120, x1 likewise from v, a, j (ops/oracle.py simulate_hermite6). eta enters its step
criterion linearly (0.2 to 0.5). load() then also takes snap and crackle, carried() returns
(acc, jerk, snap, crackle) and derivs() (a4, j4, s4). fp32 or fp64, one rank; one shared step, or
(fp64 only, cfg.block_steps6) block mode: the block step below with the order-6 predictor, evaluation, corrector
and criterion (ops/oracle.py simulate_hermite6_block).

Block mode (cfg.block_steps; Makino 1991): body i steps by dt 2^-k_i, time is an integer count
of ticks of dt 2^-max_level, and a block step predicts every body to the earliest due time,
evaluates the due bodies against all and corrects them (the rules: ops/oracle.py
simulate_hermite_block). step(n) then advances n macro steps of dt, after each of which all
bodies stand at the same time.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..config import SimConfig
from ..models.initial_conditions import DEVICE_IC_IDS, BodySet, make
from ..ops import _native
from ..parallel.partition import Layout, hermite_layout, layout as make_layout


@dataclass
class HermiteStatus:
    time: float       # time reached [s]
    dt_last: float    # size of the last step taken (0 before the first)
    dt_next: float    # min(dt, min_i dt_i): the next step before the t_end cut
    dt_min: float     # smallest step so far (inf before the first; a last step cut short by
                      # t_end is not counted)
    steps: int        # steps taken (steps enqueued past t_end are no-ops, not counted)
    finished: bool    # t_end is set and reached
    # block mode (`steps` then counts macro steps of dt; 0 otherwise)
    block_steps: int = 0     # block steps taken
    body_steps: int = 0      # sum of their active bodies
    level_max: int = 0       # deepest level any body has had
    level_clamped: int = 0   # times a body wanted a step below dt 2^-max_level
    overlaps: int = 0        # collisions: bodies the evaluations have seen overlapping their
                             # nearest neighbour

PATH_IDS = {None: 0, "auto": 0, "narrow": 1, "wide": 2}
# native collision modes: record only, or record and stop the shared step at the first overlap
# (what a merge needs: the bodies of a shared-step run all stand at that step's time)
COLLISION_IDS = {"off": 0, "detect": 1, "merge": 2}
_PI32 = ctypes.POINTER(ctypes.c_int32)


def _i32ptr(a):
    return a.ctypes.data_as(_PI32)


def _reported(dt: Optional[float]) -> float:
    """A step size a status() reported, as the native set_state takes it (-1: none)."""
    return float(dt) if dt is not None and math.isfinite(dt) else -1.0


def _require_one_rank(nranks: int) -> None:
    if nranks != 1:
        raise ValueError("hermite runs on one rank on the CPU (--device cpu)")


class HermiteHipEngine:
    """GPU engine: one native gs_hermite per process (rank `rank` of `nranks`)."""

    kind = "gpu"
    gathers_all = True  # state(), carried() and derivs() return every rank's rows

    def __init__(self, cfg: SimConfig, rank: int = 0, nranks: int = 1, device: int = 0,
                 dist=None):
        from .engines import _gs_config

        if nranks > 1:  # (the refusals of SimConfig.validate for a run launched with P ranks)
            cfg.replace(gpus=nranks, device="gpu").validate()
        self.cfg = cfg
        self.rank, self.nranks, self.device, self.dist = rank, nranks, device, dist
        self.layout: Layout = hermite_layout(cfg.n, rank, nranks, cfg.chunk)
        self.step_timeout_s = 0.0
        self.lib = _native.hip_lib()
        c = _gs_config(cfg.replace(kernel="auto", mode="auto"), rank, nranks, device)
        self._h = ctypes.c_void_p()
        _native.check(self.lib, self.lib.gs_hermite_create(ctypes.byref(c), ctypes.byref(self._h)),
                      "gs_hermite_create")
        L = _native.GsLayout()
        _native.check(self.lib, self.lib.gs_hermite_layout(self._h, ctypes.byref(L)), "layout")
        self.native_layout = L.as_dict()
        assert (self.layout.n_pad, self.layout.local_begin, self.layout.n_local) == \
            (L.n_pad, L.local_begin, L.n_local), "Python layout mirror disagrees with native"
        _native.check(self.lib, self.lib.gs_hermite_set_adaptive(
            self._h, float(cfg.eta), float(cfg.dt),
            -1.0 if cfg.t_end is None else float(cfg.t_end)), "set_adaptive")
        self.order = int(cfg.hermite_order)
        if self.order == 6:
            _native.check(self.lib, self.lib.gs_hermite_set_order(self._h, 6), "set_order")
            _native.check(self.lib, self.lib.gs_hermite_layout(self._h, ctypes.byref(L)), "layout")
            self.native_layout = L.as_dict()
        self.block = cfg.block_mode
        if self.block:  # (order 6: its own entry; gs_hermite_set_block refuses it)
            set_block = self.lib.gs_hermite_set_block6 if cfg.block_steps6 else \
                self.lib.gs_hermite_set_block
            _native.check(self.lib, set_block(self._h, 1, int(cfg.max_level)), "set_block")
        self.collisions = cfg.collisions != "off"
        if self.collisions:
            _native.check(self.lib, self.lib.gs_hermite_set_collisions(
                self._h, COLLISION_IDS[cfg.collisions]), "set_collisions")
            # (mixed runs 2 bodies per lane with collisions on: the layout says what runs)
            _native.check(self.lib, self.lib.gs_hermite_layout(self._h, ctypes.byref(L)), "layout")
            self.native_layout = L.as_dict()
        self.radius = np.zeros(cfg.n)

    def _need_collisions(self) -> None:
        if not self.collisions:
            raise ValueError("collisions are off (SimConfig.collisions)")

    def neighbours(self) -> tuple[np.ndarray, np.ndarray]:
        """(q, nn) of every body from its latest evaluation: q = r^2 - (R_i + R_nn)^2 of the
        nearest neighbour nn ((+inf, -1): none). Waits for the enqueued steps."""
        self._need_collisions()
        q, nn = np.zeros(self.cfg.n), np.zeros(self.cfg.n, dtype=np.int32)
        _native.check(self.lib, self.lib.gs_hermite_neighbours(self._h, _native.dptr(q),
                                                               _i32ptr(nn)), "neighbours")
        return q, nn

    def closest(self, clear: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """The closest-approach record (min q per body, the neighbour then) since the state was
        set or the record last cleared."""
        self._need_collisions()
        q, nn = np.zeros(self.cfg.n), np.zeros(self.cfg.n, dtype=np.int32)
        _native.check(self.lib, self.lib.gs_hermite_closest(self._h, _native.dptr(q), _i32ptr(nn),
                                                            int(bool(clear))), "closest")
        return q, nn

    def clear_overlap(self) -> None:
        _native.check(self.lib, self.lib.gs_hermite_clear_overlap(self._h), "clear_overlap")

    def derivs_nn(self, active=None, path: Optional[str] = None):
        """derivs() with (q, nn) of each row as well: (a4, j4, q, nn). It touches neither the
        records nor the overlap count."""
        self._need_collisions()
        if active is not None:
            idx = np.ascontiguousarray(active, dtype=np.int32)
            m = len(idx)
            a4, j4, q, nn = np.zeros((m, 4)), np.zeros((m, 4)), np.zeros(m), np.zeros(m, np.int32)
            _native.check(self.lib, self.lib.gs_hermite_derivs_active_nn(
                self._h, _i32ptr(idx), m, PATH_IDS[path], _native.dptr(a4), _native.dptr(j4),
                _native.dptr(q), _i32ptr(nn)), "derivs_active_nn")
            return a4, j4, q, nn
        n = self.cfg.n
        a4, j4, q, nn = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros(n), np.zeros(n, np.int32)
        _native.check(self.lib, self.lib.gs_hermite_derivs_nn(
            self._h, _native.dptr(a4), _native.dptr(j4), _native.dptr(q), _i32ptr(nn)),
            "derivs_nn")
        return a4, j4, q, nn

    def set_block_tuning(self, narrow_max: int = -1) -> None:
        """Active sets up to narrow_max bodies take the j-parallel evaluate kernel (0: never;
        n: always; -1: the default for n and dtype). It changes the summation order."""
        _native.check(self.lib, self.lib.gs_hermite_set_block_tuning(self._h, int(narrow_max)),
                      "set_block_tuning")

    def status_narrow_max(self) -> int:
        s = _native.GsHermiteInfo()
        _native.check(self.lib, self.lib.gs_hermite_status(self._h, ctypes.byref(s)), "status")
        return int(s.narrow_max)

    def levels(self) -> np.ndarray:
        lev = np.zeros(self.cfg.n, dtype=np.int32)
        _native.check(self.lib, self.lib.gs_hermite_get_block_state(
            self._h, None, lev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "get_block_state")
        return lev

    def body_times(self) -> np.ndarray:
        """Per-body time in ticks of dt 2^-max_level."""
        tb = np.zeros(self.cfg.n, dtype=np.int64)
        _native.check(self.lib, self.lib.gs_hermite_get_block_state(
            self._h, tb.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None), "get_block_state")
        return tb

    def init_ics(self, family: str, seed: int) -> None:
        if family in DEVICE_IC_IDS and not self.collisions:
            _native.check(self.lib, self.lib.gs_hermite_init_ics(self._h, DEVICE_IC_IDS[family],
                                                                 seed), "init_ics")
        else:
            self.load(make(family, self.cfg.n, seed, self.cfg.G))

    def load(self, b: BodySet, acc=None, jerk=None, t: float = 0.0,
             dt_next: Optional[float] = None, dt_min: Optional[float] = None,
             levels=None, body_times=None, snap=None, crackle=None) -> None:
        """Set the state at time t. acc, jerk None: evaluated from (pos, vel); given (with the
        dt_next and dt_min a status() reported): a run continues as if never interrupted.
        Block mode: t is a whole multiple of dt; levels (and body_times, ticks) None: afresh.
        Order 6: a run continues only with all of acc, jerk, snap, crackle; else all afresh."""
        pos = np.ascontiguousarray(b.pos, dtype=np.float64)
        vel = np.ascontiguousarray(b.vel, dtype=np.float64)
        mass = np.ascontiguousarray(b.mass, dtype=np.float64)
        # the carried rows of the run's order: it continues only with every one of them
        rows = [acc, jerk, snap, crackle] if self.order == 6 else [acc, jerk]
        have = all(y is not None for y in rows)
        rows = [np.ascontiguousarray(y, dtype=np.float64) if have else None for y in rows]
        if self.collisions:
            self.radius = np.ascontiguousarray(b.radii(self.cfg.body_density), dtype=np.float64)
            _native.check(self.lib, self.lib.gs_hermite_set_radii(
                self._h, _native.dptr(self.radius)), "set_radii")
        name = "set_state6" if self.order == 6 else "set_state"
        _native.check(self.lib, getattr(self.lib, "gs_hermite_" + name)(
            self._h, _native.dptr(pos), _native.dptr(vel), _native.dptr(mass),
            *[_native.dptr(y) if have else None for y in rows], float(t),
            _reported(dt_next), _reported(dt_min)), name)
        if self.block and (levels is not None or body_times is not None):
            lev = None if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
            tb = None if body_times is None else np.ascontiguousarray(body_times, dtype=np.int64)
            _native.check(self.lib, self.lib.gs_hermite_set_block_state(
                self._h,
                None if tb is None else tb.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                None if lev is None else lev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                "set_block_state")

    def comm_init(self, uid: bytes) -> None:
        """Form the RCCL communicator of a multi-rank run (collective; before the state)."""
        buf = ctypes.create_string_buffer(uid, 128)
        self._comm = "in comm_init"
        _native.check(self.lib, self.lib.gs_hermite_comm_init(self._h, buf, self.rank,
                                                              self.nranks), "comm_init")
        self._comm = "done"

    def comm_info(self) -> dict:
        """What RCCL formed for this rank (as HipEngine.comm_info): rccl_nranks 0 when no
        communicator is held."""
        c, r, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _native.check(self.lib, self.lib.gs_hermite_comm_info(
            self._h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(d)), "comm info")
        return {"rccl_nranks": c.value, "rccl_rank": r.value, "rccl_device": d.value}

    def comm_check(self) -> None:
        _native.check(self.lib, self.lib.gs_hermite_comm_check(self._h), "rccl health")

    def set_step_timeout(self, seconds: float) -> None:
        """sync() aborts the communicator when no step completes for this long (0: unbounded)."""
        self.step_timeout_s = float(seconds)
        _native.check(self.lib, self.lib.gs_hermite_set_step_timeout(self._h, float(seconds)),
                      "set_step_timeout")

    _comm = "not started"

    def abort(self) -> bool:
        """The run guard's abort hook: ncclCommAbort the live communicator once (True if one was
        aborted). One rank holds none, so there is nothing to abort (the guard's stage deadline
        still ends the job)."""
        return self.nranks > 1 and bool(self._h) and bool(self.lib.gs_hermite_abort(self._h))

    def comm_stage(self) -> str:
        """The run guard's probe (HipEngine.comm_stage)."""
        return self._comm if self.nranks > 1 else "no communicator (one rank)"

    def step(self, n: int) -> None:
        if n > 0:
            _native.check(self.lib, self.lib.gs_hermite_step(self._h, int(n)), "step")

    def sync(self, timeout_s: float = 0.0) -> None:
        _native.check(self.lib, self.lib.gs_hermite_sync(self._h), "sync")

    def status(self) -> HermiteStatus:
        """Waits for the enqueued steps."""
        s = _native.GsHermiteInfo()
        _native.check(self.lib, self.lib.gs_hermite_status(self._h, ctypes.byref(s)), "status")
        return HermiteStatus(s.time, s.dt_last, s.dt_next, s.dt_min, int(s.steps),
                             bool(s.finished), int(s.block_steps), int(s.body_steps),
                             int(s.level_max), int(s.level_clamped), int(s.overlaps))

    def _get(self, want_deriv: bool):
        n = self.cfg.n
        pos, vel, mass = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        acc = np.zeros((n, 3)) if want_deriv else None
        jerk = np.zeros((n, 3)) if want_deriv else None
        _native.check(self.lib, self.lib.gs_hermite_get_state(
            self._h, _native.dptr(pos), _native.dptr(vel), _native.dptr(mass),
            _native.dptr(acc) if want_deriv else None, _native.dptr(jerk) if want_deriv else None),
            "get_state")
        return BodySet(pos, vel, mass, self.radius.copy() if self.collisions else None), acc, jerk

    def state(self) -> BodySet:
        return self._get(False)[0]

    def carried(self):
        """(acc, jerk) (n, 3) as the integrator carries them (evaluated at the last predicted
        state): what a checkpoint keeps so that a resumed run is bit-exact. Order 6:
        (acc, jerk, snap, crackle)."""
        _, a, j = self._get(True)
        if self.order == 6:
            s, c = np.zeros((self.cfg.n, 3)), np.zeros((self.cfg.n, 3))
            _native.check(self.lib, self.lib.gs_hermite_get_carried6(
                self._h, _native.dptr(s), _native.dptr(c)), "get_carried6")
            return a, j, s, c
        return a, j

    def derivs(self, active=None, path: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
        """(n, 4) (ax, ay, az, phi) and (jx, jy, jz, 0) of the current (x, v), through the
        step's own kernel. Block mode, active = body indices: their rows only, through the block
        path's evaluate and reduce (path "narrow", "wide" or None: by narrow_max). Order 6:
        (a4, j4, s4), for active bodies in one pass at the rows (x, v, carried a)."""
        if active is not None and self.order == 6:
            idx = np.ascontiguousarray(active, dtype=np.int32)
            a4, j4, s4 = (np.zeros((len(idx), 4)) for _ in range(3))
            _native.check(self.lib, self.lib.gs_hermite_derivs_active6(
                self._h, _i32ptr(idx), len(idx), PATH_IDS[path], _native.dptr(a4),
                _native.dptr(j4), _native.dptr(s4)), "derivs_active6")
            return a4, j4, s4
        if active is not None:
            idx = np.ascontiguousarray(active, dtype=np.int32)
            a4, j4 = np.zeros((len(idx), 4)), np.zeros((len(idx), 4))
            _native.check(self.lib, self.lib.gs_hermite_derivs_active(
                self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(idx),
                PATH_IDS[path], _native.dptr(a4), _native.dptr(j4)), "derivs_active")
            return a4, j4
        n = self.cfg.n
        a4, j4 = np.zeros((n, 4)), np.zeros((n, 4))
        if self.order == 6:  # (and the snap at that acceleration: (a4, j4, s4))
            s4 = np.zeros((n, 4))
            _native.check(self.lib, self.lib.gs_hermite_derivs6(
                self._h, _native.dptr(a4), _native.dptr(j4), _native.dptr(s4)), "derivs6")
            return a4, j4, s4
        _native.check(self.lib, self.lib.gs_hermite_derivs(self._h, _native.dptr(a4),
                                                           _native.dptr(j4)), "derivs")
        return a4, j4

    def time_active(self, active, path: str, reps: int = 10) -> float:
        """Milliseconds per evaluate + reduce of the listed bodies on one block path (device
        events around `reps` back-to-back launches)."""
        idx = np.ascontiguousarray(active, dtype=np.int32)
        ms = ctypes.c_double(0.0)
        if self.order == 6:
            _native.check(self.lib, self.lib.gs_hermite_time_active6(
                self._h, _i32ptr(idx), len(idx), PATH_IDS[path], int(reps), ctypes.byref(ms),
                None, None, None), "time_active6")
            return ms.value
        _native.check(self.lib, self.lib.gs_hermite_time_active(
            self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(idx), PATH_IDS[path],
            int(reps), ctypes.byref(ms), None, None), "time_active")
        return ms.value

    def accel(self, step_path: bool = False) -> np.ndarray:
        """(n_local, 4) = (ax, ay, az, phi) of the rows this rank owns, ghost rows zero
        (collective when nranks > 1)."""
        out = np.zeros((self.layout.n_local, 4))
        rows = self.layout.real_local
        out[: len(rows)] = self.derivs()[0][rows.start:rows.stop]
        return out

    def nonfinite(self) -> int:
        r = int(self.lib.gs_hermite_count_nonfinite(self._h))
        if r < 0:
            raise RuntimeError("nonfinite check failed: " + self.lib.gs_last_error().decode())
        return r

    @property
    def steps_done(self) -> int:
        return self.status().steps

    def close(self) -> None:
        if self._h:
            self.lib.gs_hermite_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HermiteVirtualGroup:
    """The P ranks of a shared-step run as shards of one process on one device: every shard is
    a HermiteHipEngine of rank r of P and runs the slice kernels and the control kernel of the
    RCCL path; the gathers are device copies between the shards' arrays. The reads return all n
    rows. For tests and for bench/hermite_rate.py --ranks."""

    kind = "gpu"

    def __init__(self, cfg: SimConfig, nranks: int, device: int = 0, order=None):
        self.cfg, self.nranks = cfg, int(nranks)
        self.shards: list[HermiteHipEngine] = []
        try:
            for r in range(self.nranks):
                self.shards.append(HermiteHipEngine(cfg, r, self.nranks, device))
        except Exception:
            self.close()
            raise
        self.lib = self.shards[0].lib
        # (order: a test passes the shards to the native group in another order)
        idx = list(range(self.nranks)) if order is None else list(order)
        self._arr = (ctypes.c_void_p * self.nranks)(*[self.shards[i]._h for i in idx])

    @property
    def layouts(self) -> list[Layout]:
        return [e.layout for e in self.shards]

    def _finish_start(self) -> None:
        _native.check(self.lib, self.lib.gs_hermite_group_step(self._arr, self.nranks, 0),
                      "group start")

    def init_ics(self, family: str, seed: int) -> None:
        for e in self.shards:
            e.init_ics(family, seed)
        self._finish_start()

    def load(self, b: BodySet, acc=None, jerk=None, t: float = 0.0,
             dt_next: Optional[float] = None, dt_min: Optional[float] = None) -> None:
        for e in self.shards:
            e.load(b, acc, jerk, t=t, dt_next=dt_next, dt_min=dt_min)
        self._finish_start()

    def step(self, n: int) -> None:
        if n > 0:
            _native.check(self.lib, self.lib.gs_hermite_group_step(self._arr, self.nranks, int(n)),
                          "group step")

    def sync(self, timeout_s: float = 0.0) -> None:
        for e in self.shards:
            e.sync()

    def statuses(self) -> list[HermiteStatus]:
        """Every shard's own control block (they are equal); waits for the enqueued steps."""
        return [e.status() for e in self.shards]

    def status(self) -> HermiteStatus:
        return self.shards[0].status()

    def _get(self, want_deriv: bool):
        n = self.cfg.n
        pos, vel, mass = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        acc = np.zeros((n, 3)) if want_deriv else None
        jerk = np.zeros((n, 3)) if want_deriv else None
        _native.check(self.lib, self.lib.gs_hermite_group_get_state(
            self._arr, self.nranks, _native.dptr(pos), _native.dptr(vel), _native.dptr(mass),
            _native.dptr(acc) if want_deriv else None, _native.dptr(jerk) if want_deriv else None),
            "group get_state")
        return BodySet(pos, vel, mass), acc, jerk

    def state(self) -> BodySet:
        return self._get(False)[0]

    def carried(self) -> tuple[np.ndarray, np.ndarray]:
        _, a, j = self._get(True)
        return a, j

    def derivs(self) -> tuple[np.ndarray, np.ndarray]:
        n = self.cfg.n
        a4, j4 = np.zeros((n, 4)), np.zeros((n, 4))
        _native.check(self.lib, self.lib.gs_hermite_group_derivs(
            self._arr, self.nranks, _native.dptr(a4), _native.dptr(j4)), "group derivs")
        return a4, j4

    def time_eval(self, reps: int = 10) -> list[float]:
        """Milliseconds per evaluate launch of each shard, one shard at a time."""
        ms = np.zeros(self.nranks)
        _native.check(self.lib, self.lib.gs_hermite_group_time_eval(
            self._arr, self.nranks, int(reps), _native.dptr(ms)), "group time_eval")
        return [float(x) for x in ms]

    @property
    def steps_done(self) -> int:
        return self.status().steps

    def close(self) -> None:
        for e in self.shards:
            e.close()
        self.shards = []


class HermiteCpuEngine:
    """Native CPU engine: gs_cpu_hermite_step_* per step; the step-size bookkeeping (a few
    scalars) stays in Python."""

    kind = "cpu"

    def __init__(self, cfg: SimConfig, rank: int = 0, nranks: int = 1):
        _require_one_rank(nranks)
        self.cfg = cfg
        self.rank, self.nranks = 0, 1
        self.lib = _native.cpu_lib()
        self.layout: Layout = make_layout(cfg.n, 0, 1, cfg.chunk)
        self.np_dtype = np.float32 if cfg.dtype == "fp32" else np.float64  # (mixed: fp64 arrays)
        n, T = cfg.n, self.np_dtype
        self.order = int(cfg.hermite_order)
        six = self.order == 6
        if six:  # (the refusals of SimConfig.validate for a bare engine)
            cfg.validate()
        self.X, self.V = np.zeros((n, 4), T), np.zeros((n, 4), T)
        # the rows the integrator carries beside x, v: (A, J), order 6 (A, J, S, C); the native
        # step takes them in this order and a scratch of the predicted and the new rows
        self._rows = [np.zeros((n, 4), T) for _ in range(4 if six else 2)]
        self.A, self.J = self._rows[:2]
        self._scratch = np.zeros(((6 if six else 4) * n, 4), T)
        self.mass = np.zeros(n)
        self._step, self._ptr = _native.cpu_entry(
            self.lib, "hermite6_step" if six else "hermite_step", cfg.dtype)
        if six:
            self.S, self.C = self._rows[2:]
            self._ajs = _native.cpu_entry(self.lib, "accjerksnap", cfg.dtype)[0]
            self._ajs_idx = self.lib.gs_cpu_accjerksnap_idx_f64  # (block steps: fp64 only)
        self._accjerk, self._accjerk_idx, self._first_dt, self._nn, self._nn_idx = (
            _native.cpu_entry(self.lib, stem, cfg.dtype)[0]
            for stem in ("accjerk", "accjerk_idx", "hermite_first_dt", "nn", "nn_idx"))
        self.block = cfg.block_mode
        self.L = int(cfg.max_level)
        self.tb = np.zeros(n, dtype=np.int64)       # body times [ticks of dt 2^-L]
        self.lev = np.zeros(n, dtype=np.int32)
        self.block_log: list[tuple[int, int]] = []  # (t_ticks, n_active) per block step
        self.body_steps = self.level_clamped = self.level_max = 0
        self._macro0 = 0
        self._cut2 = T(cfg.cutoff ** 2)
        self._eps2 = T(cfg.softening ** 2)
        self.t, self.dt_last, self.dt_min, self.k = 0.0, 0.0, math.inf, 0
        self._next = math.inf  # min_i dt_i of the last step (adaptive)
        # collisions: the records of the GPU engine (latest and closest (q, nn), overlap count)
        self.collisions = cfg.collisions != "off"
        self.radius = np.zeros(n)
        self._R = np.zeros(n, T)
        self._clear_records()
        if cfg.threads:
            self.lib.gs_cpu_set_threads(int(cfg.threads))

    def init_ics(self, family: str, seed: int) -> None:
        self.load(make(family, self.cfg.n, seed, self.cfg.G))

    def _need_collisions(self) -> None:
        if not self.collisions:
            raise ValueError("collisions are off (SimConfig.collisions)")

    def _clear_records(self) -> None:
        n = self.cfg.n
        self.q, self.nn = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        self.ca_q, self.ca_nn = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        self.overlaps = 0

    def _nearest(self, X, idx=None) -> tuple[np.ndarray, np.ndarray]:
        """(q, nn) of all bodies (or of idx) at the rows X, in the run's pair arithmetic."""
        n, T = self.cfg.n, self.np_dtype
        m = n if idx is None else len(idx)
        q, nn = np.zeros(m, T), np.zeros(m, dtype=np.int32)
        if idx is None:
            rc = self._nn(self._ptr(X), self._ptr(self._R), n, 0, n, self._cut2, self._eps2,
                          self._ptr(q), _i32ptr(nn))
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            rc = self._nn_idx(self._ptr(X), self._ptr(self._R), n, _i32ptr(idx), m, self._cut2,
                              self._eps2, self._ptr(q), _i32ptr(nn))
        _native.check(self.lib, rc, "cpu nn")
        return q, nn

    def _see(self, X, idx=None) -> None:
        """Record an evaluation at the rows X (of every body, or of the bodies idx)."""
        q, nn = self._nearest(X, idx)
        r = slice(None) if idx is None else idx
        # the overlap test in the pair type (fp32 runs: q and eps2 in fp32; mixed: q is an fp32
        # value and eps2 rounds to fp32 as on the GPU)
        eps2 = np.float32(self._eps2) if self.cfg.dtype != "fp64" else self._eps2
        self.overlaps += int((q < eps2).sum())
        q = q.astype(np.float64)
        self.q[r], self.nn[r] = q, nn
        less = q < self.ca_q[r]
        self.ca_q[r] = np.where(less, q, self.ca_q[r])
        self.ca_nn[r] = np.where(less, nn, self.ca_nn[r])

    def neighbours(self) -> tuple[np.ndarray, np.ndarray]:
        self._need_collisions()
        return self.q.copy(), self.nn.copy()

    def closest(self, clear: bool = False) -> tuple[np.ndarray, np.ndarray]:
        self._need_collisions()
        out = self.ca_q.copy(), self.ca_nn.copy()
        if clear:
            self.ca_q[:], self.ca_nn[:] = np.inf, -1
        return out

    def clear_overlap(self) -> None:
        self.overlaps = 0

    def derivs_nn(self, active=None, path: Optional[str] = None):
        self._need_collisions()
        a4, j4 = self.derivs(active)
        q, nn = self._nearest(self.X, active)
        return a4, j4, q.astype(np.float64), nn

    def _derivs6(self):
        """(a4, j4, s4) of the current (x, v) in the two passes a 6th-order run starts with:
        ap = 0 for a, then ap = a for the snap."""
        n, T = self.cfg.n, self.np_dtype
        a4, j4, s4 = np.zeros((n, 4), T), np.zeros((n, 4), T), np.zeros((n, 4), T)
        ap = np.zeros((n, 4), T)
        for _ in range(2):
            rc = self._ajs(self._ptr(self.X), self._ptr(self.V), self._ptr(ap), n, 0, n,
                           self.layout.chunk, self._cut2, self._eps2, self._ptr(a4),
                           self._ptr(j4), self._ptr(s4))
            _native.check(self.lib, rc, "cpu accjerksnap")
            ap = a4.copy()
        return a4, j4, s4

    def _derivs(self) -> tuple[np.ndarray, np.ndarray]:
        n, T = self.cfg.n, self.np_dtype
        a4, j4 = np.zeros((n, 4), T), np.zeros((n, 4), T)
        rc = self._accjerk(self._ptr(self.X), self._ptr(self.V), n, 0, n, self.layout.chunk,
                           self._cut2, self._eps2, self._ptr(a4), self._ptr(j4))
        _native.check(self.lib, rc, "cpu accjerk")
        return a4, j4

    def _derivs_idx(self, X, V, idx) -> tuple[np.ndarray, np.ndarray]:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        a4, j4 = np.zeros((len(idx), 4), self.np_dtype), np.zeros((len(idx), 4), self.np_dtype)
        rc = self._accjerk_idx(self._ptr(X), self._ptr(V), self.cfg.n,
                               idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(idx),
                               self.layout.chunk, self._cut2, self._eps2, self._ptr(a4),
                               self._ptr(j4))
        _native.check(self.lib, rc, "cpu accjerk_idx")
        return a4, j4

    def levels(self) -> np.ndarray:
        return self.lev.copy()

    def body_times(self) -> np.ndarray:
        return self.tb.copy()

    def _block_start(self, t: float, levels=None, body_times=None) -> None:
        from ..ops import oracle

        cfg = self.cfg
        macro = int(round(t / cfg.dt))
        if macro * cfg.dt != t:
            raise ValueError("block steps: the state's time must be a whole multiple of dt")
        self._macro0 = macro
        self.block_log, self.body_steps, self.level_clamped = [], 0, 0
        self.lev = (np.array(levels, dtype=np.int32) if levels is not None else
                    oracle.block_first_levels(self.A[:, :3].astype(np.float64),
                                              self.J[:, :3].astype(np.float64), cfg.dt, cfg.eta,
                                              self.L))
        self.tb = (np.array(body_times, dtype=np.int64) if body_times is not None else
                   np.full(cfg.n, macro << self.L, dtype=np.int64))
        if (self.lev < 0).any() or (self.lev > self.L).any() or \
                (self.tb % (np.int64(1) << (self.L - self.lev).astype(np.int64))).any():
            raise ValueError("block state: level out of 0..max_level, or a body time that is no "
                             "multiple of its step")
        self.level_max = int(self.lev.max())

    def _block_step(self) -> None:
        """One block step: the schedule and the level rule of oracle._simulate_block around the
        order's own predict, evaluate and correct in the run's dtype (_advance4, _advance6)."""
        from ..ops import oracle

        cfg, L = self.cfg, self.L
        stp = np.int64(1) << (L - self.lev).astype(np.int64)
        t_next = int((self.tb + stp).min())
        act = np.nonzero(self.tb + stp == t_next)[0]
        hd = cfg.dt * np.ldexp((t_next - self.tb).astype(np.float64), -L)
        want, valid = (self._advance6 if self.order == 6 else self._advance4)(act, hd)
        self.tb[act] = t_next
        self.lev[act], hit = oracle.block_new_levels(self.lev[act], want, valid, t_next, cfg.dt, L)
        self.level_clamped += int(hit.sum())
        self.level_max = max(self.level_max, int(self.lev.max()))
        self.body_steps += len(act)
        self.block_log.append((t_next, len(act)))

    def _advance4(self, act, hd):
        """Order 4: the bodies `act` over the steps hd (n,) from every body's own time; the step
        each wants (the rules of oracle.simulate_hermite_block)."""
        from ..ops import oracle

        T = self.np_dtype
        h = hd.astype(T)[:, None]
        x, v, a, j = self.X[:, :3], self.V[:, :3], self.A[:, :3], self.J[:, :3]
        XP, VP = self.X.copy(), np.zeros_like(self.V)
        XP[:, :3] = x + (v * h + (a * ((h * h) / T(2)) + j * ((h * h * h) / T(6))))
        VP[:, :3] = v + (a * h + j * ((h * h) / T(2)))
        a4, j4 = self._derivs_idx(XP, VP, act)
        if self.collisions:
            self._see(XP, act)
        a1, j1 = a4[:, :3], j4[:, :3]
        ha = h[act]
        a0, j0, v0 = a[act], j[act], v[act]
        v1 = v0 + ((a0 + a1) * (ha / T(2)) + (j0 - j1) * ((ha * ha) / T(12)))
        self.X[act, :3] = x[act] + ((v0 + v1) * (ha / T(2)) + (a0 - a1) * ((ha * ha) / T(12)))
        self.V[act, :3], self.A[act, :3], self.J[act, :3] = v1, a1, j1
        return oracle.hermite_dt_bodies(a0.astype(np.float64), j0.astype(np.float64),
                                        a1.astype(np.float64), j1.astype(np.float64),
                                        hd[act], self.cfg.eta)

    def _advance6(self, act, hd):
        """Order 6 (fp64), as _advance4 (the rules of oracle.simulate_hermite6_block)."""
        from ..ops import oracle

        n = self.cfg.n
        h = hd[:, None]
        h2, h3, h4, h5 = (h * h) / 2, (h * h * h) / 6, (h * h * h * h) / 24, \
            (h * h * h * h * h) / 120
        x, v, a, j, s, c = (y[:, :3] for y in (self.X, self.V, self.A, self.J, self.S, self.C))
        XP, VP, AP = self.X.copy(), np.zeros_like(self.V), np.zeros_like(self.V)
        XP[:, :3] = x + (v * h + (a * h2 + (j * h3 + (s * h4 + c * h5))))
        VP[:, :3] = v + (a * h + (j * h2 + (s * h3 + c * h4)))
        AP[:, :3] = a + (j * h + (s * h2 + c * h3))
        idx = np.ascontiguousarray(act, dtype=np.int32)
        a4, j4, s4 = (np.zeros((len(idx), 4)) for _ in range(3))
        rc = self._ajs_idx(self._ptr(XP), self._ptr(VP), self._ptr(AP), n, _i32ptr(idx), len(idx),
                           self.layout.chunk, self._cut2, self._eps2, self._ptr(a4),
                           self._ptr(j4), self._ptr(s4))
        _native.check(self.lib, rc, "cpu accjerksnap_idx")
        a1, j1, s1 = a4[:, :3], j4[:, :3], s4[:, :3]
        ha = h[act]
        hh, h10, h120 = ha / 2, (ha * ha) / 10, (ha * ha * ha) / 120
        a0, j0, s0, v0 = a[act], j[act], s[act], v[act]
        v1 = v0 + ((a0 + a1) * hh + ((j0 - j1) * h10 + (s0 + s1) * h120))
        self.X[act, :3] = x[act] + ((v0 + v1) * hh + ((a0 - a1) * h10 + (j0 + j1) * h120))
        want, valid = oracle.hermite6_dt_bodies(a0, j0, s0, a1, j1, s1, hd[act], self.cfg.eta)
        self.C[act, :3] = oracle.hermite6_high(a0, j0, s0, a1, j1, s1, hd[act])[0]
        self.V[act, :3], self.A[act, :3], self.J[act, :3], self.S[act, :3] = v1, a1, j1, s1
        return want, valid

    def load(self, b: BodySet, acc=None, jerk=None, t: float = 0.0,
             dt_next: Optional[float] = None, dt_min: Optional[float] = None,
             levels=None, body_times=None, snap=None, crackle=None) -> None:
        self.X[:, :3] = b.pos
        self.X[:, 3] = self.cfg.G * np.asarray(b.mass, dtype=np.float64)
        self.V[:] = 0
        self.V[:, :3] = b.vel
        self.mass = np.array(b.mass, dtype=np.float64)
        for y in self._rows:
            y[:] = 0
        self._clear_records()
        if self.collisions:
            self.radius = np.array(b.radii(self.cfg.body_density), dtype=np.float64)
            self._R = self.radius.astype(self.np_dtype)
        given = [acc, jerk, snap, crackle][: len(self._rows)]
        if all(y is not None for y in given):  # a run continues with every carried row
            for y, g in zip(self._rows, given):
                y[:, :3] = g
            self._next = math.inf if dt_next is None else float(dt_next)
        else:  # (order 6: a, j, s of the state; the crackle starts at 0)
            for y, d in zip(self._rows, self._derivs6() if self.order == 6 else self._derivs()):
                y[:, :3] = d[:, :3]
            if self.collisions:
                self._see(self.X)
            self._next = math.inf
            if self.cfg.eta > 0:
                self._next = float(self._first_dt(self._ptr(self.A), self._ptr(self.J),
                                                  self.cfg.n, float(self.cfg.eta)))
        self.t, self.dt_last, self.k = float(t), 0.0, 0
        self.dt_min = math.inf if dt_min is None else float(dt_min)
        if self.block:
            self._block_start(float(t), levels, body_times)

    def step(self, n: int) -> None:
        cfg = self.cfg
        if self.block:  # n macro steps of dt
            for _ in range(int(n)):
                if cfg.t_end is not None and self.t >= cfg.t_end:
                    return
                macro = int(self.tb.min()) >> self.L
                while int(self.tb.min()) < (macro + 1) << self.L:
                    self._block_step()
                self.t = cfg.dt * (macro + 1)
                self.dt_last = cfg.dt
                self.k += 1
            return
        out = ctypes.c_double(math.inf)
        for _ in range(int(n)):
            if cfg.t_end is not None and self.t >= cfg.t_end:
                return
            if cfg.collisions == "merge" and self.overlaps:
                return  # (the run stops at the step that first saw an overlap)
            h = min(cfg.dt, self._next) if cfg.eta > 0 else cfg.dt
            cut = cfg.t_end is not None and h >= cfg.t_end - self.t
            if cut:
                h = cfg.t_end - self.t
            rc = self._step(self._ptr(self.X), self._ptr(self.V), *map(self._ptr, self._rows),
                            self._ptr(self._scratch), cfg.n, self.layout.chunk, h, self._cut2,
                            self._eps2, float(cfg.eta), ctypes.byref(out))
            _native.check(self.lib, rc, "cpu hermite step")
            if self.collisions:  # (the step leaves its predicted rows at the scratch's head)
                self._see(self._scratch[: cfg.n])
            self._next = out.value
            self.t = cfg.t_end if cut else self.t + h
            self.dt_last = h
            if not cut:
                self.dt_min = min(self.dt_min, h)
            self.k += 1

    def sync(self, timeout_s: float = 0.0) -> None:
        pass

    def status(self) -> HermiteStatus:
        cfg = self.cfg
        if self.block:
            return HermiteStatus(self.t, self.dt_last, cfg.dt,
                                 float(np.ldexp(cfg.dt, -self.level_max)), self.k,
                                 cfg.t_end is not None and self.t >= cfg.t_end,
                                 len(self.block_log), self.body_steps, self.level_max,
                                 self.level_clamped, self.overlaps)
        nxt = min(cfg.dt, self._next) if cfg.eta > 0 else cfg.dt
        return HermiteStatus(self.t, self.dt_last, nxt, self.dt_min, self.k,
                             cfg.t_end is not None and self.t >= cfg.t_end,
                             overlaps=self.overlaps)

    def state(self) -> BodySet:
        return BodySet(self.X[:, :3].astype(np.float64), self.V[:, :3].astype(np.float64),
                       self.mass.copy(), self.radius.copy() if self.collisions else None)

    def carried(self):
        return tuple(y[:, :3].astype(np.float64) for y in self._rows)

    def derivs(self, active=None, path: Optional[str] = None):
        if self.order == 6:
            return tuple(y.astype(np.float64) for y in self._derivs6())
        a4, j4 = self._derivs() if active is None else self._derivs_idx(self.X, self.V, active)
        return a4.astype(np.float64), j4.astype(np.float64)

    def accel(self) -> np.ndarray:
        out = np.zeros((self.layout.n_local, 4))
        out[: self.cfg.n] = self.derivs()[0]
        return out

    def nonfinite(self) -> int:
        return int((~np.isfinite(self.X[:, :3])).sum() + (~np.isfinite(self.V[:, :3])).sum())

    @property
    def steps_done(self) -> int:
        return self.k

    def close(self) -> None:
        pass
