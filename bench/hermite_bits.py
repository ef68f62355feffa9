"""Digests of what the Hermite kernels compute, for comparing two native builds bit for bit.

A fixed list of small cases runs through HermiteHipEngine / HermiteVirtualGroup; one JSON object
is printed that maps each case to the SHA-256 of the raw bytes of its outputs. Two builds whose
kernels compute the same bits print the same object:

    python bench/hermite_bits.py > a.json
    GRAVSIM_NATIVE_DIR=<other build> python bench/hermite_bits.py > b.json

--ab DIR runs both in fresh child processes (the in-tree build, then the build in DIR, as
bench/knn_rate.py --ab does) and prints {"equal": ..., "differ": [...], "digests": {...}};
the exit status is 1 when they differ. The tests already hold every case reproducible from run
to run and independent of the launch shape; this adds "equal to another build".

Cases (fp32, fp64, mixed): derivs() at n = 3, 257, 2049, 5000 and, at 5000, every bodies-per-lane
x chunk-group shape; 3 shared steps fixed and adaptive; derivs_nn() and 3 detect-mode steps; the
block path's derivs / derivs_nn of three active sets on both evaluate paths; two block macro
steps under three narrow_max; the shared step on 2 and 3 virtual ranks (n = 3000, 3100, 4097).
Order 6 (fp32, fp64): derivs() (a4, j4, s4) at the same n and, at 5000, every built bodies-per-lane
x chunk-group (1, 3, 7, 20) shape; 3 steps fixed and 3 adaptive (eta 0.25) with state(), the four
carried rows and (time, dt_next); a resume from the four carried rows, then 2 more steps.
Order 6 block steps (fp64, eta 0.25): derivs() (a4, j4, s4) of the three active sets on both
evaluate paths; two block macro steps at n = 200, 2049 under three narrow_max, with the four
carried rows.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = ("fp32", "fp64", "mixed")


def digest(*arrays) -> str:
    import numpy as np

    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def cases() -> dict:
    import numpy as np

    import gravsim  # noqa: F401
    from gravsim.config import SimConfig
    from gravsim.models import initial_conditions as ic
    from gravsim.runtime.hermite import HermiteHipEngine, HermiteVirtualGroup

    out: dict = {}

    def bodies(n):
        return ic.solar_random(n, 7 + n)

    def engine(n, dtype, **kw):
        kw.setdefault("integrator", "hermite")
        return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate())

    def status(st):
        return np.array([st.time, st.dt_last, st.dt_min, float(st.steps)])

    def run(name, eng, b, fn):
        try:
            eng.load(b)
            out[name] = fn(eng)
        finally:
            eng.close()

    for dtype in DTYPES:
        # derivs
        for n in (3, 257, 2049, 5000):
            run(f"derivs/{dtype}/n{n}", engine(n, dtype), bodies(n), lambda e: digest(*e.derivs()))
        for ipl in (1, 2, 4):
            if ipl == 4 and dtype == "fp64":
                continue  # (not built)
            for groups in (1, 3):
                run(f"derivs/{dtype}/n5000/ipl{ipl}/groups{groups}",
                    engine(5000, dtype, ipl=ipl, split_groups=groups), bodies(5000),
                    lambda e: digest(*e.derivs()))

        # shared step
        def stepped(e):
            e.step(3)
            e.sync()
            s = e.state()
            return digest(s.pos, s.vel, *e.carried(), status(e.status()))

        run(f"step/{dtype}/fixed", engine(5000, dtype, dt=3600.0), bodies(5000), stepped)
        run(f"step/{dtype}/eta0.05", engine(5000, dtype, dt=3600.0, eta=0.05), bodies(5000),
            stepped)

        # collisions
        for n in (257, 5000):
            run(f"nn/{dtype}/n{n}", engine(n, dtype, collisions="detect"), bodies(n),
                lambda e: digest(*e.derivs_nn()[2:]))

        def detected(e):
            e.step(3)
            e.sync()
            return digest(*e.neighbours(), *e.closest(), np.array([e.status().overlaps]))

        run(f"nn/{dtype}/detect3", engine(2049, dtype, collisions="detect", dt=3600.0),
            bodies(2049), detected)

        # block path derivs: a narrow group with spare slots, wide i-blocks beyond n_act
        n = 2049
        sets = {"one": [0], "four": [5, 6, 7, 2048], "third": list(range(0, n, 3))}
        blk = dict(block_steps=True, eta=0.02, dt=3600.0, max_level=6)

        def active(e, nn):
            e.set_block_tuning(n)  # (any active set may take the narrow path)
            d = []
            for name, idx in sets.items():
                idx = np.asarray(idx, dtype=np.int32)
                for path in ("narrow", "wide"):
                    d.extend(e.derivs_nn(idx, path) if nn else e.derivs(idx, path))
            return digest(*d)

        run(f"active/{dtype}", engine(n, dtype, **blk), bodies(n), lambda e: active(e, False))
        run(f"active_nn/{dtype}", engine(n, dtype, collisions="detect", **blk), bodies(n),
            lambda e: active(e, True))

        # block runs
        for n in (200, 2049):
            for tag, cut in (("default", None), ("wide", 0), ("narrow", n)):
                def macro(e, cut=cut):
                    if cut is not None:
                        e.set_block_tuning(cut)
                    e.step(2)
                    e.sync()
                    s, st = e.state(), e.status()
                    return digest(s.pos, s.vel, e.body_times(), e.levels(),
                                  np.array([st.block_steps, st.body_steps, st.level_max]))

                run(f"block/{dtype}/n{n}/{tag}", engine(n, dtype, **blk), bodies(n), macro)

        # ranks
        for P in (2, 3):
            # (3000 bodies on 3 ranks are refused, the last rank's rows 3072.. would hold no body;
            # at 3100 it holds 28 bodies and 996 ghost rows)
            for n in (3000, 3100, 4097):
                cfg = SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite", dt=3600.0)
                try:
                    g = HermiteVirtualGroup(cfg, P)
                except ValueError as e:
                    out[f"ranks/{dtype}/P{P}/n{n}"] = "refused: " + str(e).split(":")[0]
                    continue
                try:
                    g.load(bodies(n))
                    g.step(3)
                    g.sync()
                    s = g.state()
                    out[f"ranks/{dtype}/P{P}/n{n}"] = digest(s.pos, s.vel, *g.carried(),
                                                            status(g.status()), *g.derivs())
                finally:
                    g.close()

    # order 6 (fp32 and fp64 only)
    for dtype in ("fp32", "fp64"):
        six = dict(hermite_order=6, dt=3600.0)
        for n in (3, 257, 2049, 5000):
            run(f"derivs6/{dtype}/n{n}", engine(n, dtype, **six), bodies(n),
                lambda e: digest(*e.derivs()))
        for ipl in (1, 2):
            if ipl == 2 and dtype == "fp64":
                continue  # (not built)
            for groups in (1, 3, 7, 20):
                run(f"derivs6/{dtype}/n5000/ipl{ipl}/groups{groups}",
                    engine(5000, dtype, ipl=ipl, split_groups=groups, **six), bodies(5000),
                    lambda e: digest(*e.derivs()))

        def stepped6(e, k=3):
            e.step(k)
            e.sync()
            s, st = e.state(), e.status()
            return digest(s.pos, s.vel, *e.carried(), np.array([st.time, st.dt_next]))

        run(f"step6/{dtype}/fixed", engine(5000, dtype, **six), bodies(5000), stepped6)
        run(f"step6/{dtype}/eta0.25", engine(5000, dtype, eta=0.25, **six), bodies(5000),
            stepped6)

        # a resume: the state and the four carried rows of a run after 3 steps, 2 more steps
        e = engine(5000, dtype, eta=0.25, **six)
        try:
            e.load(bodies(5000))
            e.step(3)
            e.sync()
            s, (a, j, sn, cr), st = e.state(), e.carried(), e.status()
        finally:
            e.close()
        e = engine(5000, dtype, eta=0.25, **six)
        try:
            e.load(s, a, j, t=st.time, dt_next=st.dt_next, dt_min=st.dt_min, snap=sn, crackle=cr)
            out[f"resume6/{dtype}"] = stepped6(e, 2)
        finally:
            e.close()

    # order 6, block steps (fp64 only): the cases of active/ and block/ above
    blk6 = dict(hermite_order=6, block_steps6=True, eta=0.25, dt=3600.0, max_level=6)
    n = 2049
    sets = {"one": [0], "four": [5, 6, 7, 2048], "third": list(range(0, n, 3))}

    def active6(e):
        e.set_block_tuning(n)  # (any active set may take the narrow path)
        d = []
        for idx in sets.values():
            idx = np.asarray(idx, dtype=np.int32)
            for path in ("narrow", "wide"):
                d.extend(e.derivs(idx, path))
        return digest(*d)

    run("active6/fp64", engine(n, "fp64", **blk6), bodies(n), active6)
    for n in (200, 2049):
        for tag, cut in (("default", None), ("wide", 0), ("narrow", n)):
            def macro6(e, cut=cut):
                if cut is not None:
                    e.set_block_tuning(cut)
                e.step(2)
                e.sync()
                s, st = e.state(), e.status()
                return digest(s.pos, s.vel, *e.carried(), e.body_times(), e.levels(),
                              np.array([st.block_steps, st.body_steps, st.level_max]))

            run(f"block6/fp64/n{n}/{tag}", engine(n, "fp64", **blk6), bodies(n), macro6)
    return out


def child(native_dir: str | None) -> dict:
    env = dict(os.environ)
    if native_dir:
        env["GRAVSIM_NATIVE_DIR"] = os.path.abspath(native_dir)
    else:
        env.pop("GRAVSIM_NATIVE_DIR", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True,
                       text=True, timeout=540)
    if r.returncode:
        raise SystemExit(f"hermite_bits: the run with {native_dir or 'the in-tree build'} failed:\n"
                         f"{r.stdout}\n{r.stderr}")
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--ab", default="", help="a second native build directory to compare with")
    ap.add_argument("--label", default="", help="--ab: what the other build is (a commit hash)")
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps(cases(), sort_keys=True), flush=True)
        return 0
    here, other = child(None), child(a.ab)
    differ = sorted(k for k in set(here) | set(other) if here.get(k) != other.get(k))
    print(json.dumps({"equal": not differ, "cases": len(here), "differ": differ,
                      "other_build": a.label or a.ab, "digests": here}, sort_keys=True), flush=True)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
