"""Digests of what the one-sided force kernels and the k-nearest-neighbour kernel compute, for
comparing two native builds bit for bit.

The counterpart of bench/hermite_bits.py for the two kernel families it does not run: a fixed
list of small cases goes through HipEngine / VirtualGroup and gs_hip_knn, and one JSON object is
printed that maps each case to the SHA-256 of the raw bytes of its outputs (digest() of
hermite_bits):

    python bench/force_bits.py > a.json
    GRAVSIM_NATIVE_DIR=<other build> python bench/force_bits.py > b.json

--ab DIR runs both in fresh child processes (the in-tree build, then the build in DIR) and prints
{"equal": ..., "differ": [...], "digests": {...}}; the exit status is 1 when they differ.

Cases. One-sided force (fp32, fp64; kernel lds, smem; mode split, fused; every built bodies-per-
lane count; cutoff mode exact, fast): chunk 1024 at n = 3, 257, 2049, 5000 (1, 1, 3, 5 chunks; 8
bodies per lane need whole blocks of 2048 rows: chunk 2048, 1, 1, 2, 3 chunks) under 1, 3, 7, 20
chunk groups (3 over 5 chunks: a short last group; 7 and 20: empty ones; the fused schedule has no
groups), each with accel() (the diagnostics path, with phi), accel(step_path=True) and the state
after 2 steps. 2 and 3 virtual ranks at n = 3000, 4097 with the all-gather and the ring (own
chunks first, then the rest minus the own). knn (fp32, fp64, mixed): k = 1, 8, 1 and 2 bodies per lane, 1, 3, 7, 20 chunk groups at
the same n. A shape a build refuses is recorded as refused.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hermite_bits import digest  # noqa: E402  (bench/ is the script's directory)

SIZES = (3, 257, 2049, 5000)
GROUPS = (1, 3, 7, 20)
IPLS = {"fp32": (1, 2, 4, 8), "fp64": (1, 2, 4)}


def cases() -> dict:
    import gravsim  # noqa: F401
    from gravsim.config import SimConfig
    from gravsim.models import initial_conditions as ic
    from gravsim.ops import neighbours
    from gravsim.runtime.engines import HipEngine, VirtualGroup

    out: dict = {}

    def bodies(n):
        return ic.solar_random(n, 7 + n)

    def run(name, make, n, fn):
        try:
            eng = make()
        except (ValueError, RuntimeError) as e:
            out[name] = "refused: " + str(e).split(":")[0]
            return
        try:
            eng.load(bodies(n))
            out[name] = fn(eng)
        except RuntimeError as e:
            out[name] = "refused: " + str(e).split(":")[0]
        finally:
            eng.close()

    def force(e):
        d = [e.accel(), e.accel(step_path=True)]
        e.step(2)
        e.sync()
        s = e.state()
        return digest(*d, s.pos, s.vel)

    for dtype, ipls in IPLS.items():
        for kernel in ("lds", "smem"):
            for mode in ("split", "fused"):
                for ipl in ipls:
                    for cutoff_mode in ("exact", "fast"):
                        for groups in GROUPS if mode == "split" else (0,):
                            for n in SIZES:
                                cfg = SimConfig(n=n, dtype=dtype, device="gpu", kernel=kernel,
                                                mode=mode, ipl=ipl, chunk=2048 if ipl == 8 else 1024,
                                                split_groups=groups, cutoff_mode=cutoff_mode)
                                run(f"force/{dtype}/{kernel}/{mode}/ipl{ipl}/{cutoff_mode}/"
                                    f"groups{groups}/n{n}", lambda: HipEngine(cfg.validate()), n,
                                    force)

        def ranks(g):
            d = [s.accel() for s in g.shards] + [s.accel(step_path=True) for s in g.shards]
            g.step(2)
            g.sync()
            s = g.state()
            return digest(*d, s.pos, s.vel)

        for kernel in ("lds", "smem"):
            for P in (2, 3):
                for strategy in ("allgather", "ring"):
                    for n in (3000, 4097):
                        cfg = SimConfig(n=n, dtype=dtype, device="gpu", kernel=kernel, mode="split",
                                        chunk=1024, strategy=strategy)
                        run(f"ranks/{dtype}/{kernel}/P{P}/{strategy}/n{n}",
                            lambda: VirtualGroup(cfg.validate(), P), n, ranks)

    for dtype in ("fp32", "fp64", "mixed"):
        for n in SIZES:
            pos = bodies(n).pos
            for k in (1, 8):
                for ipl in (1, 2):
                    for groups in GROUPS:
                        out[f"knn/{dtype}/k{k}/ipl{ipl}/groups{groups}/n{n}"] = digest(
                            *neighbours.k_nearest(pos, k, "gpu", dtype, ipl, groups))
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
        raise SystemExit(f"force_bits: the run with {native_dir or 'the in-tree build'} failed:\n"
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
                      "refused": sum(str(v).startswith("refused") for v in here.values()),
                      "other_build": a.label or a.ab, "digests": here}, sort_keys=True), flush=True)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
