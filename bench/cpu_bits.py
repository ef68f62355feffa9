"""Digests of what the native CPU engine computes, for comparing two builds bit for bit.

The CPU counterpart of bench/hermite_bits.py: a fixed list of small cases runs through every
gs_cpu_* entry of libgravsim_cpu.so, and one JSON object is printed that maps each case to the
SHA-256 of the raw bytes of its outputs (digest() of hermite_bits):

    python bench/cpu_bits.py > a.json
    GRAVSIM_NATIVE_DIR=<other build> python bench/cpu_bits.py > b.json

--ab DIR runs both in fresh child processes (the in-tree build, then the build in DIR) and
prints {"equal": ..., "differ": [...], "digests": {...}}; the exit status is 1 when they differ.
The thread count is OMP_NUM_THREADS of the caller; no result depends on it.

Cases: n in 1, 2, 3, 257, 1024, 1031, 2055, 5000 with chunk 1024 and the automatic one. Per n and
chunk: accel, accel_abs and two plain steps (fp64, fp32); accjerk over all rows, over a sub-range
with i0 > 0 and over a permuted list with repeats and an empty list; first_dt; three Hermite
steps with a fixed and three with an adaptive step (fp64, fp32, mixed); accjerksnap over all rows
and over a sub-range with i0 > 0, and three 6th-order steps fixed and three adaptive (fp64, fp32;
a build without the 6th-order entries fails the run); nn with zero and non-zero
radii over rows and a list; knn with k = 1, 3, 8 over all rows and a sub-range.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hermite_bits import digest  # noqa: E402  (bench/ is the script's directory)

DTYPES = ("fp64", "fp32", "mixed")
SIZES = (1, 2, 3, 257, 1024, 1031, 2055, 5000)


def cases() -> dict:
    import numpy as np

    import gravsim  # noqa: F401
    from gravsim.models import initial_conditions as ic
    from gravsim.ops import _native

    lib = _native.cpu_lib()
    out: dict = {}
    ip = lambda a: a.ctypes.data_as(_native.PI32)  # noqa: E731
    cutoff, soft, G = 1e-10, 1.0e7, 6.674e-11

    def ok(rc):
        if rc != 0:
            raise SystemExit("cpu_bits: " + lib.gs_last_error().decode())

    for n in SIZES:
        b = ic.solar_random(n, 7 + n)
        rng = np.random.default_rng(n)
        sub = (n // 3 + (n > 1), n - n // 5) if n > 1 else (0, 1)  # i0 > 0 where n allows it
        lst = np.ascontiguousarray(np.concatenate([rng.permutation(n), rng.integers(0, n, 5)]),
                                   dtype=np.int32)
        radii = np.abs(b.pos).max() * 1e-3 * rng.random(n)
        for chunk in (1024, int(lib.gs_auto_chunk(n))):
            for dtype in DTYPES:
                T = np.float32 if dtype == "fp32" else np.float64
                X, V = np.zeros((n, 4), T), np.zeros((n, 4), T)
                X[:, :3], X[:, 3], V[:, :3] = b.pos, G * b.mass, b.vel
                cut2, eps2 = T(cutoff ** 2), T(soft ** 2)
                tag = f"{dtype}/n{n}/chunk{chunk}"

                def entry(stem):
                    return _native.cpu_entry(lib, stem, dtype)
                _, p = entry("accjerk")

                if dtype != "mixed":
                    acc = np.zeros((n, 4), T)
                    ok(entry("accel")[0](p(X), n, 0, n, chunk, cut2, eps2, p(acc)))
                    part = np.zeros((sub[1] - sub[0], 4), T)
                    ok(entry("accel")[0](p(X), n, *sub, chunk, cut2, eps2, p(part)))
                    cur, nxt, vel = X.copy(), np.zeros((n, 4), T), V.copy()
                    for _ in range(2):
                        ok(entry("step")[0](p(cur), p(nxt), p(vel), n, 0, n, chunk, T(3600.0),
                                            cut2, eps2))
                        cur, nxt = nxt, cur
                    out[f"accel_step/{tag}"] = digest(acc, part, cur, vel)

                # accjerk: all rows, a sub-range, a list, an empty list
                d = []
                for rows in ((0, n), sub):
                    a4, j4 = np.zeros((rows[1] - rows[0], 4), T), np.zeros((rows[1] - rows[0], 4), T)
                    ok(entry("accjerk")[0](p(X), p(V), n, *rows, chunk, cut2, eps2, p(a4), p(j4)))
                    d += [a4, j4]
                A, J = d[0], d[1]
                for idx in (lst, lst[:0]):
                    a4, j4 = np.full((len(idx), 4), 7, T), np.full((len(idx), 4), 7, T)
                    ok(entry("accjerk_idx")[0](p(X), p(V), n, ip(idx), len(idx), chunk, cut2, eps2,
                                               p(a4), p(j4)))
                    d += [a4, j4]
                fn, _ = entry("hermite_first_dt")
                d.append(np.array([fn(p(A), p(J), n, 0.02)]))
                out[f"accjerk/{tag}"] = digest(*d)

                # Hermite steps
                for eta in (0.0, 0.02):
                    x, v, a, j = X.copy(), V.copy(), A.copy(), J.copy()
                    a[:, 3] = 0
                    scratch, h, dts = np.zeros((4 * n, 4), T), 3600.0, []
                    for _ in range(3):
                        dt = ctypes.c_double(0.0)
                        ok(entry("hermite_step")[0](p(x), p(v), p(a), p(j), p(scratch), n, chunk,
                                                    h, cut2, eps2, eta, ctypes.byref(dt)))
                        dts.append(dt.value)
                        if eta > 0.0 and np.isfinite(dt.value):
                            h = min(3600.0, dt.value)
                    out[f"hermite_step/{tag}/eta{eta}"] = digest(x, v, a, j, np.array(dts))

                if dtype == "mixed":  # (the 6th-order scheme has no mixed precision)
                    continue
                # accjerksnap at ap = a: all rows and a sub-range
                A0 = A.copy()
                A0[:, 3] = 0
                d = []
                for rows in ((0, n), sub):
                    o = [np.zeros((rows[1] - rows[0], 4), T) for _ in range(3)]
                    ok(entry("accjerksnap")[0](p(X), p(V), p(A0), n, *rows, chunk, cut2, eps2,
                                               *map(p, o)))
                    d += o
                out[f"accjerksnap/{tag}"] = digest(*d)
                # 6th-order steps (eta linear in this criterion)
                for eta in (0.0, 0.25):
                    x, v, a, j, s = X.copy(), V.copy(), A0.copy(), d[1].copy(), d[2].copy()
                    c = np.zeros((n, 4), T)
                    scratch, h, dts = np.zeros((6 * n, 4), T), 3600.0, []
                    for _ in range(3):
                        dt = ctypes.c_double(0.0)
                        ok(entry("hermite6_step")[0](p(x), p(v), p(a), p(j), p(s), p(c), p(scratch),
                                                     n, chunk, h, cut2, eps2, eta, ctypes.byref(dt)))
                        dts.append(dt.value)
                        if eta > 0.0 and np.isfinite(dt.value):
                            h = min(3600.0, dt.value)
                    out[f"hermite6_step/{tag}/eta{eta}"] = digest(x, v, a, j, s, c, np.array(dts))

            # nn and knn take no chunk
            if chunk != 1024:
                continue
            for dtype in DTYPES:
                T = np.float32 if dtype == "fp32" else np.float64
                X = np.zeros((n, 4), T)
                X[:, :3], X[:, 3] = b.pos, G * b.mass
                _, p = _native.cpu_entry(lib, "nn", dtype)
                d = []
                for R in (np.zeros(n, T), radii.astype(T)):
                    for rows in ((0, n), sub):
                        q, nn = np.zeros(rows[1] - rows[0], T), np.zeros(rows[1] - rows[0], np.int32)
                        ok(_native.cpu_entry(lib, "nn", dtype)[0](
                            p(X), p(R), n, *rows, T(cutoff ** 2), T(soft ** 2), p(q), ip(nn)))
                        d += [q, nn]
                    q, nn = np.zeros(len(lst), T), np.zeros(len(lst), np.int32)
                    ok(_native.cpu_entry(lib, "nn_idx", dtype)[0](
                        p(X), p(R), n, ip(lst), len(lst), T(cutoff ** 2), T(0.0), p(q), ip(nn)))
                    d += [q, nn]
                out[f"nn/{dtype}/n{n}"] = digest(*d)
                d = []
                for k in (1, 3, 8):
                    for rows in ((0, n), sub):
                        m = rows[1] - rows[0]
                        r2, ix = np.zeros((m, k), T), np.zeros((m, k), np.int32)
                        ok(_native.cpu_entry(lib, "knn", dtype)[0](p(X), n, *rows, k, p(r2),
                                                                   ip(ix)))
                        d += [r2, ix]
                out[f"knn/{dtype}/n{n}"] = digest(*d)

        # the accuracy references (fp64 input, double and long double sums)
        X = np.zeros((n, 4))
        X[:, :3], X[:, 3] = b.pos, G * b.mass
        d = []
        for fn in (lib.gs_cpu_accel_abs_f64, lib.gs_cpu_accel_abs_ld):
            o8 = np.zeros((sub[1] - sub[0], 8))
            ok(fn(_native.dptr(X), n, *sub, cutoff ** 2, soft ** 2, _native.dptr(o8)))
            d.append(o8)
        out[f"accel_abs/n{n}"] = digest(*d)
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
        raise SystemExit(f"cpu_bits: the run with {native_dir or 'the in-tree build'} failed:\n"
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
                      "threads": os.environ.get("OMP_NUM_THREADS", ""),
                      "other_build": a.label or a.ab, "digests": here}, sort_keys=True), flush=True)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
