"""Binary checkpoints and resume (absent from the reference: SURVEY.md §5).

Format (little-endian, rank-agnostic global body order):
    magic   8 B   b"GRAVSIM1"
    header  JSON  (u32 length + UTF-8): n, step, time, dt, dtype, G, cutoff, softening,
                  init, seed, version
    pos     n*3 float64
    vel     n*3 float64
    mass    n   float64
    extra   the arrays the header names in "extra" (a Hermite run: ["acc", "jerk"], n*3 float64
            each, with "time" and "dt_next" in the header; a block-step run appends "level",
            the per-body level in column 0 of an n*3 array, header "level_column": 0);
            readers that do not know them stop after mass
State is always stored in fp64 so an fp32 run resumes exactly (fp32 -> fp64 -> fp32 is exact).
Writes go to a temp file + rename, so a crash never leaves a torn checkpoint.
"""
from __future__ import annotations

import json
import os
import struct
from dataclasses import dataclass, field

import numpy as np

from ..models.initial_conditions import BodySet

MAGIC = b"GRAVSIM1"


@dataclass
class Checkpoint:
    bodies: BodySet
    step: int
    meta: dict
    extra: dict = field(default_factory=dict)  # name -> (n, 3) float64 array


def save(path: str, bodies: BodySet, step: int, meta: dict, extra: dict | None = None) -> str:
    n = bodies.n
    head = dict(meta)
    head.update(n=n, step=int(step), version=1)
    extra = extra or {}
    if extra:
        head["extra"] = list(extra)
    hb = json.dumps(head, sort_keys=True).encode()
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<I", len(hb)))
        f.write(hb)
        f.write(np.ascontiguousarray(bodies.pos, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(bodies.vel, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(bodies.mass, dtype="<f8").tobytes())
        for name in extra:
            a = np.ascontiguousarray(extra[name], dtype="<f8")
            if a.shape != (n, 3):
                raise ValueError(f"checkpoint extra {name!r} must be (n, 3)")
            f.write(a.tobytes())
    os.replace(tmp, path)
    return path


def load(path: str) -> Checkpoint:
    with open(path, "rb") as f:
        if f.read(8) != MAGIC:
            raise ValueError(f"{path}: not a gravsim checkpoint")
        (hl,) = struct.unpack("<I", f.read(4))
        head = json.loads(f.read(hl).decode())
        n = int(head["n"])
        pos = np.frombuffer(f.read(n * 24), dtype="<f8").reshape(n, 3).copy()
        vel = np.frombuffer(f.read(n * 24), dtype="<f8").reshape(n, 3).copy()
        mass = np.frombuffer(f.read(n * 8), dtype="<f8").copy()
        if mass.shape[0] != n:
            raise ValueError(f"{path}: truncated checkpoint")
        extra = {}
        for name in head.get("extra", []):
            a = np.frombuffer(f.read(n * 24), dtype="<f8")
            if a.shape[0] != n * 3:
                raise ValueError(f"{path}: truncated checkpoint ({name})")
            extra[name] = a.reshape(n, 3).copy()
    return Checkpoint(BodySet(pos, vel, mass), int(head["step"]), head, extra)


def path_for(directory: str, step: int) -> str:
    return os.path.join(directory, f"ckpt_{step:08d}.gsck")


def latest(directory: str) -> str | None:
    if not os.path.isdir(directory):
        return None
    c = sorted(f for f in os.listdir(directory) if f.startswith("ckpt_") and f.endswith(".gsck"))
    return os.path.join(directory, c[-1]) if c else None
