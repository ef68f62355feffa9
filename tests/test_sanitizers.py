"""Host sanitizers on the native CPU code (ASan + UBSan), and a TSan-free determinism check of
the OpenMP engine. GPU ASan / XNACK runs are not available on the target pool, so device code
is covered by the bitwise determinism and schedule-independence tests instead (no atomics or
inter-workgroup communication exist in the force kernels)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# The stand-alone programs under csrc/tests/ (each has its own main and prints "<name> ok").
SELFTESTS = sorted(f[:-4] for f in os.listdir(os.path.join(ROOT, "csrc", "tests"))
                   if f.endswith(".cpp"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name", SELFTESTS)
def test_cpu_engine_asan_ubsan(tmp_path, name):
    exe = tmp_path / name
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           f"-I{ROOT}/csrc/include", f"{ROOT}/csrc/tests/{name}.cpp",
           f"{ROOT}/csrc/common/layout.cpp", f"{ROOT}/csrc/cpu/cpu_engine.cpp", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{name} ok" in r.stdout


def test_openmp_engine_deterministic_across_thread_counts():
    """Fixed per-body summation order: results do not depend on the OpenMP thread count."""
    import sys

    code = ("import sys; sys.path.insert(0, %r); import gravsim, numpy as np;"
            "from gravsim.models import initial_conditions as ic;"
            "from gravsim.ops.force import cpu_accelerations;"
            "b = ic.solar_random(3000, 5); a, _ = cpu_accelerations(b.pos, b.mass);"
            "sys.stdout.buffer.write(a.tobytes())") % ROOT
    outs = []
    for t in ("1", "3", "8"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                           env=dict(os.environ, OMP_NUM_THREADS=t), timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        outs.append(np.frombuffer(r.stdout, dtype=np.float64))
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
