"""Shared-step Hermite across ranks, the parts that need no GPU: the ownership partition (native
gs_hermite_partition against parallel/partition.py hermite_partition) and what the configuration
refuses with more than one rank.
"""
import ctypes

import pytest

from gravsim.config import SimConfig
from gravsim.ops import _native
from gravsim.parallel import partition

UNIT = 1024


def _native_partition(lib, n, chunk, nranks, rank):
    b, c = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.gs_hermite_partition(n, chunk, nranks, rank, ctypes.byref(b), ctypes.byref(c))
    return rc, b.value, c.value


def test_native_partition_equals_python_and_tiles_the_rows():
    lib = _native.cpu_lib()
    assert partition.HERMITE_UNIT == UNIT
    for units in range(1, 301):
        n_pad = units * UNIT
        n = n_pad - 71  # (a part-ghost last unit; n_pad is n rounded up to the chunk)
        for P in range(1, 9):
            if P > units:
                rc, _, _ = _native_partition(lib, n, UNIT, P, 0)
                assert rc != 0 and b"more ranks than units" in lib.gs_last_error()
                with pytest.raises(ValueError, match="unit"):
                    partition.hermite_partition(n, UNIT, P, 0)
                continue
            end = 0
            for r in range(P):
                rc, b, c = _native_partition(lib, n, UNIT, P, r)
                assert rc == 0, lib.gs_last_error()
                assert (b, c) == partition.hermite_partition(n, UNIT, P, r)
                assert b == end and c % UNIT == 0  # contiguous, whole units
                # mpi.c's remainder rule: the first `units mod P` ranks hold one more unit
                assert c // UNIT == units // P + (1 if r < units % P else 0)
                end = b + c
            assert end == n_pad  # the slices tile [0, n_pad)


def test_partition_pads_to_the_chunk_and_checks_its_arguments():
    lib = _native.cpu_lib()
    # n_pad is n rounded up to the chunk (not to P * chunk): 5000 -> 6144 = 6 units at chunk 2048
    assert [partition.hermite_partition(5000, 2048, 4, r) for r in range(4)] == \
        [(0, 2048), (2048, 2048), (4096, 1024), (5120, 1024)]
    assert _native_partition(lib, 5000, 2048, 4, 2) == (0, 4096, 1024)
    # chunk 0: the canonical chunk of n
    c = partition.auto_chunk(100000)
    assert _native_partition(lib, 100000, 0, 1, 0) == (0, 0, partition.round_up(100000, c))
    assert partition.hermite_partition(100000, 0, 1, 0) == (0, partition.round_up(100000, c))
    for bad in ((0, 1024, 1, 0), (100, 1000, 1, 0), (100, 1024, 0, 0), (100, 1024, 1, 1),
                (100, 1024, 1, -1)):
        assert _native_partition(lib, *bad)[0] != 0
        with pytest.raises(ValueError):
            partition.hermite_partition(*bad)


def test_layout_of_a_rank_and_the_rank_without_a_body():
    L = partition.hermite_layout(3000, 2, 3, 1024)
    assert (L.n_pad, L.local_begin, L.n_local, L.n_chunks) == (3072, 2048, 1024, 3)
    assert L.real_local == range(2048, 3000)
    one = partition.hermite_layout(3000, 0, 1, 1024)
    assert one == partition.layout(3000, 0, 1, 1024)  # one rank: the layout it always had
    # 64 bodies pad to one chunk of 2048 rows, two units, but the second holds ghosts only
    with pytest.raises(ValueError, match="hermite runs on one rank"):
        partition.hermite_layout(64, 0, 2)
    with pytest.raises(ValueError, match="unit"):
        partition.hermite_layout(1024, 0, 2, 1024)


def test_config_refusals_with_two_ranks():
    ok = dict(integrator="hermite", device="gpu", eta=0.02, dt=100.0)
    assert SimConfig().gpus == 0
    SimConfig(integrator="hermite", gpus=2).validate()
    SimConfig(**ok, gpus=2, t_end=250.0, dtype="mixed").validate()
    SimConfig(**ok, gpus=1, block_steps=True).validate()
    SimConfig(**ok, gpus=1, collisions="detect").validate()
    SimConfig(integrator="hermite", device="cpu", gpus=1).validate()
    with pytest.raises(ValueError, match="block steps"):
        SimConfig(**ok, gpus=2, block_steps=True).validate()
    with pytest.raises(ValueError, match="collisions"):
        SimConfig(**ok, gpus=2, collisions="detect").validate()
    with pytest.raises(ValueError, match="collisions"):
        SimConfig(**ok, gpus=2, collisions="merge").validate()
    with pytest.raises(ValueError, match="device cpu"):
        SimConfig(integrator="hermite", device="cpu", gpus=2).validate()
    with pytest.raises(ValueError):
        SimConfig(gpus=-1).validate()
    SimConfig(device="cpu", gpus=2).validate()  # (the kick-drift stepper runs on CPU ranks)


def test_cli_refuses_before_launching_ranks(monkeypatch):
    from gravsim import cli

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(cli, "_launch", lambda *a: pytest.fail("ranks were launched"))
    base = ["--n", "4097", "--integrator", "hermite", "--eta", "0.02", "--gpus", "2"]
    for extra, word in ((["--block-steps"], "block-steps"), (["--collisions", "detect"],
                                                             "collisions"),
                        (["--device", "cpu"], "device cpu")):
        with pytest.raises(SystemExit, match=word):
            cli.main(base + extra)
