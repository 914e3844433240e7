"""N > 1 orchestration on CPU: gloo with 2 and with 8 ranks.  GOPs are independent units, so sharding
needs no data-path collective; what must hold is that the shards partition the work, that a
rank's output does not depend on the world size, and that the timing reduction used by
bench.py (barrier, MAX over ranks) behaves.  The per-GOP work here is the host half of the
product path (libdcvc_rans entropy coding of seeded symbol planes) -- the device half needs a
GPU and is covered by the -m gpu tests."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import ROOT, golden
from vcm_ts_amd.pipeline import shard_gops, timed_region


def _encode_fake_gop(g, tables):
    from vcm_ts_amd import entropy as E

    cdf, ln, off = tables
    rng = np.random.default_rng(1000 + g)
    enc = E.BufferedRansEncoder()
    out = []
    for _ in range(4):  # 4 pictures per GOP
        enc.reset()
        for n in (256, 2048, 2048):
            enc.encode_with_indexes(np.rint(rng.laplace(0, 2, n)).astype(np.int32), rng.integers(0, 256, n).astype(np.int32), cdf, ln, off)
        out.append(enc.flush())
    return out


def _worker(rank, world, port, n_gops, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = golden("tables")
    tables = (t["dmc_scale_cdf"], t["dmc_scale_len"], t["dmc_scale_off"])
    mine = shard_gops(n_gops, rank, world)
    dt, coded = timed_region(lambda: {g: _encode_fake_gop(g, tables) for g in mine})
    gathered = [None] * world
    dist.all_gather_object(gathered, (mine, coded, dt))
    if rank == 0:
        q.put(gathered)
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_shards_partition_the_gops():
    for n, w in ((8, 2), (7, 3), (1, 4), (16, 8), (0, 2)):
        shards = [shard_gops(n, r, w) for r in range(w)]
        flat = sorted(g for s in shards for g in s)
        assert flat == list(range(n))
        assert max(len(s) for s in shards) - min(len(s) for s in shards) <= 1


@pytest.mark.timeout(240)
@pytest.mark.parametrize("n_gops,world", [(5, 2), (19, 8)], ids=["2-ranks", "8-ranks"])
def test_gloo_run_matches_single_process(n_gops, world):
    """world 8 is the rank count of the node BASELINE's configs[3] and the scaling curve are quoted on: no such node
    was available to any round, so the orchestration (shards, barrier, MAX-reduced time, gather) is at least run at
    that size here (gloo, CPU; 19 GOPs: ranks with three and with two GOPs)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_gops, q)) for r in range(world)]
    for p in procs:
        p.start()
    gathered = q.get(timeout=100)
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    t = golden("tables")
    tables = (t["dmc_scale_cdf"], t["dmc_scale_len"], t["dmc_scale_off"])
    seen = {}
    times = set()
    for mine, coded, dt in gathered:
        assert sorted(coded) == mine
        seen.update(coded)
        times.add(dt)
    assert sorted(seen) == list(range(n_gops))
    assert len(times) == 1  # every rank reports the same (max-reduced) time
    for g in range(n_gops):  # bytes do not depend on how the GOPs were sharded
        assert seen[g] == _encode_fake_gop(g, tables)


def test_timed_region_single_process():
    dt, r = timed_region(lambda: 41 + 1)
    assert r == 42 and dt >= 0


def test_bench_self_launch_starts_one_rank_per_gpu_and_propagates_failure():
    """`python bench.py --gpus 2` without torchrun around it: the parent must start two ranks as a child
    torch.distributed.run (env:// rendezvous on 127.0.0.1) and return the child's exit code.  There is no GPU
    here, so each rank stops at "needs a GPU" -- which is exactly what shows that two ranks were started,
    that they got their RANK / WORLD_SIZE and that the failure came back as a non-zero exit."""
    import re

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--dist-backend", "gloo"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert len(re.findall(r"bench\.py needs a GPU", r.stderr + r.stdout)) >= 2, (r.stderr + r.stdout)[-1500:]
    # a world size that contradicts --gpus is refused before anything else happens
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"],
                         env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE=2" in bad.stderr + bad.stdout


def test_bench_dump_outputs_samples_large_arrays_within_budget(tmp_path):
    """bench.py --dump-outputs: small arrays are written whole (float64 host lists kept as float64, tensors and bytes as
    float32), an array over its share of the 64 MB budget as a sample at positions seeded by its name -- the same
    positions in every run, so two builds can be compared output for output."""
    sys.path.insert(0, ROOT)
    import bench

    big = torch.arange(3 << 20, dtype=torch.float32).reshape(3, 1 << 20)
    payload = bytes(range(256)) * 8
    arrays = [("bits", np.array([12345.0])), ("small", torch.ones(2, 3, dtype=torch.float64)), ("payload", payload),
              ("big", big), ("parts", [big[0], big[1:]])]
    total = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert total <= bench.DUMP_BUDGET_BYTES
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n, _ in arrays}
    assert got["bits"].dtype == np.float64 and got["bits"].tolist() == [12345.0]
    assert got["small"].dtype == np.float32 and got["small"].shape == (2, 3)
    assert got["payload"].dtype == np.float32 and np.array_equal(got["payload"], np.frombuffer(payload, np.uint8))
    for n in ("big", "parts"):
        a = got[n]
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < big.numel()
        assert np.all(np.diff(a) >= 0) and np.array_equal(a, np.rint(a))  # elements of arange, in order
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{n}.npy"))
    # a list of tensors is sampled as their concatenation: the same positions under the same name
    bench.dump_outputs(str(tmp_path / "c"), [("big", [big[0], big[1:]])] + arrays[:4])
    assert np.array_equal(got["big"], np.load(tmp_path / "c" / "big.npy"))
