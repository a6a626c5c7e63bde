"""world_size-2 tests of the batch-sharding layer on CPU (gloo): split order, id all-gather, object gather."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from opus_pllm_amd import dist as odist


def test_shard_bounds_match_accelerate_split():
    # accelerate.split_between_processes: first n % world ranks get one extra, contiguous, order-preserving
    for n in (0, 1, 7, 8, 9, 64, 513):
        for world in (1, 2, 3, 8):
            parts = [odist.split_between_processes(list(range(n)), r, world) for r in range(world)]
            assert [x for p in parts for x in p] == list(range(n))
            sizes = [len(p) for p in parts]
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    odist.init_process_group("gloo", rank, world, timeout_s=120)
    try:
        n = 7                                         # 7 inputs over 2 ranks -> 4 + 3
        lo, hi = odist.shard_bounds(n, rank, world)
        n_new = 5 if rank == 0 else 3                  # ranks may stop at different lengths (EOS)
        local = torch.arange(lo, hi)[:, None] * 100 + torch.arange(n_new)[None, :]
        allg = odist.all_gather_ids(local, pad_id=-1)
        objs = odist.gather_object([f"r{rank}-{i}" for i in range(lo, hi)])
        logits = odist.all_gather_logits(torch.arange(lo, hi, dtype=torch.float32)[:, None] + torch.arange(6)[None, :] / 8)
        q.put((rank, allg.tolist(), objs, logits.tolist()))
    finally:
        dist.destroy_process_group()


def test_all_gather_ids_and_objects_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    expect = [[i * 100 + j if j < (5 if i < 4 else 3) else -1 for j in range(5)] for i in range(7)]
    for rank, allg, objs, logits in res:
        assert allg == expect                            # same on every rank, rows in input order
        assert objs == [f"r{0 if i < 4 else 1}-{i}" for i in range(7)]
        assert logits == [[i + j / 8 for j in range(6)] for i in range(7)]      # uneven shards (4 + 3 rows), rank order


def test_single_process_passthrough():
    t = torch.arange(6).view(2, 3)
    assert odist.all_gather_ids(t) is t and odist.gather_object([1, 2]) == [1, 2]


# ------------------------------------------------------------------------------------------------ bench.py launch plumbing
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(args, env_extra, timeout=300):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_gpus2_starts_two_ranks_by_itself():
    """`python bench.py --gpus 2` with no launcher: the parent starts 2 ranks (torch.distributed.run on 127.0.0.1), they
    rendezvous (gloo here), run the same sequence of collectives - the timed loops of both workloads, the max-reduce, the rank
    census - and rank 0 prints ONE line with n_gpus = 2.  OPUS_BENCH_DRYRUN replaces the model by a stub (no GPU in this
    container): what is covered is the launch / collective plumbing that deadlocked in round 1's review."""
    import json
    r = _run_bench(["--gpus", "2", "--batch", "3", "--steps", "2", "--warmup", "1", "--new-tokens", "4", "--full"],
                   {"OPUS_BENCH_DRYRUN": "1", "OPUS_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["invalid"] is True
    assert d["config"]["batch_per_gpu"] == 3 and d["scaling"] == "weak" and "c2" in d
    assert d["value"] > 0 and abs(d["value"] - 2 * 3 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    rk = d["ranks"]                                               # the N > 1 line tells a slow rank from a slow collective
    assert rk["rank_census"] == [0, 1] and rk["path_ms_per_rank"]["min"] <= rk["path_ms_per_rank"]["max"]
    assert rk["id_gather_ms"]["min"] >= 0 and 0 <= rk["path_ms_per_rank"]["slowest_rank"] < 2


def test_bench_gpus8_plumbing_dry_run():
    """The driver's N = 8 line, plumbing only (8 CPU ranks, gloo, stub workload): self-launch, rendezvous, the sequence of
    collectives of both workloads, the per-rank diagnostics and ONE JSON line with n_gpus = 8."""
    import json
    r = _run_bench(["--gpus", "8", "--batch", "2", "--steps", "2", "--warmup", "1", "--new-tokens", "3", "--full"],
                   {"OPUS_BENCH_DRYRUN": "1", "OPUS_BENCH_BACKEND": "gloo"}, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["batch_per_gpu"] == 2 and d["invalid"] is True
    assert abs(d["value"] - 8 * 2 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert d["ranks"]["rank_census"] == list(range(8))
    assert set(d["ranks"]["path_ms_per_rank"]) == {"min", "median", "max", "slowest_rank"}


def test_bench_plain_run_measures_the_headline_only():
    """Without --full a run times the headline steps and prints their line: no batch-1 sub-run and no rank diagnostics
    (--full and the tests above have them)."""
    import json
    r = _run_bench(["--gpus", "2", "--batch", "3", "--steps", "2", "--warmup", "1", "--new-tokens", "4"],
                   {"OPUS_BENCH_DRYRUN": "1", "OPUS_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["collective_backend"] == "gloo"
    assert abs(d["value"] - 2 * 3 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert "c2" not in d and "ranks" not in d and "batch 1" not in r.stderr, d


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    r = _run_bench(["--gpus", "2"], {"OPUS_BENCH_DRYRUN": "1", "WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)
    r = _run_bench(["--gpus", "1"], {"OPUS_BENCH_DRYRUN": "1", "WORLD_SIZE": "2", "RANK": "0", "OPUS_BENCH_BACKEND": "gloo"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_bench_dump_outputs_dry_run(tmp_path):
    """--dump-outputs DIR: after the timed steps rank 0 writes the ids the last timed step returned - every rank's, in rank
    order - as DIR/ids.npy (and DIR/c2_ids.npy for the batch-1 line), float64; the line says what it wrote."""
    import json
    import numpy as np
    out = tmp_path / "dump"
    r = _run_bench(["--gpus", "2", "--batch", "3", "--steps", "3", "--warmup", "1", "--new-tokens", "4", "--dump-outputs", str(out)],
                   {"OPUS_BENCH_DRYRUN": "1", "OPUS_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dumped_outputs"]["arrays"] == ["c2_ids", "ids"]
    ids, c2 = np.load(out / "ids.npy"), np.load(out / "c2_ids.npy")
    assert ids.dtype == np.float64 and c2.dtype == np.float64
    stub = lambda b, rank: np.arange(b * 4).reshape(b, 4) + 1000 * rank           # bench.DryWorkload's ids
    assert np.array_equal(ids, np.concatenate([stub(3, 0), stub(3, 1)]))
    assert np.array_equal(c2, np.concatenate([stub(1, 0), stub(1, 1)]))


def test_bench_rejects_zero_steps():
    r = _run_bench(["--gpus", "1", "--steps", "0"], {"OPUS_BENCH_DRYRUN": "1"})
    assert r.returncode != 0 and "--steps" in r.stderr
