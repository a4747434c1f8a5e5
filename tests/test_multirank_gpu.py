"""The product library under more than one rank, on the GPU.

SURVEY.md §8e: stripes are independent, so ranks shard them round-robin
(rank r codes global stripe ids r, r+N, ...) with no data-path collective.
Here two rank processes share cuda:0 (the one-GPU box) and each codes its own
stripes through the library -- batched plan encode, the fused decode of
erasures {0,1,2,3} (C4's pattern), and the synchronous drop-in decode -- and
the union of their results is checked against the CPU oracle on the same
seeded stripes: every stripe coded exactly once, bytes identical.

Also bench.py itself: a plain run with --dump-outputs; `--full --gpus 2` with the one-device
rehearsal flag spawns two ranks and reports both; without it a one-GPU box
refuses with a non-zero exit; `--config C5` runs and names C5.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M_PAR, SIZE, TOTAL, CFG = 10, 4, (256 << 10) + 48, 6, 21
ERASED = [0, 1, 2, 3]
DROPIN_ERASED = [1, 5, 11]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        import torch

        import bench
        import erasure_coding_test_amd as E
        from ecdata import fnv1a64, shard_seed, splitmix_bytes

        r, _, w = bench.dist_setup()
        assert (r, w) == (rank, world)
        torch.cuda.set_device(0)  # both ranks on the one GPU of the box
        dev = torch.device("cuda", 0)
        ids = bench.stripes_for_rank(TOTAL, rank, world)
        Mx = E.reed_sol.reed_sol_vandermonde_coding_matrix(K, M_PAR, 8)
        slab, shards = E.alloc_stripes(len(ids), K, M_PAR, SIZE, dev)
        originals = {}
        for b, s in enumerate(ids):
            for j in range(K):
                shards[b][j].copy_(torch.from_numpy(splitmix_bytes(SIZE, shard_seed(CFG, s, j))))
        enc = E.encode_plan(K, M_PAR, Mx, 0).bind([st[:K] for st in shards], [st[K:] for st in shards], SIZE)
        enc.launch()
        torch.cuda.synchronize()
        mine = {}
        for b, s in enumerate(ids):
            originals[s] = [t.clone() for t in shards[b]]
            mine[s] = {"parity": [fnv1a64(t.cpu().numpy()) for t in shards[b][K:]]}
        # C4's worst-case pattern, batched over this rank's stripes
        for b in range(len(ids)):
            for e in ERASED:
                shards[b][e].zero_()
        dec = E.DecodePlan(K, M_PAR, Mx, ERASED, 0, 0).bind_stripes(shards, SIZE)
        dec.launch()
        torch.cuda.synchronize()
        for b, s in enumerate(ids):
            mine[s]["decode_ok"] = all(bool(torch.equal(shards[b][i], originals[s][i])) for i in range(K + M_PAR))
        # the synchronous drop-in decode (reference semantics) on host buffers
        s0 = ids[0]
        host = [originals[s0][i].cpu().numpy().copy() for i in range(K + M_PAR)]
        for e in DROPIN_ERASED:
            host[e][:] = 0
        rc = E.jerasure.jerasure_matrix_decode(K, M_PAR, 8, Mx, 0, DROPIN_ERASED, host[:K], host[K:], SIZE)
        mine[s0]["dropin_rc"] = rc
        mine[s0]["dropin_ok"] = all(np.array_equal(host[i], originals[s0][i].cpu().numpy()) for i in range(K + M_PAR))
        bench.barrier(world)
        t = bench.max_over_ranks(float(rank + 1), world)
        gathered = bench.gather(mine, world)
        import torch.distributed as dist
        dist.destroy_process_group()
        q.put((rank, t, gathered, None))
    except BaseException as ex:  # report, never hang the parent
        q.put((rank, None, None, repr(ex)))
        raise


def test_two_ranks_code_their_stripes_with_the_library(gpu):
    import torch.multiprocessing as mp

    from ecdata import fnv1a64, shard_seed, splitmix_bytes
    from oracle.oracle import Restatement, alloc_shards
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, t, gathered, err in results:
        assert err is None, f"rank {rank}: {err}"
        assert t == float(world)
    for p in procs:
        assert p.exitcode == 0
    gathered = results[0][2]
    merged = {}
    for part in gathered:
        assert not (set(part) & set(merged)), "a stripe was coded by two ranks"
        merged.update(part)
    assert sorted(merged) == list(range(TOTAL))
    o = Restatement()
    Mx = o.vandermonde_coding_matrix(K, M_PAR)
    for s in range(TOTAL):
        data = alloc_shards(K, SIZE)
        for j in range(K):
            data[j][:SIZE] = splitmix_bytes(SIZE, shard_seed(CFG, s, j))
        coding = alloc_shards(M_PAR, SIZE)
        o.matrix_encode(K, M_PAR, Mx, data, coding, SIZE)
        assert merged[s]["parity"] == [fnv1a64(c[:SIZE]) for c in coding], s
        assert merged[s]["decode_ok"], s
    for s in (0, 1):  # each rank's first stripe went through the drop-in decode
        assert merged[s]["dropin_rc"] == 0 and merged[s]["dropin_ok"], s


def _bench(args, env_extra=None, timeout=180):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def _line(out):
    # stdout is exactly the one JSON line (gloo's connection reports go to stderr)
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out
    return json.loads(lines[0])


@pytest.mark.timeout(420)
def test_bench_gpus2_rehearsal_spawns_two_ranks(gpu):
    # the N > 1 line is complete: rank 0's CPU baseline on
    # its stripe 0, every rank's encode / decode fractions and configs block
    # (incl. C4), the worst-rank roofline fraction beside rank 0's
    r = _bench(["--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--stripes", "4", "--cpu-seconds", "1"],
               {"ECGPU_BENCH_ONE_DEVICE": "1"}, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 2 and d["rehearsal"] is True
    assert [p["rank"] for p in d["per_rank"]] == [0, 1]
    assert all(p["parity_ok"] for p in d["per_rank"])
    assert [p["stripe_ids"] for p in d["per_rank"]] == [[0, 6, 4], [1, 7, 4]]  # round-robin global ids
    assert d["selfcheck_parity_ok"] is True
    roof = d["roofline"]
    assert roof["frac"] > 0 and len(roof["frac_per_rank"]) == 2
    assert roof["frac_worst_rank"] == min(roof["frac_per_rank"])
    # the contract's achieved: algorithmic bytes / the AVERAGE timed launch (round 6)
    want = roof["algorithmic_bytes_per_launch"] / (roof["mean_launch_ms"] / 1e3) / 1e9 / roof["peak"]
    assert abs(roof["frac"] - want) < 2e-3, (roof["frac"], want)
    assert roof["mean_launch_ms"] > 0 and roof["median_launch_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    assert d["selfcheck_vs_reference_cpu"] is True
    for p in d["per_rank"]:
        assert p["encode_frac"] > 0 and p["decode_frac"] > 0
        assert {"C2_encode", "C3_encode", "C3_decode_0", "C3_decode_parity", "C3_decode_data_random",
                "C4_decode_0123", "C5_encode"} <= set(p["configs"])
        assert p["configs"]["C4_decode_0123"]["frac"] > 0
    assert d["configs"]["C3_decode_parity"]["algorithmic_bytes_per_launch"] == 11 * (4 << 20) * 4
    # PCIe-inclusive host-pipeline rates: every rank runs
    # its own pass at once after the timed work; the line carries each rank's
    # rates (and where its pinned buffers live) and the whole job's
    e2e = d["e2e"]
    assert e2e["encode"]["parity_ok"] and e2e["encode"]["data_GiBps"] > 1
    assert e2e["decode"]["rebuilt_ok"] and e2e["decode"]["erasures"] == [0]
    assert d["e2e_ok"] is True
    assert len(d["e2e_per_rank"]) == 2 and d["e2e_per_rank"][0] == e2e
    for r_ in d["e2e_per_rank"]:
        assert r_["encode"]["parity_ok"] and r_["decode"]["rebuilt_ok"] and "host_numa_node" in r_
        assert "gpu_numa_node" in r_ and "threads_on_gpu_node" in r_
    agg = d["e2e_aggregate"]
    assert agg["ranks"] == 2 and agg["encode"]["ok"] and agg["decode"]["ok"]
    assert agg["encode"]["data_GiBps"] > 0 and len(agg["encode"]["per_rank_GiBps"]) == 2
    assert d["cpu_fallbacks"] == 0 and all(p["cpu_fallbacks"] == 0 for p in d["per_rank"])
    # each rank names its physical GPU; both sit on cuda:0 here, which the
    # rehearsal flag exempts from the distinct-device check
    buses = [p["pci_bus_id"] for p in d["per_rank"]]
    assert all(b and b.count(":") == 2 for b in buses) and buses[0] == buses[1], buses
    assert d["distinct_devices_ok"] is True and "rehearsal" in d["distinct_devices"]
    assert d["cpu_baseline_per_gpu_share"]["cores"] >= 1 and d["cpu_baseline_all_cores"]["cores"] >= 1
    # BASELINE config 5 as a whole job over both ranks (barrier-bracketed, slowest rank)
    c5 = d["c5_sharded"]
    assert c5["n_gpus"] == 2 and c5["parity_ok"] is True and c5["data_GiBps"] > 0 and c5["hbm_frac_per_gpu"] > 0


def test_bench_gpus_beyond_visible_devices_fails(gpu):
    import torch
    n = torch.cuda.device_count()
    r = _bench(["--gpus", str(n + 1), "--steps", "1", "--warmup", "0", "--cpu-seconds", "0"], timeout=60)
    assert r.returncode != 0
    assert "visible GPUs" in r.stderr


def test_bench_config_c5(gpu):
    r = _bench(["--full", "--config", "C5", "--stripes", "2", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                "--no-configs"])
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["config"]["workload"].startswith("C5: RS(12,4)")
    assert (d["config"]["k"], d["config"]["m"], d["config"]["shard_bytes"]) == (12, 4, 16 << 20)
    assert d["decode_kernel"] is None and d["selfcheck_parity_ok"] is True
    assert d["e2e"]["encode"]["parity_ok"] and "decode" not in d["e2e"]  # C5 has no decode


def test_bench_plain_run_is_lean_and_dumps_its_outputs(gpu, tmp_path, capfd):
    """A plain run (no --full) times the steps and prints the line with every
    further measurement absent; --dump-outputs writes the last step's parity
    and rebuilt shards as float32, identically for both multiply engines on the
    same seeded inputs (so two builds compare output for output)."""
    import bench
    lines, dumps = {}, {}
    for kernel in ("perm", "lds"):
        out = tmp_path / kernel
        capfd.readouterr()
        rc = bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--stripes", "2", "--kernel", kernel,
                         "--dump-outputs", str(out)])
        assert rc == 0
        lines[kernel] = _line(capfd.readouterr().out)
        dumps[kernel] = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    d = lines["perm"]
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["metric"] == bench.HEADLINE_METRIC
    # ms_per_step is the wall time of one timed step: value's own denominator
    want = 3 * 2 * 2 * 10 * (4 << 20) / (d["ms_per_step"] * 3 / 1e3) / 2**30
    # the line rounds ms_per_step to 1e-4 ms and value to 1e-3 GiB/s
    assert abs(d["value"] - want) <= want * 1e-4 / d["ms_per_step"] + 2e-3, (d["value"], want)
    assert len(d["per_rank"][0]["encode_launch_ms"]) == 3  # --steps sets the number of timed steps
    for moved in ("configs", "c5_sharded", "cpu_baseline", "cpu_baseline_per_gpu_share", "cpu_baseline_all_cores",
                  "cpu_baseline_o3", "e2e", "copy_ceiling", "xor_stream_probe", "selfcheck_parity_ok",
                  "selfcheck_vs_reference_cpu", "e2e_ok"):
        assert d[moved] is None, moved
    assert d["cpu_fallbacks"] == 0 and d["cpu_calls"] == 0
    names = ["parity_edges.npy", "parity_sample.npy", "rebuilt_edges.npy", "rebuilt_sample.npy"]
    assert sorted(d["outputs_dumped"]) == names == sorted(dumps["perm"])
    total = 0
    for f in names:
        a, b = dumps["perm"][f], dumps["lds"][f]
        assert a.dtype == np.float32 and list(a.shape) == d["outputs_dumped"][f]
        assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.floor(a))  # bytes
        assert np.array_equal(a, b), f  # same inputs, the other engine: the same bytes
        total += a.nbytes
    assert total <= 64 * 10**6
    assert dumps["perm"]["parity_edges.npy"].shape == (2, 4, 2 * bench.DUMP_EDGE_BYTES)
    assert dumps["perm"]["rebuilt_edges.npy"].shape == (2, 1, 2 * bench.DUMP_EDGE_BYTES)
    assert dumps["perm"]["parity_sample.npy"].shape == (bench.DUMP_SAMPLE_BYTES,)
    assert len(np.unique(dumps["perm"]["parity_sample.npy"])) == 256  # random data: not a blank buffer
