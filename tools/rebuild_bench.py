"""A rebuild whose stripes lost different shards: one RebuildPlan launch
against what a caller did before it, in one process.

Two shapes, RS(10,4), shards from alloc_stripes, every stripe a codeword:

  S1  4 MiB shards, 96 stripes; stripe s lost shard s % 14 (a failed device
      under rotated placement): 14 patterns, all one output row
  S2  64 KiB shards, 1365 stripes; stripe s lost the (s % 91)-th pair of
      shards: 91 patterns, one or two data shards among them

After a warm-up, `--rounds` rounds alternate (order shuffled per round), each
arm timed with device events as the median of `--reps` launches:

  A   the RebuildPlan launch: one multi-map launch per (n_out, n_src) group
  B   one DecodePlan per pattern, all bound beforehand, launched back to back
      on one stream -- what a caller did before ecgpu_multiplan_*
  C   context only: ONE DecodePlan over all stripes as if every stripe had
      lost the same shards ({0} for S1, {0, 1} for S2), the specialised kernel
      with its unit structure

and the host time to create and bind A's and B's plans (median of 3).

Writes JSON (medians, min / max over the rounds, build IDs, algorithmic bytes
and the expectation: A's median within B's median plus B's own spread) to
--out and prints it.

    python tools/rebuild_bench.py [--rounds 20] [--reps 5] [--out profiles/rebuild.json]
"""
import argparse
import itertools
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import erasure_coding_test_amd as E  # noqa: E402
from erasure_coding_test_amd import _native as N  # noqa: E402

K, M_ = 10, 4
PAIRS = list(itertools.combinations(range(K + M_), 2))
SHAPES = {
    "S1": {"size": 4 << 20, "stripes": 96, "erasures": lambda s: [s % (K + M_)], "uniform": [0]},
    "S2": {"size": 64 << 10, "stripes": 1365, "erasures": lambda s: list(PAIRS[s % len(PAIRS)]), "uniform": [0, 1]},
}
FAMILIES = ("build", "kernels", "wide", "packets", "scrub", "rebuild")


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def run_shape(name, spec, matrix, dev, stream, rounds, reps):
    size, stripes = spec["size"], spec["stripes"]
    slab, shards = E.alloc_stripes(stripes, K, M_, size, dev)
    slab.random_(0, 256)
    E.encode_plan(K, M_, matrix, 0).bind([st[:K] for st in shards], [st[K:] for st in shards], size).launch()
    erasures = [spec["erasures"](s) for s in range(stripes)]
    lost = [(s, e) for s in range(stripes) for e in erasures[s]]
    original = [shards[s][e].clone() for s, e in lost]

    def erase():
        for s, e in lost:
            shards[s][e].fill_(0xA5)

    def intact():
        torch.cuda.synchronize(dev)
        return all(torch.equal(shards[s][e], o) for (s, e), o in zip(lost, original))

    def make_a():
        return E.RebuildPlan(K, M_, matrix, 0).bind_stripes(shards, erasures, size)

    def make_b():
        by_pattern = {}
        for s, er in enumerate(erasures):
            by_pattern.setdefault(tuple(sorted(er)), []).append(s)
        return [E.DecodePlan(K, M_, matrix, list(p), device=0).bind_stripes([shards[s] for s in ss], size)
                for p, ss in by_pattern.items()]

    def close_b(plans):
        for p in plans:
            p.close()

    # host time to create and bind (the last set of plans is the one timed below)
    plan_a, v = None, []
    for _ in range(3):
        if plan_a:
            plan_a.close()
        t0 = time.perf_counter()
        plan_a = make_a()
        v.append((time.perf_counter() - t0) * 1e3)
    bind_a = round(sorted(v)[1], 3)
    plans_b, v = None, []
    for _ in range(3):
        if plans_b:
            close_b(plans_b)
        t0 = time.perf_counter()
        plans_b = make_b()
        v.append((time.perf_counter() - t0) * 1e3)
    bind_b = round(sorted(v)[1], 3)
    plan_c = E.DecodePlan(K, M_, matrix, spec["uniform"], device=0).bind_stripes(shards, size)

    def run_a():
        plan_a.launch(stream.cuda_stream)

    def run_b():
        for p in plans_b:
            p.launch(stream.cuda_stream)

    def run_c():
        plan_c.launch(stream.cuda_stream)

    arms = [("A", run_a), ("B", run_b), ("C", run_c)]
    for arm, fn in arms:  # warm-up; every arm leaves the codewords that were there
        if arm != "C":  # C's sources are only intact on whole codewords
            erase()
        bench.time_launches(fn, stream, 3, 2)
        assert intact(), f"{name} arm {arm}: the rebuilt shards differ from the originals"
    ts = {arm: [] for arm, _ in arms}
    for r in range(rounds):
        order = list(arms)
        random.Random(r).shuffle(order)
        for arm, fn in order:
            ts[arm].append(bench.time_launches(fn, stream, reps, 1))
    run_a()
    assert intact()
    moved = {"A": sum((g.n_src + g.n_out) * len(g.stripes) for g in plan_a.groups) * size,
             "C": (len(plan_c.src_ids) + len(plan_c.out_ids)) * stripes * size}
    moved["B"] = moved["A"]
    out = {"shape": {"k": K, "m": M_, "shard_bytes": size, "stripes": stripes, "stride": int(slab.shape[2]),
                     "patterns": len({tuple(sorted(e)) for e in erasures}),
                     "groups": [[g.n_out, g.n_src, len(g.maps), len(g.stripes)] for g in plan_a.groups]},
           "launches": {"A": len(plan_a.plans), "B": len(plans_b), "C": 1},
           "create_and_bind_host_ms": {"A": bind_a, "B": bind_b},
           "algorithmic_bytes": moved,
           "arms": {arm: stats(v) for arm, v in ts.items()}}
    for arm, nbytes in moved.items():
        out["arms"][arm]["GBps"] = round(nbytes / (out["arms"][arm]["median_ms"] / 1e3) / 1e9, 1)
    b = out["arms"]["B"]
    margin = b["max_ms"] - b["min_ms"]  # B's spread (max - min) / median, times its median
    out["expectation"] = {"b_spread": round(margin / b["median_ms"], 4),
                          "a_limit_ms": round(b["median_ms"] + margin, 4),
                          "a_within_b_spread": out["arms"]["A"]["median_ms"] <= b["median_ms"] + margin,
                          "a_over_b": round(out["arms"]["A"]["median_ms"] / b["median_ms"], 4),
                          "a_over_c": round(out["arms"]["A"]["median_ms"] / out["arms"]["C"]["median_ms"], 4)}
    plan_a.close()
    close_b(plans_b)
    plan_c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="S1,S2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    matrix = E.reed_sol.reed_sol_vandermonde_coding_matrix(K, M_, 8)
    out = {"rounds": a.rounds, "reps_per_round": a.reps, "device": torch.cuda.get_device_name(0),
           "build_ids": {n: N.lib.ecgpu_build_id(i).decode() for i, n in enumerate(FAMILIES)},
           "ecgpu_build_id": N.lib.ecgpu_build_id(FAMILIES.index("rebuild")).decode(),
           "shapes": {}}
    for name in a.shapes.split(","):
        out["shapes"][name] = run_shape(name, SHAPES[name], matrix, dev, stream, a.rounds, a.reps)
        torch.cuda.empty_cache()
    assert N.fallback_count() == 0 and N.cpu_call_count() == 0
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
