"""Scrub against what a caller did before it, in one process.

The C3 shape: RS(10,4), 4 MiB shards, 96 stripes from alloc_stripes, clean
codewords.  After a warm-up, `--rounds` rounds alternate (order shuffled per
round, so no arm always follows the same one), each arm timed with device
events as the median of `--reps` launches:

  A       the scrub launch (init + verify + locate), the library's default form
  A_alt   the same with ECGPU_SCRUB_LATE flipped: the parity columns loaded
          with the sources instead of after the combine (or the reverse)
  B       the encode-plan launch into a separate scratch parity slab
  C       B plus the torch comparison of the 4 parity pairs -- the scrub a
          caller had to write before ecgpu_scrub_*

then A alone with one stripe's data shard fully corrupted and with a data
shard of every stripe corrupted (the atomic path and the locate kernel).

Writes JSON (medians, min / max over the rounds, build IDs, algorithmic bytes
and the two expectations: A within B's own spread, A below C) to --out and
prints it.

    python tools/scrub_bench.py [--rounds 20] [--reps 5] [--out profiles/scrub_c3.json]
"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import erasure_coding_test_amd as E  # noqa: E402
from erasure_coding_test_amd import _native as N  # noqa: E402

K, M_, SIZE, STRIPES = 10, 4, 4 << 20, 96


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    matrix = E.reed_sol.reed_sol_vandermonde_coding_matrix(K, M_, 8)
    slab, shards = E.alloc_stripes(STRIPES, K, M_, SIZE, dev)
    slab.random_(0, 256)
    data, coding = [st[:K] for st in shards], [st[K:] for st in shards]
    enc = E.encode_plan(K, M_, matrix, 0).bind(data, coding, SIZE)
    enc.launch()  # the stripes are codewords from here on
    scratch = torch.empty((STRIPES, M_, slab.shape[2]), dtype=torch.uint8, device=dev)
    enc_b = E.encode_plan(K, M_, matrix, 0).bind(data, [[scratch[s, i, :SIZE] for i in range(M_)]
                                                        for s in range(STRIPES)], SIZE)
    scrub = E.ScrubPlan(K, M_, matrix, 0).bind_stripes(shards, SIZE)
    stored, fresh = slab[:, K:, :SIZE], scratch[:, :, :SIZE]
    verdict = []

    def run_a():
        scrub.launch(stream.cuda_stream)

    late = N.get_knob("ECGPU_SCRUB_LATE")

    def run_a_alt():
        N.set_knob("ECGPU_SCRUB_LATE", 0 if late else 1)
        scrub.launch(stream.cuda_stream)
        N.set_knob("ECGPU_SCRUB_LATE", late)

    def run_b():
        enc_b.launch(stream.cuda_stream)

    def run_c():
        enc_b.launch(stream.cuda_stream)
        verdict[:] = [(stored == fresh).all()]  # stays on the device: no host round trip in the timing

    arms = [("A", run_a), ("A_alt", run_a_alt), ("B", run_b), ("C", run_c)]
    for _, fn in arms:  # warm-up
        bench.time_launches(fn, stream, 3, 2)
    assert all(r.clean for r in scrub.results()), "the clean slab does not scrub clean"
    assert bool(verdict[0]), "the caller's own compare disagrees"
    ts = {name: [] for name, _ in arms}
    for r in range(a.rounds):
        order = list(arms)
        random.Random(r).shuffle(order)
        for name, fn in order:
            ts[name].append(bench.time_launches(fn, stream, a.reps, 1))
    unit = SIZE * STRIPES
    out = {"shape": {"k": K, "m": M_, "shard_bytes": SIZE, "stripes": STRIPES, "stride": int(slab.shape[2])},
           "rounds": a.rounds, "reps_per_round": a.reps, "scrub_late": {"A": late, "A_alt": 0 if late else 1},
           "device": torch.cuda.get_device_name(0),
           "build_ids": {n: N.lib.ecgpu_build_id(i).decode()
                         for i, n in enumerate(("build", "kernels", "wide", "packets", "scrub"))},
           "algorithmic_bytes": {"A": (K + M_) * unit, "B": (K + M_) * unit, "C": (K + M_ + 2 * M_) * unit},
           "arms": {name: stats(v) for name, v in ts.items()}}
    for name, nbytes in out["algorithmic_bytes"].items():
        out["arms"][name]["GBps"] = round(nbytes / (out["arms"][name]["median_ms"] / 1e3) / 1e9, 1)
    out["arms"]["A_alt"]["GBps"] = round(out["algorithmic_bytes"]["A"] / (out["arms"]["A_alt"]["median_ms"] / 1e3) / 1e9, 1)
    b = out["arms"]["B"]
    margin = b["max_ms"] - b["min_ms"]  # B's spread (max - min) / median, times its median
    out["expectation"] = {
        "b_spread": round(margin / b["median_ms"], 4),
        "a_limit_ms": round(b["median_ms"] + margin, 4),
        "a_within_b_spread": out["arms"]["A"]["median_ms"] <= b["median_ms"] + margin,
        "a_alt_within_b_spread": out["arms"]["A_alt"]["median_ms"] <= b["median_ms"] + margin,
        "a_below_c": out["arms"]["A"]["max_ms"] < out["arms"]["C"]["min_ms"]}

    # the atomic path: one stripe's data shard, then a data shard of every stripe, XORed with non-zero bytes
    noise = torch.randint(1, 256, (SIZE,), dtype=torch.uint8, device=dev)
    damaged = {}
    for label, stripes in (("A_one_stripe_corrupt", [STRIPES // 2]), ("A_every_stripe_corrupt", list(range(STRIPES)))):
        for s in stripes:
            if s not in damaged:
                damaged[s] = (3 * s) % K
                shards[s][damaged[s]].bitwise_xor_(noise)
        v = [bench.time_launches(run_a, stream, a.reps, 1) for _ in range(max(3, a.rounds // 2))]
        res = scrub.results()
        assert all(res[s].bad_cols == SIZE and res[s].suspects == [j] for s, j in damaged.items()), label
        assert all(r.clean for s, r in enumerate(res) if s not in damaged), label
        out["arms"][label] = stats(v)
    for s, j in damaged.items():
        shards[s][j].bitwise_xor_(noise)
    run_a()
    assert all(r.clean for r in scrub.results())
    assert N.fallback_count() == 0 and N.cpu_call_count() == 0
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
