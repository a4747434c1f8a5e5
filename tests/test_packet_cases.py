"""tests/packet_cases.py checked without a GPU: the builders have the
properties the GPU sweep (tests/test_packet_kernels_gpu.py) relies on, the
replay reference agrees with direct evaluation of the bit-matrices, and every
case run on host arrays through the library's CPU executor (ECGPU_GPU=0, a
child process as in tests/test_cpu_exec.py) equals the replay bit for bit --
so the expectations are proven before any GPU run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import packet_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fused(c):
    """{output (dev, row): set of source (dev, row)} of the case's schedule by
    set algebra over GF(2) -- and the outputs whose set is themselves alone
    are dropped: unchanged content is no output."""
    state = {}

    def get(key):
        return state.get(key, frozenset([key]))
    for sd, sr, dd, dr, x in c.ops:
        state[(dd, dr)] = get((dd, dr)) ^ get((sd, sr)) if x else get((sd, sr))
    return {d: s for d, s in state.items() if s != frozenset([d])}


def test_exact_map_has_exactly_its_nsrc_and_r():
    ran = 0
    for nsrc in pc.NSRCS:
        for R in pc.RS:
            for spread in (False, True):
                c = pc.exact_map(nsrc, R, pc.rng_for(1, nsrc, R), spread=spread)
                f = fused(c)
                assert len(f) == R and all(f.values()), c.name          # R outputs, none empty
                assert len(set().union(*f.values())) == nsrc, c.name    # every source used
                assert not set(f) & set().union(*f.values()), c.name    # no output is a source
                assert (c.k, c.m, c.w) == ((nsrc, R, 1) if spread else (1, 1, max(nsrc, R)))
                M = np.asarray(c.bm)
                assert M.shape == (R, nsrc) and M.any(axis=0).all() and M.any(axis=1).all()
                ran += 1
    assert ran == 2 * len(pc.NSRCS) * len(pc.RS) == 180
    assert sorted({n >> 2 for n in pc.NSRCS}) == [0, 1, 2, 3, 4]
    for tail in range(4):  # every tail length after an even and after an odd number of chunks
        assert {(n >> 2) % 2 for n in pc.NSRCS if n % 4 == tail} == {0, 1}


def conforming(bm, k, m=4):
    """The unit form as the issue states it, on the bit-matrix: coding device 0
    identity blocks, data device 0 identity blocks into every coding device."""
    eye = np.eye(8, dtype=np.uint8)
    return (bm.shape == (m * 8, k * 8) and all(np.array_equal(bm[0:8, x * 8:x * 8 + 8], eye) for x in range(k))
            and all(np.array_equal(bm[i * 8:i * 8 + 8, 0:8], eye) for i in range(m)))


@pytest.mark.parametrize("k", pc.UNIT_KS)
def test_unit_shaped_is_conforming_and_otherwise_random(k):
    c = pc.unit_shaped(k, pc.rng_for(2, k))
    bm = np.asarray(c.bm)
    assert conforming(bm, k) and (c.k, c.m, c.w) == (k, 4, 8)
    assert bm.any(axis=1).all() and bm.any(axis=0).all()  # no all-zero output, no unused source
    if k >= 3:
        free = bm[8:, 8:]
        assert 0.3 < free.mean() < 0.7  # the free bits are random, not a Vandermonde pattern


def test_near_misses_differ_in_exactly_the_stated_place():
    k = 3
    nm = pc.near_misses(k, pc.rng_for(3, k))
    assert [v for v, _, _ in pc.NEAR_MISSES] == list(nm) == ["a", "b", "c", "d", "e", "f"]
    for v, (c, base, cells) in nm.items():
        assert conforming(base, k), v
        bm = np.asarray(c.bm)
        if v == "e":
            assert bm.shape == (24, k * 8) and np.array_equal(bm, base[:24]) and c.m == 3
            continue
        diff = sorted(map(tuple, np.argwhere(bm != base)))
        assert diff == sorted(cells), v
        assert bm.any(axis=1).all(), v  # no all-zero output row
    (r, col), = nm["a"][2]
    assert r < 8 and col >= 8 and nm["a"][1][r, col] == 0           # an extra low-8 bit, source >= 8
    (r, col), = nm["b"][2]
    assert col < 8 and r >= 8 and r % 8 == col and nm["b"][1][r, col] == 1  # an identity bit of device 0, removed
    (r, col), = nm["c"][2]
    assert col < 8 and r >= 8 and r % 8 != col and nm["c"][1][r, col] == 0  # an extra bit on device 0, above the low 8
    cols = {c for _, c in nm["d"][2]}
    assert len(cols) == 1 and min(cols) >= 8 and not np.asarray(nm["d"][0].bm)[:, min(cols)].any()
    used = np.asarray(nm["d"][0].bm).any(axis=0).sum()
    assert used == k * 8 - 1 and used % 8 != 0
    assert nm["f"][2] == [] and pc.NEAR_MISS_OFFSET == {"f": 8}


def test_two_unit_groups_both_conform():
    k = 3
    bm = np.asarray(pc.two_unit_groups(k, pc.rng_for(4, k)).bm)
    assert bm.shape == (64, k * 8) and conforming(bm[:32], k) and conforming(bm[32:], k)
    assert not np.array_equal(bm[:32], bm[32:])


@pytest.mark.parametrize("rows", sorted(pc.ACCUMULATE_LAUNCHES))
def test_accumulate_reads_every_destination(rows):
    f = fused(pc.accumulate(rows))
    assert len(f) == rows and all(f.values())
    srcs = set().union(*f.values())
    assert srcs == {(s, p) for s in (0, 1) for p in range(rows)}  # every old destination packet is a source
    assert (rows + 31) // 32 == pc.ACCUMULATE_LAUNCHES[rows]


def test_zero_cases_fold_to_zero_where_stated():
    for rows in pc.ALL_ZERO_GROUPS:
        c = pc.all_zero(rows)
        f = fused(c)
        assert sorted(f) == [(1, p) for p in range(rows)] and not any(f.values()) and c.w == rows + 2
    f = fused(pc.some_zero(9))
    assert [p for (_, p), s in sorted(f.items()) if not s] == [0, 3, 6] and len(f) == 9
    assert all(len(s) == 2 for (_, p), s in f.items() if p % 3)
    k = 2
    f = fused(pc.some_zero_beside_unit(k, pc.rng_for(6)))
    assert len(f) == 64 and sorted(d for d, s in f.items() if not s) == [(k + 4, 1), (k + 5, 0)]
    first = np.zeros((32, k * 8), dtype=np.uint8)
    for (dev, row), s in f.items():
        if dev < k + 4:
            for sd, sr in s:
                first[(dev - k) * 8 + row, sd * 8 + sr] = 1
    assert conforming(first, k)


def test_staging_and_dotprod_cases():
    c = pc.staging_bits(pc.rng_for(7))
    bm = np.asarray(c.bm)
    assert [r for r in range(10) if not bm[r].any()] == [2, 7] and bm.any(axis=0).all()
    assert len(fused(c)) == 8
    for ids, dest in pc.DOTPRODS:
        assert sorted(ids + [dest]) != list(range(3)) and max(ids) >= 3 and dest not in ids
        d = pc.dotprod_case(3, 2, 3, ids, dest, pc.rng_for(8, dest))
        f = fused(d)
        assert sorted(f) == [(dest, j) for j in range(3)] and all(f.values())
        assert {sd for s in f.values() for sd, _ in s} <= set(ids)
    assert {dest < 3 for _, dest in pc.DOTPRODS} == {True, False}
    assert len(pc.DECODE_SETS) == 16


def test_replay_vectorised_equals_one_super_packet_after_the_other():
    rng = pc.rng_for(11)
    for c, nsp, ps in [(pc.accumulate(40), 5, 5), (pc.some_zero(9), 4, 8), (pc.sweep_case(13, 17), 3, 16)]:
        size = nsp * c.w * ps
        slots = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(c.k + c.m)]
        a = pc.replay(c.ops, slots, nsp, c.w * ps, ps)
        b = pc.replay_literal(c.ops, slots, nsp, c.w * ps, ps)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), c.name


def test_replay_equals_direct_evaluation_of_the_bitmatrices():
    """The lowering (first set bit copies, later ones XOR, a zero row writes
    nothing) and the replay against the XOR of the named packets."""
    rng = pc.rng_for(12)
    cases = [pc.unit_shaped(k, pc.rng_for(2, k)) for k in pc.UNIT_KS]
    cases += [c for c, _, _ in pc.near_misses(3, pc.rng_for(3, 3)).values()]
    cases += [pc.two_unit_groups(3, pc.rng_for(4, 3)), pc.staging_bits(pc.rng_for(7))]
    for c in cases:
        nsp, ps = 3, 5
        slots = [rng.integers(0, 256, nsp * c.w * ps, dtype=np.uint8) for _ in range(c.k + c.m)]
        a = pc.replay(c.ops, slots, nsp, c.w * ps, ps)
        b = pc.direct_bitmatrix(c.k, c.m, c.w, np.asarray(c.bm), slots, nsp, ps)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), c.name
    # exact_map: output r is the XOR of the sources M[r] names
    c = pc.sweep_case(11, 9)
    slots = [rng.integers(0, 256, 2 * 11 * 8, dtype=np.uint8) for _ in range(2)]
    out = pc.replay(c.ops, slots, 2, 11 * 8, 8)[1].reshape(2, 11, 8)
    src = slots[0].reshape(2, 11, 8)
    for r in range(9):
        want = np.bitwise_xor.reduce(src[:, np.flatnonzero(np.asarray(c.bm)[r]), :], axis=1)
        assert np.array_equal(out[:, r, :], want)
    assert np.array_equal(out[:, 9:, :], slots[1].reshape(2, 11, 8)[:, 9:, :])


def test_every_case_on_the_cpu_executor_equals_the_replay():
    env = {k: v for k, v in os.environ.items()
           if k not in ("ECGPU_GPU", "EC_GPU", "ECGPU_MIN_OFFLOAD_KIB", "ECGPU_CPU_SIMD", "ECGPU_PACKET")}
    env.update(ECGPU_GPU="0", ECGPU_CPU_FALLBACK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "packet_cases.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(lines[-1])
    assert out["mismatches"] == [] and out["fallbacks"] == 0, out
    # 90 sweep maps + 5 unit + 6 near misses + two groups + spread + 9 accumulate + 2 + 2 zero + staging + 2 dot
    # products + 2 x 17 decodes; the decode without an erasure and the two refused ones execute nothing
    assert out["checked"] == 90 + 5 + 6 + 1 + 1 + 9 + 2 + 2 + 1 + 2 + 34, out
    assert out["cpu_calls"] == out["checked"] - 4, out
    assert out["launches"] == [0] * pc.KINDS, out
