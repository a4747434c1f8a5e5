"""Stripes with different erasure patterns decoded in one launch on the MI355X
(RebuildPlan / MultiMapPlan / ecgpu_multiplan_*).

Expected bytes come from the live reference: every stripe is encoded with
jerasure_matrix_encode, its erased shards are overwritten with a filler, and
jerasure_matrix_decode runs per stripe with that stripe's own erasure list.
All k + m shards of every stripe are compared, and the slab around them (at
least 32 guard bytes behind each shard).  Raw multiplans with arbitrary maps
are checked against a numpy model over the reference's multiply table.  Sizes
are those of tests/test_scrub_gpu.py, for the same reasons: 16 one column;
4096 exactly one block; 4112 a second block with one live lane; 4099 and 1000
vector part plus byte tail; 7 and 1 the byte kernel only; 4096 with every
pointer offset by 1, unaligned, byte kernel only.
"""
import itertools

import numpy as np
import pytest

from oracle.oracle import alloc_shards

pytestmark = pytest.mark.gpu

SCHEMES = [(4, 2), (6, 3), (10, 4), (12, 4)]  # K > 10 takes the all-loads-first window
SIZES = [(16, 0), (4096, 0), (4112, 0), (4099, 0), (1000, 0), (7, 0), (1, 0), (4096, 1)]  # (size, pointer offset)
FILL = 0xA5    # what an erased shard holds before the rebuild
GUARD = 0x5C   # what the slab holds outside the shards
GUARD_BYTES = 32


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


@pytest.fixture(scope="module")
def mul(reference):
    """The reference's GF(2^8) multiply table, [a][b]."""
    return np.array([[reference.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)


@pytest.fixture(scope="module")
def scenario(reference):
    """scenario(k, m, size, erasures_per_stripe, seed=0) -> (matrix, damaged, want), both [stripes, k+m, size]
    uint8: the stripes as the rebuild finds them (erased shards = FILL) and as the reference's decode leaves
    them; computed once per key and never modified."""
    cache = {}

    def get(k, m, size, erasures, seed=0):
        key = (k, m, size, tuple(tuple(e) for e in erasures), seed)
        if key not in cache:
            Mnp = reference.vandermonde_coding_matrix(k, m)
            rng = np.random.default_rng([k, m, size, len(erasures), seed])
            damaged = np.zeros((len(erasures), k + m, size), dtype=np.uint8)
            want = np.zeros_like(damaged)
            for s, er in enumerate(erasures):
                data, coding = alloc_shards(k, size), alloc_shards(m, size)
                for j in range(k):
                    data[j][:size] = rng.integers(0, 256, size, dtype=np.uint8)
                reference.matrix_encode(k, m, Mnp, data, coding, size)
                for e in set(er):
                    (data + coding)[e][:size] = FILL
                for i, a in enumerate(data + coding):
                    damaged[s, i] = a[:size]
                if er:
                    assert reference.matrix_decode(k, m, Mnp, 0, sorted(set(er)), data, coding, size) == 0
                for i, a in enumerate(data + coding):
                    want[s, i] = a[:size]
            damaged.setflags(write=False)
            want.setflags(write=False)
            cache[key] = ([int(c) for c in Mnp.ravel()], damaged, want)
        return cache[key]

    return get


def frame(host, offset=0):
    """[stripes, n, size] shard bytes inside a GUARD-filled [stripes, n, stride] host slab."""
    stripes, n, size = host.shape
    full = np.full((stripes, n, (offset + size + GUARD_BYTES + 15) // 16 * 16), GUARD, dtype=np.uint8)
    full[:, :, offset:offset + size] = host
    return full


def upload(host, gpu, offset=0):
    """The stripes in one device slab; shard views start `offset` bytes past a 16-B boundary."""
    import torch
    size = host.shape[2]
    slab = torch.from_numpy(frame(host, offset)).to(gpu)
    shards = [[slab[s, i, offset:offset + size] for i in range(host.shape[1])] for s in range(host.shape[0])]
    assert all(sh.data_ptr() % 16 == offset for st in shards for sh in st)
    return slab, shards


def assert_slab(slab, want, offset=0):
    got, exp = slab.cpu().numpy(), frame(want, offset)
    if not np.array_equal(got, exp):
        s, i, x = (int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError(f"first difference at stripe {s}, shard {i}, slab byte {x} "
                             f"(shard byte {x - offset}): got {got[s, i, x]:#x}, want {exp[s, i, x]:#x}")


def model(mul, coefs, srcs):
    """[R, size] = coefs[R][K] applied to srcs [K, size] over the reference's multiply table."""
    out = np.zeros((len(coefs), srcs.shape[1]), dtype=np.uint8)
    for r, row in enumerate(coefs):
        for j, c in enumerate(row):
            out[r] ^= mul[c][srcs[j]]
    return out


def mixed(k, m):
    """No erasure, one data, one parity, data + parity, two data, m data."""
    return [[], [1], [k + m - 1], [k - 1, k], [0, 2], list(range(m)), [k]]


@pytest.mark.parametrize("size,offset", SIZES)
@pytest.mark.parametrize("k,m", SCHEMES)
def test_schemes_and_sizes(ec, gpu, scenario, k, m, size, offset):
    erasures = mixed(k, m)
    M, damaged, want = scenario(k, m, size, erasures)
    slab, shards = upload(damaged, gpu, offset)
    plan = ec.RebuildPlan(k, m, M).bind_stripes(shards, erasures, size)
    assert all(isinstance(p, ec.MultiMapPlan) for p in plan.plans) and len(plan.plans) == len(plan.groups) <= m
    assert {(p.rows, p.nsrc) for p in plan.plans} == {(1, k), (2, k), (m, k)}
    assert all(p.engine == (0 if offset == 0 and size >= 16 else 1) for p in plan.plans)
    plan.launch()
    assert_slab(slab, want, offset)
    plan.close()


@pytest.mark.parametrize("k,m", [(10, 4), (6, 3)])
def test_rotating_single_failure(ec, gpu, scenario, k, m):
    """A failed device under rotated placement: stripe s lost shard s mod (k + m)."""
    from erasure_coding_test_amd import _native as N
    n, size = k + m, 4099
    erasures = [[s % n] for s in range(2 * n + 1)]
    M, damaged, want = scenario(k, m, size, erasures)
    slab, shards = upload(damaged, gpu)
    cpu_calls, fallbacks = N.cpu_call_count(), N.fallback_count()
    plan = ec.RebuildPlan(k, m, M).bind_stripes(shards, erasures, size)
    assert len(plan.groups) == 1 and len(plan.groups[0].maps) == n
    assert len(plan.plans) == 1 and isinstance(plan.plans[0], ec.MultiMapPlan)  # one group, one launch
    assert (plan.plans[0].rows, plan.plans[0].nsrc, plan.plans[0].stripes, plan.plans[0].engine) == (1, k, 2 * n + 1, 0)
    plan.launch()
    assert_slab(slab, want)
    assert (N.cpu_call_count(), N.fallback_count()) == (cpu_calls, fallbacks)
    plan.close()


def test_mixed_counts(ec, gpu, scenario):
    k, m, size = 10, 4, 4112
    erasures = mixed(k, m) * 2 + [[3], [k + 1], [4, 5], []]
    order = np.random.default_rng(5).permutation(len(erasures))
    erasures = [erasures[i] for i in order]
    M, damaged, want = scenario(k, m, size, erasures)
    # untouched stripes and untouched shards of a rebuilt stripe are what they were
    for s, er in enumerate(erasures):
        keep = [i for i in range(k + m) if i not in er]
        assert np.array_equal(want[s, keep], damaged[s, keep])
    slab, shards = upload(damaged, gpu)
    plan = ec.RebuildPlan(k, m, M).bind_stripes(shards, erasures, size)
    assert [(g.n_out, g.n_src) for g in plan.groups] == [(1, k), (2, k), (m, k)]
    assert sorted(s for g in plan.groups for s in g.stripes) == [s for s, er in enumerate(erasures) if er]
    plan.launch()
    assert_slab(slab, want)
    plan.close()


def test_rs12_4_four_data_erasures(ec, gpu, scenario):
    """K = 12, R = 4: the all-loads-first window of the sequential body, two patterns."""
    k, m, size = 12, 4, 4099
    erasures = [[0, 1, 2, 3], [2, 5, 7, 11], [0, 1, 2, 3], [8, 9, 10, 11]]
    M, damaged, want = scenario(k, m, size, erasures)
    slab, shards = upload(damaged, gpu)
    plan = ec.RebuildPlan(k, m, M).bind_stripes(shards, erasures, size)
    assert [(p.rows, p.nsrc, p.engine) for p in plan.plans] == [(4, 12, 0)] and plan.groups[0].map_of == [0, 1, 0, 2]
    plan.launch()
    assert_slab(slab, want)
    plan.close()


def raw_case(nsrc, rows, nmaps, stripes, size, seed):
    rng = np.random.default_rng(seed)
    maps = rng.integers(0, 256, (nmaps, rows, nsrc))
    maps[rng.random(maps.shape) < 0.15] = 0
    maps[rng.random(maps.shape) < 0.15] = 1
    srcs = rng.integers(0, 256, (stripes, nsrc, size), dtype=np.uint8)
    return [[int(c) for c in mp.ravel()] for mp in maps], [[[int(c) for c in r] for r in mp] for mp in maps], srcs


def run_raw(ec, gpu, mul, nsrc, rows, maps_flat, maps, srcs, map_of, size, offset=0):
    stripes = len(map_of)
    sslab, s_sh = upload(srcs, gpu, offset)
    dslab, d_sh = upload(np.full((stripes, rows, size), FILL, dtype=np.uint8), gpu, offset)
    plan = ec.MultiMapPlan(rows, nsrc, maps_flat).bind(map_of, s_sh, d_sh, size)
    engine = plan.engine
    plan.launch()
    assert_slab(dslab, np.stack([model(mul, maps[mi], srcs[s]) for s, mi in enumerate(map_of)]), offset)
    assert_slab(sslab, srcs, offset)
    plan.close()
    return engine


@pytest.mark.parametrize("size,offset", [(4099, 0), (16, 0), (7, 0), (4096, 1)])
def test_raw_16_sources_4_rows(ec, gpu, mul, size, offset):
    """The widest specialised shape, random coefficients with zeros and ones among them."""
    flat, maps, srcs = raw_case(16, 4, 3, 5, size, 16)
    assert {0, 1} <= {c for f in flat for c in f} and max(c for f in flat for c in f) > 1
    engine = run_raw(ec, gpu, mul, 16, 4, flat, maps, srcs, [2, 0, 1, 1, 2], size, offset)
    assert engine == (0 if offset == 0 and size >= 16 else 1)


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_raw_17_sources_is_the_byte_kernel_alone(ec, gpu, mul, rows):
    flat, maps, srcs = raw_case(17, rows, 3, 4, 4099, 17 + rows)
    assert run_raw(ec, gpu, mul, 17, rows, flat, maps, srcs, [1, 2, 0, 1], 4099) == 1


def test_map_order_and_unused_map(ec, gpu, mul):
    nsrc, rows, size = 5, 2, 4099
    map_of = [2, 0, 2, 1, 0, 2, 1]  # map 3 is never used
    flat, maps, srcs = raw_case(nsrc, rows, 4, len(map_of), size, 44)
    # every stripe's output under its own map differs from its output under any other map
    for s, mi in enumerate(map_of):
        own = model(mul, maps[mi], srcs[s])
        for other in range(4):
            assert other == mi or not np.array_equal(model(mul, maps[other], srcs[s]), own), (s, other)
    assert run_raw(ec, gpu, mul, nsrc, rows, flat, maps, srcs, map_of, size) == 0


def test_launch_without_work_is_a_no_op(ec, gpu):
    import torch
    plan = ec.MultiMapPlan(1, 2, [[1, 1], [2, 3]])
    plan.launch()                       # not bound
    plan.bind([], [], [], 4096).launch()  # no stripes
    buf = torch.full((3, 64), GUARD, dtype=torch.uint8, device=gpu)
    plan.bind([1], [[buf[0], buf[1]]], [[buf[2]]], 0).launch()  # no bytes
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    with pytest.raises(ec._native.EcgpuError, match="stripe 0"):
        plan.bind([2], [[buf[0], buf[1]]], [[buf[2]]], 16)
    plan.close()


def test_chunk_boundary(ec, gpu, mul):
    """65537 stripes: a second chunk of gridDim.y that starts at stripe 65535, for the column kernel (one
    16-B column) and the byte kernel (a 3-byte tail) alike; map_of must move with the pointer tables."""
    import torch
    stripes, size, pitch = 65537, 19, 32
    maps = [[[3, 7]], [[1, 0xC5]]]
    map_of = np.arange(stripes) % 2
    assert map_of[65535] != map_of[0] and map_of[65536] != map_of[1]
    rng = np.random.default_rng(65537)
    pool = rng.integers(0, 256, (8, size), dtype=np.uint8)
    a, b = rng.integers(0, 8, stripes), rng.integers(0, 8, stripes)
    prod = np.stack([np.stack([mul[mp[0][j]][pool] for j in range(2)]) for mp in maps])  # [map][j][pool shard][x]
    want = prod[map_of, 0, a] ^ prod[map_of, 1, b]
    wrong = prod[1 - map_of, 0, a] ^ prod[1 - map_of, 1, b]
    assert (want[65535:] != wrong[65535:]).any(axis=1).all()
    pslab = torch.from_numpy(frame(pool[None])[0]).to(gpu)        # [8, 64]
    dslab = torch.full((stripes, pitch), GUARD, dtype=torch.uint8, device=gpu)
    pbase, pstride, dbase = pslab.data_ptr(), pslab.shape[1], dslab.data_ptr()
    srcs = [[pbase + int(a[s]) * pstride, pbase + int(b[s]) * pstride] for s in range(stripes)]
    dsts = [[dbase + s * pitch] for s in range(stripes)]
    plan = ec.MultiMapPlan(1, 2, [[c for r in mp for c in r] for mp in maps]).bind([int(v) for v in map_of], srcs, dsts,
                                                                               size)
    assert plan.engine == 0
    plan.launch()
    exp = np.full((stripes, pitch), GUARD, dtype=np.uint8)
    exp[:, :size] = want
    got = dslab.cpu().numpy()
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} stripes differ, first {bad[:5]}"
    assert np.array_equal(pslab.cpu().numpy(), frame(pool[None])[0])
    plan.close()


def test_capture_replay(ec, gpu, scenario):
    import torch
    k, m, size = 10, 4, 4099
    erasures = [[s % (k + m)] for s in range(5)] + [[0, 11], [], [2, 3]]
    M, damaged, want = scenario(k, m, size, erasures)
    slab, shards = upload(damaged, gpu)
    plan = ec.RebuildPlan(k, m, M).bind_stripes(shards, erasures, size)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.launch()  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    assert_slab(slab, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.launch()
    for seed in (1, 2):  # other survivors behind the same pointers
        M2, damaged2, want2 = scenario(k, m, size, erasures, seed)
        assert not np.array_equal(damaged2, damaged)
        slab.copy_(torch.from_numpy(frame(damaged2)).to(gpu))
        g.replay()
        torch.cuda.synchronize()
        assert_slab(slab, want2)
    plan.close()


def test_repair_mixed_suspects(ec, gpu, scenario):
    """ScrubPlan.repair: six stripes damaged in four different shards and a clean one, rebuilt together."""
    import torch
    k, m, size = 6, 3, 4099
    M, _, clean = scenario(k, m, size, [[]] * 7)
    slab, shards = upload(clean, gpu)
    suspects = [2, k + 1, 0, 2, k + 1, 5]
    for s, t in enumerate(suspects):
        idx = torch.tensor(sorted({0, size - 1, 16 * s + 3}), dtype=torch.long, device=gpu)
        shards[s][t][idx] ^= torch.tensor(0x40 + s, dtype=torch.uint8, device=gpu)
    plan = ec.ScrubPlan(k, m, M)
    repaired, unrepaired, after = plan.repair(shards, size)
    assert repaired == list(enumerate(suspects))
    assert unrepaired == []
    assert len(after) == 7 and all(r.clean and r.suspects == [] for r in after)
    assert_slab(slab, clean)
    plan.close()
