"""Stripe scrub on the MI355X (ScrubPlan / ecgpu_scrub_*): fused parity verify
with shard blame.

Expected parity comes from the live reference (jerasure_matrix_encode), the
syndromes and counters from a numpy model over the reference's multiply
table, and the blame is known by construction (tests/test_scrub_host.py checks
the matrices' condition for it).  Sizes are the smallest at which each code
path can go wrong: 16 one column; 4096 exactly one block; 4112 a second block
with one live lane; 4099 and 1000 vector part plus byte tail; 7 and 1 the byte
kernel only; 4096 with every pointer offset by 1, unaligned, byte kernel only.
"""
import numpy as np
import pytest

from oracle.oracle import alloc_shards

pytestmark = pytest.mark.gpu

SPECIALISED = [(4, 2), (6, 3), (10, 4), (12, 4), (3, 3), (2, 1)]
GENERIC = [(17, 2), (4, 5)]
SCHEMES = SPECIALISED + GENERIC
SIZES = [(16, 0), (4096, 0), (4112, 0), (4099, 0), (1000, 0), (7, 0), (1, 0), (4096, 1)]  # (size, pointer offset)
STRIPES = 3
NON_MDS = [1, 1, 1, 0]  # k = m = 2


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


@pytest.fixture(scope="module")
def mul(reference):
    """The reference's GF(2^8) multiply table, [a][b]."""
    return np.array([[reference.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)


@pytest.fixture(scope="module")
def codewords(reference):
    """codewords(k, m, size, matrix=None, stripes=STRIPES) -> (matrix, [stripes, k+m, size] uint8), clean
    stripes encoded by the reference; computed once per shape and never modified."""
    cache = {}

    def get(k, m, size, matrix=None, stripes=STRIPES):
        key = (k, m, size, None if matrix is None else tuple(matrix), stripes)
        if key not in cache:
            M = [int(c) for c in reference.vandermonde_coding_matrix(k, m).ravel()] if matrix is None else list(matrix)
            rng = np.random.default_rng([k, m, size, stripes])
            out = np.zeros((stripes, k + m, size), dtype=np.uint8)
            for s in range(stripes):
                data, coding = alloc_shards(k, size), alloc_shards(m, size)
                for j in range(k):
                    data[j][:size] = rng.integers(0, 256, size, dtype=np.uint8)
                reference.matrix_encode(k, m, np.array(M).reshape(m, k), data, coding, size)
                for i, a in enumerate(data + coding):
                    out[s, i] = a[:size]
            out.setflags(write=False)
            cache[key] = (M, out)
        return cache[key]

    return get


def model(mul, M, k, m, stripe):
    """(bad_bytes, bad_cols, first_bad) of one stripe [k+m, size] from its bytes."""
    syn = stripe[k:].copy()
    for i in range(m):
        for j in range(k):
            syn[i] ^= mul[M[i * k + j]][stripe[j]]
    bad = syn != 0
    cols = bad.any(axis=0)
    return tuple(int(v) for v in bad.sum(axis=1)), int(cols.sum()), int(np.argmax(cols)) if cols.any() else None


def upload(host, gpu, offset=0):
    """The stripes in one device slab; shard views start `offset` bytes past a 16-B boundary."""
    import torch
    stripes, n, size = host.shape
    slab = torch.zeros((stripes, n, (size + offset + 47) // 16 * 16), dtype=torch.uint8, device=gpu)
    slab[:, :, offset:offset + size] = torch.from_numpy(np.array(host)).to(gpu)
    shards = [[slab[s, i, offset:offset + size] for i in range(n)] for s in range(stripes)]
    assert all(sh.data_ptr() % 16 == offset for st in shards for sh in st)
    return slab, shards


def damage(shard, positions, values):
    import torch
    idx = torch.tensor(list(positions), dtype=torch.long, device=shard.device)
    shard[idx] ^= torch.tensor(list(values), dtype=torch.uint8, device=shard.device)


def spots(size):
    return sorted({0, size - 1, size // 2})


def check(got, want, suspects):
    assert (got.bad_bytes, got.bad_cols, got.first_bad) == want
    assert got.suspects == suspects


CLEAN = lambda m: ((0,) * m, 0, None)  # noqa: E731


@pytest.mark.parametrize("size,offset", SIZES)
@pytest.mark.parametrize("k,m", SCHEMES)
def test_clean_stripes_and_one_damaged_shard(ec, gpu, codewords, mul, k, m, size, offset):
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu, offset)
    before = slab.clone()
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    assert plan.engine == (0 if (k, m) in SPECIALISED and offset == 0 and size >= 16 else 1)
    plan.launch()
    for r in plan.results():
        check(r, CLEAN(m), [])
    assert bool((slab == before).all()), "scrub wrote to a shard"

    everyone = list(range(k + m))
    for t in everyone:
        pos = spots(size)
        vals = [1 + (37 * t + 11 * p) % 255 for p in range(len(pos))]
        damage(shards[1][t], pos, vals)
        stripe = np.array(host[1])
        stripe[t, pos] ^= np.array(vals, dtype=np.uint8)
        plan.launch()
        res = plan.results()
        check(res[0], CLEAN(m), [])
        check(res[2], CLEAN(m), [])
        want = model(mul, M, k, m, stripe)
        assert want[1] == len(pos) and want[2] == 0
        check(res[1], want, [t] if m >= 2 else everyone)
        damage(shards[1][t], pos, vals)  # XOR again: restored
    assert bool((slab == before).all())
    plan.close()


@pytest.mark.parametrize("size", [4099, 4112])
@pytest.mark.parametrize("k,m", SCHEMES)
def test_whole_shard_damaged(ec, gpu, codewords, mul, k, m, size):
    """Every lane of every wave live in the reductions: bad_cols == size."""
    import torch
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    rng = np.random.default_rng(size)
    for t in range(k + m):
        noise = rng.integers(1, 256, size, dtype=np.uint8)
        dn = torch.from_numpy(noise).to(gpu)
        shards[1][t].bitwise_xor_(dn)
        stripe = np.array(host[1])
        stripe[t] ^= noise
        plan.launch()
        res = plan.results()
        want = model(mul, M, k, m, stripe)
        assert want[1] == size and want[2] == 0
        check(res[1], want, [t] if m >= 2 else list(range(k + m)))
        check(res[0], CLEAN(m), [])
        check(res[2], CLEAN(m), [])
        shards[1][t].bitwise_xor_(dn)
    plan.close()


@pytest.mark.parametrize("k,m,size", [(10, 4, 4112), (6, 3, 4099), (2, 1, 16)])
def test_early_parity_load_form(ec, gpu, codewords, mul, knobs, k, m, size):
    """ECGPU_SCRUB_LATE=0: the kernel form that loads the parity columns with the sources."""
    knobs.set("ECGPU_SCRUB_LATE", 0)
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    assert plan.engine == 0
    plan.launch()
    for r in plan.results():
        check(r, CLEAN(m), [])
    for t in (0, k - 1, k, k + m - 1):
        pos = spots(size)
        damage(shards[1][t], pos, [0xC3] * len(pos))
        stripe = np.array(host[1])
        stripe[t, pos] ^= 0xC3
        plan.launch()
        res = plan.results()
        check(res[1], model(mul, M, k, m, stripe), [t] if m >= 2 else list(range(k + m)))
        check(res[0], CLEAN(m), [])
        damage(shards[1][t], pos, [0xC3] * len(pos))
    plan.close()


@pytest.mark.parametrize("k,m", [s for s in SCHEMES if s[1] >= 2])
def test_two_shards_damaged_at_different_positions(ec, gpu, codewords, mul, k, m):
    size = 4099
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    for a, b in [(0, 1), (k - 1, k), (k, k + m - 1), (0, k + m - 1)]:
        stripe = np.array(host[1])
        for t, pos in ((a, [5, 4097]), (b, [6, 2000])):
            damage(shards[1][t], pos, [0x51, 0xA7])
            stripe[t, pos] ^= np.array([0x51, 0xA7], dtype=np.uint8)
        plan.launch()
        res = plan.results()
        want = model(mul, M, k, m, stripe)
        assert want[1] == 4 and want[2] == 5
        check(res[1], want, [])
        check(res[0], CLEAN(m), [])
        for t, pos in ((a, [5, 4097]), (b, [6, 2000])):
            damage(shards[1][t], pos, [0x51, 0xA7])
    plan.close()


def test_non_mds_matrix_blames_both_lookalikes(ec, gpu, codewords, mul):
    k = m = 2
    size = 1000
    M, host = codewords(k, m, size, NON_MDS)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    damage(shards[1][1], [3, 999], [0x10, 0xFF])
    stripe = np.array(host[1])
    stripe[1, [3, 999]] ^= np.array([0x10, 0xFF], dtype=np.uint8)
    plan.launch()
    res = plan.results()
    check(res[1], model(mul, M, k, m, stripe), [1, 2])
    assert res[1].bad_bytes == (2, 0)
    check(res[0], CLEAN(m), [])
    plan.close()


def test_relaunch_resets_results(ec, gpu, codewords):
    k, m, size = 6, 3, 4099
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    assert plan.device_results != 0
    damage(shards[2][4], [17, 4098], [1, 2])
    plan.launch()
    res = plan.results()
    assert res[2].bad_cols == 2 and res[2].first_bad == 17 and res[2].suspects == [4]
    damage(shards[2][4], [17, 4098], [1, 2])
    plan.launch()
    for r in plan.results():
        check(r, CLEAN(m), [])
    plan.close()


def test_launch_is_graph_capturable(ec, gpu, codewords, mul):
    import torch
    k, m, size = 10, 4, 4099
    M, host = codewords(k, m, size)
    slab, shards = upload(host, gpu)
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.launch()  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.launch()
    for stripe_id, t, pos in [(0, 3, [0, 4098]), (2, 12, [100])]:
        vals = [0x33] * len(pos)
        damage(shards[stripe_id][t], pos, vals)
        stripe = np.array(host[stripe_id])
        stripe[t, pos] ^= np.array(vals, dtype=np.uint8)
        g.replay()
        res = plan.results()
        for s_ in range(STRIPES):
            if s_ == stripe_id:
                check(res[s_], model(mul, M, k, m, stripe), [t])
            else:
                check(res[s_], CLEAN(m), [])
        damage(shards[stripe_id][t], pos, vals)
    g.replay()
    for r in plan.results():
        check(r, CLEAN(m), [])
    plan.close()


def test_more_stripes_than_one_launch_takes(ec, gpu, reference):
    """65537 stripes: the second chunk of 65535 and a third of one stripe."""
    import torch
    k, m, size, stripes = 2, 1, 16, 65537
    M = [int(c) for c in reference.vandermonde_coding_matrix(k, m).ravel()]
    rng = np.random.default_rng(8)
    # the code is bytewise: one reference encode of stripes * size bytes is every stripe's parity
    n = stripes * size
    data, coding = alloc_shards(k, n), alloc_shards(m, n)
    for j in range(k):
        data[j][:n] = rng.integers(0, 256, n, dtype=np.uint8)
    reference.matrix_encode(k, m, np.array(M).reshape(m, k), data, coding, n)
    host = np.stack([a[:n].reshape(stripes, size) for a in data + coding], axis=1)  # [stripes, 3, 16]
    slab = torch.from_numpy(np.ascontiguousarray(host)).to(gpu)
    base = slab.data_ptr()
    shards = [[base + (s * (k + m) + i) * size for i in range(k + m)] for s in range(stripes)]
    plan = ec.ScrubPlan(k, m, M).bind_stripes(shards, size)
    plan.launch()
    assert all(r.clean and r.first_bad is None and r.suspects == [] for r in plan.results())
    slab[65536, 1, 9] ^= 0x40
    plan.launch()
    res = plan.results()
    assert len(res) == stripes
    assert [s for s, r in enumerate(res) if not r.clean] == [65536]
    check(res[65536], ((1,), 1, 9), [0, 1, 2])
    plan.close()


def test_repair(ec, gpu, codewords):
    import torch
    k, m, size = 6, 3, 4099
    M, host = codewords(k, m, size, stripes=4)
    slab, shards = upload(host, gpu)
    original = slab.clone()
    damage(shards[0][2], [0, 4098], [9, 200])        # a data shard
    damage(shards[2][k + 1], [77], [0x80])           # a coding shard
    damage(shards[3][0], [1], [1])                   # two shards: nobody alone explains it
    damage(shards[3][5], [2], [1])
    plan = ec.ScrubPlan(k, m, M)
    repaired, unrepaired, after = plan.repair(shards, size)
    assert repaired == [(0, 2), (2, k + 1)]
    assert unrepaired == [3]
    assert bool(torch.equal(slab[:3], original[:3]))
    for r in after[:3]:
        check(r, CLEAN(m), [])
    assert after[3].bad_cols == 2 and after[3].suspects == []
    plan.close()
