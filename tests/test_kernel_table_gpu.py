"""Every specialised w = 8 and scrub kernel against a table reference.

gf_spec.hip / scrub_spec.hip instantiate gf_apply, gf_apply_inl, gf_apply_lds
and scrub_verify for K = 1..16, R = 1..4 and five unit structures; the host
rule unit_variant() picks one per launch.  A fault in one instantiation, or in
the rule, corrupts exactly one (K, R, matrix shape), so this file launches
every cell the rule can return (tests/kernel_cases.py: 281 of 320) on every
path that reaches the table, and sends all 256 coefficients x all 256 byte
values x all 16 byte positions of a column through every consumer of the
coefficient tables.  The reference is the reference implementation's own
256 x 256 product table (tests/golden, vectors["gf_mul_table"]); every
comparison is bit-exact.

Size is 4,117 bytes -- one full 256-lane block, a second block with one live
lane, a 5-byte tail -- except where a test says otherwise.  Every output
buffer is pre-filled with 0xCC and followed by at least 16 guard bytes; every
check compares the whole output slab, guards included, and the sources.
"""
import numpy as np
import pytest

import kernel_cases as kc
from kernel_cases import FILL, GUARD, SIZE, SIZE_ZC

pytestmark = pytest.mark.gpu

CELLS = kc.reachable_cells()


def cells_of(K):
    return [(R, U) for k, R, U in CELLS if k == K]


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


@pytest.fixture(scope="module")
def T(vectors):
    return vectors["gf_mul_table"]


def launches(ec):
    """(v_perm, LDS) specialised column launches so far (ecgpu_engine_launches)."""
    return int(ec._native.lib.ecgpu_engine_launches(0)), int(ec._native.lib.ecgpu_engine_launches(1))


def first_difference(got, want):
    row, pos = np.argwhere(got != want)[0]
    lo = max(0, pos - 4)
    return (f"row {row} byte {pos}: expected {want[row, lo:pos + 12].tobytes().hex()} "
            f"got {got[row, lo:pos + 12].tobytes().hex()} (from byte {lo})")


class Arena:
    """One source slab and one output slab, reused across the cells of a test.

    Sources: [stripes, K, stride], source j of stripe s = kc.source(j + K * s).
    Outputs: a guard row, then [stripes, R, stride]; every view is `size`
    bytes starting `offset` bytes into its row and is followed by >= 16 guard
    bytes.  where = "device" (HBM), "numpy" (pageable host) or "pinned"."""

    def __init__(self, gpu, K, R, stripes, size, offset=0, where="device"):
        import torch
        self.K, self.R, self.stripes, self.size, self.offset, self.where = K, R, stripes, size, offset, where
        self.stride = (offset + size + GUARD + 15) // 16 * 16
        host = np.zeros((stripes, K, self.stride), dtype=np.uint8)
        for s in range(stripes):
            for j in range(K):
                host[s, j, offset:offset + size] = kc.source(j + K * s, size, s)
        host.setflags(write=False)
        self.host = host
        shape = (1 + stripes * R, self.stride)
        if where == "device":
            self.src = torch.from_numpy(host.copy()).to(gpu)
            self.out = torch.empty(shape, dtype=torch.uint8, device=gpu)
        elif where == "pinned":
            self.src = torch.from_numpy(host.copy()).pin_memory()
            self.out = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
            assert self.src.is_pinned() and self.out.is_pinned()
        else:
            self.src = host.copy()
            self.out = np.empty(shape, dtype=np.uint8)
        for s in range(stripes):
            for v in self.srcs(s, K) + self.dsts(s, R):
                ptr = v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data
                assert ptr % 16 == offset or where == "numpy"

    def data(self, s, k):
        return [self.host[s, j, self.offset:self.offset + self.size] for j in range(k)]

    def srcs(self, s, k):
        return [self.src[s, j, self.offset:self.offset + self.size] for j in range(k)]

    def dsts(self, s, r):
        return [self.out[1 + s * self.R + i, self.offset:self.offset + self.size] for i in range(r)]

    def reset(self):
        if self.where == "numpy":
            self.out[:] = FILL
        else:
            self.out.fill_(FILL)

    def check(self, want, label):
        """want[s]: [rows, size] expected outputs of stripe s; everything else stays 0xCC; sources unchanged."""
        got = self.out if self.where == "numpy" else self.out.cpu().numpy()
        image = np.full_like(got, FILL)
        for s, rows in enumerate(want):
            image[1 + s * self.R:1 + s * self.R + len(rows), self.offset:self.offset + self.size] = rows
        if not np.array_equal(got, image):
            raise AssertionError(f"{label}: {first_difference(got, image)} (rows: guard, then stripe * {self.R} + output; "
                                 f"bytes {self.offset}..{self.offset + self.size - 1} are the output)")
        src = self.src if self.where == "numpy" else self.src.cpu().numpy()
        assert np.array_equal(src, self.host), f"{label}: a source changed"


def run_plan(ec, arena, T, M, kind, nt, label, grow):
    """One StripePlan launch of matrix M over the arena's stripes; `grow` =
    expected growth of the (v_perm, LDS) launch counters."""
    rows, K = M.shape
    plan = ec.StripePlan(rows, K, M.ravel().tolist()).set_kernel(kind, bool(nt))
    plan.bind([arena.srcs(s, K) for s in range(arena.stripes)], [arena.dsts(s, rows) for s in range(arena.stripes)],
              arena.size)
    arena.reset()
    before = launches(ec)
    plan.launch()
    after = launches(ec)
    assert (after[0] - before[0], after[1] - before[1]) == grow, f"{label}: launch counters grew by the wrong amount"
    arena.check([kc.expect(T, M, arena.data(s, K)) for s in range(arena.stripes)], label)
    plan.close()


# ------------------------------------------------------------ plan sweeps ----
@pytest.mark.parametrize("K", kc.KS)
def test_plan_sweep_vperm(ec, gpu, T, K):
    """gf_apply<K, R, UNITS, ..., NT>: every reachable cell x store policy."""
    arena = Arena(gpu, K, 4, 2, SIZE)
    ran = 0
    for R, U in cells_of(K):
        for nt in (1, 0):
            M = kc.matrix_for(K, R, U, salt=nt)
            run_plan(ec, arena, T, M, 0, nt, f"plan v_perm K={K} R={R} U={U} nt={nt}", (1, 0))
            ran += 1
    assert ran == 2 * len(cells_of(K))


@pytest.mark.parametrize("K", kc.KS)
def test_plan_sweep_lds(ec, gpu, T, K):
    """gf_apply_lds<K, R>: the zero / unit column shortcuts on columns that are
    all zero, all ones, mixed 0 and 1 and general, mask bits up to R*K - 1;
    then the matrix that is all ones except its last entry."""
    arena = Arena(gpu, K, 4, 2, SIZE)
    for R in kc.RS:
        for salt in (0, 1):
            M = kc.lds_matrix_for(K, R, salt)
            run_plan(ec, arena, T, M, 1, 1, f"plan LDS K={K} R={R} salt={salt} matrix={M.tolist()}", (0, 1))
        if (K, R, 3) in CELLS:
            run_plan(ec, arena, T, kc.matrix_for(K, R, 3), 1, 1, f"plan LDS K={K} R={R} U=3", (0, 1))


# ---------------------------------------------------------- inline sweeps ----
def run_encode(ec, arena, T, M, label):
    R, K = M.shape
    arena.reset()
    before = launches(ec)
    ec.jerasure.jerasure_matrix_encode(K, R, 8, M.ravel().tolist(), arena.srcs(0, K), arena.dsts(0, R), arena.size)
    assert launches(ec) == before, f"{label}: the call ran as a plan launch, not inline"
    arena.check([kc.expect(T, M, arena.data(0, K))], label)


@pytest.mark.parametrize("K", kc.KS)
def test_inline_sweep_device(ec, gpu, T, K):
    """gf_apply_inl<K, R, UNITS, ZC=false> through jerasure_matrix_encode on
    device tensors.

    What csrc/planner.cpp and inline_ok() do with the matrix: the call is
    replayed as m dot products on a LinearTracker and fused into one map.  A
    matrix without zero rows or columns keeps its K, R and coefficients, and
    with w = 8, K <= 16 and the v_perm engine inline_ok() holds at this size,
    so the map reaches launch_inline -- but the tracker lists the sources in
    the order the dot products first touch them (a row's unit coefficients
    first, then its other non-zero ones), so the launch sees the columns in
    that order (kernel_cases.fused_order).  Every matrix_for matrix keeps its
    order except the one-row variant-0 ones, which would be launched ones
    first as variant 1; kernel_cases.inline_matrix_for replaces those, and
    tests/test_kernel_cases.py checks that each cell's matrix still lands on
    its cell after the reordering.  The plan launch counters must not move:
    a call that took the cached-plan route instead would move them."""
    N = ec._native
    assert N.get_knob("ECGPU_INLINE") == 1 and N.get_knob("ECGPU_KERNEL") == 0
    arena = Arena(gpu, K, 4, 1, SIZE)
    for R, U in cells_of(K):
        M = kc.inline_matrix_for(K, R, U)
        assert kc.unit_variant(M[:, kc.fused_order(M)], K, R) == U
        run_encode(ec, arena, T, M, f"inline device K={K} R={R} U={U}")


@pytest.mark.parametrize("K", kc.KS)
def test_inline_sweep_host_in_place(ec, gpu, T, knobs, K):
    """gf_apply_inl<K, R, UNITS, ZC=true>, the grid-stride loop: pageable numpy
    buffers (copied through coherent pinned staging the kernel uses in place)
    and, for a sixth of the cells, pinned tensors the kernel reads and writes
    directly.  ECGPU_ZC_GRID = 1 and 514 columns: lanes 0 and 1 make three
    trips, lanes 2..255 two, and 5 tail bytes remain."""
    N = ec._native
    knobs.set("ECGPU_ZC_GRID", 1)
    assert N.get_knob("ECGPU_ZC_GRID") == 1
    assert N.get_knob("ECGPU_INLINE") == 1 and N.get_knob("ECGPU_ZC_PINNED") == 1
    assert SIZE_ZC // 16 == 514 and (K + 4) * SIZE_ZC <= N.get_knob("ECGPU_ZC_KIB") << 10
    pageable = Arena(gpu, K, 4, 1, SIZE_ZC, where="numpy")
    pinned = Arena(gpu, K, 4, 1, SIZE_ZC, where="pinned")
    ran_pinned = 0
    for R, U in cells_of(K):
        M = kc.inline_matrix_for(K, R, U, salt=1)
        run_encode(ec, pageable, T, M, f"inline host pageable K={K} R={R} U={U}")
        if CELLS.index((K, R, U)) % 6 == 0:
            run_encode(ec, pinned, T, M, f"inline host pinned K={K} R={R} U={U}")
            ran_pinned += 1
    assert ran_pinned >= 2


# ------------------------------------------------------------ scrub sweep ----
CLEAN = lambda m: ((0,) * m, 0, None, [])  # noqa: E731


def verdict(r):
    return (r.bad_bytes, r.bad_cols, r.first_bad, r.suspects)


class ScrubSlab:
    """[stripes, n, stride] on the device; stripe rows 0..k-1 data, then parity."""

    def __init__(self, gpu, n, stripes, size, offset=0):
        import torch
        self.size, self.offset, self.stripes = size, offset, stripes
        self.stride = (offset + size + GUARD + 15) // 16 * 16
        self.slab = torch.zeros((stripes, n, self.stride), dtype=torch.uint8, device=gpu)
        self.gpu = gpu

    def put(self, image):
        """image: [stripes, k + m, size] uint8."""
        import torch
        self.n = image.shape[1]
        self.slab[:, :self.n, self.offset:self.offset + self.size] = torch.from_numpy(image).to(self.gpu)

    def shards(self):
        return [[self.slab[s, i, self.offset:self.offset + self.size] for i in range(self.n)]
                for s in range(self.stripes)]

    def holds(self, image):
        got = self.slab[:, :self.n, self.offset:self.offset + self.size].cpu().numpy()
        return np.array_equal(got, image)


def codewords(T, M, arena_data):
    """[stripes, K + R, size]: data and the parity the table reference gives."""
    return np.stack([np.concatenate([np.stack(d), kc.expect(T, M, d)]) for d in arena_data])


@pytest.mark.parametrize("K", kc.KS)
def test_scrub_sweep(ec, gpu, T, knobs, K):
    """scrub_verify<K, R, UNITS, LATE>: every reachable cell x both load
    orders.  Clean stripes first; then stripe 1 with the first byte, the last
    vector byte and the last tail byte of one data shard flipped and stripe 2
    with one coding shard damaged everywhere; counters and suspects from
    kernel_cases.scrub_model."""
    stripes = 3
    data = [[kc.source(j + K * s, SIZE, s) for j in range(K)] for s in range(stripes)]
    dev = ScrubSlab(gpu, K + 4, stripes, SIZE)
    noise = (1 + np.arange(SIZE) % 255).astype(np.uint8)
    ran = 0
    for R, U in cells_of(K):
        M = kc.matrix_for(K, R, U)
        clean = codewords(T, M, data)
        t, p = (7 * K + 3 * R + U) % K, (K + U) % R
        bad = clean.copy()
        bad[1, t, [0, SIZE // 16 * 16 - 1, SIZE - 1]] ^= np.array([0x01, 0x80, 0xA5], dtype=np.uint8)
        bad[2, K + p] ^= noise
        want = [CLEAN(R), kc.scrub_model(T, M, K, R, bad[1]), kc.scrub_model(T, M, K, R, bad[2])]
        assert want[1][1] == 3 and want[1][2] == 0 and want[2][1] == SIZE and want[2][0][p] == SIZE

        dev.put(clean)
        plan = ec.ScrubPlan(K, R, M.ravel().tolist()).bind_stripes(dev.shards(), SIZE)
        assert plan.engine == 0
        for late in (1, 0):
            label = f"scrub K={K} R={R} U={U} LATE={late}"
            knobs.set("ECGPU_SCRUB_LATE", late)
            plan.launch()
            assert [verdict(r) for r in plan.results()] == [CLEAN(R)] * stripes, f"{label}: clean stripes"
        assert dev.holds(clean), f"scrub K={K} R={R} U={U}: the scrub wrote to a shard"
        dev.put(bad)
        for late in (1, 0):
            label = f"scrub K={K} R={R} U={U} LATE={late}"
            knobs.set("ECGPU_SCRUB_LATE", late)
            plan.launch()
            got = [verdict(r) for r in plan.results()]
            assert got == want, f"{label}: data shard {t} of stripe 1 and coding shard {p} of stripe 2 damaged"
            ran += 1
        assert dev.holds(bad), f"scrub K={K} R={R} U={U}: the scrub wrote to a shard"
        plan.close()
    assert ran == 2 * len(cells_of(K))


# ------------------------------------------------------- exhaustive tables ----
# All 256 coefficients x the pattern block (every byte value at every position
# of a column) through each consumer of the coefficient tables.  The matrices
# hold 0 and 1 as ordinary entries: no unit structure, no column shortcut.
@pytest.mark.parametrize("nt", [1, 0])
def test_tables_p3_plan(ec, gpu, T, nt):
    """build_tables' 3-bit-slice tables -> gf_apply<16, 4, none>."""
    arena = Arena(gpu, 16, 4, 2, SIZE)
    for i, M in enumerate(kc.table_matrices(4, 16)):
        run_plan(ec, arena, T, M, 0, nt, f"p3 tables, coefficients {64 * i}..{64 * i + 63}, nt={nt}", (1, 0))


def test_tables_nibble_lds(ec, gpu, T):
    """build_tables' nibble tables -> gf_apply_lds<16, 4>."""
    arena = Arena(gpu, 16, 4, 2, SIZE)
    for i, M in enumerate(kc.table_matrices(4, 16)):
        run_plan(ec, arena, T, M, 1, 1, f"nibble tables, coefficients {64 * i}..{64 * i + 63}", (0, 1))


def test_tables_p3_inline(ec, gpu, T):
    """build_p3 (the inline launches' own copy) -> gf_apply_inl<16, 4, none, false>."""
    arena = Arena(gpu, 16, 4, 1, SIZE)
    for i, M in enumerate(kc.table_matrices(4, 16)):
        assert kc.unit_variant(M[:, kc.fused_order(M)], 16, 4) == 0
        run_encode(ec, arena, T, M, f"inline p3 tables, coefficients {64 * i}..{64 * i + 63}")


def test_tables_q_generic(ec, gpu, T):
    """build_tables' 2-bit tables -> gf_apply_perm_generic<4>, K = 32."""
    arena = Arena(gpu, 32, 4, 2, SIZE)
    for i, M in enumerate(kc.table_matrices(4, 32)):
        run_plan(ec, arena, T, M, 0, 1, f"q tables (generic K=32), coefficients {128 * i}..{128 * i + 127}", (0, 0))


def test_tables_q_bytes(ec, gpu, T):
    """build_tables' 2-bit tables -> gf_apply_bytes: every pointer 1 past a 16-B boundary."""
    arena = Arena(gpu, 16, 4, 2, SIZE, offset=1)
    for i, M in enumerate(kc.table_matrices(4, 16)):
        run_plan(ec, arena, T, M, 0, 1, f"q tables (byte kernel), coefficients {64 * i}..{64 * i + 63}", (0, 0))


def test_tables_q_scrub_bytes(ec, gpu, T):
    """2-bit tables -> scrub_verify_bytes (k = 16, m = 4, pointers offset by 1): clean, then one byte damaged."""
    stripes = 2
    data = [[kc.source(j + 16 * s, SIZE, s) for j in range(16)] for s in range(stripes)]
    dev = ScrubSlab(gpu, 20, stripes, SIZE, offset=1)
    for i, M in enumerate(kc.table_matrices(4, 16)):
        label = f"scrub byte kernel, coefficients {64 * i}..{64 * i + 63}"
        clean = codewords(T, M, data)
        dev.put(clean)
        plan = ec.ScrubPlan(16, 4, M.ravel().tolist()).bind_stripes(dev.shards(), SIZE)
        assert plan.engine == 1
        plan.launch()
        assert [verdict(r) for r in plan.results()] == [CLEAN(4)] * stripes, f"{label}: clean stripes"
        bad = clean.copy()
        bad[1, 3 + i, 2049] ^= 0x3C
        dev.put(bad)
        plan.launch()
        got = [verdict(r) for r in plan.results()]
        assert got == [CLEAN(4), kc.scrub_model(T, M, 16, 4, bad[1])], label
        assert got[1][1] == 1 and got[1][2] == 2049
        assert dev.holds(bad)
        plan.close()


# ------------------------------------------------------------------ edges ----
def test_scrub_all_zero_column(ec, gpu, T):
    """Pivot -1: damage in a data shard no parity row reads is invisible; damage elsewhere is still blamed."""
    k, m = 4, 2
    M = np.array([[1, 0, 2, 3], [1, 0, 4, 5]], dtype=np.int64)
    pivots, _ = ec.scrub.blame_matrix(k, m, M.ravel().tolist())
    assert pivots == [0, -1, 0, 0]
    data = [[kc.source(j + k * s, SIZE, s) for j in range(k)] for s in range(2)]
    clean = codewords(T, M, data)
    dev = ScrubSlab(gpu, k + m, 2, SIZE)
    plan = None
    for t, suspects in ((1, []), (2, [2]), (k + 1, [k + 1])):
        bad = clean.copy()
        bad[1, t, [0, SIZE - 1]] ^= np.array([0x77, 0x01], dtype=np.uint8)
        dev.put(bad)
        if plan is None:
            plan = ec.ScrubPlan(k, m, M.ravel().tolist()).bind_stripes(dev.shards(), SIZE)
            assert plan.engine == 0
        plan.launch()
        got = [verdict(r) for r in plan.results()]
        want = kc.scrub_model(T, M, k, m, bad[1])
        assert want[3] == suspects and (want == CLEAN(m)) == (t == 1)
        assert got == [CLEAN(m), want], f"shard {t} damaged"
    plan.close()


@pytest.mark.parametrize("extra,U", [(1, 4), (1, 1), (2, 1), (2, 4), (3, 1), (3, 4)])
def test_second_row_group_has_its_own_variant(ec, gpu, T, extra, U):
    """R = 5..7: rows 0-3 launch as variant 3, the remaining rows as variant 1 or 4."""
    K = 5
    M = np.concatenate([kc.matrix_for(K, 4, 3), kc.matrix_for(K, extra, U)])
    assert kc.unit_variant(M[:4], K, 4) == 3 and kc.unit_variant(M[4:], K, extra) == U
    arena = Arena(gpu, K, 7, 2, SIZE)
    for nt in (1, 0):
        run_plan(ec, arena, T, M, 0, nt, f"plan K={K} R=4+{extra} U=3 then {U} nt={nt}", (2, 0))


def test_one_live_lane_in_the_grid(ec, gpu, T):
    """K = 16, R = 4, no unit structure, size 16: one column, lane 0 of the only block."""
    arena = Arena(gpu, 16, 4, 2, 16)
    for nt in (1, 0):
        run_plan(ec, arena, T, kc.matrix_for(16, 4, 0), 0, nt, f"plan K=16 R=4 U=0 size=16 nt={nt}", (1, 0))
    run_plan(ec, arena, T, kc.matrix_for(16, 4, 0), 1, 1, "plan LDS K=16 R=4 U=0 size=16", (0, 1))
