"""The case generator of the kernel-table sweep (tests/kernel_cases.py),
checked without a GPU: it must land on every cell it claims to, miss the
neighbouring cells narrowly, and model the scrub's verdicts correctly --
otherwise tests/test_kernel_table_gpu.py sweeps less than it says.
"""
import numpy as np
import pytest

import kernel_cases as kc

SALTS = (0, 1, 2, 5)


@pytest.fixture(scope="module")
def T(vectors):
    return vectors["gf_mul_table"]


def test_reachable_cells():
    cells = kc.reachable_cells()
    assert len(cells) == len(set(cells)) == 281
    missing = {(K, R, U) for K in kc.KS for R in kc.RS for U in range(5)} - set(cells)
    assert missing == {(K, R, U) for K in kc.KS for R in kc.RS for U in range(5)
                       if (R == 1 and U in (2, 3)) or (K == 1 and U in (1, 3))}
    with pytest.raises(ValueError):
        kc.matrix_for(5, 1, 2)


@pytest.mark.parametrize("make", [kc.matrix_for, kc.inline_matrix_for])
def test_matrix_lands_on_its_cell(make):
    for K, R, U in kc.reachable_cells():
        for salt in SALTS:
            m = make(K, R, U, salt)
            assert m.shape == (R, K) and m.min() >= 0 and m.max() <= 255
            assert kc.unit_variant(m, K, R) == U, (K, R, U, salt)
            assert kc.unit_variant(m.ravel().tolist(), K, R) == U
            assert (m != 0).any(axis=0).all() and (m != 0).any(axis=1).all(), "a zero row or column shrinks the launch"
            assert np.array_equal(m, make(K, R, U, salt)), "not deterministic"


def test_near_misses():
    for K, R, U in kc.reachable_cells():
        m = kc.matrix_for(K, R, U, 1)
        if U == 4:
            assert (m == 1).all()
            continue
        misses = []  # the entries that alone keep the matrix off a neighbouring cell
        if U == 0 and (R == 1 or K == 1):
            # a single row or column: the corner decides both structures
            assert m[0, 0] > 1 and (m == 1).sum() == K * R - 1, (K, R, U)
            misses.append((0, 0))
        else:
            if not U & kc.COL0:
                assert (m[:-1, 0] == 1).all() and m[-1, 0] > 1, (K, R, U)
                misses.append((R - 1, 0))
            if not U & kc.ROW0:
                assert (m[0, :-1] == 1).all() and m[0, -1] > 1, (K, R, U)
                misses.append((0, K - 1))
        if U == 3:
            assert m[-1, -1] > 1 and (m == 1).sum() == K * R - 1, (K, R, U)
            misses.append((R - 1, K - 1))
        elif (K - 1) * (R - 1) >= 2:
            inner = m[1:, 1:]
            assert (inner == 0).sum() == 1 and (inner == 1).sum() == 1, (K, R, U)
        # a dispatch that skipped one of these entries would pick another kernel
        assert misses
        for p in misses:
            n = m.copy()
            n[p] = 1
            assert kc.unit_variant(n, K, R) != U, (K, R, U, p)


def test_sweep_uses_every_general_coefficient():
    want = set(range(2, 256))
    for make in (kc.matrix_for, kc.inline_matrix_for):
        seen = set()
        for K, R, U in kc.reachable_cells():
            seen |= set(make(K, R, U, 0).ravel().tolist())
        assert seen - {0, 1} == want
        assert {0, 1} <= seen
    seen = set()
    for K in kc.KS:
        for R in kc.RS:
            for salt in (0, 1):  # the two salts of the LDS sweep
                seen |= set(kc.lds_matrix_for(K, R, salt).ravel().tolist())
    assert seen - {0, 1} == want


def test_inline_matrix_keeps_its_cell_through_the_source_ordering():
    changed = []
    for K, R, U in kc.reachable_cells():
        plain, m = kc.matrix_for(K, R, U), kc.inline_matrix_for(K, R, U)
        order = kc.fused_order(m)
        assert sorted(order) == list(range(K))
        assert kc.unit_variant(m[:, order], K, R) == U
        if not np.array_equal(plain, m):
            changed.append((K, R, U))
        else:
            assert order == list(range(K)), (K, R, U)
    assert changed == [(K, 1, 0) for K in range(2, 17)]
    # the ordering itself: units of the first row that names them first, then its other non-zero entries
    assert kc.fused_order([[5, 1, 0, 1], [1, 1, 7, 1]]) == [1, 3, 0, 2]


def test_lds_matrix_columns():
    for K in kc.KS:
        for R in kc.RS:
            for salt in (0, 1):
                m = kc.lds_matrix_for(K, R, salt)
                assert m.shape == (R, K)
                assert m[R - 1, K - 1] == 1 - salt, "mask bit R*K - 1 unused"
                body = m[:, :K - 1]
                ones = int(((body == 1).all(axis=0)).sum())
                zeros = int(((body == 0).all(axis=0)).sum())
                mixed = int((((body == 0) | (body == 1)).all(axis=0) & (body == 0).any(axis=0)
                             & (body == 1).any(axis=0)).sum())
                assert ones == (K >= 2) and zeros == (K >= 3) and mixed == (K >= 4 and R >= 2), (K, R, salt)
                if K >= 5:
                    assert (body > 1).all(axis=0).sum() == K - 1 - 3 + (R == 1)
    m = kc.lds_matrix_for(16, 4, 0)
    assert m[3, 15] == 1 and 3 * 16 + 15 == 63


def test_pattern_block_and_sources():
    blk = kc.pattern_block()
    assert blk.dtype == np.uint8 and blk.shape == (4096,)
    for j in (0, 1, 7, 15, 31):
        s = kc.source(j, kc.SIZE, 3)
        assert s.dtype == np.uint8 and s.shape == (kc.SIZE,)
        cols = s[:4096].reshape(256, 16)
        for pos in range(16):
            assert len(set(cols[:, pos].tolist())) == 256, (j, pos)
        assert np.array_equal(s, kc.source(j, kc.SIZE, 3))
        assert not np.array_equal(s[4096:], kc.source(j + 1, kc.SIZE, 3)[4096:])
    assert np.array_equal(kc.source(0, 16), blk[:16])
    assert not np.array_equal(kc.source(0, 4096), kc.source(1, 4096))
    assert kc.SIZE == 256 * 16 + 16 + 5 and kc.SIZE_ZC == 514 * 16 + 5


def test_table_matrices_hold_every_coefficient_once():
    for rows, K, count in ((4, 16, 4), (4, 32, 2)):
        ms = kc.table_matrices(rows, K)
        assert len(ms) == count
        assert sorted(np.concatenate([m.ravel() for m in ms]).tolist()) == list(range(256))
        if K <= 16:
            assert all(kc.unit_variant(m, K, rows) == 0 for m in ms)


def test_expect_is_the_field_product(T):
    assert T.shape == (256, 256) and (T[1] == np.arange(256)).all() and not T[0].any()
    assert T[2][0x80] == 0x1D and T[3][7] == 9
    srcs = [kc.source(j, 64, 1) for j in range(3)]
    out = kc.expect(T, [[1, 0, 2], [3, 1, 1]], srcs)
    assert np.array_equal(out[0], srcs[0] ^ T[2][srcs[2]])
    assert np.array_equal(out[1], T[3][srcs[0]] ^ srcs[1] ^ srcs[2])


def _stripe(T, M, k, m, size, seed):
    data = [kc.source(j, size, seed) for j in range(k)]
    return np.concatenate([np.stack(data), kc.expect(T, np.asarray(M).reshape(m, k), data)])


def test_scrub_model_counters_agree_with_the_scrub_tests_model(T, restatement):
    from test_scrub_gpu import model
    k, m, size = 6, 3, 4117
    M = [int(c) for c in restatement.vandermonde_coding_matrix(k, m).ravel()]
    stripe = _stripe(T, M, k, m, size, 9)
    assert kc.scrub_model(T, M, k, m, stripe) == ((0, 0, 0), 0, None, [])
    assert model(T, M, k, m, stripe) == ((0, 0, 0), 0, None)
    for t, pos in ((0, [0, 4111, 4116]), (4, [17]), (k + 1, [5, 6]), (k + 2, list(range(size)))):
        bad = stripe.copy()
        bad[t, pos] ^= 0x5A
        got = kc.scrub_model(T, M, k, m, bad)
        assert got[:3] == model(T, M, k, m, bad)
        assert got[1] == len(pos) and got[2] == pos[0]
        assert got[3] == [t]
    two = stripe.copy()
    two[1, 3] ^= 1
    two[5, 900] ^= 1
    assert kc.scrub_model(T, M, k, m, two)[3] == []


def test_scrub_model_blame_rs_4_2_and_edges(T, restatement):
    k, m, size = 4, 2, 333
    M = [int(c) for c in restatement.vandermonde_coding_matrix(k, m).ravel()]
    stripe = _stripe(T, M, k, m, size, 2)
    for t in range(k + m):
        bad = stripe.copy()
        bad[t, [0, 100, size - 1]] ^= np.array([1, 0x80, 0xFF], dtype=np.uint8)
        assert kc.scrub_model(T, M, k, m, bad)[3] == [t]
    # m == 1: every shard is a candidate
    one = _stripe(T, [1, 2, 3], 3, 1, 64, 0)
    one[1, 5] ^= 9
    assert kc.scrub_model(T, [1, 2, 3], 3, 1, one) == ((1,), 1, 5, [0, 1, 2, 3])
    # include/ecgpu.h's non-MDS example: data shard 1 looks like coding shard 0
    nm = _stripe(T, [1, 1, 1, 0], 2, 2, 64, 0)
    nm[1, 7] ^= 0x10
    assert kc.scrub_model(T, [1, 1, 1, 0], 2, 2, nm)[3] == [1, 2]
    # an all-zero column: that shard's damage is invisible and it is never a candidate
    zc = _stripe(T, [1, 0, 3, 1, 0, 7], 3, 2, 64, 0)
    zc[1, 3] ^= 0xFF
    assert kc.scrub_model(T, [1, 0, 3, 1, 0, 7], 3, 2, zc) == ((0, 0), 0, None, [])
    zc[2, 3] ^= 0xFF
    assert kc.scrub_model(T, [1, 0, 3, 1, 0, 7], 3, 2, zc)[3] == [2]
