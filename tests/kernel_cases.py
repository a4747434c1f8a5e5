"""Case generator for the sweep of the specialised w = 8 kernel table
(tests/test_kernel_table_gpu.py; checked without a GPU by
tests/test_kernel_cases.py).  Plain Python / numpy.

The hot path is a compile-time table: gf_apply / gf_apply_inl / scrub_verify
<K, R, UNITS> for K = 1..16, R = 1..4 and five unit structures, picked per
launch by unit_variant() in csrc/dispatch_w8.hip.  A cell (K, R, U) is one
entry of that table; the functions here build, for every cell the host rule
can return, a coefficient matrix that lands exactly on it and misses the
neighbouring cells as narrowly as possible, the source bytes that put every
byte value at every position of a 16-B column, and the expected outputs from
the reference's own 256 x 256 product table.
"""
import numpy as np

KS = range(1, 17)   # K specialised at compile time (kMaxSpecK)
RS = range(1, 5)    # rows per launch (kMaxRows)
COL0, ROW0, ALL = 1, 2, 4

SIZE = 4117     # one full 256-lane block, a second block with one live lane, a 5-byte tail
SIZE_ZC = 8229  # 514 columns: with a one-block grid lane 0 makes three trips, lanes 2..255 two; 5-byte tail
GUARD = 16
FILL = 0xCC


def unit_variant(coefs, K, R):
    """The host rule of csrc/dispatch_w8.hip: which compile-time unit
    structure holds exactly for an R x K launch."""
    c = np.asarray(coefs).reshape(R, K)
    if (c == 1).all():
        return 4
    return (COL0 if (c[:, 0] == 1).all() else 0) | (ROW0 if (c[0] == 1).all() else 0)


def reachable_cells():
    """Every (K, R, U) the rule can return, by enumeration: each of the four
    parts of a matrix the rule looks at (the corner, the rest of column 0, the
    rest of row 0, the interior) is either all ones or not."""
    cells = set()
    for K in KS:
        for R in RS:
            parts = [p for p in ([(0, 0)], [(r, 0) for r in range(1, R)], [(0, j) for j in range(1, K)],
                                 [(r, j) for r in range(1, R) for j in range(1, K)]) if p]
            for bits in range(1 << len(parts)):
                m = np.ones((R, K), dtype=np.int64)
                for i, p in enumerate(parts):
                    if (bits >> i) & 1:
                        m[p[0]] = 2
                cells.add((K, R, unit_variant(m, K, R)))
    return sorted(cells)


def _seed(K, R, U, salt):
    return ((K * 4 + R) * 5 + U) * 13 + 101 * salt


class _General:
    """A running counter over the general coefficients 2..255."""

    def __init__(self, start):
        self.i = start

    def __call__(self):
        v = 2 + self.i % 254
        self.i += 1
        return v


def matrix_for(K, R, U, salt=0):
    """An R x K matrix whose variant is exactly U, a near miss of every
    structure not in U: column 0 all ones except the last row (Col0 not in U),
    row 0 all ones except the last column (Row0 not in U) -- with a single row
    or column and U = 0, all ones except the corner; U = 3 is all ones except
    (R-1, K-1).  The interior holds general coefficients from a running
    counter, with one 0 and one extra 1 where it has two entries or more.  No
    row or column is all zero."""
    if (K, R, U) not in _REACHABLE:
        raise ValueError(f"unit_variant cannot return {U} for K = {K}, R = {R}")
    seed = _seed(K, R, U, salt)
    g = _General(seed)
    m = np.ones((R, K), dtype=np.int64)
    if U == 4:
        return m
    if U == 3:
        m[R - 1, K - 1] = g()
        return m
    interior = [(r, j) for r in range(1, R) for j in range(1, K)]
    for p in interior:
        m[p] = g()
    n = len(interior)
    if n >= 2:
        z = seed % n
        m[interior[z]] = 0
        m[interior[(z + 1 + (seed // n) % (n - 1)) % n]] = 1
    if U == 0 and (R == 1 or K == 1):
        m[0, 0] = g()  # a single row or column: the corner is the one entry that misses both structures
    else:
        if not U & COL0:
            m[R - 1, 0] = g()
        if not U & ROW0:
            m[0, K - 1] = g()
    assert unit_variant(m, K, R) == U
    return m


def fused_order(coefs):
    """The order in which a synchronous jerasure_matrix_encode hands the data
    shards to the kernel (csrc/planner.cpp): LinearTracker numbers a buffer
    when a dot product first touches it -- the row's unit coefficients in
    index order, then its other non-zero ones -- and finish() lists the
    sources of the fused map in that order.  Returns the data indices; the
    launch sees coefs[:, order]."""
    c = np.asarray(coefs)
    order = []
    for row in c:
        for j in [j for j, v in enumerate(row) if v == 1] + [j for j, v in enumerate(row) if v > 1]:
            if j not in order:
                order.append(j)
    return order


def inline_matrix_for(K, R, U, salt=0):
    """matrix_for, adjusted where the synchronous calls' source ordering
    (fused_order) would move the launch to another cell: a one-row matrix of
    variant 0 with ones in it is launched ones first, as variant 1, so those
    ones become general coefficients.  Every other matrix_for result keeps
    its column order."""
    m = matrix_for(K, R, U, salt)
    if unit_variant(m[:, fused_order(m)], K, R) != U:
        g = _General(_seed(K, R, U, salt) + 64)
        for j in range(K):
            if m[0, j] == 1:
                m[0, j] = g()
    order = fused_order(m)
    assert len(order) == K and unit_variant(m[:, order], K, R) == U
    return m


def lds_matrix_for(K, R, salt=0):
    """General coefficients plus the columns the LDS engine's zero_mask /
    unit_mask shortcuts must tell apart: the last column special in the last
    row (mask bit R*K - 1; 1 for an even salt, 0 for an odd one), then, as K
    allows, an all-ones column, an all-zero column and (R >= 2) a column that
    mixes 0 and 1 and must take neither shortcut."""
    g = _General(_seed(K, R, 0, salt) + 7)
    m = np.array([[g() for _ in range(K)] for _ in range(R)], dtype=np.int64)
    m[R - 1, K - 1] = 1 - salt % 2
    free = list(range(K - 1))
    if salt % 2:
        free.reverse()
    if free:
        m[:, free.pop(0)] = 1
    if free:
        m[:, free.pop(0)] = 0
    if free and R >= 2:
        j = free.pop(0)
        m[:, j] = [(r + salt) % 2 for r in range(R)]
    return m


def pattern_block():
    """4,096 bytes, byte x = (x // 16 + 17 * (x % 16)) & 0xFF: every byte
    value at each of the 16 positions of a 16-B column."""
    x = np.arange(4096)
    return ((x // 16 + 17 * (x % 16)) & 0xFF).astype(np.uint8)


def source(j, size, seed=0):
    """Source j: the pattern block rotated by 31 * j, then seeded random bytes."""
    blk = np.roll(pattern_block(), 31 * j)
    rnd = np.random.default_rng([seed, j]).integers(0, 256, max(0, size - blk.size), dtype=np.uint8)
    return np.concatenate([blk, rnd])[:size]


def expect(T, coefs, srcs):
    """[R, size]: XOR over j of T[coefs[r][j]][srcs[j]], T the reference's product table."""
    c = np.asarray(coefs)
    out = np.zeros((c.shape[0], len(srcs[0])), dtype=np.uint8)
    for r in range(c.shape[0]):
        for j in range(c.shape[1]):
            out[r] ^= T[int(c[r, j]) & 0xFF][srcs[j]]
    return out


def table_matrices(rows, K):
    """All 256 coefficients, 0 and 1 included, as 256 / (rows * K) matrices of
    rows x K consecutive values: none has a unit structure, so every entry is
    plain table contents."""
    n = rows * K
    return [np.arange(i * n, (i + 1) * n, dtype=np.int64).reshape(rows, K) for i in range(256 // n)]


def scrub_model(T, M, k, m, stripe):
    """(bad_bytes, bad_cols, first_bad, blame) of one stripe [k + m, size].

    The counters are those of include/ecgpu.h: syn[i] = coding[i] ^ XOR_j
    M[i][j] * data[j]; a position is bad when any syn[i] is non-zero.  blame
    is the sorted list of shards that alone explain every bad position: the
    intersection over the bad positions of coding shard p iff only syn[p] is
    non-zero, and data shard j iff the syndrome is e * column j for some e."""
    M = np.asarray(M).reshape(m, k)
    stripe = np.asarray(stripe)
    syn = stripe[k:] ^ expect(T, M, list(stripe[:k]))
    bad = syn != 0
    cols = bad.any(axis=0)
    counters = (tuple(int(v) for v in bad.sum(axis=1)), int(cols.sum()), int(np.argmax(cols)) if cols.any() else None)
    if not cols.any():
        return counters + ([],)
    seen = np.unique(syn[:, cols], axis=1)                                      # [m, distinct bad syndromes]
    blame = []
    for j in range(k):
        multiples = T[M[:, j] & 0xFF][:, 1:]                                    # [m, 255]: e * column j, e = 1..255
        if (seen[:, :, None] == multiples[:, None, :]).all(axis=0).any(axis=1).all():
            blame.append(j)
    for p in range(m):
        if not np.delete(seen, p, axis=0).any():
            blame.append(k + p)
    return counters + (blame,)


_REACHABLE = frozenset(reachable_cells())
