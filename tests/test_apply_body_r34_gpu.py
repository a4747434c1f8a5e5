"""The register-bounded R >= 3 body of gf_apply against the table reference.

gf_apply<K, R, UNITS> for R >= 3 consumes its sources one after the other
(csrc/gf_kernels_w8.hpp, gf_apply_body): K = 10 and 12, R = 3 and 4, unit
structure none and col0|row0, both store policies, 1 and 3 stripes, at the
sizes where a column kernel with a byte tail can go wrong: one column, one
lane short of a block, exactly a block, one lane into a second block, and a
block plus one column plus a 5-byte tail.  Expected bytes come from the
reference's 256 x 256 product table (tests/kernel_cases.py expect), and the
whole output slab is compared, guard bytes included.
"""
import pytest

import kernel_cases as kc
from test_kernel_table_gpu import Arena, run_plan

pytestmark = pytest.mark.gpu

SIZES = [16, 255 * 16, 256 * 16, 257 * 16, 4096 + 16 + 5]


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


@pytest.fixture(scope="module")
def T(vectors):
    return vectors["gf_mul_table"]


@pytest.mark.parametrize("R", [3, 4])
@pytest.mark.parametrize("K", [10, 12])
def test_sequential_body_matches_the_table(ec, gpu, T, K, R):
    ran = 0
    for stripes in (1, 3):
        for size in SIZES:
            arena = Arena(gpu, K, R, stripes, size)
            for U in (0, kc.COL0 | kc.ROW0):
                for nt in (1, 0):
                    M = kc.matrix_for(K, R, U, salt=nt)
                    run_plan(ec, arena, T, M, 0, nt,
                             f"plan v_perm K={K} R={R} U={U} nt={nt} size={size} stripes={stripes}", (1, 0))
                    ran += 1
    assert ran == 2 * len(SIZES) * 2 * 2
