"""The lab forms of the w = 8 kernel, launched through ecgpu_diag_launch.

diag_kernels_w8.hpp holds measurement-only forms of gf_apply as kernels of
their own: gf_apply_vec (VEC columns per lane, variant 8), gf_apply_2bit (the
2-bit-slice tables, variant 10); variant 13 picks gf_apply<K, R, UNITS, NT>
by its cache-policy bits.  Nothing else runs them, so this file does, against
the reference's 256 x 256 product table (tests/kernel_cases.py expect),
bit-exact.

Two stripes (the stripe stride of the pointer tables) of 16 * (256 * VEC + 3)
bytes: a second block in which only three columns of the first sub-column are
live -- the smallest shape where a lost live[v] guard or a wrong per-block
stride shows.  Outputs lie in a slab pre-filled with 0xCC; the whole slab is
compared, so every byte outside the outputs must stay 0xCC.
"""
import ctypes
import os

import numpy as np
import pytest

import kernel_cases as kc
from kernel_cases import FILL, GUARD

pytestmark = pytest.mark.gpu

STRIPES = 2
K = 10


@pytest.fixture(scope="module")
def diag(gpu):
    from erasure_coding_test_amd import _native as N
    lib = ctypes.CDLL(os.path.join(N.LIB_DIR, "libecgpu_diag.so"))
    lib.ecgpu_diag_launch.restype = ctypes.c_int
    lib.ecgpu_diag_launch.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4 + [
        ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def T(vectors):
    return vectors["gf_mul_table"]


def tables(gpu, coefs):
    """(qtab, ptab) of a coefficient list, laid out as tools/tune_kernels.py
    does: 4 words of 2-bit-slice products, then T0lo T0hi T1lo T1hi T2 + 3 pad."""
    import torch
    from erasure_coding_test_amd.galois import galois_single_multiply as gm
    word = lambda vals: sum(v << (8 * e) for e, v in enumerate(vals))
    q, p3 = [], []
    for c in (int(c) for c in coefs):
        q += [word([gm(c, e << (2 * p), 8) for e in range(4)]) for p in range(4)]
        p3 += [word([gm(c, e, 8) for e in range(4)]), word([gm(c, e, 8) for e in range(4, 8)]),
               word([gm(c, e << 3, 8) for e in range(4)]), word([gm(c, e << 3, 8) for e in range(4, 8)]),
               word([gm(c, e << 6, 8) for e in range(4)]), 0, 0, 0]
    dev = lambda w: torch.tensor(w, dtype=torch.int64).to(torch.int32).to(gpu)
    return dev(q), dev(p3)


def run(diag, gpu, T, M, size, variant, vec, mode, nt, label):
    import torch
    R = M.shape[0]
    stride = (size + GUARD + 15) // 16 * 16
    host = np.zeros((STRIPES, K, stride), dtype=np.uint8)
    for s in range(STRIPES):
        for j in range(K):
            host[s, j, :size] = kc.source(j + K * s, size, s)
    src = torch.from_numpy(host).to(gpu)
    out = torch.full((1 + STRIPES * R, stride), FILL, dtype=torch.uint8, device=gpu)  # row 0: a guard row
    src_tab = torch.tensor([src[s, j].data_ptr() for s in range(STRIPES) for j in range(K)], dtype=torch.int64).to(gpu)
    dst_tab = torch.tensor([out[1 + s * R + r].data_ptr() for s in range(STRIPES) for r in range(R)],
                           dtype=torch.int64).to(gpu)
    qtab, ptab = tables(gpu, M.ravel())
    torch.cuda.synchronize()
    rc = diag.ecgpu_diag_launch(variant, K, R, vec, mode, qtab.data_ptr(), None, src_tab.data_ptr(), dst_tab.data_ptr(),
                                STRIPES, size, 0, 0, nt, None, ptab.data_ptr())
    assert rc == 0, f"{label}: ecgpu_diag_launch returned {rc}"
    torch.cuda.synchronize()
    image = np.full((1 + STRIPES * R, stride), FILL, dtype=np.uint8)
    for s in range(STRIPES):
        image[1 + s * R:1 + (s + 1) * R, :size] = kc.expect(T, M, list(host[s, :, :size]))
    got = out.cpu().numpy()
    if not np.array_equal(got, image):
        row, pos = np.argwhere(got != image)[0]
        raise AssertionError(f"{label}: output row {row} (guard, then stripe * {R} + row) byte {pos} of {size}: "
                             f"expected {image[row, pos]:#04x} got {got[row, pos]:#04x}")
    assert np.array_equal(src.cpu().numpy(), host), f"{label}: a source changed"


# the unit structures the diagnostic library compiles in: RS(10,4) encode rows
# (column 0 and row 0 all ones) and the all-ones decode row
def shape_matrix(R):
    return kc.matrix_for(K, 4, 3) if R == 4 else kc.matrix_for(K, 1, 4)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("vec", [2, 4])
@pytest.mark.parametrize("R", [4, 1])
def test_vec_columns_per_lane(diag, gpu, T, R, vec, nt):
    run(diag, gpu, T, shape_matrix(R), 16 * (256 * vec + 3), 8, vec, 0, nt, f"variant 8 R={R} vec={vec} nt={nt}")


@pytest.mark.parametrize("R,mode,U", [(4, 3, 3), (1, 4, 4), (1, 0, 0)])
def test_two_bit_slice_tables(diag, gpu, T, R, mode, U):
    run(diag, gpu, T, kc.matrix_for(K, R, U), 16 * 259, 10, 1, mode, 1, f"variant 10 R={R} units={U}")


@pytest.mark.parametrize("ntb", [0, 1, 2, 3])
def test_production_kernel_by_cache_policy_bits(diag, gpu, T, ntb):
    run(diag, gpu, T, kc.matrix_for(K, 4, 3), 16 * 259, 13, ntb, 3, 1, f"variant 13 NT={ntb}")
