"""gf_apply at the lanes per workgroup each launch runs with.

csrc/gf_kernels_w8.hpp apply_block<K, R, UNITS, NT>() gives the RS(10,4) and
RS(6,3) Vandermonde encodes one-wave workgroups (B = 64) and every other
kernel B = 256; each of the two is also instantiated at 256 lanes (NT bit 2),
and the dispatcher (csrc/dispatch_w8.hip) launches that form for shards above
4 MiB, taking block and grid from the kernel it picked.  What can go wrong is
a column index or a grid that assumes the other size: columns skipped or
written twice at the edges of a workgroup.  Every shape below therefore runs,
through ecgpu_plan_*, at 1, B - 1, B, B + 1 and 2B + 3 columns of 16 B for
both values of B, at 255 and 257 columns, with a byte tail (16 (B + 1) + 5
bytes) and with one shard pointer misaligned by 1 (the whole shard then goes
through the byte kernel), for 1 and 3 stripes and both store policies; and
the two encodes run at exactly 4 MiB (the last size of the one-wave form) and
one column and a byte tail above it (the first of the 256-lane form).

Each output slab is compared byte for byte -- 0xCC guard bytes after every
shard's end and a guard row included -- with a numpy reference built from the
package's own GF(2^8) product table (galois_get_mult_table) and with the
LDS engine's output (ecgpu_plan_set_kernel), which keeps 256 lanes.

Residency: for the bench's two timed kernels, and the encode's 256-lane
form, the runtime must grant under the cap's dynamic-LDS allocation exactly
the intended waves per CU divided by the waves per workgroup (libecgpu_diag.so
ecgpu_diag_apply_residency).  That checks the kernels' lane counts, the
allocation arithmetic the dispatcher launches with (csrc/residency_w8.hpp)
and the LDS granularity of the device.  It does NOT check the dispatcher's
rule: the waves per CU are stated here (10 and 12, as
residency_waves_per_cu in dispatch_w8.hip has them), because the rule and
its constants live in libecgpu.so, out of the diagnostic library's reach; a
dispatcher that launched at another wave count would still pass this test.
"""
import ctypes
import os

import numpy as np
import pytest

import kernel_cases as kc
from kernel_cases import FILL, GUARD

pytestmark = pytest.mark.gpu

B_SMALL, B_FULL = 64, 256
COLUMNS = sorted({1, 255, 257} | {c for B in (B_SMALL, B_FULL) for c in (B - 1, B, B + 1, 2 * B + 3)})
SIZES = [16 * c for c in COLUMNS] + [16 * (B + 1) + 5 for B in (B_SMALL, B_FULL)]
MISALIGNED_SIZE = 16 * (B_SMALL + 1) + 5
ONE_WAVE_MAX_SHARD = 4 << 20  # gf_kernels_w8.hpp kOneWaveMaxShard
# waves per CU the dispatcher intends (dispatch_w8.hip residency_waves_per_cu): one-wave workgroups 10,
# 256-lane workgroups 12 for K + R >= 10
WAVES_ONE_WAVE, WAVES_FULL = 10, 12


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


@pytest.fixture(scope="module")
def T(ec):
    """The package's own 256 x 256 product table."""
    ec.galois.galois_create_mult_tables(8)
    t = np.array(ec.galois.galois_get_mult_table(8), dtype=np.uint8).reshape(256, 256)
    assert t[2, 0x80] == 0x1D and (t[1] == np.arange(256)).all() and not t[0].any()
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def shapes(ec):
    """name -> R x K coefficient matrix of one launch."""
    def encode(k, m):
        return np.array(ec.reed_sol.reed_sol_vandermonde_coding_matrix(k, m, 8), dtype=np.int64).reshape(m, k)

    def decode(k, m, erased):
        p = ec.DecodePlan(k, m, encode(k, m).ravel().tolist(), erased)
        c = np.array(p.coefs, dtype=np.int64).reshape(p.rows, p.nsrc)
        p.close()
        return c

    out = {"encode_10_4": encode(10, 4), "decode0_10_1": decode(10, 4, [0]), "decode0123_10_4": decode(10, 4, [0, 1, 2, 3]),
           "encode_6_3": encode(6, 3), "encode_12_4": encode(12, 4), "dense_16_4": kc.matrix_for(16, 4, 0)}
    assert out["decode0_10_1"].shape == (1, 10) and (out["decode0_10_1"] == 1).all()
    assert out["decode0123_10_4"].shape == (4, 10) and (out["decode0123_10_4"] > 1).sum() >= 30  # dense
    assert out["dense_16_4"].shape == (4, 16)
    return out


class Slab:
    """Sources [stripes, K, stride] and outputs [1 + stripes * R, stride] (row 0 a guard row); every shard is
    `size` bytes and followed by at least 16 guard bytes.  off_src: the one source whose pointer is misaligned
    by 1."""

    def __init__(self, gpu, K, R, stripes, size, off_src=None):
        import torch
        self.K, self.R, self.stripes, self.size, self.off_src = K, R, stripes, size, off_src
        self.stride = (1 + size + GUARD + 15) // 16 * 16
        host = np.zeros((stripes, K, self.stride), dtype=np.uint8)
        for s in range(stripes):
            for j in range(K):
                host[s, j, self._o(j):self._o(j) + size] = kc.source(j + K * s, size, s)
        host.setflags(write=False)
        self.host = host
        self.src = torch.from_numpy(host.copy()).to(gpu)
        self.out = torch.empty((1 + stripes * R, self.stride), dtype=torch.uint8, device=gpu)
        for s in range(stripes):
            assert [v.data_ptr() % 16 for v in self.srcs(s)] == [self._o(j) for j in range(K)]
            assert all(v.data_ptr() % 16 == 0 for v in self.dsts(s))

    def _o(self, j):
        return 1 if j == self.off_src else 0

    def data(self, s):
        return [self.host[s, j, self._o(j):self._o(j) + self.size] for j in range(self.K)]

    def srcs(self, s):
        return [self.src[s, j, self._o(j):self._o(j) + self.size] for j in range(self.K)]

    def dsts(self, s):
        return [self.out[1 + s * self.R + i, :self.size] for i in range(self.R)]

    def image(self, T, M):
        """The whole output slab as it must look: the products, 0xCC everywhere else."""
        img = np.full((1 + self.stripes * self.R, self.stride), FILL, dtype=np.uint8)
        for s in range(self.stripes):
            img[1 + s * self.R:1 + (s + 1) * self.R, :self.size] = kc.expect(T, M, self.data(s))
        return img

    def run(self, ec, M, kind, nt):
        """One plan launch; returns the output slab and the growth of the (v_perm, LDS) launch counters."""
        lib = ec._native.lib
        plan = ec.StripePlan(self.R, self.K, M.ravel().tolist()).set_kernel(kind, bool(nt))
        plan.bind([self.srcs(s) for s in range(self.stripes)], [self.dsts(s) for s in range(self.stripes)], self.size)
        self.out.fill_(FILL)
        before = (int(lib.ecgpu_engine_launches(0)), int(lib.ecgpu_engine_launches(1)))
        plan.launch()
        after = (int(lib.ecgpu_engine_launches(0)), int(lib.ecgpu_engine_launches(1)))
        got = self.out.cpu().numpy()
        plan.close()
        assert np.array_equal(self.src.cpu().numpy(), self.host), "a source changed"
        return got, (after[0] - before[0], after[1] - before[1])


def first_difference(got, want):
    row, pos = np.argwhere(got != want)[0]
    lo = max(0, pos - 4)
    return (f"row {row} byte {pos}: expected {want[row, lo:pos + 12].tobytes().hex()} "
            f"got {got[row, lo:pos + 12].tobytes().hex()} (from byte {lo}; row 0 is a guard row)")


def check(slab, ec, T, M, label, vector):
    want = slab.image(T, M)
    lds, grew = slab.run(ec, M, 1, 1)
    assert grew == ((0, 1) if vector else (0, 0)), f"{label} LDS: launch counters grew by {grew}"
    assert np.array_equal(lds, want), f"{label} LDS engine vs table: {first_difference(lds, want)}"
    for nt in (1, 0):
        got, grew = slab.run(ec, M, 0, nt)
        assert grew == ((1, 0) if vector else (0, 0)), f"{label} nt={nt}: launch counters grew by {grew}"
        assert np.array_equal(got, want), f"{label} nt={nt} vs table: {first_difference(got, want)}"
        assert np.array_equal(got, lds), f"{label} nt={nt} vs LDS engine: {first_difference(got, lds)}"


@pytest.mark.parametrize("name", ["encode_10_4", "decode0_10_1", "decode0123_10_4", "encode_6_3", "encode_12_4",
                                  "dense_16_4"])
def test_plan_launches_match_table_and_lds_engine(ec, gpu, T, shapes, name):
    M = shapes[name]
    R, K = M.shape
    ran = 0
    for stripes in (1, 3):
        for size in SIZES:
            check(Slab(gpu, K, R, stripes, size), ec, T, M, f"{name} size={size} stripes={stripes}", vector=True)
            ran += 1
        # one pointer off by 1: no 16-B columns at all, the byte kernel covers the whole shard
        check(Slab(gpu, K, R, stripes, MISALIGNED_SIZE, off_src=K - 1), ec, T, M,
              f"{name} misaligned size={MISALIGNED_SIZE} stripes={stripes}", vector=False)
    assert ran == 2 * len(SIZES) and len(SIZES) == 11


@pytest.mark.parametrize("name", ["encode_10_4", "encode_6_3"])
def test_both_forms_at_the_shard_size_threshold(ec, gpu, T, shapes, name):
    """4 MiB is the last shard size of the one-wave form; 16 bytes more (and a 5-byte tail) take the 256-lane one."""
    M = shapes[name]
    R, K = M.shape
    for size in (ONE_WAVE_MAX_SHARD, ONE_WAVE_MAX_SHARD + 16 + 5):
        check(Slab(gpu, K, R, 1, size), ec, T, M, f"{name} size={size}", vector=True)


@pytest.fixture(scope="module")
def diag(ec):
    lib = ctypes.CDLL(os.path.join(ec._native.LIB_DIR, "libecgpu_diag.so"))
    lib.ecgpu_diag_apply_residency.restype = ctypes.c_int
    lib.ecgpu_diag_apply_residency.argtypes = [ctypes.c_int] * 6 + [
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int)]
    return lib


@pytest.mark.parametrize("K,R,units,big,lanes,waves", [(10, 4, 3, 0, B_SMALL, WAVES_ONE_WAVE),
                                                       (10, 4, 3, 1, B_FULL, WAVES_FULL),
                                                       (10, 1, 4, 0, B_FULL, WAVES_FULL)])
def test_cap_allocation_grants_the_intended_residency(gpu, diag, K, R, units, big, lanes, waves):
    """The bench's encode and decode{0}: lanes per workgroup as this file's sizes assume, and the occupancy the
    runtime reports under the dispatcher's allocation is waves per CU / waves per workgroup."""
    for store_nt in (1, 0):
        got_lanes, lds, wgs = ctypes.c_int(0), ctypes.c_uint(0), ctypes.c_int(0)
        rc = diag.ecgpu_diag_apply_residency(K, R, units, store_nt, big, waves, ctypes.byref(got_lanes), ctypes.byref(lds),
                                             ctypes.byref(wgs))
        assert rc == 0
        print(f"gf_apply<{K},{R},{units}> store_nt={store_nt} big={big}: {got_lanes.value} lanes, {lds.value} B dynamic LDS, "
              f"{wgs.value} workgroups per CU for {waves} waves per CU")
        assert got_lanes.value == lanes
        assert 0 < lds.value <= 65536
        assert wgs.value * (lanes // 64) == waves and waves % (lanes // 64) == 0
