// dispatch_w8.hip -- how a w = 8 plan launches: the production v_perm engine
// or the LDS nibble-table engine (gf_kernels_w8.hpp, specialised in
// gf_spec.hip), the unit-coefficient structure of each launch, its residency
// cap and store policy, the coefficient tables a plan uploads, and the
// byte-tail kernel gf_apply_bytes.  With gf_device.hpp,
// gf_kernels_w8.hpp and gf_spec.* this file is the w = 8 kernel build ID
// (ecgpu_build_id(1), erasure_coding_test_amd/build.py): what a rocprofv3 PMC
// record of the bench's encode / decode launches is valid for.  The
// synchronous calls' staging and the C ABI live in ecgpu_runtime.hip, the
// w = 16 / 32 dispatch in dispatch_wide.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ecgpu.h"
#include "gf_host.hpp"
#include "gf_kernels_w8.hpp"
#include "knobs.hpp"
#include "residency_w8.hpp"
#include "runtime.hpp"
#include "gf_spec.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;
using dev::ApplyArgs;
using dev::u32x4;

namespace ecgpu {
namespace dev {

// --------------------------------------- bytes: tails, misaligned shards ----
// One lane per byte in [byte0, size); any K, R <= kMaxRows, any alignment.
static __global__ __launch_bounds__(kBlock) void gf_apply_bytes(ApplyArgs a) {
  const int64_t x = a.byte0 + int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= a.size) return;
  const int s = blockIdx.y;
  const uint8_t* const* sp = a.src + int64_t(s) * a.src_stride;
  uint8_t* const* dp = a.dst + int64_t(s) * a.dst_stride + a.row0;
  uint32_t acc[kMaxRows] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < a.K; ++j) {
    const uint32_t v = sp[j][x];
    const uint32_t s0 = v & 3u, s1 = (v >> 2) & 3u, s2 = (v >> 4) & 3u, s3 = v >> 6;
    for (int r = 0; r < a.R; ++r) acc[r] ^= gf_mul_perm(a.qtab[r * a.K + j], s0, s1, s2, s3);
  }
  for (int r = 0; r < a.R; ++r) dp[r][x] = uint8_t(acc[r]);
}

}  // namespace dev
}  // namespace ecgpu

ECGPU_RT_BEGIN

// Production kernels: gf_apply<K, R, UNITS> specialised at compile time
// (gf_spec.hpp, one translation unit per R): one 16-B column per lane,
// 3-bit-slice v_perm multiply, XOR3 via v_bitop3, unit-coefficient
// structure fixed per launch, non-temporal loads; store policy per launch.
// Which compile-time unit structure holds exactly for rows [r0, r0+R).
int unit_variant(const std::vector<uint32_t>& coef, int K, int r0, int R) {
  bool all = true, col0 = true, row0 = true;
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < K; ++j) {
      const bool one = coef[size_t(r0 + r) * K + j] == 1;
      all &= one;
      if (j == 0) col0 &= one;
      if (r == 0) row0 &= one;
    }
  if (all) return 4;
  return (col0 ? 1 : 0) | (row0 ? 2 : 0);
}

KernelFn generic_fn(int R) {
  switch (R) {
    case 1: return &dev::gf_apply_perm_generic<1>;
    case 2: return &dev::gf_apply_perm_generic<2>;
    case 3: return &dev::gf_apply_perm_generic<3>;
    default: return &dev::gf_apply_perm_generic<4>;
  }
}


// Residency cap for the streaming kernels.  Fewer resident workgroups per CU
// means fewer DRAM pages open at once across the chip: each lane reads K
// shards and writes R, and a kernel left to its register limit (8 workgroups
// per CU for the 46-64 VGPR kernels) keeps ~30k distinct 4 KiB shard chunks in
// flight.  What matters is the number of shard streams per lane, K + R: a
// sweep over eight encode and decode shapes (K + R = 5..16, 64 KiB..16 MiB
// shards, 3 interleaved rounds, profiles/r02_residency_sweep.json) has
// 4 blocks/CU best or within 0.3 % of the best for K + R <= 9 and 3 blocks/CU
// for K + R >= 10.  That sweep's R >= 3 rows ran kernels of 155-209 VGPRs,
// which sit at 2-3 per CU under any cap; with the sequential body (50-105
// VGPRs, gf_kernels_w8.hpp) the cap governs them too, and the same rule holds
// (profiles/r07_residency_lab.json: RS(10,4) encode 873-876 us at 2 and 3
// per CU, 959-987 at 4-6, 1011 uncapped; RS(6,3) 752-762 at 2-5).
// The rule is stated in waves per CU, and the workgroups per CU follow from
// the kernel's lanes per workgroup (gf_kernels_w8.hpp apply_block, carried by
// SpecKernel): 256-lane kernels run at 4 * kCapMaxBlocks = 16 waves per CU
// for K + R <= 9 and 12 above, as 4 and 3 workgroups; one-wave workgroups
// (the RS(10,4) and RS(6,3) encodes up to 4 MiB shards; above that their
// 256-lane instantiation runs, at the 256-lane rule) at kCapWavesOneWave = 10, which the
// 256-lane form cannot express (profiles/r09_wg_lab.json, 64 lanes at 8 / 10
// / 12 / 14 / 16 waves per CU: RS(10,4) encode 842 / 848 / 862 / 883 / 898 us,
// 256 lanes at 12: 866; the dense 4 x 10 map 919 / 907 / 882 / 893 / 908
// against 895-905; RS(6,3) 731 / 722 / 733 / 745 / 759 against 756 -- 10 is
// the one point that loses on none of them).
// A 256-thread workgroup puts one wave on each SIMD, so a cap of N per CU is
// real only while the kernel fits N waves on a SIMD: every specialised
// kernel must reach kMinWavesPerSimd (tests/test_kernel_resources.py
// compiles the bench's instantiations and checks).  The cap is an unused
// dynamic LDS allocation of LDS_per_CU / workgroups (rounded down to 512 B);
// at least 3 workgroups per CU, so never above the 64 KiB a launch may ask
// for without raising the function's limit, and what the runtime grants is
// exactly the intended count (tests/test_apply_block_gpu.py asks it).  A kernel with static LDS of
// its own (the LDS engine's tables) gets that much less and a further 4 KiB
// margin, rounded down to 4 KiB: RS(10,4) at "3 per CU" with 1,280 B of
// tables, dynamic 52,736 B (1.8 KiB spare) ran at 2 per CU's speed (989 us),
// 40,960-49,152 B at 902-905 (tools/encode_lab.hip --lds 2).
// ECGPU_BLOCKS_PER_CU fixes the residency in units of one 256-lane
// workgroup, i.e. 4 waves, per CU (0 = never cap).
constexpr int kCapMaxBlocks = 4;     // K + R <= 9; one fewer above
constexpr int kMinWavesPerSimd = 4;  // what every specialised v_perm kernel's VGPR count must allow
static_assert(kMinWavesPerSimd >= kCapMaxBlocks, "a cap above the register limit is a no-op");
constexpr int kWavesPerBlock = dev::kBlock / kLanesPerWave;  // one per SIMD
constexpr int kCapWavesOneWave = 10;                           // one-wave workgroups, any K + R
static_assert(kCapWavesOneWave <= kMinWavesPerSimd * kWavesPerBlock, "a cap above the register limit is a no-op");
int residency_waves_per_cu(int streams, int lanes) {
  const int fixed = knob(Knob::kBlocksPerCu);
  if (fixed >= 0) return fixed * kWavesPerBlock;
  if (lanes < dev::kBlock) return kCapWavesOneWave;
  return (streams <= 9 ? kCapMaxBlocks : kCapMaxBlocks - 1) * kWavesPerBlock;
}

unsigned residency_lds_bytes(int device, int streams, unsigned static_bytes, int lanes) {
  static std::once_flag once;
  static int per_cu = 0;
  std::call_once(once, [&] {
    if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) != hipSuccess)
      per_cu = 0;
  });
  return residency_lds_for(per_cu, residency_workgroups(residency_waves_per_cu(streams, lanes), lanes), static_bytes);
}

// Per-launch policy of the production kernel (A/B on MI355X in the bench's
// back-to-back context, DESIGN.md §5, profiles/r01_policy_ab.json):
//   * stores non-temporal (loads always are): bench step +4 %, RS(10,4)
//     encode 0.947 -> 0.889 ms, dense decode +9 %, RS(12,4) +6 %;
//   * residency cap: always for the sequential body (`seq`: a specialised
//     v_perm launch of dev::kSeqMinRows rows or more) -- at its 50-105 VGPRs an
//     uncapped launch runs 4-8 workgroups per CU and loses 10-15 % (dense
//     decode{0,1,2,3}: 894-899 us at 3 per CU, 997 uncapped; the 155-VGPR
//     body it replaces ran 904-918 at its register limit of 3, which is what
//     "needs the occupancy" used to mean);
//   * for the other kernels (R <= 2, generic K, the LDS engine) unless the
//     launch is dense in GF multiplies (more than 2.5 non-unit coefficients
//     per shard touched): decode{0} +9 % capped.
// The store policy is the plan's `nt` field (0 plain, 1 nt -- the default;
// ECGPU_NT, ecgpu_plan_set_kernel); the cap knob (ECGPU_CAP: 0 = never,
// 1 = always) overrides the cap rule.
bool cap_for(int K, int R, int mul_terms, bool seq) {
  const int v = knob(Knob::kCap);
  return v < 0 ? (seq || 2 * mul_terms <= 5 * (K + R)) : (v != 0);
}

// Per-coefficient tables.  PERM: word p holds c*(e << 2p) in byte e.  LDS:
// 16 low-nibble products then 16 high-nibble products.
// P3 (production, gf_device.hpp mac3): T0[e] = c*e and T1[e] = c*(e << 3)
// for e < 8 as dword pairs (low dword = entries 0..3), T2[e] = c*(e << 6).
void build_tables(int c, u32x4* q, uint32_t* p3, uint8_t* nib) {
  const auto& T = gf8().mul[c & 0xFF];
  uint32_t w[4];
  for (int p = 0; p < 4; ++p) {
    w[p] = 0;
    for (int e = 0; e < 4; ++e) w[p] |= uint32_t(T[e << (2 * p)]) << (8 * e);
  }
  *q = u32x4{w[0], w[1], w[2], w[3]};
  for (int i = 0; i < dev::kP3Words; ++i) p3[i] = 0;
  for (int e = 0; e < 8; ++e) {
    p3[e >> 2] |= uint32_t(T[e]) << (8 * (e & 3));
    p3[2 + (e >> 2)] |= uint32_t(T[e << 3]) << (8 * (e & 3));
  }
  for (int e = 0; e < 4; ++e) p3[4] |= uint32_t(T[e << 6]) << (8 * e);
  for (int x = 0; x < 16; ++x) {
    nib[x] = T[x];
    nib[16 + x] = T[x << 4];
  }
}

// The w = 8 part of plan_init: [2-bit | 3-bit-slice | nibble] tables of
// every coefficient, one upload.
int plan_init_w8(ecgpu_plan* p, const int* coefs) {
  const size_t n = p->coef.size();
  for (size_t i = 0; i < n; ++i) p->coef[i] = uint32_t(coefs[i]) & 0xFFu;
  std::vector<u32x4> q(n);
  std::vector<uint32_t> p3(n * dev::kP3Words);
  std::vector<uint8_t> nib(n * 32);
  for (size_t i = 0; i < n; ++i) build_tables(coefs[i], &q[i], &p3[i * dev::kP3Words], &nib[i * 32]);
  // [2-bit tables | 3-bit tables | nibble tables] in one allocation, ONE
  // asynchronous upload (plan_upload_tables; three blocking copies cost ~12 us
  // each, tools/hip_overheads.cpp)
  const size_t qb = n * sizeof(u32x4), pb = p3.size() * sizeof(uint32_t), nb = n * 32;
  std::vector<uint8_t> host(qb + pb + nb);
  std::memcpy(host.data(), q.data(), qb);
  std::memcpy(host.data() + qb, p3.data(), pb);
  std::memcpy(host.data() + qb + pb, nib.data(), nb);
  if (int rc = plan_upload_tables(p, std::move(host))) return rc;
  p->d_q = reinterpret_cast<u32x4*>(p->d_tabs);
  p->d_p3 = reinterpret_cast<uint32_t*>(p->d_tabs + qb);
  p->d_nib = p->d_tabs + qb + pb;
  return ECGPU_OK;
}

// Specialised w = 8 column launches per engine (ECGPU_KERNEL_PERM / _LDS),
// for tests that a knob switch reached the launches (ecgpu_engine_launches).
std::atomic<int64_t> g_engine_launches[2];

int plan_launch(ecgpu_plan* p, hipStream_t stream) {
  if (p->stripes <= 0 || p->size <= 0 || p->rows <= 0) return ECGPU_OK;
  DeviceGuard g(p->device);
  if (int rc = plan_wait_tables(p, stream)) return rc;
  if (p->w != 8) return plan_launch_wide(p, stream);
  const int K = p->nsrc;
  const int64_t nvec = p->aligned ? p->size / 16 : 0;
  const int64_t byte0 = nvec * 16;
  for (int r0 = 0; r0 < p->rows; r0 += dev::kMaxRows) {
    const int R = std::min(dev::kMaxRows, p->rows - r0);
    const bool spec = K <= dev::kMaxSpecK;
    int mul_terms = 0;  // coefficients that are neither 0 nor 1
    for (int r = 0; r < R; ++r)
      for (int j = 0; j < K; ++j) mul_terms += p->coef[size_t(r0 + r) * K + j] > 1u;
    // The v_perm engine unless ECGPU_KERNEL / ecgpu_plan_set_kernel asks for the
    // LDS nibble-table engine.  (Dense launches on the LDS engine were tried:
    // an in-process interleaved A/B has v_perm 2.5 % faster on C4 decode
    // {0,1,2,3} and even on RS(12,4) {0,1,2,3}, profiles/r02_engine_ab_inprocess.json.)
    const bool use_lds = p->kind == ECGPU_KERNEL_LDS;
    // the kernel and the lanes per workgroup it was compiled for travel together
    const bool big = p->size > dev::kOneWaveMaxShard;
    const SpecKernel vec_k = spec ? spec_kernel(use_lds, K, R, unit_variant(p->coef, K, r0, R), p->nt, big)
                                  : SpecKernel{generic_fn(R), dev::kBlock};
    if (!vec_k.fn || vec_k.block <= 0) return ECGPU_ERR_ARG;
    if (spec && nvec > 0) g_engine_launches[use_lds ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
    // Both engines follow the cap rule; the LDS engine's allocation leaves room
    // for its K * 128 B of tables (tools/encode_lab.hip --lds: RS(10,4) encode
    // 1008 us uncapped, 902 at 3 per CU, v_perm 890).
    const bool cap = cap_for(K, R, mul_terms, spec && !use_lds && R >= dev::kSeqMinRows);
    const unsigned static_lds = use_lds && spec ? unsigned(K) * 32u * 4u : 0u;
    uint64_t unit = 0, zero = 0;
    if (spec)
      for (int r = 0; r < R; ++r)
        for (int j = 0; j < K; ++j) {
          const uint32_t c = p->coef[size_t(r0 + r) * K + j];
          if (c == 1) unit |= uint64_t(1) << (r * K + j);
          if (c == 0) zero |= uint64_t(1) << (r * K + j);
        }
    for (int s0 = 0; s0 < p->stripes; s0 += dev::kMaxGridY) {
      const int ns = std::min(dev::kMaxGridY, p->stripes - s0);
      ApplyArgs a{};
      a.qtab = p->d_q + size_t(r0) * K;
      a.ptab = p->d_p3 + size_t(r0) * K * dev::kP3Words;
      a.ntab = p->d_nib + size_t(r0) * K * 32;
      a.src = p->d_src + size_t(s0) * K;
      a.dst = p->d_dst + size_t(s0) * p->rows;
      a.nvec = nvec;
      a.size = p->size;
      a.byte0 = byte0;
      a.src_stride = K;
      a.dst_stride = p->rows;
      a.row0 = r0;
      a.K = K;
      a.R = R;
      a.nt = p->nt;
      a.unit_mask = unit;
      a.zero_mask = zero;
      if (nvec > 0) {
        const int64_t per_block = vec_k.block;
        const dim3 grid(unsigned((nvec + per_block - 1) / per_block), unsigned(ns));
        const unsigned lds = cap ? residency_lds_bytes(p->device, K + R, static_lds, vec_k.block) : 0u;
        ECGPU_HIP(launch(vec_k.fn, grid, dim3(unsigned(vec_k.block)), a, stream, lds));
      }
      if (byte0 < p->size) {
        const dim3 grid(unsigned((p->size - byte0 + dev::kBlock - 1) / dev::kBlock), unsigned(ns));
        ECGPU_HIP(launch(&dev::gf_apply_bytes, grid, dim3(dev::kBlock), a, stream));
      }
    }
  }
  return ECGPU_OK;
}

ECGPU_RT_END

extern "C" ECGPU_API int64_t ecgpu_engine_launches(int kind) {
  return kind == 0 || kind == 1 ? ecgpu::rt::g_engine_launches[kind].load(std::memory_order_relaxed) : -1;
}
