// gf_kernels_w8.hpp -- the production w = 8 kernels of the library: the
// v_perm engine gf_apply, the one-stripe inline form, the LDS nibble-table
// engine and the generic-K kernel, on the device vocabulary of gf_device.hpp.
// Included by the units that instantiate them (gf_spec.hip, dispatch_w8.hip,
// which also holds the byte-tail kernel) and through gf_kernels.hpp (the
// overview) by the tools.  The measurement-only forms (VEC columns per lane,
// 2-bit PERM, LDS-DMA, occupancy-8, streaming, copy) live in
// diag_kernels_w8.hpp, compiled into libecgpu_diag.so only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.hpp"

namespace ecgpu {
namespace dev {

// R output columns from the K source columns of one lane with the launch's
// 3-bit-slice tables (combine_store: then R stores).
template <int K, int R, int UNITS>
__device__ __forceinline__ void combine(const ApplyArgs& a, const u32x4 (&x)[K], u32x4 (&acc)[R]) {
  // constant address space: always a scalar load, even after an LDS-DMA
  // (which the compiler otherwise treats as a clobber)
  combine3<K, R, UNITS>((const kconst_u32*)a.ptab, x, acc);  // C cast: generic -> constant
}

template <int K, int R, int UNITS, int NTS>
__device__ __forceinline__ void combine_store(const ApplyArgs& a, const u32x4 (&x)[K], uint8_t* const (&dp)[R],
                                              int64_t col) {
  u32x4 acc[R];
  combine<K, R, UNITS>(a, x, acc);
#pragma unroll
  for (int r = 0; r < R; ++r) store16t<NTS>(dp[r], col, acc[r]);
}

// Launches of kSeqMinRows output rows or more take the sequential form of
// gf_apply_body, whose load schedule is a window: load_window<K>() source
// loads are issued before the first multiply and one more as each source is
// consumed.  Interleaved in one process at 3 workgroups per CU
// (tools/encode_lab.hip --resid 2, profiles/r07_residency_lab.json): a
// window of 4-6 beats every load first by 1.6-3.5 % on RS(10,4) at 1, 4 and
// 16 MiB shards and by 0-2 % on RS(12,4) at 1 and 4 MiB, but loses 9 % on
// RS(12,4) at 16 MiB (C5: 1071 vs 981 us), the one shape where a late load
// costs.  Hence 6 up to K = 10 and every load first above; K <= 6 is the same
// kernel either way.  (Two points per K: a rule by shard size would need a
// second instantiation of every kernel.)
constexpr int kSeqMinRows = 3;
template <int K>
constexpr int load_window() { return K <= 10 ? 6 : K; }

// Lanes per workgroup of gf_apply<K, R, UNITS, NT>.  A workgroup is the unit
// in which the kernel bursts -- its waves start in the same cycle and its
// residency slot is held until the slowest of them has stored -- so one-wave
// workgroups under a cap in waves per CU space a CU's requests out.
// Interleaved in one process at equal waves per CU (tools/encode_lab.hip
// --wg 1, profiles/r09_wg_lab.json): 64 lanes at 10 waves per CU beat 256
// lanes at 12 by 2.0 % on RS(10,4) encode at 4 MiB shards (848 vs 866 us) and
// by 4.5 % on RS(6,3) at 1 MiB, and are level on RS(10,4) at 1 MiB; at 16 MiB
// shards they lose 31 % (1135 vs 869 us), as they do on RS(12,4) at 16 MiB,
// and RS(12,4) is best at 256 lanes at 1 and 4 MiB too.  The dense 4 x 10 map
// gains nothing (907 vs 895-905), nor does the R <= 2 body on decode{0} (683
// vs 679).  So only the two encodes that were measured to gain take the
// one-wave form, and only up to kOneWaveMaxShard bytes per shard: the shard
// size is known at the launch, so each of them is also instantiated at 256
// lanes under kNt256Lanes, a bit of NT that changes nothing else, and the
// dispatcher picks by size (dispatch_w8.hip).  Every other (K, R, UNITS) has
// one form, 256 lanes, whatever the bit says.
constexpr int kNt256Lanes = 4;  // NT bit 2: the 256-lane instantiation of a kernel that has a one-wave form
constexpr int64_t kOneWaveMaxShard = int64_t(4) << 20;
template <int K, int R, int UNITS>
constexpr bool has_one_wave_form() {
  return UNITS == (kUnitCol0 | kUnitRow0) && ((K == 10 && R == 4) || (K == 6 && R == 3));
}
template <int K, int R, int UNITS, int NT>
constexpr int apply_block() { return has_one_wave_form<K, R, UNITS>() && !(NT & kNt256Lanes) ? 64 : kBlock; }

// Lane l of block b handles the 16-byte column b*BS + l of every shard of
// stripe s (BS: apply_block of the kernel; the lab instantiates the body at
// other sizes, diag_kernels_w8.hpp gf_apply_wg); R < kSeqMinRows: all K loads
// are issued before any arithmetic, then R stores.  NT: bit 0 = non-temporal
// loads, bit 1 = store policy of store16t, bit 2 = kNt256Lanes.
template <int K, int R, int UNITS, int NT = 3, int BS = apply_block<K, R, UNITS, NT>()>
__device__ __forceinline__ void gf_apply_body(const ApplyArgs& a) {
  const unsigned cblk = a.stripe_fast ? blockIdx.y : blockIdx.x;
  const int s = a.stripe_fast ? blockIdx.x : blockIdx.y;
  const int64_t col0 = int64_t(cblk) * BS + threadIdx.x;
  if (col0 >= a.nvec) return;
  const uint8_t* const* sp = a.src + int64_t(s) * a.src_stride;
  // Fetch ALL pointers before the first store: a pointer read after a store
  // cannot use the scalar cache (not coherent with vector stores), and the
  // compiler then chains one dependent global load per output row.
  uint8_t* dp[R];
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r] = a.dst[int64_t(s) * a.dst_stride + a.row0 + r];

  if constexpr (R >= kSeqMinRows) {
    // Three or four output rows (production): the sources are consumed one
    // after the other, written out here in the kernel body.  The same
    // arithmetic through combine3 -- x[] and acc[] handed down by reference
    // -- compiles to 177 VGPRs for RS(10,4) encode, 209 for RS(12,4) and 155
    // for a dense 4 x 10 map: two or three waves per SIMD, so two or three
    // 256-thread workgroups per CU whatever the dispatcher's cap asks for.
    // This form needs 50-82 VGPRs for those shapes (K = 16 dense: 105) and no
    // scratch, with the same v_perm / v_bitop3 counts (324 / 188 for RS(10,4)
    // encode), so the residency is the dispatcher's choice (dispatch_w8.hip
    // cap_for; tests/test_kernel_resources.py holds the budget).  Scheduling
    // fences pin the load schedule, which the compiler otherwise derives from
    // its register target: G = load_window<K>() loads go out first, the load
    // of source j + G just before source j is consumed.
    constexpr int G = load_window<K>();
    const kconst_u32* ptab = (const kconst_u32*)a.ptab;  // C cast: generic -> constant (scalar loads)
    u32x4 x[K];
#pragma unroll
    for (int j = 0; j < K && j < G; ++j) x[j] = load16t<NT & 1>(sp[j], col0);
    Xacc xa[R][4];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      if (j + G < K) x[j + G] = load16t<NT & 1>(sp[j + G], col0);
      Sel3 sl[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sl[c] = sel3(x[j][c]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (is_unit<UNITS>(r, j)) {
#pragma unroll
          for (int c = 0; c < 4; ++c) xa[r][c].add(x[j][c]);
        } else {
          const kconst_u32* t = ptab + (r * K + j) * kP3Words;
#pragma unroll
          for (int c = 0; c < 4; ++c) mac3(xa[r][c], t, sl[c]);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      u32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = xa[r][c].value();
      store16t<((NT >> 1) & 1)>(dp[r], col0, o);
    }
  } else {
    // One or two output rows (46-58 VGPRs for the R = 1 decodes).
    u32x4 x[K];
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = load16t<NT & 1>(sp[j], col0);
    combine_store<K, R, UNITS, ((NT >> 1) & 1)>(a, x, dp, col0);
  }
}

// Cache policy: NT bit 0 = non-temporal loads, bit 1 = store policy
// (store16t: 0 plain, 1 nt).  The production
// instantiations (gf_spec.hip) all load `nt` and select the store policy per
// launch.
template <int K, int R, int UNITS, int NT = 3>
__global__ __launch_bounds__((apply_block<K, R, UNITS, NT>())) void gf_apply(ApplyArgs a) {
  gf_apply_body<K, R, UNITS, NT>(a);
}

// ---------------------------------------------- one-stripe inline form ----
// A synchronous one-stripe call (the drop-in jerasure_* / galois_* names)
// is latency-bound: uploading its pointer table and coefficient tables cost
// two to five small DMAs (~10 us each on MI355X, tools/hip_overheads.cpp)
// before the kernel could start.  Here the launch carries everything in its
// kernel arguments (< 4 KiB): the K source and R destination pointers and
// the rows' 3-bit-slice tables, read with scalar loads straight from the
// kernarg segment.  One launch covers the whole shard: blocks below
// nblk_vec do 16-B columns (the production combine, unit structure UNITS),
// the blocks after them one byte per lane for the tail [byte0, size) -- or
// every byte when a pointer is not 16-B aligned (nvec = 0).  The argument
// block InlineArgs is in gf_device.hpp.
template <int K, int R, int UNITS>
__device__ __forceinline__ void inl_column(const uint8_t* const (&sp)[K], uint8_t* const (&dp)[R],
                                           const kconst_u32* t, int64_t col) {
  u32x4 x[K];
#pragma unroll
  for (int j = 0; j < K; ++j) x[j] = load16t<1>(sp[j], col);
  u32x4 acc[R];
  combine3<K, R, UNITS>(t, x, acc);
#pragma unroll
  for (int r = 0; r < R; ++r) store16t<1>(dp[r], col, acc[r]);
}

// ZC = false (device buffers): one 16-B column per lane, straight-line like
// gf_apply -- in a loop the compiler hoists every table load out of it,
// which overflows the SGPR file into VGPR lanes (RS(10,4): 180 v_readlane,
// 132 VGPRs; a 64 MiB encode took 271 us against gf_apply's 157).
// ZC = true (host memory read and written in place over PCIe): grid-stride
// over a capped grid -- fewer PCIe requests in flight read faster
// (tools/zero_copy_probe.cpp); PCIe-bound, so the spills do not matter there.
template <int K, int R, int UNITS, bool ZC>
__global__ __launch_bounds__(kBlock) void gf_apply_inl(InlineArgs a) {
  const kconst_u32* ptab = (const kconst_u32*)a.ptab;  // kernarg segment: scalar loads
  if (int(blockIdx.x) < a.nblk_vec) {
    // (pointers copied out by value: a reference to the kernarg struct would
    // copy all 2.2 KiB of it to scratch)
    const uint8_t* sp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sp[j] = a.src[j];
    uint8_t* dp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) dp[r] = a.dst[r];
    int64_t col = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if constexpr (!ZC) {
      if (col < a.nvec) inl_column<K, R, UNITS>(sp, dp, ptab, col);
    } else {
      const int64_t step = int64_t(a.nblk_vec) * kBlock;
      for (; col < a.nvec; col += step) inl_column<K, R, UNITS>(sp, dp, ptab, col);
    }
    return;
  }
  const int64_t x = a.byte0 + int64_t(int(blockIdx.x) - a.nblk_vec) * kBlock + threadIdx.x;
  if (x >= a.size) return;
  Xacc xa[R];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t v = a.src[j][x];
    const Sel3 sl = sel3(v);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (is_unit<UNITS>(r, j))
        xa[r].add(v);
      else
        mac3(xa[r], ptab + (r * K + j) * kP3Words, sl);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) a.dst[r][x] = uint8_t(xa[r].value());
}

// ----------------------------------------------------------------- LDS ----
// The north star's LDS nibble-table kernel.  c*x = T_lo[x & 15] ^ T_hi[x >> 4]
// with T_lo[v] = c*v, T_hi[v] = c*(v << 4) (galois.h's multiplication
// restricted to one nibble), staged once per workgroup in LDS.  One LDS
// entry per (source j, nibble half h, nibble value v) packs the products of
// ALL R <= 4 output rows -- byte r = coef[r][j] * (v << 4h) -- so a single
// ds_read_b32 serves every row of a byte's nibble: 8 reads per source dword
// for all rows together (the round-1 form read one byte per row per nibble:
// 8 * R ds_read_u8, LDS-issue-bound at 3.7 TB/s).  Zero and unit
// coefficients are just table contents (branch-free).  The lookup address is
// the nibble times 4 extracted by one v_perm from a pre-shifted copy of the
// source dword (the table offset j*128 + 64h is the ds_read immediate); the
// lo/hi entries fold into per-byte-position accumulators with XOR3, and
// only at the end does a 4x4 byte transpose (8 v_perm per dword for R = 4)
// turn "byte position b holds all rows" into "row r holds all positions".
// A 16-entry table of 4-B entries spans 16 distinct banks: no conflicts.
__device__ __forceinline__ uint32_t lds_word(lds_u8* base, uint32_t byte_off) {
  return *(lds_u32*)(base + byte_off);  // C cast: byte address -> dword load (ds_read_b32)
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void gf_apply_lds(ApplyArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lut[K * 32];  // [j][h][v]
  // The column's K loads go out before the table staging and its barrier, so
  // their HBM latency overlaps the staging (RS(10,4) encode at 3 workgroups
  // per CU 918 -> 902 us, tools/encode_lab.hip --lds).
  const int64_t col = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = col < a.nvec;
  const int s = blockIdx.y;
  const uint8_t* const* sp = a.src + int64_t(s) * a.src_stride;
  u32x4 x[K];
#pragma unroll
  for (int j = 0; j < K; ++j) x[j] = live ? load16t<1>(sp[j], col) : u32x4{0u, 0u, 0u, 0u};
  // entry (j, h, v): byte r = coef[r][j] * (v << 4h), from the per-coefficient
  // nibble tables ntab[r][j] = {c*v (16 B), c*(v << 4) (16 B)}
  for (int i = threadIdx.x; i < K * 32; i += kBlock) {
    const int j = i >> 5, hv = i & 31;
    uint32_t e = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) e |= uint32_t(a.ntab[(r * K + j) * 32 + hv]) << (8 * r);
    lut[i] = e;
  }
  __syncthreads();
  if (!live) return;
  uint8_t* dp[R];  // all pointers before the first store (see gf_apply_body)
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r] = a.dst[int64_t(s) * a.dst_stride + a.row0 + r];

  lds_u8* lb = (lds_u8*)lut;  // C cast: generic -> LDS address space
  uint32_t e[4][4];  // [dword c][byte position b]: byte r = row r's product byte
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int b = 0; b < 4; ++b) e[c][b] = 0u;
  u32x4 ux = u32x4{0u, 0u, 0u, 0u};  // XOR of the sources whose every row coefficient is 1
#pragma unroll
  for (int j = 0; j < K; ++j) {
    // a source that is a unit (or zero) in every row of the launch needs no
    // lookup: wave-uniform branches on the host's masks (decode{0} is all
    // XOR; every Vandermonde encode has column 0 all ones)
    uint64_t colbits = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) colbits |= uint64_t(1) << (r * K + j);
    if ((a.zero_mask & colbits) == colbits) continue;
    if ((a.unit_mask & colbits) == colbits) {
      ux ^= x[j];
      continue;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t xl = (x[j][c] & 0x0F0F0F0Fu) << 2;  // lo nibble * 4 per byte
      const uint32_t xh = (x[j][c] >> 2) & 0x3C3C3C3Cu;  // hi nibble * 4 per byte
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        // byte b alone into byte 0 (selector 0x0C = zero byte): one v_perm per address
        const uint32_t sel = 0x0C0C0C00u | uint32_t(b);
        const uint32_t lo = lds_word(lb, __builtin_amdgcn_perm(xl, xl, sel) + uint32_t(j * 128));
        const uint32_t hi = lds_word(lb, __builtin_amdgcn_perm(xh, xh, sel) + uint32_t(j * 128 + 64));
        e[c][b] = xor3(e[c][b], lo, hi);
      }
    }
  }
  u32x4 acc[R];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    // 4x4 byte transpose: row r of dword c = byte r of e[c][0..3]
    const uint32_t p01l = __builtin_amdgcn_perm(e[c][1], e[c][0], 0x05010400u);  // E0.0 E1.0 E0.1 E1.1
    const uint32_t p23l = __builtin_amdgcn_perm(e[c][3], e[c][2], 0x05010400u);
    const uint32_t p01h = __builtin_amdgcn_perm(e[c][1], e[c][0], 0x07030602u);  // E0.2 E1.2 E0.3 E1.3
    const uint32_t p23h = __builtin_amdgcn_perm(e[c][3], e[c][2], 0x07030602u);
    acc[0][c] = __builtin_amdgcn_perm(p23l, p01l, 0x05040100u);
    if constexpr (R > 1) acc[1][c] = __builtin_amdgcn_perm(p23l, p01l, 0x07060302u);
    if constexpr (R > 2) acc[2][c] = __builtin_amdgcn_perm(p23h, p01h, 0x05040100u);
    if constexpr (R > 3) acc[3][c] = __builtin_amdgcn_perm(p23h, p01h, 0x07060302u);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) store16t<1>(dp[r], col, acc[r] ^ ux);
}

// ------------------------------------------- generic K (> kMaxSpecK) ----
template <int R>
__global__ __launch_bounds__(kBlock) void gf_apply_perm_generic(ApplyArgs a) {
  const int64_t col = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (col >= a.nvec) return;
  const int s = blockIdx.y;
  const uint8_t* const* sp = a.src + int64_t(s) * a.src_stride;
  uint8_t* dp[R];  // all pointers before the first store (see gf_apply_body)
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r] = a.dst[int64_t(s) * a.dst_stride + a.row0 + r];
  u32x4 acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = u32x4{0u, 0u, 0u, 0u};
  const int K = a.K;
  int j = 0;
  for (; j + 4 <= K; j += 4) {
    u32x4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = load16t<1>(sp[j + u], col);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u32x4 v = x[u];
      const u32x4 s0 = v & kLo2, s1 = (v >> 2) & kLo2, s2 = (v >> 4) & kLo2, s3 = (v >> 6) & kLo2;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u32x4 q = a.qtab[r * K + j + u];
        if (q.x == 0u) continue;
        if (q.x == kQ0Unit) {
          acc[r] ^= v;
          continue;
        }
        acc[r].x ^= gf_mul_perm(q, s0.x, s1.x, s2.x, s3.x);
        acc[r].y ^= gf_mul_perm(q, s0.y, s1.y, s2.y, s3.y);
        acc[r].z ^= gf_mul_perm(q, s0.z, s1.z, s2.z, s3.z);
        acc[r].w ^= gf_mul_perm(q, s0.w, s1.w, s2.w, s3.w);
      }
    }
  }
  for (; j < K; ++j) {
    const u32x4 v = load16t<1>(sp[j], col);
    const u32x4 s0 = v & kLo2, s1 = (v >> 2) & kLo2, s2 = (v >> 4) & kLo2, s3 = (v >> 6) & kLo2;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x4 q = a.qtab[r * K + j];
      acc[r].x ^= gf_mul_perm(q, s0.x, s1.x, s2.x, s3.x);
      acc[r].y ^= gf_mul_perm(q, s0.y, s1.y, s2.y, s3.y);
      acc[r].z ^= gf_mul_perm(q, s0.z, s1.z, s2.z, s3.z);
      acc[r].w ^= gf_mul_perm(q, s0.w, s1.w, s2.w, s3.w);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) store16t<1>(dp[r], col, acc[r]);
}

}  // namespace dev
}  // namespace ecgpu
