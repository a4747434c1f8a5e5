// scrub_kernels.hpp -- the stripe-scrub kernels (ecgpu_scrub_* in
// include/ecgpu.h): is each stripe still a codeword of the m x k coding
// matrix, and if not, which single shard explains the damage?
//
//   syn[i][x] = coding[i][x] ^ XOR_j matrix[i][j] * data[j][x]      (GF(2^8))
//
//   scrub_init          resets the per-stripe results (a kernel, so a captured
//                       launch replays correctly)
//   scrub_verify        the hot path, K <= 16 and R <= 4 at compile time: the
//                       fused apply's column (gf_kernels_w8.hpp combine3) with
//                       the stored parity XORed in; reads k + m shards once,
//                       writes nothing for a clean wave
//   scrub_verify_bytes  one byte per lane, any k, m <= ECGPU_SCRUB_MAX_M: the
//                       tail, unaligned shards, shapes outside the table
//   scrub_locate        off the hot path: the blame mask of the bad stripes
//
// scrub_verify, the one template, is defined here (instantiated in
// scrub_spec.hip); the other three are compiled once, in scrub.hip, which
// launches them.
//
// Counters are reduced per wave (ballots: scalar work, no LDS traffic) and
// leave the wave as ONE vector atomic per counter, so a fully corrupt shard
// costs R + 2 atomics per KiB column block, not one per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecgpu.h"
#include "gf_device.hpp"

namespace ecgpu {
namespace dev {

struct ScrubArgs {
  const uint32_t* ptab;           // [m][k][kP3Words] 3-bit-slice tables of the matrix (scrub_verify)
  const u32x4* qtab;              // [m][k] 2-bit PERM tables of the matrix (byte kernels)
  const u32x4* dtab;              // [m][k] 2-bit PERM tables of the blame ratios D (scrub_locate)
  const int* pivot;               // [k] pivot row of each column, -1: all-zero column
  const uint8_t* const* data;     // [stripes][k] device pointers
  const uint8_t* const* coding;   // [stripes][m] device pointers (read only)
  ecgpu_scrub_result* res;        // [stripes]
  int64_t nvec;                   // 16-B columns per shard in the vector part
  int64_t size;                   // bytes per shard
  int64_t byte0;                  // first byte handled by scrub_verify_bytes
  int k, m;
  int stripes;                    // scrub_init
};

typedef unsigned long long u64a;  // the type HIP's 64-bit atomics take

__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Sum over the active lanes of v < 32: one ballot per bit.
__device__ __forceinline__ uint32_t wave_sum5(uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < 5; ++b) s += uint32_t(__popcll(wave_ballot(((v >> b) & 1u) != 0u))) << b;
  return s;
}

// 0x80 in every byte of v that is non-zero.
__device__ __forceinline__ uint32_t nz_bytes(uint32_t v) {
  return (v | ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;
}

// The wave's leader publishes its reduced counters: row counts, bad
// positions, lowest bad position.  Zero counts are skipped.
template <int R>
__device__ __forceinline__ void scrub_publish(ecgpu_scrub_result* res, const uint32_t (&rows)[R], uint32_t cols,
                                              uint64_t first) {
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (rows[r]) atomicAdd(reinterpret_cast<u64a*>(&res->bad_bytes[r]), u64a(rows[r]));
  atomicAdd(reinterpret_cast<u64a*>(&res->bad_cols), u64a(cols));
  atomicMin(reinterpret_cast<u64a*>(&res->first_bad), u64a(first));
}

// ----------------------------------------------------- verify, 16-B ----
// The grid of gf_apply with one column per lane: blockIdx.x = column block,
// blockIdx.y = stripe.  LATE = 0 issues all K + R non-temporal loads before
// any arithmetic; LATE = 1 (the default, ECGPU_SCRUB_LATE) loads the R parity
// columns after the combine: K + R shard streams per lane are never open at
// once, and on RS(10,4) with 4 MiB shards the launch is 3-5 % faster although
// the parity loads' latency is exposed (tools/scrub_bench.py).
template <int K, int R, int UNITS, int LATE = 1>
__global__ __launch_bounds__(kBlock) void scrub_verify(ScrubArgs a) {
  const int64_t col = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (col >= a.nvec) return;
  const int s = blockIdx.y;
  const uint8_t* const* dp = a.data + int64_t(s) * K;
  const uint8_t* const* cp = a.coding + int64_t(s) * R;
  u32x4 x[K], c[R];
#pragma unroll
  for (int j = 0; j < K; ++j) x[j] = load16t<1>(kload(dp, j), col);
  if constexpr (LATE == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = load16t<1>(kload(cp, r), col);
  }
  u32x4 d[R];
  combine3<K, R, UNITS>((const kconst_u32*)a.ptab, x, d);  // C cast: generic -> constant
  if constexpr (LATE != 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = load16t<1>(kload(cp, r), col);
  }
  u32x4 o = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < R; ++r) {
    d[r] ^= c[r];
    o |= d[r];
  }
  const bool bad = (o.x | o.y | o.z | o.w) != 0u;
  const uint64_t bad_lanes = wave_ballot(bad);
  if (bad_lanes == 0) return;  // a clean wave: no store, no atomic

  // per lane: non-zero bytes of each row's difference and of their OR (each
  // <= 16), and the lowest bad byte of the column
  uint32_t rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) n += uint32_t(__popc(nz_bytes(d[r][w])));
    rows[r] = wave_sum5(n);
  }
  uint32_t n = 0, byte = 16;
#pragma unroll
  for (int w = 3; w >= 0; --w) {
    const uint32_t z = nz_bytes(o[w]);
    n += uint32_t(__popc(z));
    if (z) byte = uint32_t(w) * 4u + (uint32_t(__ffs(z)) - 1u) / 8u;
  }
  const uint32_t cols = wave_sum5(n);
  // lanes of a wave hold consecutive columns: the first bad lane has the
  // wave's lowest bad position, and publishes for the wave
  const int first_lane = __ffsll((long long)bad_lanes) - 1;
  if ((int(threadIdx.x) & 63) == first_lane) scrub_publish<R>(a.res + s, rows, cols, uint64_t(col) * 16u + byte);
}

}  // namespace dev
}  // namespace ecgpu
