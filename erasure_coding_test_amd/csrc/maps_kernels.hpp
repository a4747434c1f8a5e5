// maps_kernels.hpp -- the multi-map apply (ecgpu_multiplan_* in
// include/ecgpu.h): one launch over stripes that each pick one of `nmaps`
// coefficient matrices of a common shape,
//
//   dst[s][r][x] = XOR_j coefs[map_of[s]][r][j] * src[s][j][x]      (GF(2^8))
//
// the shape of a rebuild under rotated placement, where a failed device held
// a different shard of every stripe.
//
//   gf_apply_maps<K, R, NT>   the hot path, K <= kMaxSpecK and R <= kMaxRows at
//                             compile time: the production w = 8 column body
//                             (gf_kernels_w8.hpp gf_apply_body, dense) with the
//                             3-bit-slice tables of map map_of[s]
//   gf_apply_maps_bytes<R>    one byte per lane, runtime K: the tail size % 16,
//                             unaligned shards, K > kMaxSpecK
//
// Both are templates, instantiated in maps_spec.hip (the column kernel, one
// unit per R) and maps.hip (the byte kernel).  The stripe comes from
// blockIdx.y, so the map index is uniform per workgroup: it is read through
// the constant address space and pinned to a scalar register with
// readfirstlane, and the table base it offsets stays a scalar pointer -- the
// pointer tables and the coefficient tables are scalar loads exactly as in
// gf_apply, the K shard loads the only vector loads
// (tests/test_rebuild_resources.py).  Zero and unit coefficients are just
// table contents: a map's unit structure differs from its neighbour's, so
// none is compiled in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.hpp"

namespace ecgpu {
namespace dev {

struct MapsArgs {
  const u32x4* qtab;              // [nmaps][R][K] PERM tables (16 B each; byte kernel)
  const uint32_t* ptab;           // [nmaps][R][K][kP3Words] 3-bit-slice PERM tables (column kernel)
  const uint8_t* const* src;      // [stripes][K] device pointers
  uint8_t* const* dst;            // [stripes][R] device pointers
  const int* map_of;              // [stripes] map of each stripe, 0..nmaps-1
  int64_t nvec;                   // 16-B columns per shard in the vector part
  int64_t size;                   // bytes per shard
  int64_t byte0;                  // first byte handled by the byte kernel
  int K, R;                       // runtime copies (byte kernel)
};

// The load schedule gf_kernels_w8.hpp established for the production body,
// restated here because a family includes no other family's kernel header:
// launches of kMapsSeqMinRows rows or more consume their sources one after
// the other behind a window of maps_load_window<K>() loads, the others issue
// every load first.  Inherited, not swept for this kernel.
constexpr int kMapsSeqMinRows = 3;
template <int K>
constexpr int maps_load_window() { return K <= 10 ? 6 : K; }

// The stripe's map index as a scalar: map_of is not written while a kernel
// runs (constant address space, a scalar load), and every lane of the
// workgroup reads the same entry.
__device__ __forceinline__ int map_index(const MapsArgs& a, int s) {
  return __builtin_amdgcn_readfirstlane(kload(a.map_of, s));
}

// Lane l of block b handles the 16-byte column b * kBlock + l of every shard
// of stripe blockIdx.y.  NT: bit 0 = non-temporal loads, bit 1 = store policy
// of store16t (gf_device.hpp).
template <int K, int R, int NT = 3>
__global__ __launch_bounds__(kBlock) void gf_apply_maps(MapsArgs a) {
  static_assert(K >= 1 && K <= kMaxSpecK && R >= 1 && R <= kMaxRows, "shape outside the specialised table");
  const int s = blockIdx.y;
  const int64_t col0 = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (col0 >= a.nvec) return;
  const uint8_t* const* sp = a.src + int64_t(s) * K;
  // all pointers before the first store (gf_kernels_w8.hpp gf_apply_body: a
  // pointer read after a store cannot use the scalar cache)
  uint8_t* dp[R];
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r] = a.dst[int64_t(s) * R + r];
  // C cast: generic -> constant (scalar loads); the map's offset is scalar arithmetic on the base
  const kconst_u32* ptab = (const kconst_u32*)a.ptab + int64_t(map_index(a, s)) * (R * K * kP3Words);

  // The arithmetic is written out here for every R: through combine3 -- x[]
  // and acc[] handed down by reference -- the dense 2 x 10 map compiles to 145
  // VGPRs, three waves per SIMD, below what the residency rule assumes.
  constexpr bool kSeq = R >= kMapsSeqMinRows;
  constexpr int G = kSeq ? maps_load_window<K>() : K;  // R <= 2: every load first
  u32x4 x[K];
#pragma unroll
  for (int j = 0; j < K && j < G; ++j) x[j] = load16t<NT & 1>(sp[j], col0);
  Xacc xa[R][4];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if constexpr (kSeq) __builtin_amdgcn_sched_barrier(0);
    if (j + G < K) x[j + G] = load16t<NT & 1>(sp[j + G], col0);
    Sel3 sl[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sl[c] = sel3(x[j][c]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const kconst_u32* t = ptab + (r * K + j) * kP3Words;
#pragma unroll
      for (int c = 0; c < 4; ++c) mac3(xa[r][c], t, sl[c]);
    }
  }
  if constexpr (kSeq) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    u32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = xa[r][c].value();
    store16t<((NT >> 1) & 1)>(dp[r], col0, o);
  }
}

// One lane per byte in [byte0, size); runtime K, any alignment; the 2-bit
// tables of map map_of[s] at qtab + map_of[s] * R * K.
template <int R>
__global__ __launch_bounds__(kBlock) void gf_apply_maps_bytes(MapsArgs a) {
  static_assert(R >= 1 && R <= kMaxRows, "rows per launch");
  const int64_t x = a.byte0 + int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= a.size) return;
  const int s = blockIdx.y;
  const int K = a.K;
  const uint8_t* const* sp = a.src + int64_t(s) * K;
  uint8_t* dp[R];  // all pointers before the first store
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r] = a.dst[int64_t(s) * R + r];
  const u32x4* q = a.qtab + int64_t(map_index(a, s)) * (R * K);
  uint32_t acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0u;
  for (int j = 0; j < K; ++j) {
    const uint32_t v = sp[j][x];
    const uint32_t s0 = v & 3u, s1 = (v >> 2) & 3u, s2 = (v >> 4) & 3u, s3 = v >> 6;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] ^= gf_mul_perm(q[r * K + j], s0, s1, s2, s3);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) dp[r][x] = uint8_t(acc[r]);
}

}  // namespace dev
}  // namespace ecgpu
