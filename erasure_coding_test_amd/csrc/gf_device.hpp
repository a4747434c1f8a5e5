// gf_device.hpp -- the device vocabulary every kernel family uses: argument
// blocks, constants, cache-policy loads / stores, constant-address table
// reads, the v_perm / XOR3 multiply helpers of the 3-bit-slice tables.  No
// __global__ here: a unit that only needs the argument types and the
// kernel-pointer types (runtime.hpp, the *_spec.hpp tables) includes this and
// emits no device code.  The kernels are in gf_kernels_w8.hpp, _wide.hpp,
// _packets.hpp and scrub_kernels.hpp (overview: gf_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ecgpu {
namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;              // 4 waves
constexpr int kMaxRows = 4;              // rows per launch
constexpr int kMaxSpecK = 16;            // K specialised at compile time
constexpr int kMaxGridY = 65535;         // stripes per launch (gridDim.y)
constexpr uint32_t kQ0Unit = 0x03020100u;  // PERM table word 0 of coefficient 1
constexpr uint32_t kLo2 = 0x03030303u;

struct ApplyArgs {
  const u32x4* qtab;              // [R][K] PERM tables (16 B each)
  const uint32_t* ptab;           // [R][K][kP3Words] 3-bit-slice PERM tables (production kernel)
  const uint8_t* ntab;            // [R][K][32] nibble tables (LDS engine)
  const uint8_t* const* src;      // [stripes][src_stride] device pointers
  uint8_t* const* dst;            // [stripes][dst_stride] device pointers
  int64_t nvec;                   // 16-B columns per shard in the vector part
  int64_t size;                   // bytes per shard
  int64_t byte0;                  // first byte handled by the byte kernel
  uint64_t unit_mask;             // bit r*K+j: coefficient == 1 (this launch's rows)
  uint64_t zero_mask;             // bit r*K+j: coefficient == 0
  int src_stride, dst_stride, row0;  // row0 = first dst column of this launch
  int K, R;                       // runtime copies (generic / byte kernels)
  int nt;                         // 1: non-temporal loads/stores (read by lab launches only)
  int stripe_fast;                // 1: blockIdx.x = stripe, blockIdx.y = column block (set by lab launches only)
  const uint32_t* wtab;           // [R][K][2 * Wide<W>::kPerms] wide-word tables (w = 16 / 32)
  const uint8_t* wcls;            // [R][K] wide coefficient class: 0 general, 1 unit, 2 zero
};

__device__ __forceinline__ uint32_t perm_lookup(uint32_t table, uint32_t sel) {
  // v_perm_b32: selector bytes 0..3 pick bytes of the second operand.
  return __builtin_amdgcn_perm(table, table, sel);
}

__device__ __forceinline__ uint32_t gf_mul_perm(const u32x4& q, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  return perm_lookup(q.x, s0) ^ perm_lookup(q.y, s1) ^ perm_lookup(q.z, s2) ^ perm_lookup(q.w, s3);
}

// Shards live in global memory: address space 1 makes these global_load /
// global_store (not flat_*, which also arbitrates the LDS aperture).
typedef __attribute__((address_space(1))) u32x4 gu32x4;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) u32x2 gu32x2;

// Compile-time cache policy.  A runtime `nt ? nontemporal : plain` pair is
// merged by the compiler into ONE plain access (the two loads differ only in
// metadata), so the production kernels take the policy as a template
// argument: NT = 1 emits the `nt` bit on the global_load / global_store.
template <int NT>
__device__ __forceinline__ u32x4 load16t(const uint8_t* p, int64_t col) {
  const gu32x4* a = (const gu32x4*)p + col;  // C cast: generic -> global address space
  if constexpr (NT != 0) return __builtin_nontemporal_load(a);
  else return *a;
}

// A kernel-invariant table entry (pointer tables, row masks) read through the
// constant address space: always a scalar load.  A generic load issued after
// the kernel's own vector stores must be a VECTOR load (the scalar cache is
// not coherent with vector stores), and waiting for it (vmcnt(0)) waits for
// every shard load issued before it -- in a column loop that serialised the
// K source loads of each iteration.  Valid because no table is written while
// a kernel runs.
template <class T>
__device__ __forceinline__ T kload(const T* p, int64_t i) {
  typedef __attribute__((address_space(4))) const T kT;
  return ((const kT*)p)[i];  // C cast: generic -> constant
}

// Store cache policy POL: 0 plain, 1 non-temporal (`nt`).  (Stores that
// bypass the XCD's L2 -- `sc1`, `sc0 sc1`, inline asm -- were probed in round
// 1 and were equal or slower in the bench's back-to-back launches, DESIGN.md
// §5; they live only in the diagnostic library.)
template <int POL>
__device__ __forceinline__ void store16t(uint8_t* p, int64_t col, const u32x4& v) {
  gu32x4* a = (gu32x4*)p + col;
  if constexpr (POL == 1) {
    __builtin_nontemporal_store(v, a);
  } else {
    *a = v;
  }
}

typedef __attribute__((address_space(3))) const u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) const uint8_t lds_u8;
typedef __attribute__((address_space(3))) const uint32_t lds_u32;

// Unit-coefficient structure known at compile time (host checks it exactly):
//   kUnitCol0 -- coefficient (r, 0) == 1 for every row of the launch
//   kUnitRow0 -- coefficient (0, j) == 1 for every source (launch row 0)
//   kUnitAll  -- every coefficient == 1 (pure XOR, e.g. decode of one data
//                shard with the all-ones parity row)
// reed_sol_vandermonde_coding_matrix always has row 0 and column 0 all ones
// (reed_sol.cpp:324-349), so RS encode launches take kUnitCol0|kUnitRow0.
// A unit term costs one XOR and no selectors; every other term is 4 v_perm
// + 2 v_bitop3 (XOR3) per dword.
enum UnitMask : int { kUnitNone = 0, kUnitCol0 = 1, kUnitRow0 = 2, kUnitAll = 4 };

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

template <int UNITS>
__device__ __forceinline__ constexpr bool is_unit(int r, int j) {
  return (UNITS & kUnitAll) || ((UNITS & kUnitCol0) && j == 0) || ((UNITS & kUnitRow0) && r == 0);
}

// 3-bit slices (production): v_perm picks from EIGHT bytes -- the pair
// {hi, lo} -- so a byte splits into slices [0:2], [3:5], [6:7] and
//   c*x = T0[x & 7] ^ T1[(x >> 3) & 7] ^ T2[x >> 6],  Tp[e] = c*(e << 3p),
// T0 and T1 each a dword pair, T2 one dword: 3 v_perm per coefficient-dword
// instead of 4, and 5 selector ops per source dword instead of 7.  Table
// layout per coefficient (kP3Words dwords): T0lo T0hi T1lo T1hi T2 (pad).
constexpr int kP3Words = 8;
constexpr uint32_t kLo3 = 0x07070707u;

struct Sel3 {
  uint32_t s0, s1, s2;
};

__device__ __forceinline__ Sel3 sel3(uint32_t x) { return Sel3{x & kLo3, (x >> 3) & kLo3, (x >> 6) & kLo2}; }

// XOR accumulator that folds terms three at a time: v_bitop3 (XOR3) takes
// the running value plus TWO new terms, so one odd term is parked until its
// partner arrives.  N terms cost ceil(N/2) instead of N XORs (the compiler
// does not reassociate the chain itself).  `has` is a compile-time constant
// after full unrolling.
struct Xacc {
  uint32_t acc = 0u, pend = 0u;
  bool has = false;
  __device__ __forceinline__ void add(uint32_t v) {
    if (has) {
      acc = xor3(acc, pend, v);
      has = false;
    } else {
      pend = v;
      has = true;
    }
  }
  __device__ __forceinline__ uint32_t value() const { return has ? (acc ^ pend) : acc; }
};

typedef __attribute__((address_space(4))) const uint32_t kconst_u32;

__device__ __forceinline__ void mac3(Xacc& x, const kconst_u32* __restrict__ t, const Sel3& s) {
  x.add(__builtin_amdgcn_perm(t[1], t[0], s.s0));
  x.add(__builtin_amdgcn_perm(t[3], t[2], s.s1));
  x.add(__builtin_amdgcn_perm(t[4], t[4], s.s2));
}

// R output columns from the K source columns of one lane with the
// 3-bit-slice tables at `ptab` ([R][K][kP3Words], constant address space: a
// device table or the launch's own kernel arguments, see gf_apply_inl).
template <int K, int R, int UNITS>
__device__ __forceinline__ void combine3(const kconst_u32* __restrict__ ptab, const u32x4 (&x)[K], u32x4 (&acc)[R]) {
  Xacc xa[R][4];
#pragma unroll
  for (int j = 0; j < K; ++j) {
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
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = xa[r][c].value();
}

// The argument block of the one-stripe inline form (gf_kernels_w8.hpp
// gf_apply_inl): the launch carries its pointers and its rows' 3-bit-slice
// tables in the kernel arguments (< 4 KiB).
struct InlineArgs {
  const uint8_t* src[kMaxSpecK];
  uint8_t* dst[kMaxRows];
  int64_t nvec, size, byte0;
  int nblk_vec;
  int pad_;
  uint32_t ptab[kMaxRows * kMaxSpecK * kP3Words];  // [R][K][kP3Words], this launch's rows
};
static_assert(sizeof(InlineArgs) <= 4096, "kernel arguments are limited to 4 KiB");

}  // namespace dev
}  // namespace ecgpu
