// scrub.hip -- stripe scrub (ecgpu_scrub_* in include/ecgpu.h): a fused
// parity verify with shard blame over device-resident stripes.  The column
// kernel is in scrub_kernels.hpp (specialised in scrub_spec.hip); this file
// is the init, byte and locate kernels, the scrub object, its launch sequence
// and its C ABI.
//
// A scrub owns two internal plans (runtime.hpp ecgpu_plan): `mat` carries
// the m x k coding matrix's tables and the pointer tables (rows = m, nsrc =
// k, src = data, dst = coding -- which the kernels only read), `rat` the
// tables of the blame ratios D.  The pointer tables go up through plan_bind
// itself, below the C ABI's buffer-contract check: nothing is written to a
// shard, so shards may overlap or repeat freely.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ecgpu.h"
#include "gf_host.hpp"
#include "knobs.hpp"
#include "runtime.hpp"
#include "scrub_kernels.hpp"
#include "scrub_spec.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;
using dev::ScrubArgs;

// The non-template kernels (overview: scrub_kernels.hpp).
namespace ecgpu {
namespace dev {

// ------------------------------------------------------------- init ----
static __global__ __launch_bounds__(kBlock) void scrub_init(ScrubArgs a) {
  const int s = int(blockIdx.x) * kBlock + int(threadIdx.x);
  if (s >= a.stripes) return;
  ecgpu_scrub_result* r = a.res + s;
#pragma unroll
  for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) r->bad_bytes[i] = 0;
  r->bad_cols = 0;
  r->first_bad = ~uint64_t(0);
  const int n = a.k + a.m;
  r->blame = n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
}

// --------------------------------------------------- verify, bytes ----
// One lane per byte in [byte0, size); runtime k and m <= ECGPU_SCRUB_MAX_M.
static __global__ __launch_bounds__(kBlock) void scrub_verify_bytes(ScrubArgs a) {
  const int64_t x = a.byte0 + int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= a.size) return;
  const int s = blockIdx.y;
  const uint8_t* const* dp = a.data + int64_t(s) * a.k;
  const uint8_t* const* cp = a.coding + int64_t(s) * a.m;
  uint32_t syn[ECGPU_SCRUB_MAX_M];
#pragma unroll
  for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) syn[i] = i < a.m ? uint32_t(cp[i][x]) : 0u;
  for (int j = 0; j < a.k; ++j) {
    const uint32_t v = dp[j][x];
    const uint32_t s0 = v & 3u, s1 = (v >> 2) & 3u, s2 = (v >> 4) & 3u, s3 = v >> 6;
#pragma unroll
    for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i)
      if (i < a.m) syn[i] ^= gf_mul_perm(a.qtab[i * a.k + j], s0, s1, s2, s3) & 0xFFu;
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) any |= syn[i];
  const uint64_t bad_lanes = wave_ballot(any != 0u);
  if (bad_lanes == 0) return;
  uint32_t rows[ECGPU_SCRUB_MAX_M];
#pragma unroll
  for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) rows[i] = uint32_t(__popcll(wave_ballot(syn[i] != 0u)));
  const int first_lane = __ffsll((long long)bad_lanes) - 1;
  if ((int(threadIdx.x) & 63) == first_lane)
    scrub_publish<ECGPU_SCRUB_MAX_M>(a.res + s, rows, uint32_t(__popcll(bad_lanes)), uint64_t(x));
}

// ----------------------------------------------------------- locate ----
// blame[s] &= candidates(x) for every bad position x of a bad stripe.  A
// coding shard p is a candidate at x iff syn[i] == 0 for all i != p; a data
// shard j iff syn[i] == D[i][j] * syn[pivot[j]] for all i, D[i][j] =
// matrix[i][j] / matrix[pivot[j]][j] (host: ecgpu_scrub_blame_matrix) -- i.e.
// the syndrome is a multiple of column j, tested without a division.  A
// grid-stride loop with a block-uniform trip count keeps every lane in the
// closing wave reduction; one atomicAnd per wave that narrowed the mask.
constexpr int kLocateBlocks = 256;

static __global__ __launch_bounds__(kBlock) void scrub_locate(ScrubArgs a) {
  const int s = blockIdx.y;
  ecgpu_scrub_result* res = a.res + s;
  if (res->bad_cols == 0) return;  // written by the verify kernels earlier on the stream
  const uint8_t* const* dp = a.data + int64_t(s) * a.k;
  const uint8_t* const* cp = a.coding + int64_t(s) * a.m;
  const int n = a.k + a.m;
  const uint64_t all = n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
  uint64_t cand = all;
  const int64_t step = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock; base < a.size; base += step) {
    const int64_t x = base + threadIdx.x;
    if (x >= a.size) continue;
    uint32_t syn[ECGPU_SCRUB_MAX_M];
#pragma unroll
    for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) syn[i] = i < a.m ? uint32_t(cp[i][x]) : 0u;
    for (int j = 0; j < a.k; ++j) {
      const uint32_t v = dp[j][x];
      const uint32_t s0 = v & 3u, s1 = (v >> 2) & 3u, s2 = (v >> 4) & 3u, s3 = v >> 6;
#pragma unroll
      for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i)
        if (i < a.m) syn[i] ^= gf_mul_perm(a.qtab[i * a.k + j], s0, s1, s2, s3) & 0xFFu;
    }
    uint32_t nzrows = 0;  // bit i: syn[i] != 0
#pragma unroll
    for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) nzrows |= (syn[i] != 0u ? 1u : 0u) << i;
    if (nzrows == 0) continue;  // a good position constrains nothing
    uint64_t mask = 0;
    if ((nzrows & (nzrows - 1u)) == 0u) mask |= uint64_t(nzrows) << a.k;  // one row only: its coding shard
    for (int j = 0; j < a.k; ++j) {
      const int pj = a.pivot[j];
      if (pj < 0) continue;
      uint32_t sp = 0;
#pragma unroll
      for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i) sp = i == pj ? syn[i] : sp;
      const uint32_t s0 = sp & 3u, s1 = (sp >> 2) & 3u, s2 = (sp >> 4) & 3u, s3 = sp >> 6;
      bool ok = true;
#pragma unroll
      for (int i = 0; i < ECGPU_SCRUB_MAX_M; ++i)
        if (i < a.m) ok &= syn[i] == (gf_mul_perm(a.dtab[i * a.k + j], s0, s1, s2, s3) & 0xFFu);
      if (ok) mask |= uint64_t(1) << j;
    }
    cand &= mask;
  }
  // every lane of the block is back here (the loop's `continue`s reconverge)
  uint32_t lo = uint32_t(cand), hi = uint32_t(cand >> 32);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo &= uint32_t(__shfl_xor(int(lo), o));
    hi &= uint32_t(__shfl_xor(int(hi), o));
  }
  cand = (uint64_t(hi) << 32) | lo;
  if ((threadIdx.x & 63u) == 0u && cand != all) atomicAnd(reinterpret_cast<u64a*>(&res->blame), u64a(cand));
}

}  // namespace dev
}  // namespace ecgpu

struct ecgpu_scrub {
  int device = 0, k = 0, m = 0;
  ecgpu_plan* mat = nullptr;
  ecgpu_plan* rat = nullptr;
  int* d_pivot = nullptr;
  ecgpu_scrub_result* d_res = nullptr;
  size_t cap_res = 0;
};

ECGPU_RT_BEGIN

// Pivot row and ratios of every column (ecgpu.h, ecgpu_scrub_blame_matrix).
void blame_matrix(int k, int m, const int* matrix, int* pivots, int* ratios) {
  const Gf8Tables& T = gf8();
  for (int j = 0; j < k; ++j) {
    int p = -1;
    for (int i = 0; i < m && p < 0; ++i)
      if ((matrix[i * k + j] & 0xFF) != 0) p = i;
    pivots[j] = p;
    const uint8_t inv = p < 0 ? 0 : T.inv[matrix[p * k + j] & 0xFF];
    for (int i = 0; i < m; ++i) ratios[i * k + j] = p < 0 ? 0 : T.mul[matrix[i * k + j] & 0xFF][inv];
  }
}

bool scrub_specialised(const ecgpu_scrub* s) { return s->k <= dev::kMaxSpecK && s->m <= dev::kMaxRows; }

void scrub_free(ecgpu_scrub* s) {
  if (!s) return;
  {
    DeviceGuard g(s->device);
    if (s->d_pivot) (void)hipFree(s->d_pivot);
    if (s->d_res) (void)hipFree(s->d_res);
  }
  plan_free(s->mat);
  plan_free(s->rat);
  delete s;
}

int scrub_init_object(ecgpu_scrub* s, const int* matrix) {
  const int k = s->k, m = s->m;
  std::vector<int> pivots(k), ratios(size_t(m) * k);
  blame_matrix(k, m, matrix, pivots.data(), ratios.data());
  s->mat = new ecgpu_plan();
  if (int rc = plan_init(s->mat, m, k, matrix, s->device)) return rc;
  s->rat = new ecgpu_plan();
  if (int rc = plan_init(s->rat, m, k, ratios.data(), s->device)) return rc;
  DeviceGuard g(s->device);
  ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_pivot), size_t(k) * sizeof(int)));
  ECGPU_HIP(hipMemcpy(s->d_pivot, pivots.data(), size_t(k) * sizeof(int), hipMemcpyHostToDevice));
  return ECGPU_OK;
}

hipError_t launch_scrub(ScrubKernelFn fn, dim3 grid, ScrubArgs& a, hipStream_t s, unsigned lds_bytes = 0) {
  void* args[] = {&a};
  return hipLaunchKernel(reinterpret_cast<const void*>(fn), grid, dim3(dev::kBlock), args, lds_bytes, s);
}

// init, verify (16-B columns, then the byte tail -- or bytes only), locate;
// stripes in chunks of 65535 (gridDim.y), like plan_launch.
int scrub_launch(ecgpu_scrub* sc, hipStream_t stream) {
  ecgpu_plan* p = sc->mat;
  if (p->stripes <= 0) return ECGPU_OK;
  DeviceGuard g(sc->device);
  if (int rc = plan_wait_tables(p, stream)) return rc;
  if (int rc = plan_wait_tables(sc->rat, stream)) return rc;
  const int K = sc->k, R = sc->m;
  const bool spec = scrub_specialised(sc);
  const int64_t nvec = spec && p->aligned ? p->size / 16 : 0;
  ScrubArgs a{};
  a.ptab = p->d_p3;
  a.qtab = p->d_q;
  a.dtab = sc->rat->d_q;
  a.pivot = sc->d_pivot;
  a.nvec = nvec;
  a.size = p->size;
  a.byte0 = nvec * 16;
  a.k = K;
  a.m = R;
  ScrubKernelFn vec_fn = nullptr;
  unsigned lds = 0;
  if (nvec > 0) {
    vec_fn = scrub_kernel(K, R, unit_variant(p->coef, K, 0, R), knob(Knob::kScrubLate) != 0);
    if (!vec_fn) return fail(ECGPU_ERR, "ecgpu_scrub_launch: no specialised kernel for this shape");
    int mul_terms = 0;  // coefficients that are neither 0 nor 1 (dispatch_w8.hip cap_for)
    for (uint32_t c : p->coef) mul_terms += c > 1u;
    if (cap_for(K, R, mul_terms)) lds = residency_lds_bytes(sc->device, K + R);
  }
  for (int s0 = 0; s0 < p->stripes; s0 += dev::kMaxGridY) {
    const int ns = std::min(dev::kMaxGridY, p->stripes - s0);
    a.data = p->d_src + size_t(s0) * K;
    a.coding = p->d_dst + size_t(s0) * R;
    a.res = sc->d_res + s0;
    a.stripes = ns;
    ECGPU_HIP(launch_scrub(&dev::scrub_init, dim3(unsigned((ns + dev::kBlock - 1) / dev::kBlock)), a, stream));
    if (p->size <= 0) continue;
    if (nvec > 0)
      ECGPU_HIP(launch_scrub(vec_fn, dim3(unsigned((nvec + dev::kBlock - 1) / dev::kBlock), unsigned(ns)), a, stream,
                             lds));
    if (a.byte0 < p->size)
      ECGPU_HIP(launch_scrub(&dev::scrub_verify_bytes,
                             dim3(unsigned((p->size - a.byte0 + dev::kBlock - 1) / dev::kBlock), unsigned(ns)), a,
                             stream));
    const int64_t blocks = (p->size + dev::kBlock - 1) / dev::kBlock;
    ECGPU_HIP(launch_scrub(&dev::scrub_locate,
                           dim3(unsigned(std::min<int64_t>(blocks, dev::kLocateBlocks)), unsigned(ns)), a, stream));
  }
  return ECGPU_OK;
}

ECGPU_RT_END

// ================================================================ C ABI ====
extern "C" {

ECGPU_API int ecgpu_scrub_blame_matrix(int k, int m, const int* matrix, int* pivots, int* ratios) {
  if (k < 1 || m < 1 || !matrix || !pivots || !ratios)
    return fail(ECGPU_ERR_ARG, "ecgpu_scrub_blame_matrix: k, m >= 1 and matrix, pivots, ratios required");
  blame_matrix(k, m, matrix, pivots, ratios);
  return ECGPU_OK;
}

ECGPU_API ecgpu_scrub* ecgpu_scrub_create(int k, int m, int w, const int* matrix, int device) {
  const char* why = nullptr;
  if (w != 8) why = "w must be 8";
  else if (k < 1) why = "k must be >= 1";
  else if (m < 1) why = "m must be >= 1";
  else if (m > ECGPU_SCRUB_MAX_M) why = "m must be <= ECGPU_SCRUB_MAX_M (8)";
  else if (k + m > 64) why = "k + m must be <= 64 (the blame mask has one bit per shard)";
  else if (!matrix) why = "matrix is NULL";
  if (why) {
    fail(ECGPU_ERR_ARG, std::string("ecgpu_scrub_create: ") + why);
    return nullptr;
  }
  auto* s = new ecgpu_scrub();
  s->k = k;
  s->m = m;
  s->device = device < 0 ? current_device() : device;
  if (scrub_init_object(s, matrix) != ECGPU_OK) {
    scrub_free(s);
    return nullptr;
  }
  return s;
}

ECGPU_API int ecgpu_scrub_bind(ecgpu_scrub* s, int stripes, const uint8_t* const* data, const uint8_t* const* coding,
                               int64_t size) {
  if (!s || stripes < 0 || size < 0 || (stripes && (!data || !coding)))
    return fail(ECGPU_ERR_ARG, "ecgpu_scrub_bind: bad arguments");
  DeviceGuard g(s->device);
  if (int rc = plan_sync_tables(s->rat)) return rc;
  if (size_t(stripes) > s->cap_res) {
    if (s->d_res) ECGPU_HIP(hipFree(s->d_res));
    s->d_res = nullptr;
    s->cap_res = 0;
    ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_res), size_t(stripes) * sizeof(ecgpu_scrub_result)));
    s->cap_res = size_t(stripes);
  }
  // scrub reads the coding shards only; plan_bind's table type is the apply's
  return plan_bind(s->mat, stripes, data, const_cast<uint8_t* const*>(coding), size, nullptr);
}

ECGPU_API int ecgpu_scrub_launch(ecgpu_scrub* s, void* stream) {
  if (!s) return fail(ECGPU_ERR_ARG, "ecgpu_scrub_launch: null scrub");
  return scrub_launch(s, static_cast<hipStream_t>(stream));
}

ECGPU_API int ecgpu_scrub_read(ecgpu_scrub* s, void* stream, ecgpu_scrub_result* out, int cap) {
  if (!s || cap < 0 || (cap && !out)) return fail(ECGPU_ERR_ARG, "ecgpu_scrub_read: bad arguments");
  const int n = std::min(cap, s->mat->stripes);
  DeviceGuard g(s->device);
  ECGPU_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  if (n <= 0) return 0;
  ECGPU_HIP(hipMemcpy(out, s->d_res, size_t(n) * sizeof(ecgpu_scrub_result), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    if (out[i].bad_cols == 0) out[i].blame = 0;
  return n;
}

ECGPU_API const ecgpu_scrub_result* ecgpu_scrub_device_results(ecgpu_scrub* s) { return s ? s->d_res : nullptr; }

ECGPU_API int ecgpu_scrub_engine(ecgpu_scrub* s) {
  if (!s) return fail(ECGPU_ERR_ARG, "ecgpu_scrub_engine: null scrub");
  const bool bound = s->mat->stripes > 0;
  return scrub_specialised(s) && (!bound || (s->mat->aligned && s->mat->size >= 16)) ? 0 : 1;
}

ECGPU_API void ecgpu_scrub_destroy(ecgpu_scrub* s) { scrub_free(s); }

}  // extern "C"
