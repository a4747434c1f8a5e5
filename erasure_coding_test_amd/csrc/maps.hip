// maps.hip -- the multi-map plan (ecgpu_multiplan_* in include/ecgpu.h):
// `nmaps` coefficient matrices of one shape, a map index per stripe, one
// launch.  The column kernel is in maps_kernels.hpp (specialised in
// maps_spec.hip); this file instantiates the byte kernel and holds the
// object, its bind, its launch sequence and its C ABI.  With gf_device.hpp,
// maps_kernels.hpp and maps_spec.* it is the rebuild build ID
// (ecgpu_build_id(5), erasure_coding_test_amd/build.py).
//
// A multiplan owns one internal plan (runtime.hpp ecgpu_plan) for the
// asynchronous upload of its tables -- [2-bit | 3-bit-slice] tables of every
// coefficient of every map, one allocation, one copy -- and one device
// allocation of its own for [source pointers | destination pointers | map_of],
// uploaded together by the blocking bind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ecgpu.h"
#include "knobs.hpp"
#include "maps_kernels.hpp"
#include "maps_spec.hpp"
#include "runtime.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;
using dev::MapsArgs;
using dev::u32x4;

struct ecgpu_multiplan {
  int device = 0, rows = 0, nsrc = 0, nmaps = 0;
  int nt = 1;                  // store policy, from ECGPU_NT at creation
  ecgpu_plan* tabs = nullptr;  // the table upload (d_q, d_p3 carved from d_tabs)
  uint8_t* d_bind = nullptr;   // [src | dst | map_of]
  size_t cap_bind = 0;
  const uint8_t** d_src = nullptr;
  uint8_t** d_dst = nullptr;
  int* d_map = nullptr;
  int stripes = 0;
  int64_t size = 0;
  bool aligned = true;
};

ECGPU_RT_BEGIN

void multiplan_free(ecgpu_multiplan* mp) {
  if (!mp) return;
  {
    DeviceGuard g(mp->device);
    if (mp->d_bind) (void)hipFree(mp->d_bind);
  }
  plan_free(mp->tabs);
  delete mp;
}

// [2-bit tables | 3-bit-slice tables] of all maps, one asynchronous upload.
int multiplan_init(ecgpu_multiplan* mp, const int* coefs) {
  const size_t n = size_t(mp->nmaps) * mp->rows * mp->nsrc;
  const size_t qb = n * sizeof(u32x4), pb = n * dev::kP3Words * sizeof(uint32_t);
  std::vector<uint8_t> host(qb + pb);
  u32x4* q = reinterpret_cast<u32x4*>(host.data());
  uint32_t* p3 = reinterpret_cast<uint32_t*>(host.data() + qb);
  uint8_t nib[32];  // the LDS engine's tables: not used here
  for (size_t i = 0; i < n; ++i) build_tables(coefs[i], &q[i], &p3[i * dev::kP3Words], nib);
  mp->tabs = new ecgpu_plan();
  mp->tabs->device = mp->device;
  if (int rc = plan_upload_tables(mp->tabs, std::move(host))) return rc;
  mp->tabs->d_q = reinterpret_cast<u32x4*>(mp->tabs->d_tabs);
  mp->tabs->d_p3 = reinterpret_cast<uint32_t*>(mp->tabs->d_tabs + qb);
  return ECGPU_OK;
}

bool multiplan_specialised(const ecgpu_multiplan* mp) { return mp->nsrc <= dev::kMaxSpecK; }

int multiplan_bind(ecgpu_multiplan* mp, int stripes, const int* map_of, const uint8_t* const* src,
                   uint8_t* const* dst, int64_t size) {
  const size_t ns = size_t(stripes) * mp->nsrc, nd = size_t(stripes) * mp->rows;
  const size_t pbytes = (ns + nd) * sizeof(void*), bytes = pbytes + size_t(stripes) * sizeof(int);
  DeviceGuard g(mp->device);
  if (int rc = plan_sync_tables(mp->tabs)) return rc;  // blocking: settles the table upload too
  if (bytes > mp->cap_bind) {
    if (mp->d_bind) ECGPU_HIP(hipFree(mp->d_bind));
    mp->d_bind = nullptr;
    mp->cap_bind = 0;
    ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&mp->d_bind), bytes));
    mp->cap_bind = bytes;
  }
  mp->d_src = reinterpret_cast<const uint8_t**>(mp->d_bind);
  mp->d_dst = reinterpret_cast<uint8_t**>(mp->d_bind + ns * sizeof(void*));
  mp->d_map = reinterpret_cast<int*>(mp->d_bind + pbytes);
  bool aligned = true;
  for (size_t i = 0; i < ns; ++i) aligned &= (reinterpret_cast<uintptr_t>(src[i]) & 15u) == 0;
  for (size_t i = 0; i < nd; ++i) aligned &= (reinterpret_cast<uintptr_t>(dst[i]) & 15u) == 0;
  if (bytes) {
    // one upload of [sources | destinations | map_of]
    std::vector<uint8_t> host(bytes);
    std::memcpy(host.data(), src, ns * sizeof(void*));
    std::memcpy(host.data() + ns * sizeof(void*), dst, nd * sizeof(void*));
    std::memcpy(host.data() + pbytes, map_of, size_t(stripes) * sizeof(int));
    ECGPU_HIP(hipMemcpy(mp->d_bind, host.data(), bytes, hipMemcpyHostToDevice));
  }
  mp->stripes = stripes;
  mp->size = size;
  mp->aligned = aligned;
  return ECGPU_OK;
}

MapsKernelFn maps_bytes_fn(int R) {
  switch (R) {
    case 1: return &dev::gf_apply_maps_bytes<1>;
    case 2: return &dev::gf_apply_maps_bytes<2>;
    case 3: return &dev::gf_apply_maps_bytes<3>;
    case 4: return &dev::gf_apply_maps_bytes<4>;
    default: return nullptr;
  }
}

hipError_t launch_maps(MapsKernelFn fn, dim3 grid, MapsArgs& a, hipStream_t s, unsigned lds_bytes = 0) {
  void* args[] = {&a};
  return hipLaunchKernel(reinterpret_cast<const void*>(fn), grid, dim3(dev::kBlock), args, lds_bytes, s);
}

// 16-B columns, then the byte tail -- or bytes only; stripes in chunks of
// 65535 (gridDim.y) like plan_launch, map_of offset with the pointer tables.
// The residency is the w = 8 rule (dispatch_w8.hip cap_for,
// residency_lds_bytes) for a launch dense in GF multiplies: inherited, not
// swept for this kernel.
int multiplan_launch(ecgpu_multiplan* mp, hipStream_t stream) {
  if (mp->stripes <= 0 || mp->size <= 0) return ECGPU_OK;
  DeviceGuard g(mp->device);
  if (int rc = plan_wait_tables(mp->tabs, stream)) return rc;
  const int K = mp->nsrc, R = mp->rows;
  const int64_t nvec = multiplan_specialised(mp) && mp->aligned ? mp->size / 16 : 0;
  const int64_t byte0 = nvec * 16;
  MapsKernelFn vec_fn = nullptr;
  unsigned lds = 0;
  if (nvec > 0) {
    vec_fn = maps_kernel(K, R, mp->nt);
    if (!vec_fn) return fail(ECGPU_ERR, "ecgpu_multiplan_launch: no specialised kernel for this shape");
    if (cap_for(K, R, R * K, R >= dev::kMapsSeqMinRows)) lds = residency_lds_bytes(mp->device, K + R, 0, dev::kBlock);
  }
  const MapsKernelFn byte_fn = maps_bytes_fn(R);
  if (!byte_fn) return fail(ECGPU_ERR_ARG, "ecgpu_multiplan_launch: rows outside 1..4");
  for (int s0 = 0; s0 < mp->stripes; s0 += dev::kMaxGridY) {
    const int ns = std::min(dev::kMaxGridY, mp->stripes - s0);
    MapsArgs a{};
    a.qtab = mp->tabs->d_q;
    a.ptab = mp->tabs->d_p3;
    a.src = mp->d_src + size_t(s0) * K;
    a.dst = mp->d_dst + size_t(s0) * R;
    a.map_of = mp->d_map + s0;
    a.nvec = nvec;
    a.size = mp->size;
    a.byte0 = byte0;
    a.K = K;
    a.R = R;
    if (nvec > 0)
      ECGPU_HIP(launch_maps(vec_fn, dim3(unsigned((nvec + dev::kBlock - 1) / dev::kBlock), unsigned(ns)), a, stream,
                            lds));
    if (byte0 < mp->size)
      ECGPU_HIP(launch_maps(byte_fn, dim3(unsigned((mp->size - byte0 + dev::kBlock - 1) / dev::kBlock), unsigned(ns)),
                            a, stream));
  }
  return ECGPU_OK;
}

ECGPU_RT_END

// ================================================================ C ABI ====
extern "C" {

ECGPU_API ecgpu_multiplan* ecgpu_multiplan_create(int rows, int nsrc, int nmaps, const int* coefs, int device) {
  const char* why = nullptr;
  if (rows < 1) why = "rows must be >= 1";
  else if (rows > dev::kMaxRows) why = "rows must be <= 4";
  else if (nsrc < 1) why = "nsrc must be >= 1";
  else if (nmaps < 1) why = "nmaps must be >= 1";
  else if (!coefs) why = "coefs is NULL";
  if (why) {
    fail(ECGPU_ERR_ARG, std::string("ecgpu_multiplan_create: ") + why);
    return nullptr;
  }
  auto* mp = new ecgpu_multiplan();
  mp->rows = rows;
  mp->nsrc = nsrc;
  mp->nmaps = nmaps;
  mp->nt = clamp_store_policy(knob(Knob::kNt));
  mp->device = device < 0 ? current_device() : device;
  if (multiplan_init(mp, coefs) != ECGPU_OK) {
    multiplan_free(mp);
    return nullptr;
  }
  return mp;
}

ECGPU_API int ecgpu_multiplan_bind(ecgpu_multiplan* mp, int stripes, const int* map_of,
                                   const uint8_t* const* src_ptrs, uint8_t* const* dst_ptrs, int64_t size) {
  if (!mp || stripes < 0 || size < 0 || (stripes && (!map_of || !src_ptrs || !dst_ptrs)))
    return fail(ECGPU_ERR_ARG, "ecgpu_multiplan_bind: bad arguments");
  if (int rc = ecgpu_multiplan_check(mp->rows, mp->nsrc, mp->nmaps, stripes, map_of, src_ptrs, dst_ptrs, size))
    return rc;
  return multiplan_bind(mp, stripes, map_of, src_ptrs, dst_ptrs, size);
}

ECGPU_API int ecgpu_multiplan_launch(ecgpu_multiplan* mp, void* stream) {
  if (!mp) return fail(ECGPU_ERR_ARG, "ecgpu_multiplan_launch: null multiplan");
  return multiplan_launch(mp, static_cast<hipStream_t>(stream));
}

ECGPU_API int ecgpu_multiplan_engine(ecgpu_multiplan* mp) {
  if (!mp) return fail(ECGPU_ERR_ARG, "ecgpu_multiplan_engine: null multiplan");
  const bool bound = mp->stripes > 0;
  return multiplan_specialised(mp) && (!bound || (mp->aligned && mp->size >= 16)) ? 0 : 1;
}

ECGPU_API void ecgpu_multiplan_destroy(ecgpu_multiplan* mp) { multiplan_free(mp); }

}  // extern "C"
