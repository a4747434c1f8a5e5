// plans.hip -- the lifecycle of a bound coefficient matrix (ecgpu_plan in
// runtime.hpp): the asynchronous upload of its coefficient tables, the bind
// of its pointer tables, its release, and the ecgpu_plan_* / ecgpu_encode_batch
// C ABI.  What the tables hold and how a plan launches is dispatch_w8.hip
// (w = 8) and dispatch_wide.hip (w = 16 / 32).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "ecgpu.h"
#include "host_sync.hpp"
#include "knobs.hpp"
#include "runtime.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;

ECGPU_RT_BEGIN

// One non-blocking stream per device for coefficient-table uploads: a plan's
// creation does not wait for its tables (one blocking copy cost ~12 us,
// tools/hip_overheads.cpp); its launches wait on the upload's event instead.
hipStream_t upload_stream(int device) {
  static hostsync::PerDevice<hipStream_t> streams;
  return streams.get(device, [](int dev) {
    DeviceGuard g(dev);
    hipStream_t s = nullptr;
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? s : nullptr;
  });
}

// Allocates p->d_tabs and uploads `host` into it without waiting (the plan
// keeps `host` alive until the upload has completed).
int plan_upload_tables(ecgpu_plan* p, std::vector<uint8_t>&& host) {
  DeviceGuard g(p->device);
  ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_tabs), host.size()));
  p->host_tabs = std::move(host);
  const hipStream_t s = upload_stream(p->device);
  if (!s) {  // no stream: a blocking copy
    ECGPU_HIP(hipMemcpy(p->d_tabs, p->host_tabs.data(), p->host_tabs.size(), hipMemcpyHostToDevice));
    return ECGPU_OK;
  }
  ECGPU_HIP(hipEventCreateWithFlags(&p->uploaded, hipEventDisableTiming));
  ECGPU_HIP(hipMemcpyAsync(p->d_tabs, p->host_tabs.data(), p->host_tabs.size(), hipMemcpyHostToDevice, s));
  ECGPU_HIP(hipEventRecord(p->uploaded, s));
  p->upload_pending = true;
  return ECGPU_OK;
}

// Waits for the plan's table upload on the host (a no-op once it completed).
int plan_sync_tables(ecgpu_plan* p) {
  if (!p->upload_pending) return ECGPU_OK;
  ECGPU_HIP(hipEventSynchronize(p->uploaded));
  p->upload_pending = false;
  std::vector<uint8_t>().swap(p->host_tabs);
  return ECGPU_OK;
}

// Orders `stream` after the plan's table upload (a no-op once it completed).
// A blocking bind has already waited for it, so a bound plan launches inside
// a stream capture without touching the event; a plan bound on a stream
// (the synchronous calls) may not be captured before its upload completed.
int plan_wait_tables(ecgpu_plan* p, hipStream_t stream) {
  if (!p->upload_pending) return ECGPU_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(ECGPU_ERR, "plan tables still uploading: bind the plan without a stream before capturing it");
  (void)hipGetLastError();
  const hipError_t q = hipEventQuery(p->uploaded);
  if (q == hipSuccess) {
    p->upload_pending = false;
    std::vector<uint8_t>().swap(p->host_tabs);
    return ECGPU_OK;
  }
  if (q != hipErrorNotReady) return fail_hip(q, "table upload");
  (void)hipGetLastError();  // not ready is not an error
  ECGPU_HIP(hipStreamWaitEvent(stream, p->uploaded, 0));
  return ECGPU_OK;
}

void plan_free(ecgpu_plan* p) {
  if (!p) return;
  DeviceGuard g(p->device);
  if (p->uploaded) {
    (void)hipEventSynchronize(p->uploaded);  // the table upload may still read host_tabs
    (void)hipEventDestroy(p->uploaded);
  }
  if (p->d_tabs) (void)hipFree(p->d_tabs);
  if (p->d_ptrs) (void)hipFree(p->d_ptrs);
  delete p;
}

int plan_init(ecgpu_plan* p, int rows, int nsrc, const int* coefs, int device, int w) {
  p->device = device;
  p->rows = rows;
  p->nsrc = nsrc;
  p->w = w;
  p->kind = knob(Knob::kKernel);
  p->nt = clamp_store_policy(knob(Knob::kNt));
  const size_t n = size_t(rows) * nsrc;
  p->coef.resize(n);
  if (w != 8) return plan_init_wide(p, coefs);
  return plan_init_w8(p, coefs);
}

// With a stream the pointer tables are uploaded asynchronously on it; unless
// `keep_alive` (the caller keeps src/dst alive until it synchronises the
// stream, as execute() does) the call waits for the upload.
int plan_bind(ecgpu_plan* p, int stripes, const uint8_t* const* src, uint8_t* const* dst, int64_t size,
              hipStream_t stream, bool keep_alive) {
  const size_t ns = size_t(stripes) * p->nsrc, nd = size_t(stripes) * p->rows;
  DeviceGuard g(p->device);
  // a blocking bind settles the table upload too (it overlapped the table
  // build-up to here); a bind on a stream leaves it to the launch
  if (!stream)
    if (int rc = plan_sync_tables(p)) return rc;
  if (ns + nd > p->cap_ptrs) {
    if (p->d_ptrs) ECGPU_HIP(hipFree(p->d_ptrs));
    p->d_ptrs = nullptr;
    p->cap_ptrs = 0;
    ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_ptrs), (ns + nd) * sizeof(void*)));
    p->cap_ptrs = ns + nd;
  }
  p->d_src = static_cast<const uint8_t**>(static_cast<void*>(p->d_ptrs));
  p->d_dst = static_cast<uint8_t**>(static_cast<void*>(p->d_ptrs + ns));
  bool aligned = true;
  for (size_t i = 0; i < ns; ++i) aligned &= (reinterpret_cast<uintptr_t>(src[i]) & 15u) == 0;
  for (size_t i = 0; i < nd; ++i) aligned &= (reinterpret_cast<uintptr_t>(dst[i]) & 15u) == 0;
  if (stream && keep_alive) {
    // the caller's arrays outlive the stream sync: no wait here
    ECGPU_HIP(hipMemcpyAsync(p->d_src, src, ns * sizeof(void*), hipMemcpyHostToDevice, stream));
    ECGPU_HIP(hipMemcpyAsync(p->d_dst, dst, nd * sizeof(void*), hipMemcpyHostToDevice, stream));
  } else {
    // one upload of [sources | destinations]
    std::vector<const void*> host(ns + nd);
    std::memcpy(host.data(), src, ns * sizeof(void*));
    std::memcpy(host.data() + ns, dst, nd * sizeof(void*));
    if (stream) {
      ECGPU_HIP(hipMemcpyAsync(p->d_ptrs, host.data(), (ns + nd) * sizeof(void*), hipMemcpyHostToDevice, stream));
      ECGPU_HIP(hipStreamSynchronize(stream));  // the host table dies on return
    } else {
      ECGPU_HIP(hipMemcpy(p->d_ptrs, host.data(), (ns + nd) * sizeof(void*), hipMemcpyHostToDevice));
    }
  }
  p->stripes = stripes;
  p->size = size;
  p->aligned = aligned;
  return ECGPU_OK;
}

ECGPU_RT_END
// ================================================================ C ABI ====
extern "C" {

ECGPU_API ecgpu_plan* ecgpu_plan_create(int rows, int nsrc, const int* coefs, int device) {
  if (rows <= 0 || nsrc <= 0 || !coefs) {
    fail(ECGPU_ERR_ARG, "ecgpu_plan_create: rows, nsrc > 0 and coefs required");
    return nullptr;
  }
  if (device < 0) device = current_device();
  auto* p = new ecgpu_plan();
  if (plan_init(p, rows, nsrc, coefs, device) != ECGPU_OK) {
    plan_free(p);
    return nullptr;
  }
  return p;
}

ECGPU_API int ecgpu_plan_bind(ecgpu_plan* p, int stripes, const uint8_t* const* src_ptrs, uint8_t* const* dst_ptrs,
                              int64_t size) {
  if (!p || stripes < 0 || size < 0 || (stripes && (!src_ptrs || !dst_ptrs)))
    return fail(ECGPU_ERR_ARG, "ecgpu_plan_bind: bad arguments");
  if (int rc = ecgpu_plan_check_buffers(p->rows, p->nsrc, stripes, src_ptrs, dst_ptrs, size)) return rc;
  return plan_bind(p, stripes, src_ptrs, dst_ptrs, size, nullptr);
}

ECGPU_API int ecgpu_plan_set_kernel(ecgpu_plan* p, int kind, int nontemporal) {
  if (!p || (kind != ECGPU_KERNEL_PERM && kind != ECGPU_KERNEL_LDS))
    return fail(ECGPU_ERR_ARG, "ecgpu_plan_set_kernel: bad arguments");
  p->kind = kind;
  p->nt = clamp_store_policy(nontemporal);
  return ECGPU_OK;
}

ECGPU_API int ecgpu_plan_launch(ecgpu_plan* p, void* stream) {
  if (!p) return fail(ECGPU_ERR_ARG, "ecgpu_plan_launch: null plan");
  return plan_launch(p, static_cast<hipStream_t>(stream));
}

ECGPU_API void ecgpu_plan_destroy(ecgpu_plan* p) { plan_free(p); }

ECGPU_API int ecgpu_encode_batch(int k, int m, const int* matrix, int stripes, const uint8_t* const* data,
                                 uint8_t* const* coding, int64_t size, void* stream) {
  if (k <= 0 || m <= 0 || !matrix || stripes < 0 || size < 0 || (stripes && (!data || !coding)))
    return fail(ECGPU_ERR_ARG, "ecgpu_encode_batch: bad arguments");
  if (int rc = ecgpu_plan_check_buffers(m, k, stripes, data, coding, size)) return rc;
  ecgpu_plan* p = ecgpu_plan_create(m, k, matrix, -1);
  if (!p) return ECGPU_ERR_HIP;
  int rc = plan_bind(p, stripes, data, coding, size, static_cast<hipStream_t>(stream));
  if (rc == ECGPU_OK) rc = plan_launch(p, static_cast<hipStream_t>(stream));
  if (rc == ECGPU_OK && stream) {
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) rc = fail(ECGPU_ERR_HIP, hipGetErrorString(e));
  } else if (rc == ECGPU_OK) {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = fail(ECGPU_ERR_HIP, hipGetErrorString(e));
  }
  plan_free(p);
  return rc;
}

}  // extern "C"
