// host_memory.hip -- where a buffer lives and how shards cross the link: the
// one query of HIP's pointer attributes and the predicates over it (classify,
// host_mapped, is_pinned, where / all_host), the shard copies between host
// and device (copy_shards), and the ecgpu_host_register / _unregister C ABI.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ecgpu.h"
#include "knobs.hpp"
#include "planner.hpp"
#include "runtime.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;

ECGPU_RT_BEGIN

// What HIP says about a pointer: the query's status and, where it succeeded,
// the memory type and the device.  A failed query (unregistered pageable
// memory among others) is cleared from HIP's per-thread last error, which is
// shared with the caller's HIP code.
struct PointerInfo {
  hipError_t status;
  hipMemoryType type;
  int device;
  bool on_device() const {
    return status == hipSuccess && (type == hipMemoryTypeDevice || type == hipMemoryTypeManaged);
  }
  bool pinned_host() const { return status == hipSuccess && type == hipMemoryTypeHost; }
};

PointerInfo query_pointer(const void* p) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return {e, hipMemoryTypeUnregistered, -1};
  }
  return {e, attr.type, attr.device};
}

// Is p device memory of `device` (usable in place)?  Host memory (pageable or
// pinned) is staged; device memory of another GPU is rejected.
int classify(const void* p, int device, bool* on_device) {
  const PointerInfo q = query_pointer(p);
  if (q.on_device() && q.device != device)
    return fail(ECGPU_ERR_ARG, "buffer lives on device " + std::to_string(q.device) + ", call runs on " +
                                   std::to_string(device));
  *on_device = q.on_device();
  return ECGPU_OK;
}

// Host memory the GPU addresses in place -- hipHostMalloc'd, or registered
// with hipHostRegister -- when [p, p + bytes) lies inside ONE such
// allocation (HIP's range attributes; a range that leaves it would fault).
// *dev = the device address of p.
bool host_mapped(const void* p, size_t bytes, void** dev) {
  if (!query_pointer(p).pinned_host()) return false;
  void* start = nullptr;
  size_t range = 0;
  if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, hipDeviceptr_t(p)) != hipSuccess ||
      hipPointerGetAttribute(&range, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, hipDeviceptr_t(p)) != hipSuccess ||
      hipHostGetDevicePointer(dev, const_cast<void*>(p), 0) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const char* c = static_cast<const char*>(p);
  const char* s0 = static_cast<const char*>(start);
  return c >= s0 && bytes <= range && size_t(c - s0) <= range - bytes;
}

bool is_pinned(const void* p) { return query_pointer(p).pinned_host(); }

Where where(const void* p) {
  const PointerInfo q = query_pointer(p);
  if (q.status == hipSuccess) return q.on_device() ? Where::kDevice : Where::kHost;
  // unregistered pageable memory, or no GPU runtime at all (then no device
  // memory can exist); any other failure proves nothing
  return q.status == hipErrorInvalidValue || q.status == hipErrorNoDevice || q.status == hipErrorInsufficientDriver
             ? Where::kHost
             : Where::kUnknown;
}

bool all_host(const std::vector<void*>& bufs) {
  for (void* p : bufs)
    if (where(p) != Where::kHost) return false;
  return true;
}

bool all_host(const FusedOp& op) { return all_host(op.srcs) && all_host(op.dsts); }

// Moves n shards of `bytes` between host pointers hp[i] and device shards
// d0 + i * dstride.  Every run of >= 2 evenly spaced host shards (a stripe
// laid out in one host slab, as the reference client's stripe buffer is,
// client_main.cpp:1619-1647) goes as ONE 2-D copy, the rest one copy per
// shard.  ECGPU_PIPE_2D=0 always copies per shard.  Used by the pipelines and
// by synchronous calls on large host buffers.
int copy_shards(bool h2d, uint8_t* d0, size_t dstride, const std::vector<char*>& hp, size_t bytes, hipStream_t s) {
  const bool two_d = knob(Knob::kPipe2d) != 0;
  const size_t n = hp.size();
  for (size_t a = 0; a < n;) {
    size_t b = a + 1;  // [a, b): maximal run with one pitch >= bytes
    const ptrdiff_t pitch = b < n ? hp[b] - hp[a] : 0;
    // pageable memory only when the run is contiguous (pitch == bytes): a
    // pageable 2-D copy with gaps between rows ran 15x slower than per-shard
    // copies (RS(6,3) 1 MiB, shards malloc'd one by one, 16 B apart)
    bool ok = two_d && pitch > 0 && size_t(pitch) >= bytes;
    if (ok && size_t(pitch) != bytes) ok = is_pinned(hp[a]);  // pinned or registered
    if (ok)
      while (b < n && hp[b] - hp[b - 1] == pitch) ++b;
    // a gapped run must be pinned at both ends (one registration or
    // allocation spans it; HIP rejects a span across separately registered
    // buffers at enqueue, which falls back below)
    if (b - a >= 2 && size_t(pitch) != bytes && !is_pinned(hp[b - 1] + bytes - 1)) b = a + 1;
    uint8_t* d = d0 + a * dstride;
    if (b - a >= 2) {
      // contiguous on both sides: one 1-D copy.  HIP's 2-D copies lost 40 % of
      // the link when two processes shared the GPU in some allocation states
      // (bench.py's N = 2 rehearsal after its C5 leg: 27 vs 44 GiB/s; 1-D
      // copies 41)
      // (ECGPU_PIPE_FLAT=0 keeps flat runs on hipMemcpy2DAsync too: an A/B switch)
      const bool flat = size_t(pitch) == bytes && dstride == bytes && knob(Knob::kPipeFlat) != 0;
      const hipError_t e =
          flat ? (h2d ? hipMemcpyAsync(d, hp[a], bytes * (b - a), hipMemcpyHostToDevice, s)
                      : hipMemcpyAsync(hp[a], d, bytes * (b - a), hipMemcpyDeviceToHost, s))
          : h2d ? hipMemcpy2DAsync(d, dstride, hp[a], size_t(pitch), bytes, b - a, hipMemcpyHostToDevice, s)
                : hipMemcpy2DAsync(hp[a], size_t(pitch), d, dstride, bytes, b - a, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) {
        a = b;
        continue;
      }
      // not enqueued: fall back to one copy per shard (the error is not sticky)
      (void)hipGetLastError();
    }
    for (size_t i = a; i < b; ++i) {
      if (h2d)
        ECGPU_HIP(hipMemcpyAsync(d0 + i * dstride, hp[i], bytes, hipMemcpyDefault, s));
      else
        ECGPU_HIP(hipMemcpyAsync(hp[i], d0 + i * dstride, bytes, hipMemcpyDefault, s));
    }
    a = b;
  }
  return ECGPU_OK;
}

ECGPU_RT_END
// ================================================================ C ABI ====
extern "C" {

ECGPU_API int ecgpu_host_register(void* ptr, int64_t bytes) {
  if (!ptr || bytes <= 0) return fail(ECGPU_ERR_ARG, "ecgpu_host_register: bad arguments");
  ECGPU_HIP(hipHostRegister(ptr, size_t(bytes), hipHostRegisterDefault));
  return ECGPU_OK;
}

ECGPU_API int ecgpu_host_unregister(void* ptr) {
  if (!ptr) return fail(ECGPU_ERR_ARG, "ecgpu_host_unregister: null");
  ECGPU_HIP(hipHostUnregister(ptr));
  return ECGPU_OK;
}

}  // extern "C"
