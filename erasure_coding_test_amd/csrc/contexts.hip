// contexts.hip -- the contexts of the synchronous calls (Ctx in runtime.hpp):
// a process-wide pool of stream + staging buffers + plan cache, so concurrent
// callers never share a stream or a lock on the submit path, and the growth
// of a context's three staging buffers.  When a call uses which buffer is
// ecgpu_runtime.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "ecgpu.h"
#include "host_sync.hpp"
#include "knobs.hpp"
#include "runtime.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;

ECGPU_RT_BEGIN

// ------------------------------------------------------ context pool ----

hostsync::IdlePool<Ctx> g_pool;  // idle contexts (process lifetime)

Ctx* acquire_ctx(int device, int* rc) {
  if (Ctx* c = g_pool.acquire(device)) {
    *rc = ECGPU_OK;
    return c;
  }
  auto* c = new Ctx();
  c->device = device;
  DeviceGuard g(device);
  // A blocking stream: a synchronous call on device buffers is ordered after
  // work the caller queued on the null stream (PyTorch's default stream,
  // e.g. the fill of a freshly allocated output), and that stream's later
  // work after the call.  Calls from different threads still run on
  // different contexts, unordered against each other.
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault);
  if (e != hipSuccess) {
    *rc = fail_hip(e, "hipStreamCreateWithFlags");
    delete c;
    return nullptr;
  }
  *rc = ECGPU_OK;
  return c;
}

void release_ctx(Ctx* c) { g_pool.release(c->device, c); }


int ctx_plan(Ctx* c, int rows, int nsrc, const std::vector<uint32_t>& coef, int w, ecgpu_plan** out) {
  // the engine and store policy are part of the key: a knob switched between
  // calls (an in-process A/B) must reach the next launch (plan_init reads them)
  const int kind = knob(Knob::kKernel), nt = clamp_store_policy(knob(Knob::kNt));
  PlanKey key{rows, nsrc, w, kind, nt, coef};
  for (auto it = c->plans.begin(); it != c->plans.end(); ++it)
    if (it->first == key) {
      c->plans.splice(c->plans.begin(), c->plans, it);
      *out = it->second;
      return ECGPU_OK;
    }
  auto* p = new ecgpu_plan();
  std::vector<int> ci(coef.begin(), coef.end());
  int rc = plan_init(p, rows, nsrc, ci.data(), c->device, w);
  if (rc != ECGPU_OK) {
    plan_free(p);
    return rc;
  }
  c->plans.emplace_front(std::move(key), p);
  if (c->plans.size() > 64) {
    plan_free(c->plans.back().second);
    c->plans.pop_back();
  }
  *out = p;
  return ECGPU_OK;
}

int ensure_bounce(Ctx* c, size_t bytes) {
  if (bytes <= c->bounce_cap) return ECGPU_OK;
  DeviceGuard g(c->device);
  if (c->bounce) ECGPU_HIP(hipHostFree(c->bounce));
  c->bounce = nullptr;
  c->bounce_cap = 0;
  ECGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->bounce), bytes, hipHostMallocDefault));
  c->bounce_cap = bytes;
  return ECGPU_OK;
}

// Coherent (fine-grained) pinned memory: the GPU does not cache it, so CPU
// writes before a launch and GPU writes before its completion are visible to
// the other side without cache maintenance.  Grows geometrically.
int ensure_zc(Ctx* c, size_t bytes) {
  if (bytes <= c->zc_cap) return ECGPU_OK;
  DeviceGuard g(c->device);
  if (c->zc) ECGPU_HIP(hipHostFree(c->zc));
  c->zc = nullptr;
  c->zc_cap = 0;
  const size_t want = std::max(bytes, size_t(256) << 10);
  ECGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->zc), want, hipHostMallocMapped | hipHostMallocCoherent));
  c->zc_cap = want;
  return ECGPU_OK;
}

int ensure_stage(Ctx* c, size_t bytes) {
  if (bytes <= c->stage_cap) return ECGPU_OK;
  DeviceGuard g(c->device);
  if (c->stage) ECGPU_HIP(hipFree(c->stage));
  c->stage = nullptr;
  c->stage_cap = 0;
  ECGPU_HIP(hipMalloc(reinterpret_cast<void**>(&c->stage), bytes));
  c->stage_cap = bytes;
  return ECGPU_OK;
}

ECGPU_RT_END
