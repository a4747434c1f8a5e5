// devices.hip -- which device a call runs on, and whether that device is
// still usable: the classification of HIP errors with the "device lost" mark
// (fail_hip), device selection (ECGPU_DEVICE, ECGPU_DEVICES, one device per
// calling thread in turn), and the ecgpu_set_devices / ecgpu_get_devices /
// ecgpu_call_device / ecgpu_device_pci_bus_id C ABI.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "cpu_fallback.hpp"
#include "ecgpu.h"
#include "knobs.hpp"
#include "runtime.hpp"

using namespace ecgpu;
using namespace ecgpu::rt;

ECGPU_RT_BEGIN

// t_err / fail / ecgpu_last_error live in capi_host.cpp (host code, so the
// host-only checks -- buffer contract, knobs -- report through them too)

// Errors after which the device's context is unusable for the rest of the
// process (a kernel fault, a lost / missing device or driver): the device is
// marked lost, and with ECGPU_CPU_FALLBACK later synchronous calls on it go
// straight to the CPU (cpu_fallback.hpp).  hipErrorInvalidDevice is not one:
// a bad ordinal argument returns it (ecgpu_device_pci_bus_id(99)) on a
// healthy device.
bool sticky(hipError_t e) {
  switch (e) {
    case hipErrorNotInitialized:
    case hipErrorDeinitialized:
    case hipErrorInsufficientDriver:
    case hipErrorNoDevice:
    case hipErrorNoBinaryForGpu:
    case hipErrorECCNotCorrectable:
    case hipErrorIllegalAddress:
    case hipErrorLaunchTimeOut:
    case hipErrorContextIsDestroyed:
    case hipErrorAssert:
    case hipErrorLaunchFailure:
      return true;
    default:
      return false;
  }
}

// The device the current synchronous call targets (CallDeviceScope), -1
// outside one.
thread_local int t_call_device = -1;

CallDeviceScope::CallDeviceScope(int device) : prev(t_call_device) { t_call_device = device; }
CallDeviceScope::~CallDeviceScope() { t_call_device = prev; }

int fail_hip(hipError_t e, const char* what) {
  std::string msg = std::string(what) + ": " + hipGetErrorString(e);
  int d = t_call_device;
  if (d < 0 && hipGetDevice(&d) != hipSuccess) d = -1;
  bool lost = sticky(e);
  if (!lost && e == hipErrorUnknown && d >= 0) {
    // ordinary failures return it too: sticky only when the device still
    // fails a synchronize afterwards
    DeviceGuard g(d);
    (void)hipGetLastError();
    lost = hipDeviceSynchronize() != hipSuccess;
    (void)hipGetLastError();
  }
  if (lost && d >= 0) mark_device_lost(d);
  // The library reports the error through its own channel; HIP's per-thread
  // last error is shared with the caller's HIP code in the same process, so
  // a handled failure (a bad ordinal, an OOM the CPU completed) must not
  // surface in the caller's next error check (torch's launch checks did).
  (void)hipGetLastError();
  return fail(ECGPU_ERR_HIP, msg);
}

// Visible devices, or 0 when HIP cannot tell (no GPU: lists are not checked).
int visible_devices() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 0) {
    (void)hipGetLastError();
    n = 0;
  }
  return n;
}

// A forced ECGPU_DEVICE that names a visible device (or any, when HIP cannot
// tell), else -1: a device this process cannot see is ignored, with one
// stderr line, instead of failing every call (or sending it to the CPU).
int forced_device() {
  const int forced = knob(Knob::kDevice);
  if (forced < 0) return -1;
  static const int visible = visible_devices();
  if (visible <= 0 || forced < visible) return forced;
  static std::once_flag once;
  std::call_once(once, [&] {
    std::fprintf(stderr, "libecgpu: ECGPU_DEVICE=%d ignored (%d visible)\n", forced, visible);
  });
  return -1;
}

int current_device() {
  const int forced = forced_device();
  if (forced >= 0) return forced;
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  return d;
}

// ECGPU_DEVICES (or ecgpu_set_devices): the devices the synchronous
// host-memory calls spread over.  Each calling thread is given one of them,
// round-robin in the order threads make their first such call, and keeps it
// -- so the reference client's byte-range encode pthreads
// (client_main.cpp:1074-1164) each drive their own GPU and PCIe link.  Unset
// (the default): the caller's current device, as before.  "all" = every
// visible device; otherwise a comma-separated list (repeats allowed).
std::mutex g_devices_mu;
std::shared_ptr<const std::vector<int>> g_devices;  // null: unset
std::atomic<uint64_t> g_device_rr{0};

std::vector<int> parse_devices(const char* s, int visible) {
  std::vector<int> out;
  if (!s || !*s) return out;
  if (std::strcmp(s, "all") == 0) {
    for (int d = 0; d < visible; ++d) out.push_back(d);
    return out;
  }
  const char* q = s;
  while (*q) {
    char* end = nullptr;
    const long v = std::strtol(q, &end, 10);
    if (end == q || v < 0 || v > 1023) return {};  // malformed: ignored as a whole
    out.push_back(int(v));
    q = end;
    if (*q == ',') ++q;
    else if (*q) return {};
  }
  return out;
}

// The first entry of `list` that is not a visible device, or -1.
int invisible_entry(const std::vector<int>& list, int visible) {
  for (int d : list)
    if (visible > 0 && d >= visible) return d;
  return -1;
}

std::shared_ptr<const std::vector<int>> device_list() {
  static std::once_flag once;
  std::call_once(once, [] {
    const char* e = std::getenv("ECGPU_DEVICES");
    if (!e || !*e) return;
    const int n = visible_devices();
    auto v = std::make_shared<const std::vector<int>>(parse_devices(e, n));
    // a malformed list, or one naming a device this process cannot see, is
    // ignored as a whole (every call would otherwise fail or fall back)
    const int bad = invisible_entry(*v, n);
    if (v->empty() || bad >= 0) {
      std::fprintf(stderr, "libecgpu: ECGPU_DEVICES=\"%s\" ignored (%s)\n", e,
                   bad >= 0 ? ("device " + std::to_string(bad) + " is not visible; " + std::to_string(n) +
                               " visible").c_str()
                            : "expected \"all\" or a comma-separated list of device ordinals");
      return;
    }
    std::lock_guard<std::mutex> lk(g_devices_mu);
    if (!g_devices) g_devices = v;
  });
  std::lock_guard<std::mutex> lk(g_devices_mu);
  return g_devices;
}

// The device a synchronous call on host memory runs on: a forced
// ECGPU_DEVICE, else this thread's device from the ECGPU_DEVICES list, else
// the caller's current device.
int host_call_device() {
  if (const int forced = forced_device(); forced >= 0) return forced;
  const auto list = device_list();
  if (!list || list->empty()) return current_device();
  thread_local std::shared_ptr<const std::vector<int>> t_list;
  thread_local int t_dev = -1;
  if (t_list != list) {
    t_list = list;
    t_dev = (*list)[size_t(g_device_rr.fetch_add(1, std::memory_order_relaxed) % list->size())];
  }
  return t_dev;
}

// A call naming device memory runs where that memory is (the current device,
// as before: classify() rejects another device's buffers); an all-host call
// takes host_call_device().
int call_device(const std::vector<void*>& a, const std::vector<void*>& b) {
  if (const int forced = forced_device(); forced >= 0) return forced;
  const auto list = device_list();
  if (!list || list->empty()) return current_device();
  if (!all_host(a) || !all_host(b)) return current_device();
  return host_call_device();
}

ECGPU_RT_END
// ================================================================ C ABI ====
extern "C" {

ECGPU_API int ecgpu_set_devices(int n, const int* devices) {
  if (n < 0 || (n > 0 && !devices)) return fail(ECGPU_ERR_ARG, "ecgpu_set_devices: bad arguments");
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0) return fail(ECGPU_ERR_ARG, "ecgpu_set_devices: negative device");
  const int visible = visible_devices();
  if (const int bad = invisible_entry(std::vector<int>(devices, devices + n), visible); bad >= 0)
    return fail(ECGPU_ERR_ARG, "ecgpu_set_devices: device " + std::to_string(bad) + " is not visible (" +
                                   std::to_string(visible) + " visible)");
  (void)device_list();  // the environment's list is read first, so this call overrides it
  std::lock_guard<std::mutex> lk(g_devices_mu);
  g_devices = n > 0 ? std::make_shared<const std::vector<int>>(devices, devices + n) : nullptr;
  return ECGPU_OK;
}

ECGPU_API int ecgpu_get_devices(int* out, int cap) {
  const auto list = device_list();
  const int n = list ? int(list->size()) : 0;
  for (int i = 0; i < n && i < cap && out; ++i) out[i] = (*list)[size_t(i)];
  return n;
}

ECGPU_API int ecgpu_call_device(void) { return host_call_device(); }

ECGPU_API int ecgpu_device_pci_bus_id(int device, char* buf, int len) {
  if (!buf || len < 13) return fail(ECGPU_ERR_ARG, "ecgpu_device_pci_bus_id: buffer of >= 13 bytes required");
  ECGPU_HIP(hipDeviceGetPCIBusId(buf, len, device));
  return ECGPU_OK;
}

}  // extern "C"
