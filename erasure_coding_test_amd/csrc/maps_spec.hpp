// maps_spec.hpp -- the compile-time-specialised multi-map kernels
// (maps_kernels.hpp gf_apply_maps<K, R, NT>) for K = 1..kMaxSpecK sources and
// R = 1..kMaxRows rows.  Instantiated in four translation units, one per R
// (maps_spec.hip built with -DECGPU_SPEC_R=1..4), like gf_spec.hpp.  Every
// cell is one 256-lane kernel: there is no one-wave form (gf_kernels_w8.hpp
// adopted that only on measured gains, and nothing is measured here).
#pragma once
#include "gf_device.hpp"

namespace ecgpu {
namespace dev {
struct MapsArgs;  // maps_kernels.hpp
}

using MapsKernelFn = void (*)(dev::MapsArgs);
constexpr int kMapsStorePolicies = 2;

// store_pol: store cache policy (gf_device.hpp store16t: 0 plain, 1 nt; loads
// are always non-temporal).  nullptr if K is outside 1..kMaxSpecK.
MapsKernelFn maps_kernel_r1(int K, int store_pol);
MapsKernelFn maps_kernel_r2(int K, int store_pol);
MapsKernelFn maps_kernel_r3(int K, int store_pol);
MapsKernelFn maps_kernel_r4(int K, int store_pol);

inline MapsKernelFn maps_kernel(int K, int R, int store_pol) {
  switch (R) {
    case 1: return maps_kernel_r1(K, store_pol);
    case 2: return maps_kernel_r2(K, store_pol);
    case 3: return maps_kernel_r3(K, store_pol);
    case 4: return maps_kernel_r4(K, store_pol);
    default: return nullptr;
  }
}

}  // namespace ecgpu
