// maps_spec.hip -- one R's share of the specialised multi-map kernel table
// (maps_spec.hpp).  Built four times: -DECGPU_SPEC_R=1..4.
#include <hip/hip_runtime.h>

#include "maps_kernels.hpp"
#include "maps_spec.hpp"

#ifndef ECGPU_SPEC_R
#error "build with -DECGPU_SPEC_R=<1..4>"
#endif

namespace ecgpu {
namespace {

constexpr int kR = ECGPU_SPEC_R;

// NT: loads always non-temporal (bit 0), bit 1 = store policy
template <int K>
struct Row {
  static constexpr MapsKernelFn apply[kMapsStorePolicies] = {&dev::gf_apply_maps<K, kR, 1>,
                                                             &dev::gf_apply_maps<K, kR, 3>};
};

template <int... Ks>
MapsKernelFn pick(int K, int store_pol) {
  MapsKernelFn out = nullptr;
  ((K == Ks ? (out = Row<Ks>::apply[store_pol], 0) : 0), ...);
  return out;
}

}  // namespace

#define ECGPU_CAT2(a, b) a##b
#define ECGPU_CAT(a, b) ECGPU_CAT2(a, b)
MapsKernelFn ECGPU_CAT(maps_kernel_r, ECGPU_SPEC_R)(int K, int store_pol) {
  if (store_pol < 0 || store_pol >= kMapsStorePolicies) return nullptr;
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(K, store_pol);
}

}  // namespace ecgpu
