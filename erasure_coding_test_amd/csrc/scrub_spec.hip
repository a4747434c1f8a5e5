// scrub_spec.hip -- one R's share of the specialised scrub kernel table
// (scrub_spec.hpp).  Built four times: -DECGPU_SPEC_R=1..4.
#include <hip/hip_runtime.h>

#include "scrub_kernels.hpp"
#include "scrub_spec.hpp"

#ifndef ECGPU_SPEC_R
#error "build with -DECGPU_SPEC_R=<1..4>"
#endif

namespace ecgpu {
namespace {

constexpr int kR = ECGPU_SPEC_R;
constexpr int kUnitVariants[5] = {dev::kUnitNone, dev::kUnitCol0, dev::kUnitRow0, dev::kUnitCol0 | dev::kUnitRow0,
                                  dev::kUnitAll};

template <int K, int U, int LATE>
constexpr ScrubKernelFn verify_fn() { return &dev::scrub_verify<K, kR, kUnitVariants[U], LATE>; }

template <int K>
struct Row {
  static constexpr ScrubKernelFn verify[2][5] = {
      {verify_fn<K, 0, 0>(), verify_fn<K, 1, 0>(), verify_fn<K, 2, 0>(), verify_fn<K, 3, 0>(), verify_fn<K, 4, 0>()},
      {verify_fn<K, 0, 1>(), verify_fn<K, 1, 1>(), verify_fn<K, 2, 1>(), verify_fn<K, 3, 1>(), verify_fn<K, 4, 1>()}};
};

template <int... Ks>
ScrubKernelFn pick(int K, int u, bool late) {
  ScrubKernelFn out = nullptr;
  ((K == Ks ? (out = Row<Ks>::verify[late ? 1 : 0][u], 0) : 0), ...);
  return out;
}

}  // namespace

#define ECGPU_CAT2(a, b) a##b
#define ECGPU_CAT(a, b) ECGPU_CAT2(a, b)
ScrubKernelFn ECGPU_CAT(scrub_kernel_r, ECGPU_SPEC_R)(int K, int unit_variant, bool late) {
  if (unit_variant < 0 || unit_variant > 4) return nullptr;
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(K, unit_variant, late);
}

}  // namespace ecgpu
