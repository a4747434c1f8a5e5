// gf_spec.hip -- one R's share of the specialised w = 8 kernel table
// (gf_spec.hpp).  Built four times: -DECGPU_SPEC_R=1..4.
#include <hip/hip_runtime.h>

#include "gf_kernels_w8.hpp"
#include "gf_spec.hpp"

#ifndef ECGPU_SPEC_R
#error "build with -DECGPU_SPEC_R=<1..4>"
#endif

namespace ecgpu {
namespace {

constexpr int kR = ECGPU_SPEC_R;
constexpr int kUnitVariants[5] = {dev::kUnitNone, dev::kUnitCol0, dev::kUnitRow0, dev::kUnitCol0 | dev::kUnitRow0,
                                  dev::kUnitAll};

// NT: loads always non-temporal (bit 0), NT >> 1 = store policy
// (gf_device.hpp store16t: 0 plain, 1 nt)
// and, where the kernel has a one-wave form, bit 2 (dev::kNt256Lanes) its
// 256-lane instantiation for shards above dev::kOneWaveMaxShard (BIG); every
// other cell is one kernel under both BIG values
template <int K, int U, int STORE, bool BIG>
constexpr SpecKernel apply_fn() {
  constexpr int NT = 1 | (STORE << 1) | (BIG && dev::has_one_wave_form<K, kR, kUnitVariants[U]>() ? dev::kNt256Lanes : 0);
  return SpecKernel{&dev::gf_apply<K, kR, kUnitVariants[U], NT>, dev::apply_block<K, kR, kUnitVariants[U], NT>()};
}

template <int K, int S, bool BIG>
struct Pol {
  static constexpr SpecKernel apply[5] = {apply_fn<K, 0, S, BIG>(), apply_fn<K, 1, S, BIG>(), apply_fn<K, 2, S, BIG>(),
                                          apply_fn<K, 3, S, BIG>(), apply_fn<K, 4, S, BIG>()};
};

template <int K, int U, bool ZC>
constexpr InlineKernelFn inl_fn() { return &dev::gf_apply_inl<K, kR, kUnitVariants[U], ZC>; }

template <int K>
struct Row {
  static constexpr InlineKernelFn inl[2][5] = {
      {inl_fn<K, 0, false>(), inl_fn<K, 1, false>(), inl_fn<K, 2, false>(), inl_fn<K, 3, false>(), inl_fn<K, 4, false>()},
      {inl_fn<K, 0, true>(), inl_fn<K, 1, true>(), inl_fn<K, 2, true>(), inl_fn<K, 3, true>(), inl_fn<K, 4, true>()}};
  static constexpr const SpecKernel* apply[2][kStorePolicies] = {{Pol<K, 0, false>::apply, Pol<K, 1, false>::apply},
                                                                 {Pol<K, 0, true>::apply, Pol<K, 1, true>::apply}};
  static constexpr SpecKernelFn lds = &dev::gf_apply_lds<K, kR>;
};

template <int... Ks>
SpecKernel pick(bool lds, int K, int u, int store_pol, bool big) {
  SpecKernel out;
  ((K == Ks ? (out = lds ? SpecKernel{Row<Ks>::lds, dev::kBlock} : Row<Ks>::apply[big ? 1 : 0][store_pol][u], 0) : 0), ...);
  return out;
}

template <int... Ks>
InlineKernelFn pick_inl(int K, int u, bool zc) {
  InlineKernelFn out = nullptr;
  ((K == Ks ? (out = Row<Ks>::inl[zc ? 1 : 0][u], 0) : 0), ...);
  return out;
}

}  // namespace

#define ECGPU_CAT2(a, b) a##b
#define ECGPU_CAT(a, b) ECGPU_CAT2(a, b)
SpecKernel ECGPU_CAT(spec_kernel_r, ECGPU_SPEC_R)(bool lds, int K, int unit_variant, int store_pol, bool big) {
  if (unit_variant < 0 || unit_variant > 4 || store_pol < 0 || store_pol >= kStorePolicies) return {};
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(lds, K, unit_variant, store_pol, big);
}

InlineKernelFn ECGPU_CAT(inline_kernel_r, ECGPU_SPEC_R)(int K, int unit_variant, bool zc) {
  if (unit_variant < 0 || unit_variant > 4) return nullptr;
  return pick_inl<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(K, unit_variant, zc);
}

}  // namespace ecgpu
