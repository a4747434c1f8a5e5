// gf_spec.hpp -- the compile-time-specialised production kernels
// (gf_kernels_w8.hpp gf_apply<K, R, UNITS, NT> and gf_apply_lds<K, R>)
// for K = 1..kMaxSpecK sources.  Instantiated in four translation units, one
// per output-row count R (gf_spec.hip built with -DECGPU_SPEC_R=1..4), so
// the build compiles them in parallel.  This header needs only the argument
// types (gf_device.hpp): the units that include it compile no kernel.
#pragma once
#include "gf_device.hpp"

namespace ecgpu {

using SpecKernelFn = void (*)(dev::ApplyArgs);
// A specialised kernel with the lanes per workgroup it was compiled for
// (gf_kernels_w8.hpp apply_block; kBlock for the LDS engine): the
// launch takes its block and grid from here, never from a constant of its own.
struct SpecKernel {
  SpecKernelFn fn = nullptr;
  int block = 0;
};
using InlineKernelFn = void (*)(dev::InlineArgs);
constexpr int kStorePolicies = 2;

// store_pol: store cache policy of the production kernel, 0 plain, 1 nt
// (gf_device.hpp store16t; loads are always
// non-temporal).  lds: the LDS nibble-table kernel instead.
// unit_variant indexes kUnitVariants (gf_spec.hip; runtime.hpp unit_variant
// computes it).  big: shards above dev::kOneWaveMaxShard bytes -- the 256-lane
// instantiation of the kernels that also have a one-wave form.  fn == nullptr
// if K is outside 1..kMaxSpecK.
SpecKernel spec_kernel_r1(bool lds, int K, int unit_variant, int store_pol, bool big);
SpecKernel spec_kernel_r2(bool lds, int K, int unit_variant, int store_pol, bool big);
SpecKernel spec_kernel_r3(bool lds, int K, int unit_variant, int store_pol, bool big);
SpecKernel spec_kernel_r4(bool lds, int K, int unit_variant, int store_pol, bool big);

// gf_apply_inl<K, R, UNITS, ZC> (one stripe, everything in the kernel
// arguments; zc: the grid-stride form for host memory used in place);
// nullptr if K is outside 1..kMaxSpecK.
InlineKernelFn inline_kernel_r1(int K, int unit_variant, bool zc);
InlineKernelFn inline_kernel_r2(int K, int unit_variant, bool zc);
InlineKernelFn inline_kernel_r3(int K, int unit_variant, bool zc);
InlineKernelFn inline_kernel_r4(int K, int unit_variant, bool zc);

inline InlineKernelFn inline_kernel(int K, int R, int unit_variant, bool zc) {
  switch (R) {
    case 1: return inline_kernel_r1(K, unit_variant, zc);
    case 2: return inline_kernel_r2(K, unit_variant, zc);
    case 3: return inline_kernel_r3(K, unit_variant, zc);
    case 4: return inline_kernel_r4(K, unit_variant, zc);
    default: return nullptr;
  }
}

inline SpecKernel spec_kernel(bool lds, int K, int R, int unit_variant, int store_pol, bool big) {
  switch (R) {
    case 1: return spec_kernel_r1(lds, K, unit_variant, store_pol, big);
    case 2: return spec_kernel_r2(lds, K, unit_variant, store_pol, big);
    case 3: return spec_kernel_r3(lds, K, unit_variant, store_pol, big);
    case 4: return spec_kernel_r4(lds, K, unit_variant, store_pol, big);
    default: return {};
  }
}

}  // namespace ecgpu
