// scrub_spec.hpp -- the compile-time-specialised scrub kernels
// (scrub_kernels.hpp scrub_verify<K, R, UNITS, LATE>) for K = 1..kMaxSpecK
// data shards and R = 1..kMaxRows coding shards.  Instantiated in four
// translation units, one per R (scrub_spec.hip built with
// -DECGPU_SPEC_R=1..4), like gf_spec.hpp.
#pragma once
#include "gf_device.hpp"

namespace ecgpu {
namespace dev {
struct ScrubArgs;  // scrub_kernels.hpp
}

using ScrubKernelFn = void (*)(dev::ScrubArgs);

// unit_variant: the unit-coefficient structure of the matrix (runtime.hpp
// unit_variant); late: the parity columns are loaded after the combine.
// nullptr if K is outside 1..kMaxSpecK.
ScrubKernelFn scrub_kernel_r1(int K, int unit_variant, bool late);
ScrubKernelFn scrub_kernel_r2(int K, int unit_variant, bool late);
ScrubKernelFn scrub_kernel_r3(int K, int unit_variant, bool late);
ScrubKernelFn scrub_kernel_r4(int K, int unit_variant, bool late);

inline ScrubKernelFn scrub_kernel(int K, int R, int unit_variant, bool late) {
  switch (R) {
    case 1: return scrub_kernel_r1(K, unit_variant, late);
    case 2: return scrub_kernel_r2(K, unit_variant, late);
    case 3: return scrub_kernel_r3(K, unit_variant, late);
    case 4: return scrub_kernel_r4(K, unit_variant, late);
    default: return nullptr;
  }
}

}  // namespace ecgpu
