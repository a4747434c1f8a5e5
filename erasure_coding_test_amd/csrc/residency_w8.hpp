// residency_w8.hpp -- the arithmetic of the w = 8 residency cap: from waves
// per CU and a kernel's lanes per workgroup to workgroups per CU, and from
// those to the unused dynamic LDS allocation that enforces them.  Host code,
// shared by the dispatcher (dispatch_w8.hip: the rule that picks the waves,
// its constants and the measurements behind them) and the diagnostic library
// (diag_kernels.hip), which asks the runtime what it grants under the
// allocation.
#pragma once

namespace ecgpu {

constexpr int kLanesPerWave = 64;

inline int residency_workgroups(int waves_per_cu, int lanes) {
  return waves_per_cu / ((lanes + kLanesPerWave - 1) / kLanesPerWave);
}

// LDS_per_CU / workgroups rounded down to 512 B.  A kernel with static LDS of
// its own gets that much less and a further 4 KiB margin, rounded down to
// 4 KiB (dispatch_w8.hip).  0: no cap -- no workgroups asked for, or the
// allocation would admit one more than asked.
inline unsigned residency_lds_for(int lds_per_cu, int workgroups, unsigned static_bytes) {
  if (workgroups <= 0 || lds_per_cu <= 0) return 0;
  const unsigned total = unsigned(lds_per_cu / workgroups) & ~511u;
  const unsigned reserve = static_bytes ? static_bytes + 4096u : 0u;
  if (total <= reserve) return 0;
  const unsigned b = (total - reserve) & (static_bytes ? ~4095u : ~511u);
  return b + static_bytes > unsigned(lds_per_cu / (workgroups + 1)) ? b : 0u;
}

}  // namespace ecgpu
