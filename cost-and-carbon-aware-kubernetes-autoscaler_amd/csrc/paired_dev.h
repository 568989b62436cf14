// paired_dev.h — how one per-position delta of the paired comparison is formed
// (SEMANTICS 8), shared by paired.hip and boot.hip: the integer of one
// objective of one scenario, and the flagged subtraction. Internal linkage, as
// dev_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "kparams.h"

namespace ccka {
namespace {

// objective o of scenario idx as its integer (SEMANTICS 8: units)
__device__ __forceinline__ long long paired_value(const GridSrc& g, int o, int64_t idx, long long& ovf) {
  switch (o) {
    case 0: return g.cost[idx];
    case 1: return (long long)g.slo[idx];
    case 2: return fix_chk(g.gco2[idx], 1e6, ovf);
    default: return fix_chk(g.energy[idx], 1e6, ovf);
  }
}

// a - b, flagged instead of wrapped
__device__ __forceinline__ long long sub_chk(long long a, long long b, long long& ovf) {
  long long r;
  if (__builtin_sub_overflow(a, b, &r)) ovf = 1;
  return r;
}

}  // namespace
}  // namespace ccka
