// dev_common.h — leaf device helpers every kernel unit shares: the wave width,
// Philox-4x32-10, the capacity-type bit, the down-window mask and the
// cross-lane read / reduce helpers. Internal linkage: a translation unit that
// includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ccka.h"

namespace ccka {
namespace {

constexpr int WAVE = 64;

__device__ __forceinline__ int rdl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ uint32_t rdlu(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ double rdld(double v, int lane) {
  long long b = __double_as_longlong(v);
  int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
  int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ long long rdll(long long v, int lane) {
  int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffLL), lane);
  int hi = __builtin_amdgcn_readlane((int)(v >> 32), lane);
  return ((long long)hi << 32) | (unsigned int)lo;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ void wave_argmin(double& s, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double s2 = __shfl_xor(s, o);
    const int i2 = __shfl_xor(idx, o);
    if (s2 < s || (s2 == s && i2 < idx)) { s = s2; idx = i2; }
  }
}
__device__ __forceinline__ int capbit(int c) { return c == 0 ? CCKA_CAP_SPOT : CCKA_CAP_OD; }

// down-window entries of a window (entry k is (k + 1) steps old): bit k set
// while (k + 1) * 60 < window_s
__device__ __forceinline__ int window_mask(int window_s) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < CCKA_HIST; ++k) m |= ((k + 1) * CCKA_STEP_SECONDS < window_s) ? (1 << k) : 0;
  return m;
}

// llrint(x * scale), flagged when it is not representable (NaN or
// |x * scale| >= 2^63): the fixed-point rule of the totals (util.hip) and of
// the paired comparison (paired.hip)
__device__ __forceinline__ long long fix_chk(double x, double scale, long long& ovf) {
  const double y = x * scale;
  if (!(y > -9.2233720368547758e18 && y < 9.2233720368547758e18)) {
    ovf = 1;
    return 0;
  }
  return __double2ll_rn(y);
}

// Philox-4x32-10 (SEMANTICS.md §4): the load generator, the synthetic MLP
// states and the sampled policy action all draw from this one text
__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                       uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace
}  // namespace ccka
