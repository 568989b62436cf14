// rollout_sk.hip — the general kernel on the lane-skewed schedule
// (rollout_kernel<DMAX, MAXN, 0, 1, LF2>, rollout_kernel.h): worlds of two to four HPA /
// static deployments run their quiet steps per lane and their full steps in
// per-wave batches of stalled lanes (the single-deployment kernel's event
// batching, rollout_d1.hip, for several deployments). sk_eligible
// (abi_rollout.cpp) checks the preconditions.
#include "rollout_kernel.h"

// Lane-local provisioning on this unit's kernels (variant builds pass
// -DCCKA_SK_LF2=1; measured 1-4 % slower than the cooperative scans). Used only
// as a template argument below, so no template body depends on it.
#ifndef CCKA_SK_LF2
#define CCKA_SK_LF2 0
#endif

namespace ccka {

bool rollout_sk_lane_f2() { return CCKA_SK_LF2 != 0; }

hipError_t launch_rollout_sk(const KParams& p, int block, size_t lds, hipStream_t s) {
  const unsigned grid = (unsigned)((p.N + block - 1) / block);
  int dmax, nmax;
  kernel_dims(p.D, p.maxn, &dmax, &nmax);
  if (dmax == 2 && nmax == 8)
    hipLaunchKernelGGL((rollout_kernel<2, 8, 0, 1, CCKA_SK_LF2>), dim3(grid), dim3(block), lds, s, p);
#ifdef CCKA_SK_ONE  // variant builds (tools/build_variants.py): <2, 8> only, compiled in a minute
  else
    return hipErrorInvalidValue;
#else
  else if (dmax == 2)
    hipLaunchKernelGGL((rollout_kernel<2, 16, 0, 1, CCKA_SK_LF2>), dim3(grid), dim3(block), lds, s, p);
  else if (dmax == 4 && nmax == 8)
    hipLaunchKernelGGL((rollout_kernel<4, 8, 0, 1, CCKA_SK_LF2>), dim3(grid), dim3(block), lds, s, p);
  else if (dmax == 4)  // rollout_sk416.hip
    return launch_rollout_sk416(p, block, lds, s);
  else
    return hipErrorInvalidValue;
#endif
  return hipGetLastError();
}

}  // namespace ccka
