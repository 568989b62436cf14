// rollout.hip — the general kernel's lockstep instantiations for one and two
// deployments (rollout_kernel<1|2, 8|16>, rollout_kernel.h) and the launcher
// that picks the smallest instantiation that holds the world.
#include "rollout_kernel.h"

namespace ccka {

hipError_t launch_rollout(const KParams& p, int block, size_t lds, hipStream_t s) {
  const unsigned grid = (unsigned)((p.N + block - 1) / block);
  // the smallest instantiation that holds the world (kernel_dims); four or
  // more deployments: rollout_multi.hip
  int dmax, nmax;
  kernel_dims(p.D, p.maxn, &dmax, &nmax);
  if (dmax >= 4) return launch_rollout_multi(p, block, lds, s);
  if (dmax == 1 && nmax == 8)
    hipLaunchKernelGGL((rollout_kernel<1, 8>), dim3(grid), dim3(block), lds, s, p);
  else if (dmax == 1)
    hipLaunchKernelGGL((rollout_kernel<1, 16>), dim3(grid), dim3(block), lds, s, p);
  else if (dmax == 2 && nmax == 8)
    hipLaunchKernelGGL((rollout_kernel<2, 8>), dim3(grid), dim3(block), lds, s, p);
  else
    hipLaunchKernelGGL((rollout_kernel<2, 16>), dim3(grid), dim3(block), lds, s, p);
  return hipGetLastError();
}

}  // namespace ccka
