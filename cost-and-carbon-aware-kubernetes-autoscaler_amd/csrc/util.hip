// util.hip — the small kernels around a rollout and their launchers: the
// synthetic load generator (SEMANTICS.md §4), the totals reduction, and the
// trace / trajectory layout changes the two engines read and write.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ccka.h"
#include "dev_common.h"
#include "kparams.h"

#pragma clang fp contract(off)

namespace ccka {

// ---------------------------------------------------------------------------
// The synthetic load generator (SEMANTICS.md §4)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gen_load_kernel(GenParams g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int d = blockIdx.y;
  if (i >= g.n) return;
  const uint64_t s = (uint64_t)(g.first_id + i);
  const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
  const uint32_t k0 = (uint32_t)g.seed, k1 = (uint32_t)(g.seed >> 32);
  uint32_t u[4], v[4];
  philox(0xFFFFFFFFu, slo, shi, (uint32_t)d, k0, k1, u);
  philox(0xFFFFFFFEu, slo, shi, (uint32_t)d, k0, k1, v);
  const int64_t base = g.base_lo + (int64_t)(u[0] % (uint32_t)(g.base_hi - g.base_lo + 1));
  const int64_t amp = g.amp_lo + (int64_t)(u[1] % (uint32_t)(g.amp_hi - g.amp_lo + 1));
  const int phase = (int)(u[2] % 1440u);
  const bool burst = (int)(u[3] % 1000u) < g.burst_prob;
  const int bstart = (int)(v[0] % 1440u);
  for (int t = 0; t < g.T; ++t) {
    uint32_t e4[4];
    philox((uint32_t)t, slo, shi, (uint32_t)d, k0, k1, e4);
    const int64_t e = (int64_t)(e4[0] >> 16) + (int64_t)(e4[1] >> 16) + (int64_t)(e4[2] >> 16) +
                      (int64_t)(e4[3] >> 16) - 131072;
    int64_t val = base * (65536000LL + amp * (int64_t)g.sinq[(t + phase) % 1440]) / 65536000LL;
    val = val * (37837000LL + (int64_t)g.noise * e) / 37837000LL;
    if (burst && t >= bstart && t < bstart + g.burst_len) val = val * g.burst_mult / 1000;
    if (val < 0) val = 0;
    if (val > 0x7fffffff) val = 0x7fffffff;
    g.out[((int64_t)t * g.D + d) * g.n + i] = (int32_t)val;
  }
}

hipError_t launch_gen_load(const GenParams& g, hipStream_t s) {
  dim3 grid((unsigned)((g.n + 255) / 256), (unsigned)g.D);
  hipLaunchKernelGGL(gen_load_kernel, grid, dim3(256), 0, s, g);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Totals: fixed-order block partials, then one ordered final pass.
// ---------------------------------------------------------------------------
struct Part {
  long long v[11];  // ccka_totals' int64 block (energy and gCO2 in fixed point) + overflow flag
};

// a + b into a, setting the flag instead of wrapping (signed int64)
__device__ __forceinline__ void add_chk(long long& a, long long b, long long& ovf) {
  long long r;
  if (__builtin_add_overflow(a, b, &r)) ovf = 1;
  a = r;
}
// fix_chk (dev_common.h): llrint(x * scale), flagged when it is not representable

__global__ void __launch_bounds__(256) totals_partial(TotParams q) {
  __shared__ Part sp[256];
  const int tid = threadIdx.x;
  Part a;
#pragma unroll
  for (int k = 0; k < 11; ++k) a.v[k] = 0;
  long long& ovf = a.v[10];
  const int64_t chunk = (q.N + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(lo + chunk, q.N);
  for (int64_t i = lo + tid; i < hi; i += blockDim.x) {
    a.v[0] += 1;
    add_chk(a.v[1], q.res.cost[i], ovf);
    a.v[2] += q.res.slo[i];  // int32 per scenario: < 2^31 * N, no overflow below N = 2^32
    add_chk(a.v[3], q.res.pend_min[i], ovf);
    a.v[4] += q.res.nmin_spot[i];
    a.v[5] += q.res.nmin_od[i];
    a.v[6] += q.res.launches[i];
    a.v[7] += q.res.deletions[i];
    add_chk(a.v[8], fix_chk(q.res.energy[i], 1e6, ovf), ovf);  // llrint, as ccka_oracle_totals
    add_chk(a.v[9], fix_chk(q.res.gco2[i], 1e6, ovf), ovf);
  }
  sp[tid] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 10; ++k) add_chk(sp[tid].v[k], sp[tid + s].v[k], sp[tid].v[10]);
      sp[tid].v[10] |= sp[tid + s].v[10];
    }
    __syncthreads();
  }
  if (tid == 0) q.parts[blockIdx.x] = sp[0];
}

__global__ void totals_final(TotParams q, int nparts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Part a;
  for (int k = 0; k < 11; ++k) a.v[k] = 0;
  for (int b = 0; b < nparts; ++b) {
    for (int k = 0; k < 10; ++k) add_chk(a.v[k], q.parts[b].v[k], a.v[10]);
    a.v[10] |= q.parts[b].v[10];
  }
  ccka_totals* o = q.out;
  o->scenarios = a.v[0];
  o->cost_uphmin = a.v[1];
  o->slo_minutes = a.v[2];
  o->pending_pod_minutes = a.v[3];
  o->node_min_spot = a.v[4];
  o->node_min_od = a.v[5];
  o->launches = a.v[6];
  o->deletions = a.v[7];
  o->energy_uwmin = a.v[8];
  o->gco2_ug = a.v[9];
  o->energy_wmin = (double)a.v[8] * 1e-6;
  o->gco2 = (double)a.v[9] * 1e-6;
  *q.ovf = a.v[10];
}

hipError_t launch_totals(const TotParams& q, int nparts, hipStream_t s) {
  hipLaunchKernelGGL(totals_partial, dim3(nparts), dim3(256), 0, s, q);
  hipLaunchKernelGGL(totals_final, dim3(1), dim3(64), 0, s, q, nparts);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Trace and trajectory layouts
// ---------------------------------------------------------------------------
// [T][D][NL] -> [NL][T][DP] through an LDS tile of 64 columns x TT steps x DP
// (TT * DP = 32: each column's part of the tile is one 128-byte run of the
// output): reads of 64 consecutive columns, writes of whole runs
template <int DP>
__global__ void __launch_bounds__(256) trace_nt_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                       int64_t NL, int64_t T, int D) {
  constexpr int TT = 32 / DP;
  __shared__ int32_t tile[64 * 32];  // [col][tt][d]
  const int64_t c0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * TT;
  const int tid = threadIdx.x;
  for (int x = tid; x < TT * DP * 64; x += 256) {
    const int c = x & 63, r = x >> 6, tt = r / DP, d = r % DP;
    const int64_t col = c0 + c, t = t0 + tt;
    int32_t v = 0;
    if (d < D && col < NL && t < T) v = in[(t * D + d) * NL + col];
    tile[c * 32 + tt * DP + d] = v;
  }
  __syncthreads();
  for (int x = tid; x < 64 * 32; x += 256) {
    const int c = x >> 5, k = x & 31, tt = k / DP;
    const int64_t col = c0 + c, t = t0 + tt;
    if (col < NL && t < T) out[(col * T + t0) * DP + k] = tile[x];
  }
}

hipError_t launch_trace_nt(const int32_t* in, int32_t* out, int64_t NL, int64_t T, int32_t D, int32_t DP,
                           hipStream_t s) {
  if (NL <= 0 || T <= 0 || D < 1 || D > DP) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((NL + 63) / 64), (unsigned)((T * DP + 31) / 32));
  switch (DP) {
    case 2: hipLaunchKernelGGL(trace_nt_kernel<2>, grid, dim3(256), 0, s, in, out, NL, T, D); break;
    case 4: hipLaunchKernelGGL(trace_nt_kernel<4>, grid, dim3(256), 0, s, in, out, NL, T, D); break;
    case 8: hipLaunchKernelGGL(trace_nt_kernel<8>, grid, dim3(256), 0, s, in, out, NL, T, D); break;
    case 16: hipLaunchKernelGGL(trace_nt_kernel<16>, grid, dim3(256), 0, s, in, out, NL, T, D); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// [N][T] -> [T][N] trajectory records (ccka_get_trajectory after the
// single-deployment engine), steps [t0, t0 + tc) at a time into a bounded
// staging buffer: 32 x 32 tiles through LDS, 16-byte elements, both sides
// coalesced; the tiles are numbered on grid.x alone (no grid.y limit on N).
__global__ void __launch_bounds__(256) traj_transpose_kernel(const int4* __restrict__ in, int4* __restrict__ out,
                                                             int64_t N, int64_t T, int64_t t0, int64_t tc) {
  __shared__ int4 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t ntn = (N + 31) / 32;
  const int64_t tb = (int64_t)blockIdx.x / ntn * 32, n0 = (int64_t)blockIdx.x % ntn * 32;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int64_t n = n0 + ty + k, t = tb + tx;
    if (n < N && t < tc) tile[ty + k][tx] = in[n * T + t0 + t];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int64_t t = tb + ty + k, n = n0 + tx;
    if (n < N && t < tc) out[t * N + n] = tile[tx][ty + k];
  }
}

hipError_t launch_traj_transpose(const ccka_traj_rec* in, ccka_traj_rec* out, int64_t N, int64_t T, int64_t t0,
                                 int64_t tc, hipStream_t s) {
  const int64_t blocks = (N + 31) / 32 * ((tc + 31) / 32);
  if (blocks <= 0) return hipSuccess;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(traj_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                     reinterpret_cast<const int4*>(in), reinterpret_cast<int4*>(out), N, T, t0, tc);
  return hipGetLastError();
}

// [T][N] load trace -> wave-tiled [wave][T][lpw] (the single-deployment
// kernels' read layout: a wave's rows contiguous, every row lpw wide, the last
// wave's padded: one row stride for all), once per trace / lanes-per-wave
// change (abi_rollout.cpp d1_trace_tile); reads coalesced, writes in runs of lpw ints.
__global__ void __launch_bounds__(256) trace_tile_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                         int64_t N, int64_t T, int64_t lpw) {
  const int64_t total = N * T, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const int64_t t = x / N, n = x - t * N;
    const int64_t w0 = n / lpw * lpw;
    out[w0 * T + t * lpw + (n - w0)] = in[x];
  }
}

hipError_t launch_trace_tile(const int32_t* in, int32_t* out, int64_t N, int64_t T, int32_t lpw, hipStream_t s) {
  if (N <= 0 || T <= 0 || lpw <= 0) return hipErrorInvalidValue;
  const int64_t b0 = (N * T + 255) / 256, blocks = b0 < 65536 ? b0 : 65536;
  hipLaunchKernelGGL(trace_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, out, N, T, (int64_t)lpw);
  return hipGetLastError();
}

}  // namespace ccka
