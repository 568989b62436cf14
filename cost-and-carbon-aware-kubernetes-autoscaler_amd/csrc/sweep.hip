// sweep.hip — BASELINE config 4: policy sweep of parameter grids over shared
// load traces. Per-grid sums of the rollout results (fixed-order, so
// deterministic) and the cost / gCO2 / SLO-minutes Pareto frontier
// (local non-dominated candidates, exchanged with an RCCL
// all-gather in abi_sweep.cpp, then the same filter on every rank).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"
#include "select_dev.h"

namespace ccka {

// one workgroup per grid: strided partial sums in a fixed order, then a
// fixed-shape tree over the workgroup
__global__ void __launch_bounds__(256) grid_stats_kernel(GridSrc g, ccka_grid_stats* out) {
  __shared__ long long s_cost[256], s_slo[256];
  __shared__ double s_g[256], s_e[256];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * g.grid_size;
  long long c = 0, sl = 0;
  double gc = 0.0, en = 0.0;
  for (int64_t k = tid; k < g.grid_size; k += blockDim.x) {
    c += g.cost[lo + k];
    sl += g.slo[lo + k];
    gc += g.gco2[lo + k];
    en += g.energy[lo + k];
  }
  s_cost[tid] = c;
  s_slo[tid] = sl;
  s_g[tid] = gc;
  s_e[tid] = en;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_cost[tid] += s_cost[tid + w];
      s_slo[tid] += s_slo[tid + w];
      s_g[tid] += s_g[tid + w];
      s_e[tid] += s_e[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    ccka_grid_stats o;
    o.grid = g.first_grid + blockIdx.x;
    o.scenarios = g.grid_size;
    o.cost_uphmin = s_cost[0];
    o.slo_minutes = s_slo[0];
    o.gco2 = s_g[0];
    o.energy_wmin = s_e[0];
    out[blockIdx.x] = o;
  }
}

// ---------------------------------------------------------------------------
// Per-grid order statistics (SEMANTICS 6): the rank-k value of an objective
// over the grid, and the sum of the values from rank k up. One workgroup per
// grid, one wave per objective (cost, SLO minutes, gCO2, energy), so the four
// selections run side by side and a wave only ever synchronises with itself.
// The selection is an MSB-first radix select (8 passes of 8 bits) over
// order-preserving 64-bit keys: no sort, no global atomics, exact for doubles
// (the result is an input element). Each pass histograms the digit of the
// keys that match the prefix found so far (LDS counters private to the wave)
// and a 64-lane scan picks the digit that holds the rank. Grids of up to
// kSelLds scenarios keep their keys in LDS (4 x 8 KiB); larger ones re-read
// the columns (L2-resident at sweep sizes). SUM objectives are left alone:
// grid_stats_kernel has written them. The pass loop is select_dev.h's, which
// paired_kernel (paired.hip) runs over its deltas too.
// ---------------------------------------------------------------------------
// binary64 by value: negatives flip every bit, the rest flip the sign bit
__device__ __forceinline__ uint64_t key_f64(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b ^ kSignBit;
}
__device__ __forceinline__ double unkey_f64(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ kSignBit : ~k));
}

__device__ __forceinline__ uint64_t sel_load_key(const GridSrc& g, int obj, int64_t idx) {
  switch (obj) {
    case 0: return key_i64(g.cost[idx]);
    case 1: return key_i64((int64_t)g.slo[idx]);
    case 2: return key_f64(g.gco2[idx]);
    default: return key_f64(g.energy[idx]);
  }
}

__global__ void __launch_bounds__(256) grid_select_kernel(GridSel q, ccka_grid_stats* out) {
  __shared__ uint64_t s_key[4][kSelLds];
  __shared__ uint32_t s_hist[4][256];
  const int obj = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int kind = q.kind[obj];
  if (kind == CCKA_STAT_SUM) return;  // the whole wave
  const GridSrc& g = q.g;
  const int64_t n = g.grid_size;
  const int64_t lo = (int64_t)blockIdx.x * n;
  const bool staged = n <= kSelLds;
  uint64_t* keys = s_key[obj];
  if (staged)
    for (int64_t i = lane; i < n; i += 64) keys[i] = sel_load_key(g, obj, lo + i);
  const auto key_at = [&](int64_t i) { return staged ? keys[i] : sel_load_key(g, obj, lo + i); };

  // the pass loop (select_dev.h): prefix is the key of x(k)
  const uint64_t prefix = wave_radix_select(n, (uint64_t)q.rank[obj], s_hist[obj], lane, key_at);

  int64_t ri = unkey_i64(prefix);
  double rd = unkey_f64(prefix);
  if (kind == CCKA_STAT_TAIL) {
    // values above x(k) in lane-strided index order, then a fixed tree; the
    // ties with x(k) enter as one product (SEMANTICS 6)
    const int64_t terms = n - q.rank[obj] + 1;
    if (obj < 2) {
      ri = wave_tail_i64(n, terms, prefix, lane, key_at);
    } else {
      uint32_t gt = 0;
      double acc = 0.0;
      for (int64_t i = lane; i < n; i += 64) {
        const double v = unkey_f64(key_at(i));
        if (v > rd) { acc += v; ++gt; }
      }
      for (int d = 32; d > 0; d >>= 1) {
        acc += __shfl_down(acc, d);
        gt += __shfl_down(gt, d);
      }
      rd = acc + (double)(terms - (int64_t)gt) * rd;
    }
  }
  if (lane == 0) {
    ccka_grid_stats* o = out + blockIdx.x;
    switch (obj) {
      case 0: o->cost_uphmin = ri; break;
      case 1: o->slo_minutes = ri; break;
      case 2: o->gco2 = rd; break;
      default: o->energy_wmin = rd; break;
    }
  }
}

__device__ __forceinline__ bool dominates(const ccka_grid_stats& a, const ccka_grid_stats& b) {
  const bool le = a.cost_uphmin <= b.cost_uphmin && a.gco2 <= b.gco2 && a.slo_minutes <= b.slo_minutes;
  const bool lt = a.cost_uphmin < b.cost_uphmin || a.gco2 < b.gco2 || a.slo_minutes < b.slo_minutes;
  return le && lt;
}

// flags[i] = 1 iff entry i is dominated by any other entry (one thread per entry)
__global__ void __launch_bounds__(256) pareto_mark_kernel(const ccka_grid_stats* in, int n_host,
                                                          const int32_t* n_dev, uint8_t* flags) {
  const int n = n_dev ? *n_dev : n_host;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ccka_grid_stats me = in[i];
  uint8_t dom = 0;
  for (int j = 0; j < n && !dom; ++j)
    if (j != i && dominates(in[j], me)) dom = 1;
  flags[i] = dom;
}

// ordered compaction of the non-dominated entries (one workgroup, block scan)
__global__ void __launch_bounds__(1024) pareto_compact_kernel(const ccka_grid_stats* in, int n_host,
                                                              const int32_t* n_dev, const uint8_t* flags,
                                                              ccka_grid_stats* out, int32_t* count) {
  __shared__ int s_scan[1024];
  __shared__ int s_base;
  const int n = n_dev ? *n_dev : n_host;
  const int tid = threadIdx.x;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int base = 0; base < n; base += blockDim.x) {
    const int i = base + tid;
    const int keep = (i < n && !flags[i]) ? 1 : 0;
    s_scan[tid] = keep;
    __syncthreads();
    for (int off = 1; off < (int)blockDim.x; off <<= 1) {  // inclusive Hillis-Steele scan
      const int v = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    if (keep) out[s_base + s_scan[tid] - 1] = in[i];
    __syncthreads();
    if (tid == blockDim.x - 1) s_base += s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) *count = s_base;
}

// valid prefixes of the all-gathered [ranks][cap] buffers, in rank order
// (ranks own ascending grid ranges, so the union stays sorted by grid id)
__global__ void __launch_bounds__(256) pareto_union_kernel(const ccka_grid_stats* gathered, const int64_t* counts,
                                                           int ranks, int cap, ccka_grid_stats* out, int32_t* n_dev) {
  int off = 0;
  for (int q = 0; q < ranks; ++q) {
    const int c = (int)counts[q];
    for (int k = threadIdx.x; k < c; k += blockDim.x) out[off + k] = gathered[(int64_t)q * cap + k];
    off += c;
  }
  if (threadIdx.x == 0) *n_dev = off;
}

hipError_t launch_grid_stats(const GridSrc& g, ccka_grid_stats* out, hipStream_t s) {
  hipLaunchKernelGGL(grid_stats_kernel, dim3((unsigned)g.n_grids), dim3(256), 0, s, g, out);
  return hipGetLastError();
}

hipError_t launch_grid_select(const GridSel& q, ccka_grid_stats* out, hipStream_t s) {
  hipLaunchKernelGGL(grid_select_kernel, dim3((unsigned)q.g.n_grids), dim3(256), 0, s, q, out);
  return hipGetLastError();
}

hipError_t launch_pareto(const ccka_grid_stats* in, int n, const int32_t* n_dev, uint8_t* flags,
                         ccka_grid_stats* out, int32_t* count_dev, hipStream_t s) {
  // n is the capacity bound when the live count is device-resident
  hipLaunchKernelGGL(pareto_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n, n_dev, flags);
  hipLaunchKernelGGL(pareto_compact_kernel, dim3(1), dim3(1024), 0, s, in, n, n_dev, flags, out, count_dev);
  return hipGetLastError();
}

hipError_t launch_pareto_union(const ccka_grid_stats* gathered, const int64_t* counts, int ranks, int cap,
                               ccka_grid_stats* out, int32_t* n_dev, hipStream_t s) {
  hipLaunchKernelGGL(pareto_union_kernel, dim3(1), dim3(256), 0, s, gathered, counts, ranks, cap, out, n_dev);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Copy ceiling (bench.py's roofline denominator beside the 8 TB/s peak): a
// plain streaming device copy, 16 bytes per lane (dwordx4), one element per
// thread with the grid covering the buffer, nontemporal on both sides. The
// fastest of the variants tools/probe/copyprobe.hip measured on MI355X (6.5
// TB/s read + write; grid-stride loops with 4-8 accesses in flight per lane:
// 4.4-4.8 TB/s). Profiling aid, not part of the rollout.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) copy16_kernel(const int4* __restrict__ in, int4* __restrict__ out, int64_t n) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load((const i32x4*)(in + i)), (i32x4*)(out + i));
}

hipError_t launch_copy16(const void* in, void* out, int64_t bytes, int cus, hipStream_t s) {
  (void)cus;
  const int64_t n = bytes / 16;
  const int64_t grid = (n + 255) / 256;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const int4*)in, (int4*)out, n);
  return hipGetLastError();
}

}  // namespace ccka
