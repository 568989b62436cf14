// paired.hip — paired comparison (SEMANTICS 8): a sweep's grids all read the
// same shared traces, so position j of two grids is a matched pair. The
// results of a batch are kept as integer vectors (cost, SLO minutes, gCO2 and
// energy in fixed point: the totals' llrint(x * 1e6)), and a later batch is
// reduced per grid over the per-position deltas against a baseline grid of
// that snapshot. Only integers are reduced, so sums, counts, extrema and order
// statistics are exact in any order.
//
//   paired_capture_kernel   one thread per scenario: the four result columns
//                           as [4][N] int64
//   paired_kernel           one workgroup per current grid: one streaming pass
//                           (sums, extrema, sign and dominance counts, keys
//                           staged in LDS), then one wave per objective runs
//                           the radix select of select_dev.h over the deltas
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "kparams.h"
#include "paired_dev.h"
#include "select_dev.h"

#pragma clang fp contract(off)

namespace ccka {

static_assert(sizeof(ccka_paired_spec) == 48 && sizeof(ccka_paired_obj) == 48 && sizeof(ccka_paired_row) == 232,
              "paired comparison ABI layout");

__global__ void __launch_bounds__(256) paired_capture_kernel(GridSrc g, int64_t n, int64_t* __restrict__ snap,
                                                             uint32_t* flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long ovf = 0;
#pragma unroll
  for (int o = 0; o < 4; ++o) snap[o * n + i] = paired_value(g, o, i, ovf);
  if (ovf) atomicOr(flag, 1u);
}

// one lane's running reduction of one objective's deltas
struct PairAcc {
  unsigned long long sum = 0;  // wraps like int64
  long long mn = INT64_MAX, mx = INT64_MIN;
  uint32_t less = 0, greater = 0;  // a grid holds at most 2^31 positions
  __device__ __forceinline__ void add(long long d) {
    sum += (unsigned long long)d;
    mn = min(mn, d);
    mx = max(mx, d);
    less += d < 0;
    greater += d > 0;
  }
};

__global__ void __launch_bounds__(256) paired_kernel(PairedParams p) {
  __shared__ uint64_t s_key[4][kSelLds];
  __shared__ uint32_t s_hist[4][256];
  __shared__ unsigned long long s_sum[4][4];  // [wave][objective]
  __shared__ long long s_min[4][4], s_max[4][4];
  __shared__ uint32_t s_less[4][4], s_greater[4][4], s_dom[4][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const GridSrc& g = p.cur;
  const int64_t n = g.grid_size;
  const int64_t lo = (int64_t)blockIdx.x * n;                       // position 0 in the current columns
  const int64_t bo = p.base_off + (int64_t)blockIdx.x * p.base_step;  // and in the snapshot's
  const bool staged = n <= kSelLds;

  // ---- pass A: all four waves stride the positions ----
  PairAcc a[4];
  uint32_t dom = 0, domd = 0;
  long long ovf = 0;
  for (int64_t i = tid; i < n; i += 256) {
    long long d[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) d[o] = sub_chk(paired_value(g, o, lo + i, ovf), p.snap[o * p.snap_n + bo + i], ovf);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      a[o].add(d[o]);
      if (staged && p.kind[o] != CCKA_STAT_SUM) s_key[o][i] = key_i64(d[o]);
    }
    // the frontier's three objectives: cost, gCO2, SLO minutes
    const bool le = d[0] <= 0 && d[2] <= 0 && d[1] <= 0, lt = d[0] < 0 || d[2] < 0 || d[1] < 0;
    const bool ge = d[0] >= 0 && d[2] >= 0 && d[1] >= 0, gt = d[0] > 0 || d[2] > 0 || d[1] > 0;
    dom += le && lt;
    domd += ge && gt;
  }
  if (ovf) atomicOr(p.flag, 1u);
  for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      a[o].sum += __shfl_down(a[o].sum, s);
      a[o].mn = min(a[o].mn, __shfl_down(a[o].mn, s));
      a[o].mx = max(a[o].mx, __shfl_down(a[o].mx, s));
      a[o].less += __shfl_down(a[o].less, s);
      a[o].greater += __shfl_down(a[o].greater, s);
    }
    dom += __shfl_down(dom, s);
    domd += __shfl_down(domd, s);
  }
  if (lane == 0) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      s_sum[wave][o] = a[o].sum;
      s_min[wave][o] = a[o].mn;
      s_max[wave][o] = a[o].mx;
      s_less[wave][o] = a[o].less;
      s_greater[wave][o] = a[o].greater;
    }
    s_dom[wave][0] = dom;
    s_dom[wave][1] = domd;
  }
  __syncthreads();  // the partials and the staged keys of every wave

  // ---- pass B: wave o selects over objective o's deltas ----
  const int obj = wave;
  const int kind = p.kind[obj];
  long long qv = 0;
  if (kind != CCKA_STAT_SUM) {
    const uint64_t* keys = s_key[obj];
    const auto key_at = [&](int64_t i) {
      if (staged) return keys[i];
      long long unused = 0;  // pass A has flagged what this recomputation would
      const unsigned long long v = (unsigned long long)paired_value(g, obj, lo + i, unused);
      return key_i64((int64_t)(v - (unsigned long long)p.snap[obj * p.snap_n + bo + i]));
    };
    const uint64_t kx = wave_radix_select(n, (uint64_t)p.rank[obj], s_hist[obj], lane, key_at);
    qv = unkey_i64(kx);
    if (kind == CCKA_STAT_TAIL) qv = wave_tail_i64(n, n - p.rank[obj] + 1, kx, lane, key_at);
  }
  if (lane == 0) {
    ccka_paired_row* row = p.rows + blockIdx.x;
    ccka_paired_obj r;
    r.sum = (int64_t)(s_sum[0][obj] + s_sum[1][obj] + s_sum[2][obj] + s_sum[3][obj]);
    r.min = min(min(s_min[0][obj], s_min[1][obj]), min(s_min[2][obj], s_min[3][obj]));
    r.max = max(max(s_max[0][obj], s_max[1][obj]), max(s_max[2][obj], s_max[3][obj]));
    r.q_value = qv;
    r.n_less = (int64_t)s_less[0][obj] + s_less[1][obj] + s_less[2][obj] + s_less[3][obj];
    r.n_greater = (int64_t)s_greater[0][obj] + s_greater[1][obj] + s_greater[2][obj] + s_greater[3][obj];
    row->obj[obj] = r;
    if (obj == 0) {
      row->grid = g.first_grid + blockIdx.x;
      row->base = p.base_grid + (p.base_step ? (int64_t)blockIdx.x : 0);
      row->pairs = n;
      row->n_dominates = (int64_t)s_dom[0][0] + s_dom[1][0] + s_dom[2][0] + s_dom[3][0];
      row->n_dominated = (int64_t)s_dom[0][1] + s_dom[1][1] + s_dom[2][1] + s_dom[3][1];
    }
  }
}

hipError_t launch_paired_capture(const GridSrc& src, int64_t n, int64_t* snap, uint32_t* flag, hipStream_t s) {
  const int64_t blocks = (n + 255) / 256;
  if (n < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(paired_capture_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, n, snap, flag);
  return hipGetLastError();
}

hipError_t launch_paired(const PairedParams& p, hipStream_t s) {
  if (p.cur.n_grids < 1 || p.cur.n_grids > (1 << 24)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(paired_kernel, dim3((unsigned)p.cur.n_grids), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace ccka
