// boot.hip — paired bootstrap (SEMANTICS 9): the per-position deltas of the
// paired comparison resampled with replacement, B times, and the B replicate
// sums of every grid reduced to order statistics and sign counts. The indices
// of replicate r come from Philox keyed by the seed and depend on neither the
// grid nor the objective, so one draw serves the four objectives of every grid
// of a tile. Only integers are summed and selected: every field is exact in any
// order.
//
//   boot_delta_kernel   one thread per (grid slot, position): the four deltas,
//                       formed as paired_kernel forms them, as one 32-byte
//                       record of delta[tile][position][slot][objective]
//   boot_sums_kernel    one workgroup per (tile of K grids, chunk of
//                       replicates), one wave per replicate: a lane's Philox
//                       call gives four indices; per index and grid two 16-byte
//                       reads of the record (from LDS up to the staging limit,
//                       else from the L2-resident delta array) and four 64-bit
//                       adds; a halving butterfly leaves each of the 4K sums in
//                       its own lane, which stores it
//   boot_select_kernel  one workgroup per grid, in paired_kernel's structure:
//                       sign and dominance counts over the replicates and the
//                       observed sums over the positions, then wave o selects
//                       lo and hi among objective o's sums (select_dev.h)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "kparams.h"
#include "paired_dev.h"
#include "select_dev.h"

#pragma clang fp contract(off)

namespace ccka {

static_assert(sizeof(ccka_boot_spec) == 40 && sizeof(ccka_boot_obj) == 40 && sizeof(ccka_boot_row) == 208,
              "paired bootstrap ABI layout");

constexpr uint32_t kBootTag = 0xB0075EEDu;  // counter word 3 of every resampling call
// 32-byte records a staged workgroup of tile width K holds: kBootStage positions
// of K grids (32 KiB per grid), 128 KiB at the most
constexpr int boot_recs(int K) { return K * kBootStage <= 4096 ? K * kBootStage : 4096; }
static_assert(boot_recs(kBootTile) == kBootTile * kBootStage, "the default tile fits the staged records");

__global__ void __launch_bounds__(256) boot_delta_kernel(BootParams p) {
  const int64_t n = p.cur.grid_size;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t slots = (p.gp + p.K - 1) / p.K * p.K;
  if (idx >= slots * n) return;
  const int64_t slot = idx / n, pos = idx - slot * n;  // position fastest: the columns are read coalesced
  long long d[4] = {0, 0, 0, 0}, ovf = 0;
  if (slot < p.gp) {
    const int64_t grid = p.g0 + slot;
    const int64_t lo = grid * n + pos, bo = p.base_off + grid * p.base_step + pos;
#pragma unroll
    for (int o = 0; o < 4; ++o) d[o] = sub_chk(paired_value(p.cur, o, lo, ovf), p.snap[o * p.snap_n + bo], ovf);
  }
  const int64_t tile = slot / p.K, k = slot - tile * p.K;
  longlong2* rec = (longlong2*)p.delta + ((tile * n + pos) * p.K + k) * 2;
  rec[0] = make_longlong2(d[0], d[1]);
  rec[1] = make_longlong2(d[2], d[3]);
  if (ovf) atomicOr(p.flag, 1u);
}

// The K records of position j added to the 4K running sums (wrapping like
// int64). In the delta array a position's 2K 16-byte halves are contiguous
// (one draw touches 32 K bytes of one or two cache lines): stride 1, position
// pitch 2K. In LDS half h of every position is an array of its own: stride n,
// position pitch 1. By the bank rule of ds_read_b128 ((a / 4) % 64, 16 lanes
// per group) the lanes of a group, at random positions of one half, can then
// reach all 16 bank quads ((a / 16) % 16 = (h n + j) % 16); a 128-byte record
// pitch (K = 4) would leave them two. No bank-conflict counter was collected;
// DESIGN.md has the time of an earlier build that kept the record pitch.
template <int K>
__device__ __forceinline__ void boot_draw(const ulonglong2* rec, size_t at, size_t stride,
                                          unsigned long long (&a)[4 * K]) {
  const ulonglong2* r = rec + at;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const ulonglong2 x = r[(2 * k) * stride], y = r[(2 * k + 1) * stride];
    a[4 * k] += x.x;
    a[4 * k + 1] += x.y;
    a[4 * k + 2] += y.x;
    a[4 * k + 3] += y.y;
  }
}

// The 64 lanes' NV running sums added up. Each of the first log2(NV) steps
// halves the values a lane carries: the lane keeps one half and hands the other
// to its partner, so NV - 1 exchanges do what 6 NV would in a tree per value.
// Afterwards value v is complete in the lanes l with l >> (6 - log2 NV) == v.
template <int HALF, int NV>
__device__ __forceinline__ void boot_halve(unsigned long long (&a)[NV], int lane) {
  if constexpr (HALF >= 1) {
    constexpr int m = 64 * HALF / NV;  // 32, 16, ...
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const unsigned long long send = up ? a[i] : a[i + HALF];
      const unsigned long long keep = up ? a[i + HALF] : a[i];
      a[i] = keep + __shfl_xor(send, m);
    }
    boot_halve<HALF / 2, NV>(a, lane);
  }
}

template <int NV>
__device__ __forceinline__ unsigned long long boot_reduce(unsigned long long (&a)[NV], int lane) {
  static_assert(NV >= 2 && NV <= 32 && (NV & (NV - 1)) == 0, "a power of two of values");
  boot_halve<NV / 2, NV>(a, lane);
#pragma unroll
  for (int m = 32 / NV; m >= 1; m >>= 1) a[0] += __shfl_xor(a[0], m);
  return a[0];
}

template <int K, bool STAGED>
__global__ void __launch_bounds__(STAGED ? kBootStagedThreads : 256) boot_sums_kernel(BootParams p) {
  __shared__ ulonglong2 s_rec[STAGED ? 2 * boot_recs(K) : 1];  // [half 0 .. 2K)[position]
  constexpr int NV = 4 * K;
  constexpr int kShift = 6 - (K == 1 ? 2 : K == 2 ? 3 : K == 4 ? 4 : 5);  // 6 - log2 NV
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = (int)(blockDim.x >> 6);
  const int64_t n = p.cur.grid_size;
  const int64_t tile = blockIdx.x / (unsigned)p.chunks;
  const int chunk = (int)(blockIdx.x - tile * p.chunks);
  const ulonglong2* rec = (const ulonglong2*)p.delta + tile * n * (2 * K);
  if constexpr (STAGED) {
    if (n * K > boot_recs(K)) return;  // the launcher stages only what fits
    for (int i = tid; i < (int)n * 2 * K; i += (int)blockDim.x) {
      const int pos = i / (2 * K), h = i - pos * (2 * K);
      s_rec[h * (int)n + pos] = rec[i];
    }
    __syncthreads();
  }
  const uint32_t un = (uint32_t)n;  // n <= 2^31
  const int64_t full = n >> 2;      // Philox calls whose four words are all used
  const int rem = (int)(n & 3);
  const int r_end = min(p.B, (chunk + 1) * p.per_chunk);
  for (int r = chunk * p.per_chunk + wave; r < r_end; r += waves) {
    unsigned long long a[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) a[v] = 0;
    for (int64_t c = lane; c < full; c += 64) {
      uint32_t w[4];
      philox((uint32_t)c, (uint32_t)r, 0u, kBootTag, p.k0, p.k1, w);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t j = __umulhi(w[t], un);  // (w n) div 2^32
        if constexpr (STAGED) boot_draw<K>(s_rec, j, (size_t)n, a);
        else boot_draw<K>(rec, (size_t)j * (2 * K), 1, a);
      }
    }
    if (rem && lane == 0) {  // the last call: its words past n are discarded
      uint32_t w[4];
      philox((uint32_t)full, (uint32_t)r, 0u, kBootTag, p.k0, p.k1, w);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (t < rem) {
          const uint32_t j = __umulhi(w[t], un);
          if constexpr (STAGED) boot_draw<K>(s_rec, j, (size_t)n, a);
          else boot_draw<K>(rec, (size_t)j * (2 * K), 1, a);
        }
      }
    }
    const unsigned long long total = boot_reduce<NV>(a, lane);
    if ((lane & ((1 << kShift) - 1)) == 0) {
      const int v = lane >> kShift;  // slot v / 4 of the tile, objective v % 4
      const int64_t gl = tile * K + (v >> 2);
      if (gl < p.gp) p.sums[(gl * 4 + (v & 3)) * p.B + r] = (int64_t)total;
    }
  }
}

__global__ void __launch_bounds__(256) boot_select_kernel(BootParams p) {
  __shared__ uint64_t s_key[4][kSelLds];
  __shared__ uint32_t s_hist[4][256];
  __shared__ unsigned long long s_sum[4][4];  // [wave][objective]
  __shared__ uint32_t s_less[4][4], s_greater[4][4], s_dom[4][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t gl = blockIdx.x;  // the grid inside the pass
  const int64_t n = p.cur.grid_size, B = p.B;
  const int64_t* S = p.sums + gl * 4 * B;
  const bool staged = B <= kSelLds;

  // ---- pass A: all four waves stride the replicates, then the positions ----
  uint32_t less[4] = {0, 0, 0, 0}, greater[4] = {0, 0, 0, 0}, dom = 0, domd = 0;
  for (int64_t r = tid; r < B; r += 256) {
    long long s[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      s[o] = S[o * B + r];
      less[o] += s[o] < 0;
      greater[o] += s[o] > 0;
      if (staged) s_key[o][r] = key_i64(s[o]);
    }
    // the frontier's three objectives: cost, gCO2, SLO minutes
    const bool le = s[0] <= 0 && s[2] <= 0 && s[1] <= 0, lt = s[0] < 0 || s[2] < 0 || s[1] < 0;
    const bool ge = s[0] >= 0 && s[2] >= 0 && s[1] >= 0, gt = s[0] > 0 || s[2] > 0 || s[1] > 0;
    dom += le && lt;
    domd += ge && gt;
  }
  unsigned long long sum[4] = {0, 0, 0, 0};  // the observed sums, wrapping like int64
  const int64_t tile = gl / p.K, k = gl - tile * p.K;
  const ulonglong2* rec = (const ulonglong2*)p.delta + (tile * n * p.K + k) * 2;
  for (int64_t i = tid; i < n; i += 256) {
    const ulonglong2 x = rec[i * p.K * 2], y = rec[i * p.K * 2 + 1];
    sum[0] += x.x;
    sum[1] += x.y;
    sum[2] += y.x;
    sum[3] += y.y;
  }
  for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      sum[o] += __shfl_down(sum[o], s);
      less[o] += __shfl_down(less[o], s);
      greater[o] += __shfl_down(greater[o], s);
    }
    dom += __shfl_down(dom, s);
    domd += __shfl_down(domd, s);
  }
  if (lane == 0) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      s_sum[wave][o] = sum[o];
      s_less[wave][o] = less[o];
      s_greater[wave][o] = greater[o];
    }
    s_dom[wave][0] = dom;
    s_dom[wave][1] = domd;
  }
  __syncthreads();  // the partials and the staged keys of every wave

  // ---- pass B: wave o selects lo and hi among objective o's sums ----
  const int obj = wave;
  const uint64_t* keys = s_key[obj];
  const int64_t* So = S + obj * B;
  const auto key_at = [&](int64_t i) { return staged ? keys[i] : key_i64(So[i]); };
  const uint64_t klo = wave_radix_select(B, (uint64_t)p.rank_lo, s_hist[obj], lane, key_at);
  const uint64_t khi =
      p.rank_hi == p.rank_lo ? klo : wave_radix_select(B, (uint64_t)p.rank_hi, s_hist[obj], lane, key_at);
  if (lane == 0) {
    ccka_boot_row* row = p.rows + p.g0 + gl;
    ccka_boot_obj r;
    r.sum = (int64_t)(s_sum[0][obj] + s_sum[1][obj] + s_sum[2][obj] + s_sum[3][obj]);
    r.lo = unkey_i64(klo);
    r.hi = unkey_i64(khi);
    r.n_less = (int64_t)s_less[0][obj] + s_less[1][obj] + s_less[2][obj] + s_less[3][obj];
    r.n_greater = (int64_t)s_greater[0][obj] + s_greater[1][obj] + s_greater[2][obj] + s_greater[3][obj];
    row->obj[obj] = r;
    if (obj == 0) {
      const int64_t g = p.g0 + gl;
      row->grid = p.cur.first_grid + g;
      row->base = p.base_grid + (p.base_step ? g : 0);
      row->pairs = n;
      row->replicates = B;
      row->n_dominates = (int64_t)s_dom[0][0] + s_dom[1][0] + s_dom[2][0] + s_dom[3][0];
      row->n_dominated = (int64_t)s_dom[0][1] + s_dom[1][1] + s_dom[2][1] + s_dom[3][1];
    }
  }
}

bool boot_config_ok(int K, int L) {
  if (L < 0) return false;
  switch (K) {
    case 1: return L <= boot_recs(1);
    case 2: return 2 * L <= boot_recs(2);
    case 4: return 4 * L <= boot_recs(4);
    case 8: return 8 * L <= boot_recs(8);
    default: return false;
  }
}

// the launch rules every kernel of a pass shares
static bool boot_pass_ok(const BootParams& p) {
  return boot_config_ok(p.K, p.L) && p.gp >= 1 && p.g0 >= 0 && p.g0 + p.gp <= p.cur.n_grids && p.B >= 1 &&
         p.B <= kBootMaxReplicates && p.cur.grid_size >= 1 && p.cur.grid_size <= ((int64_t)1 << 31);
}

hipError_t launch_boot_delta(const BootParams& p, hipStream_t s) {
  if (!boot_pass_ok(p)) return hipErrorInvalidValue;
  const int64_t slots = (p.gp + p.K - 1) / p.K * p.K;
  const int64_t blocks = (slots * p.cur.grid_size + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_delta_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <int K>
static void boot_sums_launch(const BootParams& p, unsigned blocks, bool staged, hipStream_t s) {
  if (staged) hipLaunchKernelGGL((boot_sums_kernel<K, true>), dim3(blocks), dim3(kBootStagedThreads), 0, s, p);
  else hipLaunchKernelGGL((boot_sums_kernel<K, false>), dim3(blocks), dim3(256), 0, s, p);
}

hipError_t launch_boot_sums(const BootParams& p, hipStream_t s) {
  if (!boot_pass_ok(p) || p.chunks < 1 || p.per_chunk < 1 || (int64_t)p.chunks * p.per_chunk < p.B)
    return hipErrorInvalidValue;
  const int64_t blocks = (p.gp + p.K - 1) / p.K * p.chunks;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const bool staged = p.cur.grid_size <= p.L;  // K L <= boot_recs(K): the tile's records fit
  switch (p.K) {
    case 1: boot_sums_launch<1>(p, (unsigned)blocks, staged, s); break;
    case 2: boot_sums_launch<2>(p, (unsigned)blocks, staged, s); break;
    case 4: boot_sums_launch<4>(p, (unsigned)blocks, staged, s); break;
    default: boot_sums_launch<8>(p, (unsigned)blocks, staged, s); break;
  }
  return hipGetLastError();
}

hipError_t launch_boot_select(const BootParams& p, hipStream_t s) {
  if (!boot_pass_ok(p) || p.gp > (1 << 24) || p.rank_lo < 1 || p.rank_hi < p.rank_lo || p.rank_hi > p.B)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_select_kernel, dim3((unsigned)p.gp), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace ccka
