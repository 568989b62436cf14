// timeline.hip — fleet timeline (SEMANTICS 7): the trajectory records of a
// rollout reduced per (grid, step bucket) without leaving the device. Every
// field of a record is an integer, so sums, counts and extrema are exact in
// any order: workgroups reduce what they read on chip (registers, cross-lane,
// LDS) and combine across workgroups with integer atomics on rows that
// timeline_init_kernel has re-initialised for this call.
//
//   timeline_sum_kernel<NT>   one streaming read of the records ([N][T] or
//                             [T][N]): sums, flag counts, extrema
//   timeline_select_kernel    q_field != NONE: the nearest-rank quantile of
//                             one field per row, an MSB-first radix select
//                             (4 passes of 8 bits, as grid_select_kernel)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"

namespace ccka {

static_assert(sizeof(ccka_traj_rec) == 16 && sizeof(ccka_timeline_row) == 144, "timeline record / row layout");

// How a launch maps its work items onto workgroups of 256 threads (host-side
// choice: the launchers below). lanes = consecutive lanes that read consecutive
// records (a power of two): steps of one scenario in [N][T], scenarios of one
// step in [T][N].
struct TlGeom {
  int64_t items;      // work items (workgroups stride over them)
  int64_t slice_len;  // scenarios of a grid per item (sum kernels)
  int32_t lanes;      // [N][T]: <= 64 (<= 32 in the select); [T][N]: <= 256
  int32_t n_tiles;    // [N][T] sum: step tiles of `lanes` steps. Select: bucket groups per grid
  int32_t n_slices;   // scenario slices per grid (sum kernels)
  int32_t nbk;        // [N][T] select: buckets per item
};

// one thread's running reduction of the records it read
struct TlAcc {
  long long rep = 0, pend = 0, spot = 0, od = 0;
  uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // a row holds at most 2^31 samples
  int mx_rep = INT32_MIN, mx_pend = INT32_MIN, mx_nodes = INT32_MIN, mn_nodes = INT32_MAX;
  __device__ __forceinline__ void add(const int4& r) {
    const int s = r.z & 0xffff, o = (int)((uint32_t)r.z >> 16);
    const uint32_t f = (uint32_t)r.w >> 16;  // last_type is the low half
    rep += r.x;
    pend += r.y;
    spot += s;
    od += o;
#pragma unroll
    for (int b = 0; b < 8; ++b) cnt[b] += (f >> b) & 1u;
    mx_rep = max(mx_rep, r.x);
    mx_pend = max(mx_pend, r.y);
    mx_nodes = max(mx_nodes, s + o);
    mn_nodes = min(mn_nodes, s + o);
  }
};

__device__ __forceinline__ int4 tl_load(const ccka_traj_rec* recs, int64_t idx) {
  return *reinterpret_cast<const int4*>(recs + idx);
}

// a reduced partial into its row; zero sums and neutral extrema are left out
// (the flag counts of quiet buckets are mostly zero)
__device__ __forceinline__ void tl_row_add(unsigned long long* field, unsigned long long v) {
  if (v) atomicAdd(field, v);
}
__device__ __forceinline__ void tl_flush(ccka_timeline_row* row, const unsigned long long sum[4],
                                         const unsigned long long cnt[8], int mx_rep, int mx_pend, int mx_nodes,
                                         int mn_nodes) {
  tl_row_add((unsigned long long*)&row->sum_replicas, sum[0]);
  tl_row_add((unsigned long long*)&row->sum_pending, sum[1]);
  tl_row_add((unsigned long long*)&row->sum_nodes_spot, sum[2]);
  tl_row_add((unsigned long long*)&row->sum_nodes_od, sum[3]);
#pragma unroll
  for (int b = 0; b < 8; ++b) tl_row_add((unsigned long long*)&row->flag_count[b], cnt[b]);
  if (mx_rep != INT32_MIN) atomicMax(&row->max_replicas, mx_rep);
  if (mx_pend != INT32_MIN) atomicMax(&row->max_pending, mx_pend);
  if (mx_nodes != INT32_MIN) atomicMax(&row->max_nodes, mx_nodes);
  if (mn_nodes != INT32_MAX) atomicMin(&row->min_nodes, mn_nodes);
}

// rows as an empty reduction: ids and sample counts final, sums and counts 0,
// extrema neutral. Runs on every call: the buffer outlives the spec.
__global__ void __launch_bounds__(256) timeline_init_kernel(TimelineParams p) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.n_grids * p.n_buckets) return;
  const int64_t g = r / p.n_buckets, b = r % p.n_buckets;
  const int64_t t0 = b * p.B, t1 = min(t0 + (int64_t)p.B, (int64_t)p.T);
  ccka_timeline_row o{};
  o.grid = p.first_grid + g;
  o.t0 = t0;
  o.samples = p.G * (t1 - t0);
  o.max_replicas = o.max_pending = o.max_nodes = INT32_MIN;
  o.min_nodes = INT32_MAX;
  p.rows[r] = o;
}

// ---------------------------------------------------------------------------
// [N][T]: lane <-> step. `lanes` consecutive lanes read one scenario's
// consecutive records (64 lanes: one 1 KiB run of 16-byte loads; horizons
// below 64 steps pack 64 / lanes scenarios into a wave). An item is (grid,
// tile of `lanes` steps, slice of the grid's scenarios); the four waves take
// the slice's scenarios in turn, four independent loads in flight per lane.
// A lane keeps its step's reduction in registers. The lanes of one bucket
// then meet in an LDS table (one entry per bucket the tile touches, at most
// `lanes`), and one thread per entry sends it to the row.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void tl_sum_nt(const TimelineParams& p, const TlGeom& q) {
  __shared__ unsigned long long s_sum[4][64];
  __shared__ uint32_t s_cnt[8][64];
  __shared__ int s_ext[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lanes = q.lanes, spw = 64 / lanes;       // scenarios per wave and trip
  const int st = lane & (lanes - 1), sub = lane / lanes;
  const int64_t stride = 4 * spw;
  for (int64_t w = blockIdx.x; w < q.items; w += gridDim.x) {
    const int64_t slice = w % q.n_slices, tile = (w / q.n_slices) % q.n_tiles, g = w / ((int64_t)q.n_slices * q.n_tiles);
    if (tid < 64) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_sum[k][tid] = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) s_cnt[k][tid] = 0;
      s_ext[0][tid] = s_ext[1][tid] = s_ext[2][tid] = INT32_MIN;
      s_ext[3][tid] = INT32_MAX;
    }
    __syncthreads();
    const int64_t t = tile * lanes + st;
    const int64_t i_end = min(p.G, (slice + 1) * q.slice_len);
    const int64_t fb = tile * lanes / p.B;  // first bucket of the tile
    if (t < p.T) {
      TlAcc a;
      const ccka_traj_rec* base = p.recs + g * p.G * p.T + t;
      int64_t i = slice * q.slice_len + wave * spw + sub;
      for (; i + 3 * stride < i_end; i += 4 * stride) {
        const int4 r0 = tl_load(base, i * p.T), r1 = tl_load(base, (i + stride) * p.T);
        const int4 r2 = tl_load(base, (i + 2 * stride) * p.T), r3 = tl_load(base, (i + 3 * stride) * p.T);
        a.add(r0); a.add(r1); a.add(r2); a.add(r3);
      }
      for (; i < i_end; i += stride) a.add(tl_load(base, i * p.T));
      const int e = (int)(t / p.B - fb);  // < lanes
      if (a.rep) atomicAdd(&s_sum[0][e], (unsigned long long)a.rep);
      if (a.pend) atomicAdd(&s_sum[1][e], (unsigned long long)a.pend);
      if (a.spot) atomicAdd(&s_sum[2][e], (unsigned long long)a.spot);
      if (a.od) atomicAdd(&s_sum[3][e], (unsigned long long)a.od);
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (a.cnt[b]) atomicAdd(&s_cnt[b][e], a.cnt[b]);
      atomicMax(&s_ext[0][e], a.mx_rep);
      atomicMax(&s_ext[1][e], a.mx_pend);
      atomicMax(&s_ext[2][e], a.mx_nodes);
      atomicMin(&s_ext[3][e], a.mn_nodes);
    }
    __syncthreads();
    // entry e holds bucket fb + e where that bucket has a step in this tile
    const int64_t t_last = min((int64_t)p.T, (tile + 1) * lanes) - 1;
    if (tid < lanes && fb + tid <= t_last / p.B) {
      unsigned long long sum[4], cnt[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[k] = s_sum[k][tid];
#pragma unroll
      for (int k = 0; k < 8; ++k) cnt[k] = s_cnt[k][tid];
      tl_flush(p.rows + g * p.n_buckets + fb + tid, sum, cnt, s_ext[0][tid], s_ext[1][tid], s_ext[2][tid],
               s_ext[3][tid]);
    }
    __syncthreads();  // the table is cleared for the next item
  }
}

// ---------------------------------------------------------------------------
// [T][N]: lane <-> scenario inside one grid. `lanes` consecutive threads read
// consecutive scenarios of one step (256: four 1 KiB runs); grids below 256
// scenarios put 256 / lanes steps side by side. A thread never leaves its
// grid: scenarios past the grid's (or the slice's) end are not read. An item
// is (row, slice of the grid's scenarios), so the whole workgroup shares one
// row: registers, a 64-lane shuffle tree, four wave partials in LDS, and one
// thread sends the item's partial to the row.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void tl_sum_tn(const TimelineParams& p, const TlGeom& q) {
  __shared__ unsigned long long s_part[4][12];
  __shared__ int s_pext[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lanes = q.lanes, phases = 256 / lanes;
  const int si = tid & (lanes - 1), sp = tid / lanes;
  for (int64_t w = blockIdx.x; w < q.items; w += gridDim.x) {
    const int64_t slice = w % q.n_slices, r = w / q.n_slices;
    const int64_t g = r / p.n_buckets, b = r % p.n_buckets;
    const int64_t t0 = b * p.B, t1 = min(t0 + (int64_t)p.B, (int64_t)p.T);
    const int64_t i0 = slice * q.slice_len + si, i_end = min(p.G, (slice + 1) * q.slice_len);
    const ccka_traj_rec* base = p.recs + g * p.G;
    TlAcc a;
    if (t1 - t0 >= 4 * phases) {  // long buckets: the independent loads are a thread's steps
      for (int64_t i = i0; i < i_end; i += lanes) {
        int64_t t = t0 + sp;
        for (; t + 3 * phases < t1; t += 4 * phases) {
          const int4 r0 = tl_load(base, t * p.N + i), r1 = tl_load(base, (t + phases) * p.N + i);
          const int4 r2 = tl_load(base, (t + 2 * phases) * p.N + i), r3 = tl_load(base, (t + 3 * phases) * p.N + i);
          a.add(r0); a.add(r1); a.add(r2); a.add(r3);
        }
        for (; t < t1; t += phases) a.add(tl_load(base, t * p.N + i));
      }
    } else {  // short buckets: its scenarios
      for (int64_t t = t0 + sp; t < t1; t += phases) {
        const ccka_traj_rec* row = base + t * p.N;
        int64_t i = i0;
        for (; i + 3 * lanes < i_end; i += 4 * lanes) {
          const int4 r0 = tl_load(row, i), r1 = tl_load(row, i + lanes);
          const int4 r2 = tl_load(row, i + 2 * lanes), r3 = tl_load(row, i + 3 * lanes);
          a.add(r0); a.add(r1); a.add(r2); a.add(r3);
        }
        for (; i < i_end; i += lanes) a.add(tl_load(row, i));
      }
    }
    unsigned long long v[12] = {(unsigned long long)a.rep, (unsigned long long)a.pend, (unsigned long long)a.spot,
                                (unsigned long long)a.od, a.cnt[0], a.cnt[1], a.cnt[2], a.cnt[3],
                                a.cnt[4], a.cnt[5], a.cnt[6], a.cnt[7]};
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] += (unsigned long long)__shfl_down((long long)v[k], d);
      a.mx_rep = max(a.mx_rep, __shfl_down(a.mx_rep, d));
      a.mx_pend = max(a.mx_pend, __shfl_down(a.mx_pend, d));
      a.mx_nodes = max(a.mx_nodes, __shfl_down(a.mx_nodes, d));
      a.mn_nodes = min(a.mn_nodes, __shfl_down(a.mn_nodes, d));
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) s_part[wave][k] = v[k];
      s_pext[wave][0] = a.mx_rep; s_pext[wave][1] = a.mx_pend;
      s_pext[wave][2] = a.mx_nodes; s_pext[wave][3] = a.mn_nodes;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long sum[4], cnt[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[k] = s_part[0][k] + s_part[1][k] + s_part[2][k] + s_part[3][k];
#pragma unroll
      for (int k = 0; k < 8; ++k) cnt[k] = s_part[0][4 + k] + s_part[1][4 + k] + s_part[2][4 + k] + s_part[3][4 + k];
      int e[4];
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] = max(max(s_pext[0][k], s_pext[1][k]), max(s_pext[2][k], s_pext[3][k]));
      e[3] = min(min(s_pext[0][3], s_pext[1][3]), min(s_pext[2][3], s_pext[3][3]));
      tl_flush(p.rows + r, sum, cnt, e[0], e[1], e[2], e[3]);
    }
    __syncthreads();  // the partials are rewritten by the next item
  }
}

template <bool NT>
__global__ void __launch_bounds__(256) timeline_sum_kernel(TimelineParams p, TlGeom q) {
  if constexpr (NT) tl_sum_nt(p, q);
  else tl_sum_tn(p, q);
}

// ---------------------------------------------------------------------------
// Nearest-rank quantile per row (SEMANTICS 7): x(k) of one field over the
// row's samples, k = max(1, ceil(q_ppm * samples / 1e6)), by an MSB-first
// radix select over order-preserving 32-bit keys (sign bit flipped): each of 4
// passes counts the byte of the keys that match the prefix found so far in an
// LDS histogram and a scan picks the byte that holds the rank. The result is
// an input value; nothing is staged, every pass re-reads the field from the
// records (4 of a record's 16 bytes), so a row may hold any number of samples.
//
// Reads stay coalesced in both layouts by the mapping of the sum kernels.
// [N][T]: lane <-> step, so with narrow buckets a workgroup owns nbk =
// lanes / B adjacent buckets, each with a histogram column of its own
// ([256 bytes][nbk columns], at most 32 columns = 32 KiB), and never strides a
// wave across scenarios; buckets of `lanes` steps or more are one item each.
// [T][N]: one row per item, a column per wave. Thread j < (rows of the item)
// scans row j's columns and keeps its prefix and remaining rank in LDS.
// A pass in which every row of the item knows its byte beforehand (the row's
// smallest and largest key agree on this byte and all above it) is skipped;
// the bounds come from the sums for NODES (min_nodes, max_nodes).
// ---------------------------------------------------------------------------
constexpr int kTlSelCols = 32;  // histogram columns of a select item

__device__ __forceinline__ uint32_t tl_key(int v) { return (uint32_t)v ^ 0x80000000u; }

__global__ void __launch_bounds__(256) timeline_select_kernel(TimelineParams p, TlGeom q) {
  __shared__ uint32_t s_hist[256 * kTlSelCols];
  __shared__ uint32_t s_prefix[kTlSelCols], s_rank[kTlSelCols], s_kmin[kTlSelCols], s_kmax[kTlSelCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lanes = q.lanes;
  const int word = p.q_field == CCKA_TL_PENDING ? 1 : p.q_field == CCKA_TL_NODES ? 2 : 0;
  const int* words = reinterpret_cast<const int*>(p.recs);
  const int ncol = p.nt ? 1 : 4;                // histogram columns per row
  const int cols = p.nt ? q.nbk : 4;            // columns of an item
  for (int64_t w = blockIdx.x; w < q.items; w += gridDim.x) {
    // this thread's samples: scenarios i0, i0 + di, ... < G at steps ta, ta + dt, ... < tb of row `myrow`
    int64_t g, b0;        // grid and first bucket of the item
    int nrows;            // rows (buckets) of the item
    int myrow = -1, col = 0;
    int64_t i0 = 0, di = 1, ta = 0, tb = 0, dt = 1;
    if (p.nt) {
      g = w / q.n_tiles;
      b0 = (w % q.n_tiles) * q.nbk;
      nrows = (int)min((int64_t)q.nbk, p.n_buckets - b0);
      const int st = lane & (lanes - 1), spw = 64 / lanes;
      const int mine = p.B < lanes ? st / p.B : 0;  // narrow buckets: lanes side by side
      if (mine < nrows) {
        const int64_t b = b0 + mine;
        myrow = mine;
        col = mine;
        ta = b0 * p.B + st;  // narrow: one step, ta + lanes >= tb
        tb = min((b + 1) * (int64_t)p.B, (int64_t)p.T);
        dt = lanes;
        i0 = wave * spw + lane / lanes;
        di = 4 * spw;
      }
    } else {
      g = w / p.n_buckets;
      b0 = w % p.n_buckets;
      nrows = 1;
      myrow = 0;
      col = wave;
      ta = b0 * p.B + tid / lanes;
      tb = min((b0 + 1) * (int64_t)p.B, (int64_t)p.T);
      dt = 256 / lanes;
      i0 = tid & (lanes - 1);
      di = lanes;
    }
    if (tid < nrows) {
      const ccka_timeline_row& row = p.rows[g * p.n_buckets + b0 + tid];
      const unsigned long long n = (unsigned long long)row.samples;  // <= 2^31, q_ppm < 2^20
      const unsigned long long k = ((unsigned long long)p.q_ppm * n + 999999ull) / 1000000ull;
      s_rank[tid] = (uint32_t)(k < 1 ? 1 : k);
      s_prefix[tid] = 0;
      const bool bounded = p.q_field == CCKA_TL_NODES;
      s_kmin[tid] = bounded ? tl_key(row.min_nodes) : 0u;
      s_kmax[tid] = bounded ? tl_key(row.max_nodes) : 0xffffffffu;
    }
    __syncthreads();
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const bool open = tid < nrows && ((s_kmin[tid] ^ s_kmax[tid]) >> shift) != 0;
      if (!__syncthreads_or(open)) {  // every row's keys share this byte and all above it
        if (tid < nrows) s_prefix[tid] |= s_kmin[tid] & (0xffu << shift);
        mask |= 0xffu << shift;
        __syncthreads();
        continue;
      }
      for (int k = tid; k < 256 * cols; k += 256) s_hist[k] = 0;
      __syncthreads();
      if (myrow >= 0) {
        const uint32_t prefix = s_prefix[myrow];
        for (int64_t i = i0; i < p.G; i += di)
          for (int64_t t = ta; t < tb; t += dt) {
            const int64_t idx = p.nt ? (g * p.G + i) * p.T + t : t * p.N + g * p.G + i;
            int v = words[idx * 4 + word];
            if (word == 2) v = (v & 0xffff) + (int)((uint32_t)v >> 16);
            const uint32_t key = tl_key(v);
            if ((key & mask) == prefix) atomicAdd(&s_hist[((key >> shift) & 255u) * cols + col], 1u);
          }
      }
      __syncthreads();
      if (tid < nrows) {
        const uint32_t rank = s_rank[tid];  // 1-based among the keys that match the prefix
        uint32_t below = 0, digit = 0, acc = 0;
        bool found = false;
        for (int d = 0; d < 256; ++d) {
          uint32_t c = 0;
          for (int k = 0; k < ncol; ++k) c += s_hist[d * cols + tid * ncol + k];
          if (!found && acc + c >= rank) {
            found = true;
            digit = (uint32_t)d;
            below = acc;
          }
          acc += c;
        }
        s_prefix[tid] |= digit << shift;
        s_rank[tid] = rank - below;
      }
      mask |= 0xffu << shift;
      __syncthreads();
    }
    if (tid < nrows) p.rows[g * p.n_buckets + b0 + tid].q_value = (int64_t)(int)(s_prefix[tid] ^ 0x80000000u);
    __syncthreads();  // s_prefix .. s_kmax are rewritten by the next item
  }
}

// ---------------------------------------------------------------------------
// Launch geometry
// ---------------------------------------------------------------------------
static int pow2_ceil(int64_t v, int cap) {
  int r = 1;
  while (r < cap && r < v) r <<= 1;
  return r;
}
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int64_t kTlMaxBlocks = 1 << 20;  // workgroups stride over the items beyond

// slices per grid so that `base` items become about 4 workgroups per CU, each
// slice a multiple of `unit` scenarios (what the workgroup reads per trip)
static void tl_slices(TlGeom& q, int64_t base, int64_t G, int64_t unit, int cus) {
  const int64_t target = 4 * (int64_t)(cus > 0 ? cus : 256);
  int64_t n = ceil_div(target, base);
  n = n < 1 ? 1 : n > ceil_div(G, unit) ? ceil_div(G, unit) : n;
  q.slice_len = ceil_div(ceil_div(G, n), unit) * unit;
  q.n_slices = (int32_t)ceil_div(G, q.slice_len);
  q.items = base * q.n_slices;
}

hipError_t launch_timeline_sum(const TimelineParams& p, int cus, hipStream_t s) {
  const int64_t rows = p.n_grids * p.n_buckets;
  hipLaunchKernelGGL(timeline_init_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, s, p);
  TlGeom q{};
  if (p.nt) {
    q.lanes = pow2_ceil(p.T, 64);
    q.n_tiles = (int32_t)ceil_div(p.T, q.lanes);
    tl_slices(q, p.n_grids * q.n_tiles, p.G, 4 * (64 / q.lanes), cus);
    hipLaunchKernelGGL(timeline_sum_kernel<true>, dim3((unsigned)(q.items < kTlMaxBlocks ? q.items : kTlMaxBlocks)),
                       dim3(256), 0, s, p, q);
  } else {
    q.lanes = pow2_ceil(p.G, 256);
    tl_slices(q, rows, p.G, q.lanes, cus);
    hipLaunchKernelGGL(timeline_sum_kernel<false>, dim3((unsigned)(q.items < kTlMaxBlocks ? q.items : kTlMaxBlocks)),
                       dim3(256), 0, s, p, q);
  }
  return hipGetLastError();
}

hipError_t launch_timeline_select(const TimelineParams& p, int cus, hipStream_t s) {
  TlGeom q{};
  if (p.nt) {
    // narrower step groups (shorter runs, down to 128 bytes) while a whole-batch
    // grid would leave CUs without an item
    q.lanes = pow2_ceil(p.T, kTlSelCols);
    for (;;) {
      q.nbk = p.B < q.lanes ? q.lanes / p.B : 1;
      q.n_tiles = (int32_t)ceil_div(p.n_buckets, q.nbk);
      q.items = p.n_grids * q.n_tiles;
      if (q.items >= 2 * (int64_t)cus || q.lanes <= 8 || p.B >= q.lanes) break;
      q.lanes >>= 1;
    }
  } else {
    q.lanes = pow2_ceil(p.G, 256);
    q.nbk = 1;
    q.items = p.n_grids * p.n_buckets;
  }
  hipLaunchKernelGGL(timeline_select_kernel, dim3((unsigned)(q.items < kTlMaxBlocks ? q.items : kTlMaxBlocks)),
                     dim3(256), 0, s, p, q);
  return hipGetLastError();
}

}  // namespace ccka
