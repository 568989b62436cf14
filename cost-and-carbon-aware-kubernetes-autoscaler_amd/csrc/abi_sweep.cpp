// abi_sweep.cpp — the policy sweep of libccka.so's C ABI (BASELINE config 4):
// per-grid statistics of the last rollout (sums, or per objective a quantile /
// tail sum: SEMANTICS 6) and their Pareto frontier (sweep.hip), local or merged
// across ranks after an RCCL all-gather.
#include <algorithm>

#include "ctx.h"

using namespace ccka;

static const ccka_sweep_stat kAllSum = {};  // CCKA_STAT_SUM == 0

int check_sweep_stat(ccka_ctx* c, const ccka_sweep_stat* st) {
  if (!st) return fail(c, CCKA_EINVAL, "null statistic");
  for (int j = 0; j < 4; ++j) {
    if (st->kind[j] < CCKA_STAT_SUM || st->kind[j] > CCKA_STAT_TAIL)
      return fail(c, CCKA_EINVAL, "statistic kind %d of objective %d not in 0..2", st->kind[j], j);
    if (st->kind[j] != CCKA_STAT_SUM && (st->q_ppm[j] < 0 || st->q_ppm[j] > 1000000))
      return fail(c, CCKA_EINVAL, "q_ppm %d of objective %d not in [0, 1000000]", st->q_ppm[j], j);
  }
  return CCKA_OK;
}

// the selection kernel's arguments; *any = some objective is not a SUM
static GridSel grid_sel(const GridSrc& g, const ccka_sweep_stat& st, bool* any) {
  GridSel q{};
  q.g = g;
  *any = false;
  for (int j = 0; j < 4; ++j) {
    q.kind[j] = st.kind[j];
    q.rank[j] = st.kind[j] == CCKA_STAT_SUM ? 1 : ccka_sweep_rank(g.grid_size, st.q_ppm[j]);
    *any = *any || st.kind[j] != CCKA_STAT_SUM;
  }
  return q;
}

// d_gstats[0 .. g.n_grids) = the statistics `st` (validated) of g's grids: the
// sums first, then the selection kernel overwrites the non-SUM objectives
static int grid_rows(ccka_ctx* c, const GridSrc& g, const ccka_sweep_stat& st) {
  if (g.n_grids > (1 << 24)) return fail(c, CCKA_EINVAL, "too many grids");
  if (!c->d_gstats.reserve(g.n_grids)) return fail(c, CCKA_ENOMEM, "grid buffers");
  HIPCHK(c, launch_grid_stats(g, c->d_gstats, c->stream));
  bool any = false;
  const GridSel q = grid_sel(g, st, &any);
  if (any) HIPCHK(c, launch_grid_select(q, c->d_gstats, c->stream));
  return CCKA_OK;
}

// the last rollout's result columns as whole grids of grid_size
static int rollout_grids(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* st, GridSrc* out) {
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  int rc;
  if ((rc = check_sweep_stat(c, st)) != CCKA_OK) return rc;
  if (grid_size < 1 || c->N % grid_size || c->first_id % grid_size)
    return fail(c, CCKA_EINVAL, "batch (first_id %lld, n %lld) does not hold whole grids of %lld",
                (long long)c->first_id, (long long)c->N, (long long)grid_size);
  GridSrc g{};
  g.cost = c->res.cost; g.gco2 = c->res.gco2; g.slo = c->res.slo; g.energy = c->res.energy;
  g.grid_size = grid_size;
  g.first_grid = c->first_id / grid_size;
  g.n_grids = c->N / grid_size;
  *out = g;
  return CCKA_OK;
}

static int sweep_grids(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* st, int64_t* n_grids) {
  GridSrc g{};
  int rc;
  if ((rc = rollout_grids(c, grid_size, st, &g)) != CCKA_OK) return rc;
  if ((rc = grid_rows(c, g, *st)) != CCKA_OK) return rc;
  *n_grids = g.n_grids;
  return CCKA_OK;
}

static int grid_stat_out(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* st, ccka_grid_stats* out,
                         int64_t n_grids) {
  (void)hipSetDevice(c->device);
  int64_t ng = 0;
  int rc;
  if ((rc = sweep_grids(c, grid_size, st, &ng)) != CCKA_OK) return rc;
  if (n_grids != ng) return fail(c, CCKA_EINVAL, "n_grids %lld != %lld", (long long)n_grids, (long long)ng);
  HIPCHK(c, hipMemcpyAsync(out, c->d_gstats, sizeof(ccka_grid_stats) * ng, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

extern "C" {

int64_t ccka_sweep_rank(int64_t n, int32_t q_ppm) {
  if (n < 1 || q_ppm < 0 || q_ppm > 1000000) return -1;
  const int64_t k = (int64_t)(((__int128)q_ppm * n + 999999) / 1000000);
  return k < 1 ? 1 : k;
}

int ccka_get_grid_stats(ccka_ctx* c, int64_t grid_size, ccka_grid_stats* out, int64_t n_grids) {
  if (!c || !out) return CCKA_EINVAL;
  return grid_stat_out(c, grid_size, &kAllSum, out, n_grids);
}

int ccka_get_grid_stat(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* stat, ccka_grid_stats* out,
                       int64_t n_grids) {
  if (!c || !out) return CCKA_EINVAL;
  return grid_stat_out(c, grid_size, stat, out, n_grids);
}

// Pareto buffers for `ng` local grids and `nranks` ranks: the local candidates
// (ng), the all-gathered candidate rows [nranks][ng] followed by their union
// (nranks * ng), the final frontier and the dominance flags (nranks * ng each:
// the global frontier can hold every rank's candidates), the per-rank counts
// (+ the local one) and two device-side sizes.
static int pareto_bufs(ccka_ctx* c, int64_t ng, int nranks) {
  const int64_t tot = ng * nranks;
  if (!all_or_none(c->d_gcand.reserve(ng) && c->d_gfront.reserve(tot) && c->d_gflags.reserve(tot) &&
                       c->d_gn.reserve(2) && c->d_ggather.reserve(tot * 2) && c->d_gcounts.reserve(nranks + 1),
                   c->d_gcand, c->d_gfront, c->d_gflags, c->d_gn, c->d_ggather, c->d_gcounts))
    return fail(c, CCKA_ENOMEM, "pareto buffers (%lld grids x %d ranks)", (long long)ng, nranks);
  return CCKA_OK;
}

// Global filter over the exchanged candidates, identical on every rank: the
// valid prefixes of gathered[nranks][ng] (counts[q] each, rank order = grid
// order) are compacted, then filtered again into d_gfront / d_gn[0].
static int pareto_merge(ccka_ctx* c, int64_t ng, int nranks) {
  ccka_grid_stats* uni = c->d_ggather + ng * nranks;
  HIPCHK(c, launch_pareto_union(c->d_ggather, c->d_gcounts, nranks, (int)ng, uni, c->d_gn + 1, c->stream));
  HIPCHK(c, launch_pareto(uni, (int)(ng * nranks), c->d_gn + 1, c->d_gflags, c->d_gfront, c->d_gn, c->stream));
  return CCKA_OK;
}

static int pareto_copy_out(ccka_ctx* c, ccka_grid_stats* out, int32_t capacity, int32_t* n_out) {
  int32_t n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, c->d_gn, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_out = n;
  if (n > capacity) return fail(c, CCKA_EINVAL, "frontier has %d grids, capacity %d", n, capacity);
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(out, c->d_gfront, sizeof(ccka_grid_stats) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return CCKA_OK;
}

int ccka_pareto_frontier_stat(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* stat, ccka_grid_stats* out,
                              int32_t capacity, int32_t* n_out) {
  if (!c || !n_out || capacity < 0 || (capacity > 0 && !out)) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  int64_t ng = 0;
  int rc;
  if ((rc = sweep_grids(c, grid_size, stat, &ng)) != CCKA_OK) return rc;
  int nranks = 1;
  if (c->comm && ncclCommCount(c->comm, &nranks) != ncclSuccess)
    return fail(c, CCKA_ERCCL, "ncclCommCount failed");
  if ((rc = pareto_bufs(c, ng, nranks)) != CCKA_OK) return rc;
  if (!c->comm) {
    // local frontier only: non-dominated grids of this batch, in grid order
    HIPCHK(c, launch_pareto(c->d_gstats, (int)ng, nullptr, c->d_gflags, c->d_gfront, c->d_gn, c->stream));
    return pareto_copy_out(c, out, capacity, n_out);
  }
  // local candidates, then the exchange: every rank's candidates (fixed
  // capacity = grids per rank, every rank holds the same number) and counts
  HIPCHK(c, launch_pareto(c->d_gstats, (int)ng, nullptr, c->d_gflags, c->d_gcand, c->d_gn, c->stream));
  int64_t* cnt_local = c->d_gcounts + nranks;
  // int32 count -> int64 slot (device copy keeps the exchange on the stream)
  HIPCHK(c, hipMemsetAsync(cnt_local, 0, sizeof(int64_t), c->stream));
  HIPCHK(c, hipMemcpyAsync(cnt_local, c->d_gn, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
  ncclGroupStart();
  ncclResult_t r1 = ncclAllGather(cnt_local, c->d_gcounts, 1, ncclInt64, c->comm, c->stream);
  ncclResult_t r2 = ncclAllGather(c->d_gcand, c->d_ggather, (size_t)ng * sizeof(ccka_grid_stats), ncclUint8,
                                  c->comm, c->stream);
  ncclResult_t r3 = ncclGroupEnd();
  if (r1 != ncclSuccess || r2 != ncclSuccess || r3 != ncclSuccess)
    return fail(c, CCKA_ERCCL, "ncclAllGather (pareto candidates) failed");
  if ((rc = pareto_merge(c, ng, nranks)) != CCKA_OK) return rc;
  return pareto_copy_out(c, out, capacity, n_out);
}

int ccka_pareto_frontier(ccka_ctx* c, int64_t grid_size, ccka_grid_stats* out, int32_t capacity, int32_t* n_out) {
  return ccka_pareto_frontier_stat(c, grid_size, &kAllSum, out, capacity, n_out);
}

// Internal (not in include/ccka.h): ccka_get_grid_stat's kernel path on
// caller-supplied result columns (n scenarios = whole grids of grid_size,
// grid ids from 0) instead of the last rollout's, so a test can feed keys no
// rollout produces. out[n / grid_size]. The sums run first here too (the one
// kernel path): on columns whose sum leaves int64 a SUM field is meaningless
// (the device's adds wrap); the QUANTILE / TAIL fields do not depend on it.
int ccka_debug_grid_stat(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const double* gco2,
                         const double* energy, int64_t n, int64_t grid_size, const ccka_sweep_stat* stat,
                         ccka_grid_stats* out) {
  if (!c || !cost || !slo || !gco2 || !energy || !out) return CCKA_EINVAL;
  int rc;
  if ((rc = check_sweep_stat(c, stat)) != CCKA_OK) return rc;
  if (n < 1 || grid_size < 1 || n % grid_size)
    return fail(c, CCKA_EINVAL, "%lld scenarios do not hold whole grids of %lld", (long long)n, (long long)grid_size);
  (void)hipSetDevice(c->device);
  DevBuf<int64_t> d_cost;
  DevBuf<int32_t> d_slo;
  DevBuf<double> d_gco2, d_energy;
  if ((rc = dupload(c, d_cost, cost, (size_t)n)) != CCKA_OK || (rc = dupload(c, d_slo, slo, (size_t)n)) != CCKA_OK ||
      (rc = dupload(c, d_gco2, gco2, (size_t)n)) != CCKA_OK || (rc = dupload(c, d_energy, energy, (size_t)n)) != CCKA_OK)
    return rc;
  GridSrc g{};
  g.cost = d_cost; g.gco2 = d_gco2; g.slo = d_slo; g.energy = d_energy;
  g.grid_size = grid_size;
  g.n_grids = n / grid_size;
  if ((rc = grid_rows(c, g, *stat)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->d_gstats, sizeof(ccka_grid_stats) * g.n_grids, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // before the columns are freed
  return CCKA_OK;
}

// Internal (not in include/ccka.h; tools/sweep_stat_time.py): device time of
// the two kernels behind ccka_get_grid_stat on the last rollout's results, each
// alone. One sample = `reps` back-to-back launches between two HIP events on
// the engine's stream, divided by reps; the median of 5 samples after a warm-up
// launch. sum_ms: grid_stats_kernel; select_ms: the selection kernel for `stat`
// (0 when every objective is a SUM).
int ccka_debug_grid_stat_ms(ccka_ctx* c, int64_t grid_size, const ccka_sweep_stat* stat, int32_t reps,
                            double* sum_ms, double* select_ms) {
  if (!c || !sum_ms || !select_ms || reps < 1 || reps > 1000) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  GridSrc g{};
  int rc;
  if ((rc = rollout_grids(c, grid_size, stat, &g)) != CCKA_OK) return rc;
  if ((rc = grid_rows(c, g, *stat)) != CCKA_OK) return rc;  // buffers + warm-up of both kernels
  bool any = false;
  const GridSel q = grid_sel(g, *stat, &any);
  hipEvent_t e0 = nullptr, e1 = nullptr;  // own events: ccka_last_kernel_ms keeps the rollout's
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    rc = fail(c, CCKA_EHIP, "timing events");
  double med[2] = {0.0, 0.0};
  for (int which = 0; which < (any ? 2 : 1) && rc == CCKA_OK; ++which) {
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 5 && rc == CCKA_OK; ++k) {
      bool ok = hipEventRecord(e0, c->stream) == hipSuccess;
      for (int r = 0; r < reps && ok; ++r)
        ok = (which ? launch_grid_select(q, c->d_gstats, c->stream) : launch_grid_stats(g, c->d_gstats, c->stream)) ==
             hipSuccess;
      ok = ok && hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
           hipEventElapsedTime(&ms[k], e0, e1) == hipSuccess;
      if (!ok) rc = fail(c, CCKA_EHIP, "timed launches (kernel %d, sample %d)", which, k);
    }
    if (rc != CCKA_OK) break;
    std::sort(ms, ms + 5);
    med[which] = (double)ms[2] / reps;
  }
  (void)hipStreamSynchronize(c->stream);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != CCKA_OK) return rc;
  *sum_ms = med[0];
  *select_ms = med[1];
  return CCKA_OK;
}

// Internal (not in include/ccka.h): the cross-rank half of
// ccka_pareto_frontier on caller-supplied exchange buffers, i.e. what every
// rank runs after the RCCL all-gather: `gathered` [nranks][cap] candidate rows
// (rank q's first counts[q] valid, each sorted by grid id, ranks in grid
// order), merged and filtered into the global frontier. Lets a single GPU
// exercise the multi-rank merge path.
int ccka_debug_pareto_merge(ccka_ctx* c, const ccka_grid_stats* gathered, const int64_t* counts, int32_t nranks,
                            int64_t cap, ccka_grid_stats* out, int32_t capacity, int32_t* n_out) {
  if (!c || !gathered || !counts || !n_out || nranks < 1 || cap < 1 || capacity < 0 || (capacity > 0 && !out))
    return CCKA_EINVAL;
  for (int q = 0; q < nranks; ++q)
    if (counts[q] < 0 || counts[q] > cap) return fail(c, CCKA_EINVAL, "count of rank %d out of range", q);
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = pareto_bufs(c, cap, nranks)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_ggather, gathered, sizeof(ccka_grid_stats) * cap * nranks, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_gcounts, counts, sizeof(int64_t) * nranks, hipMemcpyHostToDevice, c->stream));
  if ((rc = pareto_merge(c, cap, nranks)) != CCKA_OK) return rc;
  return pareto_copy_out(c, out, capacity, n_out);
}

}  // extern "C"
