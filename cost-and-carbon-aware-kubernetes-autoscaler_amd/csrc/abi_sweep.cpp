// abi_sweep.cpp — the policy sweep of libccka.so's C ABI (BASELINE config 4):
// per-grid sums of the last rollout and their Pareto frontier (sweep.hip), local
// or merged across ranks after an RCCL all-gather.
#include "ctx.h"

using namespace ccka;

static int sweep_grids(ccka_ctx* c, int64_t grid_size, int64_t* n_grids) {
  if (!c->ran) return fail(c, CCKA_ESTATE, "no rollout yet");
  if (grid_size < 1 || c->N % grid_size || c->first_id % grid_size)
    return fail(c, CCKA_EINVAL, "batch (first_id %lld, n %lld) does not hold whole grids of %lld",
                (long long)c->first_id, (long long)c->N, (long long)grid_size);
  const int64_t ng = c->N / grid_size;
  if (ng > (1 << 24)) return fail(c, CCKA_EINVAL, "too many grids");
  if (!c->d_gstats.reserve(ng)) return fail(c, CCKA_ENOMEM, "grid buffers");
  GridSrc g{};
  g.cost = c->res.cost; g.gco2 = c->res.gco2; g.slo = c->res.slo; g.energy = c->res.energy;
  g.grid_size = grid_size;
  g.first_grid = c->first_id / grid_size;
  g.n_grids = ng;
  HIPCHK(c, launch_grid_stats(g, c->d_gstats, c->stream));
  *n_grids = ng;
  return CCKA_OK;
}

extern "C" {

int ccka_get_grid_stats(ccka_ctx* c, int64_t grid_size, ccka_grid_stats* out, int64_t n_grids) {
  if (!c || !out) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  int64_t ng = 0;
  int rc;
  if ((rc = sweep_grids(c, grid_size, &ng)) != CCKA_OK) return rc;
  if (n_grids != ng) return fail(c, CCKA_EINVAL, "n_grids %lld != %lld", (long long)n_grids, (long long)ng);
  HIPCHK(c, hipMemcpyAsync(out, c->d_gstats, sizeof(ccka_grid_stats) * ng, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
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

int ccka_pareto_frontier(ccka_ctx* c, int64_t grid_size, ccka_grid_stats* out, int32_t capacity, int32_t* n_out) {
  if (!c || !n_out || capacity < 0 || (capacity > 0 && !out)) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  int64_t ng = 0;
  int rc;
  if ((rc = sweep_grids(c, grid_size, &ng)) != CCKA_OK) return rc;
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
