// abi_boot.cpp — the paired bootstrap of libccka.so's C ABI (SEMANTICS 9): per
// grid of a batch the replicate sums of its resampled deltas against the
// paired comparison's snapshot, reduced to an interval and sign counts
// (boot.hip). State, shape and baseline rules are abi_paired.cpp's.
#include <algorithm>

#include "ctx.h"

using namespace ccka;

// the rules ccka_boot_spec adds to the paired comparison's
static int check_boot_spec(ccka_ctx* c, const ccka_boot_spec* sp) {
  if (sp->replicates < 1 || sp->replicates > kBootMaxReplicates)
    return fail(c, CCKA_EINVAL, "replicates %d not in [1, %d]", sp->replicates, kBootMaxReplicates);
  if (sp->lo_ppm < 0 || sp->lo_ppm > 1000000 || sp->hi_ppm < 0 || sp->hi_ppm > 1000000)
    return fail(c, CCKA_EINVAL, "lo_ppm %d / hi_ppm %d not in [0, 1000000]", sp->lo_ppm, sp->hi_ppm);
  if (sp->lo_ppm > sp->hi_ppm) return fail(c, CCKA_EINVAL, "lo_ppm %d > hi_ppm %d", sp->lo_ppm, sp->hi_ppm);
  if (sp->_pad != 0) return fail(c, CCKA_EINVAL, "_pad must be 0");
  return CCKA_OK;
}

// the kernels' arguments, pass fields aside, for current columns `cur` against
// a snapshot of snap_n scenarios from global grid snap_first_grid, under the
// validated *sp; tile width K and staging limit L
static int boot_params(ccka_ctx* c, const GridSrc& cur, const int64_t* snap, int64_t snap_n,
                       int64_t snap_first_grid, const ccka_boot_spec* sp, int K, int L, BootParams* out) {
  PairedBase b{};
  int rc;
  if ((rc = paired_baseline(c, cur, snap_n, snap_first_grid, sp->base_grid, &b)) != CCKA_OK) return rc;
  BootParams p{};
  p.cur = cur;
  p.snap = snap;
  p.snap_n = snap_n;
  p.base_grid = b.grid;
  p.base_step = b.step;
  p.base_off = b.off;
  p.B = sp->replicates;
  p.rank_lo = ccka_sweep_rank(p.B, sp->lo_ppm);
  p.rank_hi = ccka_sweep_rank(p.B, sp->hi_ppm);
  p.k0 = (uint32_t)(sp->seed & 0xffffffffu);
  p.k1 = (uint32_t)(sp->seed >> 32);
  p.K = K;
  p.L = L;
  *out = p;
  return CCKA_OK;
}

// Grids per pass: as many whole tiles as the sums workspace (and, by default,
// a delta array of the same byte bound) holds, and at least one grid. A pass
// of fewer grids than the tile runs on the narrowest tile that holds them: the
// rows do not depend on either.
static void boot_pass_shape(const ccka_ctx* c, BootParams& p) {
  const int64_t max_sums = c->boot_max_sums > 0 ? c->boot_max_sums : kBootMaxSums;
  const int K = p.K;
  int64_t gp = std::min(max_sums / (4 * (int64_t)p.B), kBootMaxSums / (4 * p.cur.grid_size));
  gp = gp >= K ? gp / K * K : std::max<int64_t>(gp, 1);
  p.gp = std::min(gp, p.cur.n_grids);
}

static int narrow_tile(int K, int64_t grids) {
  while (K > 1 && K / 2 >= grids) K /= 2;
  return K;
}

// chunks / per_chunk of the sums kernel for a pass of p.gp grids: enough
// workgroups for the device, no chunk below one replicate per wave
static void boot_chunks(const ccka_ctx* c, BootParams& p) {
  const bool staged = p.cur.grid_size <= p.L;
  const int waves = (staged ? kBootStagedThreads : 256) / 64;
  const int64_t tiles = (p.gp + p.K - 1) / p.K;
  const int64_t want = (int64_t)std::max(c->cus, 1) * (staged ? 2 : 8);
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((want + tiles - 1) / tiles, (p.B + waves - 1) / waves));
  p.per_chunk = (int32_t)((p.B + chunks - 1) / chunks);
  p.chunks = (int32_t)((p.B + p.per_chunk - 1) / p.per_chunk);
}

// buffers of every pass and the rows; nothing is launched before they exist
static int boot_reserve(ccka_ctx* c, BootParams& p) {
  boot_pass_shape(c, p);
  const int K = narrow_tile(p.K, p.gp);  // the widest tile a pass runs on (boot_pass)
  const int64_t slots = (p.gp + K - 1) / K * K;
  if (!all_or_none(c->d_brows.reserve(p.cur.n_grids) && c->d_pflag.reserve(1) &&
                       c->d_bsums.reserve(p.gp * 4 * p.B) && c->d_bdelta.reserve(slots * p.cur.grid_size * 4),
                   c->d_brows, c->d_pflag, c->d_bsums, c->d_bdelta))
    return fail(c, CCKA_ENOMEM, "bootstrap workspace (%lld grids per pass, %d replicates)", (long long)p.gp, p.B);
  p.rows = c->d_brows;
  p.flag = c->d_pflag;
  p.sums = c->d_bsums;
  p.delta = c->d_bdelta;
  return CCKA_OK;
}

// one pass [g0, g0 + gp) of p: its tile, chunks and the three kernels
static int boot_pass(ccka_ctx* c, BootParams q, int64_t g0, int which = 7) {
  q.g0 = g0;
  q.gp = std::min(q.gp, q.cur.n_grids - g0);
  q.K = narrow_tile(q.K, q.gp);
  boot_chunks(c, q);
  if (which & 1) HIPCHK(c, launch_boot_delta(q, c->stream));
  if (which & 2) HIPCHK(c, launch_boot_sums(q, c->stream));
  if (which & 4) HIPCHK(c, launch_boot_select(q, c->stream));
  return CCKA_OK;
}

// d_brows[0 .. n_grids) = the rows of p, the flag cleared first
static int boot_launch(ccka_ctx* c, BootParams& p) {
  int rc;
  if ((rc = boot_reserve(c, p)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_pflag, 0, sizeof(uint32_t), c->stream));
  for (int64_t g0 = 0; g0 < p.cur.n_grids; g0 += p.gp)
    if ((rc = boot_pass(c, p, g0)) != CCKA_OK) return rc;
  return CCKA_OK;
}

// rows -> out, then the overflow word
static int boot_out(ccka_ctx* c, const BootParams& p, ccka_boot_row* out) {
  HIPCHK(c, hipMemcpyAsync(out, c->d_brows, sizeof(ccka_boot_row) * p.cur.n_grids, hipMemcpyDeviceToHost, c->stream));
  uint32_t ovf = 0;
  int rc;
  if ((rc = read_flag(c, c->d_pflag, &ovf)) != CCKA_OK) return rc;
  if (ovf)
    return fail(c, CCKA_EOVERFLOW, "a current value has no int64 fixed-point form, or a delta leaves int64");
  return CCKA_OK;
}

// the last rollout's batch against the context's snapshot: state, then every
// rule of the spec, all before anything is launched
static int boot_of_rollout(ccka_ctx* c, const ccka_boot_spec* sp, int K, int L, BootParams* p) {
  int rc;
  if ((rc = paired_state(c)) != CCKA_OK) return rc;
  if ((rc = check_boot_spec(c, sp)) != CCKA_OK) return rc;
  if ((rc = paired_rollout_shape(c, sp->grid_size)) != CCKA_OK) return rc;
  return boot_params(c, result_columns(c->res, sp->grid_size, c->first_id, c->N), c->d_snap, c->snap_n,
                     c->snap_first / c->snap_grid_size, sp, K, L, p);
}

extern "C" {

int32_t ccka_boot_sizes(int64_t* out, int32_t n) {
  const int64_t s[] = {sizeof(ccka_boot_spec), sizeof(ccka_boot_obj), sizeof(ccka_boot_row)};
  int32_t k = 0;
  for (; out && k < 3 && k < n; ++k) out[k] = s[k];
  return k;
}

int ccka_get_paired_bootstrap(ccka_ctx* c, const ccka_boot_spec* spec, ccka_boot_row* out, int64_t n_rows) {
  if (!c) return CCKA_EINVAL;
  if (!spec || !out) return fail(c, CCKA_EINVAL, "null bootstrap spec or output");
  (void)hipSetDevice(c->device);
  BootParams p{};
  int rc;
  if ((rc = boot_of_rollout(c, spec, kBootTile, kBootStage, &p)) != CCKA_OK) return rc;
  if (n_rows != p.cur.n_grids)
    return fail(c, CCKA_EINVAL, "n_rows %lld != %lld", (long long)n_rows, (long long)p.cur.n_grids);
  if ((rc = boot_launch(c, p)) != CCKA_OK) return rc;
  return boot_out(c, p, out);
}

// Internal (not in include/ccka.h): ccka_get_paired_bootstrap's kernels on
// caller-supplied result columns, as ccka_debug_paired: `n` current and `nb`
// baseline scenarios as whole grids of spec->grid_size, grid ids from 0 on both
// sides; the context's snapshot stays. out[n / grid_size].
int ccka_debug_boot(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const double* gco2, const double* energy,
                    int64_t n, const int64_t* bcost, const int32_t* bslo, const double* bgco2, const double* benergy,
                    int64_t nb, const ccka_boot_spec* spec, ccka_boot_row* out) {
  if (!c) return CCKA_EINVAL;
  if (!cost || !slo || !gco2 || !energy || !bcost || !bslo || !bgco2 || !benergy || !spec || !out)
    return fail(c, CCKA_EINVAL, "null columns, spec or output");
  int rc;
  if ((rc = check_boot_spec(c, spec)) != CCKA_OK) return rc;
  PairedDebugCols cols;
  rc = cols.upload(c, cost, slo, gco2, energy, n, bcost, bslo, bgco2, benergy, nb, spec->grid_size);
  BootParams p{};
  if (rc == CCKA_OK) rc = boot_params(c, cols.cur, cols.d_snap, nb, 0, spec, kBootTile, kBootStage, &p);
  if (rc == CCKA_OK) rc = boot_launch(c, p);
  if (rc == CCKA_OK) rc = boot_out(c, p, out);
  (void)hipStreamSynchronize(c->stream);  // before the columns are freed
  return rc;
}

// Internal: bounds the replicate-sum workspace of a pass to max_sums sums (a
// pass still holds at least one grid); 0 restores the default. The rows do not
// depend on it.
int ccka_debug_boot_workspace(ccka_ctx* c, int64_t max_sums) {
  if (!c || max_sums < 0) return CCKA_EINVAL;
  c->boot_max_sums = max_sums;
  return CCKA_OK;
}

// Internal: out[0] = the delta staging limit (positions per grid the sums
// kernel keeps in LDS), out[1] = the grid-tile width of this build. No context.
int ccka_debug_boot_limits(int64_t out[2]) {
  if (!out) return CCKA_EINVAL;
  out[0] = kBootStage;
  out[1] = kBootTile;
  return CCKA_OK;
}

// Internal (tools/boot_time.py): device time of the three kernels on the last
// rollout's results against the context's snapshot, each alone, in the way of
// ccka_debug_paired_ms: one sample = `reps` back-to-back launches of one
// kernel for every pass between two HIP events on the engine's stream, divided
// by reps; the median of 5 samples after a warm-up. tile / stage: the grid-tile
// width and staging limit to time (0 / negative: the build's; stage 0: gather
// from the delta array). ms[3]: boot_delta_kernel, boot_sums_kernel,
// boot_select_kernel.
int ccka_debug_boot_ms(ccka_ctx* c, const ccka_boot_spec* spec, int32_t reps, int32_t tile, int32_t stage,
                       double ms[3]) {
  if (!c || !ms || reps < 1 || reps > 1000) return CCKA_EINVAL;
  if (!spec) return fail(c, CCKA_EINVAL, "null bootstrap spec");
  const int K = tile > 0 ? tile : kBootTile, L = stage >= 0 ? stage : kBootStage;
  if (!boot_config_ok(K, L)) return fail(c, CCKA_EINVAL, "no sums kernel for tile %d, staging limit %d", K, L);
  (void)hipSetDevice(c->device);
  BootParams p{};
  int rc;
  if ((rc = boot_of_rollout(c, spec, K, L, &p)) != CCKA_OK) return rc;
  if ((rc = boot_launch(c, p)) != CCKA_OK) return rc;  // warm-up of the three kernels
  hipEvent_t e0 = nullptr, e1 = nullptr;  // own events: ccka_last_kernel_ms keeps the rollout's
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(c, CCKA_EHIP, "timing events");
  double med[3] = {0.0, 0.0, 0.0};
  for (int which = 0; which < 3 && rc == CCKA_OK; ++which) {
    float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 5 && rc == CCKA_OK; ++k) {
      bool ok = hipEventRecord(e0, c->stream) == hipSuccess;
      for (int r = 0; r < reps && ok; ++r)
        for (int64_t g0 = 0; g0 < p.cur.n_grids && ok; g0 += p.gp) ok = boot_pass(c, p, g0, 1 << which) == CCKA_OK;
      ok = ok && hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
           hipEventElapsedTime(&t[k], e0, e1) == hipSuccess;
      if (!ok) rc = fail(c, CCKA_EHIP, "timed launches (kernel %d, sample %d)", which, k);
    }
    if (rc != CCKA_OK) break;
    std::sort(t, t + 5);
    med[which] = (double)t[2] / reps;
  }
  (void)hipStreamSynchronize(c->stream);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != CCKA_OK) return rc;
  for (int i = 0; i < 3; ++i) ms[i] = med[i];
  return CCKA_OK;
}

}  // extern "C"
