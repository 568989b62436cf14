// abi_paired.cpp — the paired comparison of libccka.so's C ABI (SEMANTICS 8):
// a snapshot of a batch's results as integer vectors, kept in the context, and
// the per-grid reduction of a later batch's per-position deltas against it
// (paired.hip); export / import of one snapshot grid for sharded sweeps.
#include <algorithm>

#include "ctx.h"

using namespace ccka;

constexpr int64_t kPairedMaxGrids = 1 << 24;
constexpr int64_t kPairedMaxGridSize = (int64_t)1 << 31;  // counts fit 32 bits

// a batch (first_id, n) as whole grids of grid_size whose positions share traces
int paired_shape(ccka_ctx* c, int64_t grid_size, int64_t n_traces, int64_t first_id, int64_t n) {
  if (grid_size < 1 || grid_size > kPairedMaxGridSize)
    return fail(c, CCKA_EINVAL, "grid_size %lld not in [1, 2^31]", (long long)grid_size);
  if (n_traces < 1 || grid_size % n_traces)
    return fail(c, CCKA_EINVAL, "paired positions need shared traces: n_traces %lld must be > 0 and divide grid_size %lld",
                (long long)n_traces, (long long)grid_size);
  if (n < 1 || first_id < 0 || n % grid_size || first_id % grid_size)
    return fail(c, CCKA_EINVAL, "batch (first_id %lld, n %lld) does not hold whole grids of %lld", (long long)first_id,
                (long long)n, (long long)grid_size);
  if (n / grid_size > kPairedMaxGrids) return fail(c, CCKA_EINVAL, "more than 2^24 grids");
  return CCKA_OK;
}

GridSrc result_columns(const ResultPtrs& r, int64_t grid_size, int64_t first_id, int64_t n) {
  GridSrc g{};
  g.cost = r.cost; g.gco2 = r.gco2; g.slo = r.slo; g.energy = r.energy;
  g.grid_size = grid_size;
  g.first_grid = first_id / grid_size;
  g.n_grids = n / grid_size;
  return g;
}

// *flag (one device word) read back after everything queued on the stream
int read_flag(ccka_ctx* c, const uint32_t* flag, uint32_t* out) {
  HIPCHK(c, hipMemcpyAsync(out, flag, sizeof *out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

// snap[4][g.n_grids * g.grid_size] = the vectors of g's columns; CCKA_EOVERFLOW when one has no fixed-point form
int capture_into(ccka_ctx* c, const GridSrc& g, int64_t* snap) {
  if (!c->d_pflag.reserve(1)) return fail(c, CCKA_ENOMEM, "paired overflow word");
  HIPCHK(c, hipMemsetAsync(c->d_pflag, 0, sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_paired_capture(g, g.n_grids * g.grid_size, snap, c->d_pflag, c->stream));
  uint32_t ovf = 0;
  int rc;
  if ((rc = read_flag(c, c->d_pflag, &ovf)) != CCKA_OK) return rc;
  if (ovf) return fail(c, CCKA_EOVERFLOW, "a gCO2 or energy value has no int64 fixed-point form (llrint(x * 1e6))");
  return CCKA_OK;
}

// the baseline of current columns `cur` in a snapshot of snap_n scenarios from
// global grid snap_first_grid: one grid of it, or (CCKA_PAIRED_SAME) the grid of the same id
int paired_baseline(ccka_ctx* c, const GridSrc& cur, int64_t snap_n, int64_t snap_first_grid, int64_t base_grid,
                    PairedBase* out) {
  const int64_t gs = cur.grid_size, sng = snap_n / gs;
  PairedBase b{};
  if (base_grid == CCKA_PAIRED_SAME) {
    if (cur.first_grid < snap_first_grid || cur.first_grid + cur.n_grids > snap_first_grid + sng)
      return fail(c, CCKA_EINVAL, "grids [%lld, %lld) are not all inside the snapshot's [%lld, %lld)",
                  (long long)cur.first_grid, (long long)(cur.first_grid + cur.n_grids), (long long)snap_first_grid,
                  (long long)(snap_first_grid + sng));
    b.grid = cur.first_grid;
    b.step = gs;
  } else {
    if (base_grid < snap_first_grid || base_grid >= snap_first_grid + sng)
      return fail(c, CCKA_EINVAL, "base_grid %lld outside the snapshot's [%lld, %lld)", (long long)base_grid,
                  (long long)snap_first_grid, (long long)(snap_first_grid + sng));
    b.grid = base_grid;
    b.step = 0;
  }
  b.off = (b.grid - snap_first_grid) * gs;
  *out = b;
  return CCKA_OK;
}

// the kernel's arguments for current columns `cur` against a snapshot of
// snap_n scenarios from global grid snap_first_grid, under the validated *sp
static int paired_params(ccka_ctx* c, const GridSrc& cur, const int64_t* snap, int64_t snap_n,
                         int64_t snap_first_grid, const ccka_paired_spec* sp, PairedParams* out) {
  PairedBase b{};
  int rc;
  if ((rc = paired_baseline(c, cur, snap_n, snap_first_grid, sp->base_grid, &b)) != CCKA_OK) return rc;
  PairedParams p{};
  p.cur = cur;
  p.snap = snap;
  p.snap_n = snap_n;
  p.base_grid = b.grid;
  p.base_step = b.step;
  p.base_off = b.off;
  for (int j = 0; j < 4; ++j) {
    p.kind[j] = sp->stat.kind[j];
    p.rank[j] = p.kind[j] == CCKA_STAT_SUM ? 1 : ccka_sweep_rank(cur.grid_size, sp->stat.q_ppm[j]);
  }
  *out = p;
  return CCKA_OK;
}

// d_prows[0 .. n_grids) = the rows of p (its rows and flag are set here), the flag cleared first
static int paired_launch(ccka_ctx* c, PairedParams& p) {
  if (!all_or_none(c->d_prows.reserve(p.cur.n_grids) && c->d_pflag.reserve(1), c->d_prows, c->d_pflag))
    return fail(c, CCKA_ENOMEM, "paired rows (%lld)", (long long)p.cur.n_grids);
  p.rows = c->d_prows;
  p.flag = c->d_pflag;
  HIPCHK(c, hipMemsetAsync(c->d_pflag, 0, sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_paired(p, c->stream));
  return CCKA_OK;
}

// rows -> out, then the overflow word
static int paired_out(ccka_ctx* c, const PairedParams& p, ccka_paired_row* out) {
  HIPCHK(c, hipMemcpyAsync(out, c->d_prows, sizeof(ccka_paired_row) * p.cur.n_grids, hipMemcpyDeviceToHost,
                           c->stream));
  uint32_t ovf = 0;
  int rc;
  if ((rc = read_flag(c, c->d_pflag, &ovf)) != CCKA_OK) return rc;
  if (ovf)
    return fail(c, CCKA_EOVERFLOW, "a current value has no int64 fixed-point form, or a delta leaves int64");
  return CCKA_OK;
}

int paired_state(ccka_ctx* c) {
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  if (!c->have_snap) return fail(c, CCKA_ESTATE, "no snapshot (ccka_paired_capture / ccka_paired_import)");
  return CCKA_OK;
}

int paired_rollout_shape(ccka_ctx* c, int64_t grid_size) {
  int rc;
  if ((rc = paired_shape(c, grid_size, c->n_traces, c->first_id, c->N)) != CCKA_OK) return rc;
  if (grid_size != c->snap_grid_size || c->n_traces != c->snap_traces)
    return fail(c, CCKA_EINVAL, "grid_size %lld / n_traces %lld differ from the snapshot's %lld / %lld",
                (long long)grid_size, (long long)c->n_traces, (long long)c->snap_grid_size,
                (long long)c->snap_traces);
  return CCKA_OK;
}

// the last rollout's batch against the context's snapshot: state, then every
// rule of the spec, all before anything is launched
static int paired_of_rollout(ccka_ctx* c, const ccka_paired_spec* sp, PairedParams* p) {
  int rc;
  if ((rc = paired_state(c)) != CCKA_OK) return rc;
  if ((rc = check_sweep_stat(c, &sp->stat)) != CCKA_OK) return rc;
  if ((rc = paired_rollout_shape(c, sp->grid_size)) != CCKA_OK) return rc;
  return paired_params(c, result_columns(c->res, sp->grid_size, c->first_id, c->N), c->d_snap, c->snap_n,
                       c->snap_first / c->snap_grid_size, sp, p);
}

int PairedDebugCols::upload(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const double* gco2,
                            const double* energy, int64_t n, const int64_t* bcost, const int32_t* bslo,
                            const double* bgco2, const double* benergy, int64_t nb, int64_t gs) {
  if (gs < 1 || gs > kPairedMaxGridSize || n < 1 || nb < 1 || n % gs || nb % gs || n / gs > kPairedMaxGrids ||
      nb / gs > kPairedMaxGrids)
    return fail(c, CCKA_EINVAL, "%lld / %lld scenarios do not hold whole grids of %lld", (long long)n, (long long)nb,
                (long long)gs);
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = dupload(c, d_cost, cost, (size_t)n)) != CCKA_OK || (rc = dupload(c, d_slo, slo, (size_t)n)) != CCKA_OK ||
      (rc = dupload(c, d_gco2, gco2, (size_t)n)) != CCKA_OK || (rc = dupload(c, d_energy, energy, (size_t)n)) != CCKA_OK ||
      (rc = dupload(c, d_bcost, bcost, (size_t)nb)) != CCKA_OK || (rc = dupload(c, d_bslo, bslo, (size_t)nb)) != CCKA_OK ||
      (rc = dupload(c, d_bgco2, bgco2, (size_t)nb)) != CCKA_OK ||
      (rc = dupload(c, d_benergy, benergy, (size_t)nb)) != CCKA_OK)
    return rc;
  if (!d_snap.resize(4 * nb)) return fail(c, CCKA_ENOMEM, "snapshot of %lld scenarios", (long long)nb);
  GridSrc base{};
  cur = GridSrc{};
  cur.cost = d_cost; cur.slo = d_slo; cur.gco2 = d_gco2; cur.energy = d_energy;
  cur.grid_size = gs; cur.n_grids = n / gs;
  base.cost = d_bcost; base.slo = d_bslo; base.gco2 = d_bgco2; base.energy = d_benergy;
  base.grid_size = gs; base.n_grids = nb / gs;
  return capture_into(c, base, d_snap);  // synchronises: the uploads are done whatever it returns
}

extern "C" {

int32_t ccka_paired_sizes(int64_t* out, int32_t n) {
  const int64_t s[] = {sizeof(ccka_paired_spec), sizeof(ccka_paired_obj), sizeof(ccka_paired_row)};
  int32_t k = 0;
  for (; out && k < 3 && k < n; ++k) out[k] = s[k];
  return k;
}

int ccka_paired_capture(ccka_ctx* c, int64_t grid_size) {
  if (!c) return CCKA_EINVAL;
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  int rc;
  if ((rc = paired_shape(c, grid_size, c->n_traces, c->first_id, c->N)) != CCKA_OK) return rc;
  (void)hipSetDevice(c->device);
  c->have_snap = false;  // from here on the earlier snapshot is gone
  if (!c->d_snap.resize(4 * c->N)) return fail(c, CCKA_ENOMEM, "snapshot of %lld scenarios", (long long)c->N);
  if ((rc = capture_into(c, result_columns(c->res, grid_size, c->first_id, c->N), c->d_snap)) != CCKA_OK) return rc;
  c->snap_first = c->first_id;
  c->snap_n = c->N;
  c->snap_grid_size = grid_size;
  c->snap_traces = c->n_traces;
  c->have_snap = true;
  return CCKA_OK;
}

int ccka_paired_export(ccka_ctx* c, int64_t grid, int64_t* out, int64_t count) {
  if (!c) return CCKA_EINVAL;
  if (!out) return fail(c, CCKA_EINVAL, "null output");
  if (!c->have_snap) return fail(c, CCKA_ESTATE, "no snapshot (ccka_paired_capture / ccka_paired_import)");
  const int64_t gs = c->snap_grid_size, first = c->snap_first / gs;
  if (grid < first || grid >= first + c->snap_n / gs)
    return fail(c, CCKA_EINVAL, "grid %lld outside the snapshot's [%lld, %lld)", (long long)grid, (long long)first,
                (long long)(first + c->snap_n / gs));
  if (count != 4 * gs) return fail(c, CCKA_EINVAL, "count %lld != 4 * grid_size %lld", (long long)count, (long long)gs);
  (void)hipSetDevice(c->device);
  for (int o = 0; o < 4; ++o)
    HIPCHK(c, hipMemcpyAsync(out + o * gs, c->d_snap + o * c->snap_n + (grid - first) * gs, sizeof(int64_t) * gs,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_paired_import(ccka_ctx* c, int64_t grid_size, int64_t n_traces, int64_t grid, const int64_t* in,
                       int64_t count) {
  if (!c) return CCKA_EINVAL;
  if (!in) return fail(c, CCKA_EINVAL, "null block");
  int rc;
  if ((rc = paired_shape(c, grid_size, n_traces, 0, grid_size)) != CCKA_OK) return rc;
  if (grid < 0 || grid >= kPairedMaxGrids) return fail(c, CCKA_EINVAL, "grid %lld not in [0, 2^24)", (long long)grid);
  if (count != 4 * grid_size)
    return fail(c, CCKA_EINVAL, "count %lld != 4 * grid_size %lld", (long long)count, (long long)grid_size);
  (void)hipSetDevice(c->device);
  c->have_snap = false;
  if (!c->d_snap.resize(count)) return fail(c, CCKA_ENOMEM, "snapshot of %lld scenarios", (long long)grid_size);
  HIPCHK(c, hipMemcpyAsync(c->d_snap, in, sizeof(int64_t) * count, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's block may go
  c->snap_first = grid * grid_size;
  c->snap_n = grid_size;
  c->snap_grid_size = grid_size;
  c->snap_traces = n_traces;
  c->have_snap = true;
  return CCKA_OK;
}

int ccka_get_paired(ccka_ctx* c, const ccka_paired_spec* spec, ccka_paired_row* out, int64_t n_rows) {
  if (!c) return CCKA_EINVAL;
  if (!spec || !out) return fail(c, CCKA_EINVAL, "null paired spec or output");
  (void)hipSetDevice(c->device);
  PairedParams p{};
  int rc;
  if ((rc = paired_of_rollout(c, spec, &p)) != CCKA_OK) return rc;
  if (n_rows != p.cur.n_grids)
    return fail(c, CCKA_EINVAL, "n_rows %lld != %lld", (long long)n_rows, (long long)p.cur.n_grids);
  if ((rc = paired_launch(c, p)) != CCKA_OK) return rc;
  return paired_out(c, p, out);
}

// Internal (not in include/ccka.h): ccka_get_paired's two kernels on
// caller-supplied result columns instead of a rollout's and a context
// snapshot's, so a test can feed values no rollout produces: `n` current and
// `nb` baseline scenarios as whole grids of spec->grid_size, grid ids from 0 on
// both sides; the baseline columns go through the capture kernel into a
// snapshot of their own (the context's stays). out[n / grid_size].
int ccka_debug_paired(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const double* gco2, const double* energy,
                      int64_t n, const int64_t* bcost, const int32_t* bslo, const double* bgco2,
                      const double* benergy, int64_t nb, const ccka_paired_spec* spec, ccka_paired_row* out) {
  if (!c) return CCKA_EINVAL;
  if (!cost || !slo || !gco2 || !energy || !bcost || !bslo || !bgco2 || !benergy || !spec || !out)
    return fail(c, CCKA_EINVAL, "null columns, spec or output");
  int rc;
  if ((rc = check_sweep_stat(c, &spec->stat)) != CCKA_OK) return rc;
  PairedDebugCols cols;
  rc = cols.upload(c, cost, slo, gco2, energy, n, bcost, bslo, bgco2, benergy, nb, spec->grid_size);
  PairedParams p{};
  if (rc == CCKA_OK) rc = paired_params(c, cols.cur, cols.d_snap, nb, 0, spec, &p);
  if (rc == CCKA_OK) rc = paired_launch(c, p);
  if (rc == CCKA_OK) rc = paired_out(c, p, out);
  (void)hipStreamSynchronize(c->stream);  // before the columns are freed
  return rc;
}

// Internal (not in include/ccka.h; tools/paired_time.py): device time of the
// two kernels on the last rollout's results against the context's snapshot,
// each alone. One sample = `reps` back-to-back launches between two HIP events
// on the engine's stream, divided by reps; the median of 5 samples after a
// warm-up launch. capture_ms: paired_capture_kernel (into a scratch snapshot);
// paired_ms: paired_kernel for *spec.
int ccka_debug_paired_ms(ccka_ctx* c, const ccka_paired_spec* spec, int32_t reps, double* capture_ms,
                         double* paired_ms) {
  if (!c || !capture_ms || !paired_ms || reps < 1 || reps > 1000) return CCKA_EINVAL;
  if (!spec) return fail(c, CCKA_EINVAL, "null paired spec");
  (void)hipSetDevice(c->device);
  PairedParams p{};
  int rc;
  if ((rc = paired_of_rollout(c, spec, &p)) != CCKA_OK) return rc;
  DevBuf<int64_t> scratch;
  if (!scratch.resize(4 * c->N)) return fail(c, CCKA_ENOMEM, "scratch snapshot");
  if ((rc = capture_into(c, p.cur, scratch)) != CCKA_OK) return rc;  // warm-up of both kernels
  if ((rc = paired_launch(c, p)) != CCKA_OK) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;  // own events: ccka_last_kernel_ms keeps the rollout's
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(c, CCKA_EHIP, "timing events");
  double med[2] = {0.0, 0.0};
  for (int which = 0; which < 2 && rc == CCKA_OK; ++which) {
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 5 && rc == CCKA_OK; ++k) {
      bool ok = hipEventRecord(e0, c->stream) == hipSuccess;
      for (int r = 0; r < reps && ok; ++r)
        ok = (which ? launch_paired(p, c->stream)
                    : launch_paired_capture(p.cur, c->N, scratch, c->d_pflag, c->stream)) == hipSuccess;
      ok = ok && hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
           hipEventElapsedTime(&ms[k], e0, e1) == hipSuccess;
      if (!ok) rc = fail(c, CCKA_EHIP, "timed launches (kernel %d, sample %d)", which, k);
    }
    if (rc != CCKA_OK) break;
    std::sort(ms, ms + 5);
    med[which] = (double)ms[2] / reps;
  }
  (void)hipStreamSynchronize(c->stream);  // before the scratch snapshot is freed
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != CCKA_OK) return rc;
  *capture_ms = med[0];
  *paired_ms = med[1];
  return CCKA_OK;
}

}  // extern "C"
