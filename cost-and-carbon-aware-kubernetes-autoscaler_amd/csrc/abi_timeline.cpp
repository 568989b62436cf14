// abi_timeline.cpp — the fleet timeline of libccka.so's C ABI (SEMANTICS 7):
// the last rollout's trajectory records reduced per (grid, step bucket) on the
// device (timeline.hip), in whichever layout the engine wrote them.
#include <algorithm>

#include "ctx.h"

using namespace ccka;

constexpr int64_t kTlMaxRows = 1 << 24;
constexpr int64_t kTlMaxSamples = (int64_t)1 << 31;  // per row: counts fit 32 bits, sums stay below 2^62

// rows of the timeline of n scenarios x T steps under *sp, or -1 with the rule
// that fails in *why (nullable)
static int64_t timeline_shape(int64_t n, int32_t T, const ccka_timeline_spec* sp, const char** why) {
  auto bad = [why](const char* rule) {
    if (why) *why = rule;
    return (int64_t)-1;
  };
  if (!sp) return bad("null timeline spec");
  if (n < 1 || T < 1) return bad("no scenarios or no steps");
  if (sp->grid_size < 1 || n % sp->grid_size) return bad("the batch does not hold whole grids");
  if (sp->step_bucket < 1) return bad("step_bucket < 1");
  if (sp->q_field < CCKA_TL_NONE || sp->q_field > CCKA_TL_NODES) return bad("q_field not in 0..3");
  if (sp->q_field != CCKA_TL_NONE && (sp->q_ppm < 0 || sp->q_ppm > 1000000)) return bad("q_ppm not in [0, 1000000]");
  const int64_t width = std::min<int64_t>(sp->step_bucket, T);
  if (sp->grid_size > kTlMaxSamples / width) return bad("grid_size * min(step_bucket, n_steps) > 2^31");
  const int64_t n_buckets = ((int64_t)T + sp->step_bucket - 1) / sp->step_bucket;
  if (n / sp->grid_size > kTlMaxRows / n_buckets) return bad("more than 2^24 rows");
  return n / sp->grid_size * n_buckets;
}

// d_tlrows[0 .. rows) = the timeline of `recs` (n x T records, `nt` layout,
// grids from first_grid) under the validated *sp
static int timeline_run(ccka_ctx* c, const ccka_traj_rec* recs, int64_t n, int32_t T, bool nt, int64_t first_grid,
                        const ccka_timeline_spec* sp, int64_t rows, TimelineParams* out) {
  if (!c->d_tlrows.reserve(rows)) return fail(c, CCKA_ENOMEM, "timeline rows (%lld)", (long long)rows);
  TimelineParams p{};
  p.recs = recs;
  p.rows = c->d_tlrows;
  p.N = n;
  p.G = sp->grid_size;
  p.n_grids = n / sp->grid_size;
  p.first_grid = first_grid;
  p.T = T;
  p.B = (int32_t)std::min<int64_t>(sp->step_bucket, T);  // wider buckets are the one bucket [0, T)
  p.n_buckets = (int32_t)(rows / p.n_grids);
  p.nt = nt ? 1 : 0;
  p.q_field = sp->q_field;
  p.q_ppm = sp->q_ppm;
  HIPCHK(c, launch_timeline_sum(p, c->cus, c->stream));
  if (p.q_field != CCKA_TL_NONE) HIPCHK(c, launch_timeline_select(p, c->cus, c->stream));
  if (out) *out = p;
  return CCKA_OK;
}

// the last rollout's records under *sp: state, then the spec's rules, then the
// caller's row count (want_rows >= 0), all before anything is launched
static int timeline_of_rollout(ccka_ctx* c, const ccka_timeline_spec* sp, int64_t want_rows, int64_t* rows,
                               TimelineParams* p) {
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  if (!c->traj_valid) return fail(c, CCKA_ESTATE, "last rollout had no trajectory");
  const int32_t T = c->hw.n_steps;
  if (c->d_traj.count() != (int64_t)T * c->N) return fail(c, CCKA_ESTATE, "trajectory does not match the batch");
  const char* why = "";
  *rows = timeline_shape(c->N, T, sp, &why);
  if (*rows < 0) return fail(c, CCKA_EINVAL, "timeline: %s", why);
  if (c->first_id % sp->grid_size)
    return fail(c, CCKA_EINVAL, "batch (first_id %lld, n %lld) does not hold whole grids of %lld",
                (long long)c->first_id, (long long)c->N, (long long)sp->grid_size);
  if (want_rows >= 0 && want_rows != *rows)
    return fail(c, CCKA_EINVAL, "n_rows %lld != %lld", (long long)want_rows, (long long)*rows);
  return timeline_run(c, c->d_traj, c->N, T, c->traj_nt, c->first_id / sp->grid_size, sp, *rows, p);
}

extern "C" {

int64_t ccka_timeline_rows(int64_t n, int32_t n_steps, const ccka_timeline_spec* spec) {
  return timeline_shape(n, n_steps, spec, nullptr);
}

int ccka_get_timeline(ccka_ctx* c, const ccka_timeline_spec* spec, ccka_timeline_row* out, int64_t n_rows) {
  if (!c) return CCKA_EINVAL;
  if (!spec || !out) return fail(c, CCKA_EINVAL, "null timeline spec or output");
  (void)hipSetDevice(c->device);
  if (n_rows < 0) return fail(c, CCKA_EINVAL, "n_rows %lld", (long long)n_rows);
  int64_t rows = 0;
  int rc;
  if ((rc = timeline_of_rollout(c, spec, n_rows, &rows, nullptr)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->d_tlrows, sizeof(ccka_timeline_row) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

// Internal (not in include/ccka.h): ccka_get_timeline's kernel path on
// caller-supplied records, n scenarios x n_steps in the stated layout
// (CCKA_TRAJ_TN: [n_steps][n], CCKA_TRAJ_NT: [n][n_steps]), grid ids from 0,
// so a test can feed values no rollout produces. out[ccka_timeline_rows(...)].
int ccka_debug_timeline(ccka_ctx* c, const ccka_traj_rec* recs, int64_t n, int32_t n_steps, int32_t layout,
                        const ccka_timeline_spec* spec, ccka_timeline_row* out) {
  if (!c) return CCKA_EINVAL;
  if (!recs || !out || (layout != CCKA_TRAJ_TN && layout != CCKA_TRAJ_NT))
    return fail(c, CCKA_EINVAL, "null records or output, or an unknown layout");
  const char* why = "";
  const int64_t rows = timeline_shape(n, n_steps, spec, &why);
  if (rows < 0) return fail(c, CCKA_EINVAL, "timeline: %s", why);
  (void)hipSetDevice(c->device);
  DevBuf<ccka_traj_rec> d_recs;
  int rc;
  if ((rc = dupload(c, d_recs, recs, (size_t)(n * n_steps))) != CCKA_OK) return rc;
  if ((rc = timeline_run(c, d_recs, n, n_steps, layout == CCKA_TRAJ_NT, 0, spec, rows, nullptr)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->d_tlrows, sizeof(ccka_timeline_row) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // before the records are freed
  return CCKA_OK;
}

// Internal (not in include/ccka.h; tools/timeline_time.py): device time of the
// kernels behind ccka_get_timeline on the last rollout's records. One sample =
// `reps` back-to-back launches between two HIP events on the engine's stream,
// divided by reps; the median of 5 samples after a warm-up. sum_ms: the row
// initialisation and timeline_sum_kernel; select_ms: timeline_select_kernel
// (0 for CCKA_TL_NONE).
int ccka_debug_timeline_ms(ccka_ctx* c, const ccka_timeline_spec* spec, int32_t reps, double* sum_ms,
                           double* select_ms) {
  if (!c || !sum_ms || !select_ms || reps < 1 || reps > 1000) return CCKA_EINVAL;
  if (!spec) return fail(c, CCKA_EINVAL, "null timeline spec");
  (void)hipSetDevice(c->device);
  int64_t rows = 0;
  TimelineParams p{};
  int rc;
  if ((rc = timeline_of_rollout(c, spec, -1, &rows, &p)) != CCKA_OK) return rc;  // buffers + warm-up of the kernels
  const bool sel = p.q_field != CCKA_TL_NONE;
  hipEvent_t e0 = nullptr, e1 = nullptr;  // own events: ccka_last_kernel_ms keeps the rollout's
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(c, CCKA_EHIP, "timing events");
  double med[2] = {0.0, 0.0};
  for (int which = 0; which < (sel ? 2 : 1) && rc == CCKA_OK; ++which) {
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 5 && rc == CCKA_OK; ++k) {
      bool ok = hipEventRecord(e0, c->stream) == hipSuccess;
      for (int r = 0; r < reps && ok; ++r)
        ok = (which ? launch_timeline_select(p, c->cus, c->stream) : launch_timeline_sum(p, c->cus, c->stream)) ==
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

}  // extern "C"
