// abi_debug.cpp — libccka.so's internal hooks (not part of include/ccka.h):
// the switches tests, tools and bench.py use to force an engine, a layout or a
// diagnostic, the copy-ceiling probe, the phase stamps and the device info.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "ctx.h"
#include "host_rules.h"

using namespace ccka;

// the 12 diagnostic phase stamps, allocated once and zeroed on the stream
int stamps_buffer(ccka_ctx* c, unsigned long long** out) {
  if (!c->d_stamps.reserve(12)) return fail(c, CCKA_ENOMEM, "stamps alloc");
  HIPCHK(c, hipMemsetAsync(c->d_stamps, 0, 12 * sizeof(unsigned long long), c->stream));
  *out = c->d_stamps;
  return CCKA_OK;
}

extern "C" {

// Internal: the device copy ceiling, GB/s of read + write of a `bytes`-byte
// dwordx4 streaming copy (launch_copy16), the median of `reps` launches timed
// with HIP events on the engine's stream after one warm-up launch.
int ccka_debug_copy_gbs(ccka_ctx* c, int64_t bytes, int32_t reps, double* gbs) {
  if (!c || !gbs || bytes < (1 << 20) || reps < 1 || reps > 64) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  bytes &= ~(int64_t)4095;
  DevBuf<char> a, b;
  if (!a.resize(bytes) || !b.resize(bytes))
    return fail(c, CCKA_ENOMEM, "copy probe alloc (2 x %lld bytes)", (long long)bytes);
  int rc = CCKA_OK;
  std::vector<float> ms((size_t)reps);
  hipEvent_t e0 = nullptr, e1 = nullptr;  // own events: ccka_last_kernel_ms keeps the rollout's
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    rc = fail(c, CCKA_EHIP, "copy probe events");
  if (rc == CCKA_OK && (hipMemsetAsync(a, 1, (size_t)bytes, c->stream) != hipSuccess ||
      launch_copy16(a, b, bytes, c->cus, c->stream) != hipSuccess))
    rc = fail(c, CCKA_EHIP, "copy probe warm-up");
  for (int k = 0; k < reps && rc == CCKA_OK; ++k) {
    if (hipEventRecord(e0, c->stream) != hipSuccess || launch_copy16(a, b, bytes, c->cus, c->stream) != hipSuccess ||
        hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
        hipEventElapsedTime(&ms[(size_t)k], e0, e1) != hipSuccess)
      rc = fail(c, CCKA_EHIP, "copy probe launch %d", k);
  }
  (void)hipStreamSynchronize(c->stream);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != CCKA_OK) return rc;
  std::sort(ms.begin(), ms.end());
  *gbs = 2.0 * (double)bytes / ((double)ms[(size_t)reps / 2] * 1e-3) / 1e9;
  return CCKA_OK;
}

// Internal profiling hook: phase-ablation mask for timing attribution only;
// results of an ablated run are meaningless.
int ccka_debug_ablate(ccka_ctx* c, int32_t mask) {
  if (!c) return CCKA_EINVAL;
  c->ablate = mask;
  return CCKA_OK;
}

// Internal: 0 = choose the engine automatically, 1 = always the general kernel
// (tests compare both engines), 2 = the general kernel in lockstep (no
// lane-skewed schedule for several deployments), 3 = automatic with the skewed
// schedule's provisioning on the wave-cooperative scans (A/B of the lane-local one).
int ccka_debug_engine(ccka_ctx* c, int32_t mode) {
  if (!c || mode < 0 || mode > 3) return CCKA_EINVAL;
  c->sk_coop_f2 = mode == 3;
  c->engine_mode = mode == 3 ? 0 : mode;
  return CCKA_OK;
}

// Internal: which engine ran last (1 general, 2 single-deployment, 3 the
// launched closed loop, 4 the fused closed loop, 5 the general kernel on the
// lane-skewed schedule) and the duration of its argmin-table kernel.
int ccka_debug_last_engine(ccka_ctx* c, int32_t* engine, double* table_ms) {
  if (!c) return CCKA_EINVAL;
  if (engine) *engine = c->last_engine;
  if (table_ms) *table_ms = c->last_table_ms;
  return CCKA_OK;
}

// Internal: the launch plan of the last whole-horizon rollout
// (ccka_rollout / ccka_rollout_async), in kparams.h PlanField order:
// workgroups, span, all_hours, hlen, dynamic LDS bytes, lane-local
// provisioning, shared traces, then the single-deployment kernel's lds_tab,
// NW, NZI, JT and instantiation (slots * 100 + pools). -1 = the field does not
// apply to the engine that ran. The closed loops record none (CCKA_ESTATE).
// Reads state only.
int ccka_debug_last_plan(ccka_ctx* c, int32_t out[12]) {
  static_assert(PLAN_FIELDS == 12, "ccka_debug_last_plan's out[12]");
  if (!c || !out) return CCKA_EINVAL;
  if (!c->res_valid || c->last_engine == 3 || c->last_engine == 4) return fail(c, CCKA_ESTATE, "no whole-horizon rollout ran last");
  std::copy(c->last_plan, c->last_plan + PLAN_FIELDS, out);
  return CCKA_OK;
}

// Internal: rows per policy-gradient backward chunk (0 = the default 2^23), to
// exercise the chunked sum at test sizes. Any row count: a chunk that is no
// multiple of the 32-row tile ends in padding rows like the last one does.
int ccka_debug_pg_chunk(ccka_ctx* c, int64_t rows) {
  if (!c || rows < 0) return CCKA_EINVAL;
  c->pg_chunk = rows;
  return CCKA_OK;
}

// Internal: 0 = the fused loop scans the catalog for its launches (A/B of the
// argmin tables; same results).
int ccka_debug_policy_table(ccka_ctx* c, int32_t on) {
  if (!c) return CCKA_EINVAL;
  c->pol_table_off = on == 0;
  return CCKA_OK;
}

// Internal: 0 = the launched closed loop even where the fused one applies.
int ccka_debug_policy_fused(ccka_ctx* c, int32_t on) {
  if (!c) return CCKA_EINVAL;
  c->pol_fused_off = on == 0;
  return CCKA_OK;
}

// Internal: 0 = enqueue the closed loop's launches directly instead of
// replaying its captured hipGraph (1, the default).
int ccka_debug_policy_graph(ccka_ctx* c, int32_t on) {
  if (!c) return CCKA_EINVAL;
  c->pol_graph_off = on == 0;
  return CCKA_OK;
}

// Internal: scenarios per wave of the single-deployment kernel (1..64; 0 = automatic).
int ccka_debug_lpw(ccka_ctx* c, int32_t lpw) {
  if (!c || lpw < 0 || lpw > 64) return CCKA_EINVAL;
  c->lpw = lpw;
  return CCKA_OK;
}

// Internal: 1 = the single-deployment kernel reads the [T][N] trace instead of
// its wave-tiled copy (layout A/B; results are the same).
int ccka_debug_trace_flat(ccka_ctx* c, int32_t on) {
  if (!c) return CCKA_EINVAL;
  c->trace_flat = on != 0;
  return CCKA_OK;
}

// Internal: occupancy target of the single-deployment kernel (2, 3; 0 = automatic).
int ccka_debug_occ(ccka_ctx* c, int32_t occ) {
  if (!c || occ < 0 || occ > 3 || occ == 1) return CCKA_EINVAL;
  c->occ = occ;
  return CCKA_OK;
}

// Internal: the standalone forward's MFMA tile (16: mlp16_kernel, 32: mlp_kernel).
int ccka_debug_mlp_tile(ccka_ctx* c, int32_t tile) {
  if (!c || (tile != 16 && tile != 32)) return CCKA_EINVAL;
  c->mlp_tile = tile;
  return CCKA_OK;
}

// Internal: diagnostic phase stamps of the MLP kernel (read with ccka_debug_stamps).
int ccka_debug_mlp_stamps(ccka_ctx* c, int32_t enable) {
  if (!c) return CCKA_EINVAL;
  c->mlp_stamps = enable != 0;
  return CCKA_OK;
}

// Internal: per-phase cycle totals of the last stamped run (ablate bit 16, or
// ccka_debug_mlp_stamps), 12 words.
int ccka_debug_stamps(ccka_ctx* c, unsigned long long* out8) {
  if (!c || !out8 || !c->d_stamps) return CCKA_EINVAL;
  HIPCHK(c, hipMemcpy(out8, c->d_stamps, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return CCKA_OK;
}

// Internal: ccka_get_totals' reduction (totals_of: the same partials rule,
// buffers and overflow read-back) on caller-supplied result columns of n
// scenarios instead of the last rollout's, so a test can feed sums no rollout
// reaches. The columns are carved like a rollout's (carve_results). Needs no
// world or scenarios; the totals, or CCKA_EOVERFLOW.
int ccka_debug_totals(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const int64_t* pend_min,
                      const int32_t* nmin_spot, const int32_t* nmin_od, const int32_t* launches,
                      const int32_t* deletions, const double* energy, const double* gco2, int64_t n,
                      ccka_totals* out) {
  if (!c || !cost || !slo || !pend_min || !nmin_spot || !nmin_od || !launches || !deletions || !energy || !gco2 ||
      !out || n < 1 || n > (int64_t)1 << 31)
    return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  DevBuf<char> d_res;
  if (!d_res.resize(carve_results(nullptr, n, nullptr))) return fail(c, CCKA_ENOMEM, "totals columns (%lld)", (long long)n);
  ResultPtrs r{};
  carve_results(d_res, n, &r);
  struct { void* dst; const void* src; size_t sz; } m[] = {
      {r.cost, cost, 8}, {r.slo, slo, 4}, {r.pend_min, pend_min, 8}, {r.nmin_spot, nmin_spot, 4},
      {r.nmin_od, nmin_od, 4}, {r.launches, launches, 4}, {r.deletions, deletions, 4}, {r.energy, energy, 8},
      {r.gco2, gco2, 8}};
  for (auto& x : m) HIPCHK(c, hipMemcpyAsync(x.dst, x.src, (size_t)n * x.sz, hipMemcpyHostToDevice, c->stream));
  const int rc = totals_of(c, r, n, out);
  (void)hipStreamSynchronize(c->stream);  // before the columns are freed
  return rc;
}

// Internal: staging capacity in records of ccka_get_trajectory's transpose
// (0 = the default 4 Mi), to run blocks of 1 < tc < T steps at test sizes.
int ccka_debug_traj_stage(ccka_ctx* c, int64_t records) {
  if (!c || records < 0) return CCKA_EINVAL;
  c->traj_stage = records;
  return CCKA_OK;
}

// Internal: one of the two trace copies on a caller-supplied [T][D][NL] trace,
// the whole output buffer returned, padding included: DP > 0 runs
// launch_trace_nt (sk_trace's copy, [NL][T][DP], trace_nt_count elements),
// DP == 0 launch_trace_tile (d1_trace_tile's, D == 1, [wave][T][lpw],
// trace_tile_count elements). The buffer is filled with `sentinel` first.
int ccka_debug_trace_layout(ccka_ctx* c, const int32_t* in, int64_t T, int32_t D, int64_t NL, int32_t DP,
                            int32_t lpw, int32_t sentinel, int32_t* out, int64_t out_count) {
  if (!c || !in || !out || T < 1 || D < 1 || NL < 1 || T > 65535 || NL > (int64_t)1 << 31) return CCKA_EINVAL;
  if (DP == 0 && (D != 1 || lpw < 1 || lpw > 64)) return CCKA_EINVAL;
  if (DP != 0 && (D > DP || (DP != 2 && DP != 4 && DP != 8 && DP != 16))) return CCKA_EINVAL;
  const int64_t cnt = DP ? trace_nt_count(NL, T, DP) : trace_tile_count(NL, T, lpw);
  if (out_count != cnt) return fail(c, CCKA_EINVAL, "layout holds %lld ints, not %lld", (long long)cnt, (long long)out_count);
  (void)hipSetDevice(c->device);
  DevBuf<int32_t> d_in, d_out;
  int rc;
  if ((rc = dupload(c, d_in, in, (size_t)(T * D * NL))) != CCKA_OK) return rc;
  if (!d_out.resize(cnt)) return fail(c, CCKA_ENOMEM, "layout buffer");
  HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)d_out.get(), sentinel, (size_t)cnt, c->stream));
  HIPCHK(c, DP ? launch_trace_nt(d_in, d_out, NL, T, D, DP, c->stream) : launch_trace_tile(d_in, d_out, NL, T, lpw, c->stream));
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)cnt * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // before the buffers are freed
  return CCKA_OK;
}

int ccka_device_info(ccka_ctx* c, char* name, int32_t name_len, int32_t* cu_count) {
  if (!c) return CCKA_EINVAL;
  if (name && name_len > 0) std::snprintf(name, (size_t)name_len, "%s", c->name);
  if (cu_count) *cu_count = c->cus;
  return CCKA_OK;
}

}  // extern "C"
