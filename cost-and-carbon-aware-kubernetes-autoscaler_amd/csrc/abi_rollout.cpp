// abi_rollout.cpp — whole-horizon rollouts of libccka.so's C ABI: the launch
// geometry (LDS budget per workgroup from the catalog, the price-tile span and
// the NodeClaim scratch), the general kernel's argument block, the engine
// choice and its trace copies, and reading back results, trajectories and
// totals (summed across GPUs with RCCL).
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "ctx.h"
#include "host_rules.h"

using namespace ccka;

// scenarios per wave of the single-deployment kernel: a wave's cost is the
// union of its lanes' event paths, so when the batch is smaller than one full
// round of resident waves (two per SIMD at this kernel's register budget)
// spread it over all of them
static int32_t d1_lpw(const ccka_ctx* c) {
  if (c->lpw > 0) return c->lpw;
  const int64_t slots = 2LL * 4 * c->cus;  // resident waves: 2 per SIMD, 4 SIMDs per CU
  return (int32_t)std::min<int64_t>(64, std::max<int64_t>(32, (c->N + slots - 1) / slots));
}

// The single-deployment kernel reads a per-scenario trace wave-tiled
// ([wave][T][lanes]): with [T][N] a wave's 196-byte row shares its first and
// last 128-byte lines with the neighbouring waves, which run up to hundreds of
// steps apart (lane skew), so the L2 has evicted those lines before the
// neighbour reads them. Built lazily by the first single-deployment rollout of
// a trace and lanes-per-wave value (never by the policy loop or the general
// kernel, which read [T][N]), beside the [T][N] trace; without the memory for
// it the kernel reads [T][N] (same results). The policy loop frees it.
static int d1_trace_tile(ccka_ctx* c) {
  if (!c->d1_world || c->hw.n_deploy != 1 || c->n_traces > 0 || !c->have_load) return CCKA_OK;
  const int32_t lpw = d1_lpw(c);
  if (c->load_w_lpw == lpw && c->d_load_w) return CCKA_OK;
  const int64_t cnt = trace_tile_count(c->N, c->hw.n_steps, lpw);  // rows lpw wide
  c->load_w_lpw = 0;
  if (!c->d_load_w.resize(cnt)) return CCKA_OK;
  HIPCHK(c, launch_trace_tile(c->d_load, c->d_load_w, c->N, c->hw.n_steps, lpw, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->load_w_lpw = lpw;
  return CCKA_OK;
}

// the skewed schedule's scenario-major trace copy (built once per trace: N*T*DP*4
// bytes; without memory for it the kernel gathers from [T][D][N], same results)
static int sk_trace(ccka_ctx* c) {
  int dmax, nmax;
  kernel_dims(c->hw.n_deploy, c->hw.max_nodes, &dmax, &nmax);
  if (c->load_nt_dp == dmax && c->d_load_nt) return CCKA_OK;
  const int64_t NL = load_cols(c), cnt = trace_nt_count(NL, c->hw.n_steps, dmax);
  c->load_nt_dp = 0;
  if (!c->d_load_nt.resize(cnt)) return CCKA_OK;
  HIPCHK(c, launch_trace_nt(c->d_load, c->d_load_nt, NL, c->hw.n_steps, c->hw.n_deploy, dmax, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->load_nt_dp = dmax;
  return CCKA_OK;
}

static int plan_launch(ccka_ctx* c, KParams& k, int* block, size_t* lds) {
  const ccka_world& w = c->hw;
  const int B = 256;
  int span = 1;
  if (!c->h_region.empty()) {
    for (int64_t b = 0; b < c->N; b += B) {
      const int64_t e = std::min<int64_t>(c->N, b + B);
      int lo = 255, hi = 0;
      for (int64_t i = b; i < e; ++i) { lo = std::min<int>(lo, c->h_region[i]); hi = std::max<int>(hi, c->h_region[i]); }
      span = std::max(span, hi - lo + 1);
    }
  }
  int dmax, nmax;
  kernel_dims(w.n_deploy, w.max_nodes, &dmax, &nmax);
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t K = (size_t)w.n_types;
  size_t off = up16(K * sizeof(ccka_itype));
  k.lds_off_cap1 = (int32_t)off;
  off = up16(off + K * 4);
  k.lds_off_tile = (int32_t)off;
  const size_t tile_bytes = (size_t)span * K * w.n_zones * 2 * 4;
  // stage all 24 hourly tiles when they fit comfortably (no barrier in the step
  // loop); otherwise one hour at a time, restaged at each hour boundary
  k.all_hours = (off + 24 * tile_bytes + 8 * 1024) <= 64 * 1024 ? 1 : 0;
  off = up16(off + (k.all_hours ? 24 : 1) * tile_bytes);
  k.lds_off_claims = (int32_t)off;
  off = up16(off + (size_t)(B / 64) * nmax * (7 + dmax) * 4);
  k.lds_off_misc = (int32_t)off;
  off += 16;
  k.lds_off_ci = (int32_t)off;
  off = up16(off + (size_t)span * 24 * 2 * sizeof(double));
  if (off > 160 * 1024) return fail(c, CCKA_EINVAL, "LDS budget %zu B exceeds 160 KiB (catalog %zu types, span %d)", off, K, span);
  k.span = span;
  *block = B;
  *lds = off;
  return CCKA_OK;
}

// the general kernel's parameters for a whole-horizon rollout: buffers,
// launch geometry, HPA history, detail (shared by ccka_rollout_async and
// ccka_policy_rollout). Initialises every field of the caller's block: what a
// caller does not set afterwards is zero (padding included: the launched
// policy loop keys its captured graph on the block's bytes).
int setup_general(ccka_ctx* c, int32_t trajectory, KParams& k, int* block_out, size_t* lds_out) {
  const ccka_world& w = c->hw;
  int block = 256;
  size_t lds = 0;
  int rc;
  std::memset(&k, 0, sizeof k);  // = KParams{}, and the padding
  if ((rc = plan_launch(c, k, &block, &lds)) != CCKA_OK) return rc;
  *block_out = block;
  *lds_out = lds;
  k.res = c->res;
  k.ablate = c->ablate;
  k.w = c->d_world;
  k.types = c->d_types;
  k.price = c->d_price;
  k.ci_gpwh = c->d_ci_gpwh;
  k.ci_gpwmin = c->d_ci_gpwmin;
  k.load = c->d_load;
  k.region = c->d_region;
  k.target = c->d_target;
  k.maxr = c->d_maxr;
  k.down_stab = c->d_dstab;
  k.reset_ca = c->d_resetca;
  k.pswitch = c->d_pswitch;
  k.cw = c->d_cw;
  k.cap_sel = c->d_capsel;
  if (trajectory) {
    if (!c->d_traj.resize((int64_t)w.n_steps * c->N)) return fail(c, CCKA_ENOMEM, "trajectory alloc");
    k.traj = c->d_traj;
  }
  if (c->detail_on) {
    if (!c->d_detail.resize(c->N)) return fail(c, CCKA_ENOMEM, "detail alloc");
    HIPCHK(c, hipMemsetAsync(c->d_detail, 0, (size_t)c->N * sizeof(DetailDev), c->stream));
    k.detail = c->d_detail;
  }
  // HPA decisions: one per step over the register rings, or nsub per step /
  // long windows / > 2 policies over the HBM history (SEMANTICS 3.C)
  k.sync_s = w.hpa_sync_s > 0 ? w.hpa_sync_s : CCKA_STEP_SECONDS;
  k.nsub = CCKA_STEP_SECONDS / k.sync_s;
  {
    bool fit = k.nsub == 1 && c->sc_dstab_max <= CCKA_HIST * CCKA_STEP_SECONDS;
    int hl = 0;
    for (int d = 0; d < w.n_deploy; ++d) {
      const ccka_deployment& dp = w.deploy[d];
      if (dp.scaler != CCKA_SCALER_HPA && dp.scaler != CCKA_SCALER_KEDA) continue;
      fit = fit && rules_fit_ring(dp.up) && rules_fit_ring(dp.down);
      int dstab = dp.down.stab_window_s;
      if (dp.scaler == CCKA_SCALER_HPA && c->sc_dstab_max >= 0) dstab = std::max(dstab, c->sc_dstab_max);
      hl = std::max({hl, hist_entries(dp.up.stab_window_s, k.sync_s), hist_entries(dstab, k.sync_s)});
      for (const ccka_hpa_rules* r : {&dp.up, &dp.down})
        for (int q = 0; q < r->n_policies; ++q) hl = std::max(hl, hist_entries(r->policies[q].period_s, k.sync_s));
    }
    k.hlen = fit ? 0 : std::max(hl, 1);
    if (k.hlen) {
      const int64_t cnt = (int64_t)k.hlen * w.n_deploy * c->N;
      if (!c->d_hist.reserve(cnt)) return fail(c, CCKA_ENOMEM, "HPA history alloc (%lld entries)", (long long)cnt);
      HIPCHK(c, hipMemsetAsync(c->d_hist, 0, (size_t)cnt * sizeof(int2), c->stream));
      k.hist = c->d_hist;
    }
  }
  k.lds_lclaims = -1;
  k.t1 = w.n_steps;  // the whole horizon [0, T) in one launch, no persisted state
  k.N = c->N;
  k.NL = load_cols(c);
  k.trace_mod = c->n_traces;
  k.first_id = c->first_id;
  k.T = w.n_steps;
  k.D = w.n_deploy;
  k.K = w.n_types;
  k.Z = w.n_zones;
  k.R = w.n_regions;
  k.P = w.n_pools;
  k.maxn = w.max_nodes;
  for (int d = 0; d < CCKA_MAX_DEPLOY; ++d) k.prov[d] = c->prov[d];
  return CCKA_OK;
}

// The general kernel's lane-skewed schedule (rollout_sk.hip) holds for worlds
// of two or more deployments that are HPA-scaled or static, with one HPA
// decision per step over the register history rings, every hour's price tiles
// in LDS, no detail breakdown and no drift / replacement / multi-node
// consolidation (rollout_kernel.h, rollout_kernel's SK notes).
constexpr int kSkMax16 = 32767;
static bool sk_eligible(const ccka_ctx* c, const KParams& k) {
  const ccka_world& w = c->hw;
  if (w.n_deploy < 2 || c->engine_mode == 2 || c->detail_on) return false;
  // up to four deployments: beyond, the per-lane state of the skewed schedule
  // spills (8 x 16 slots: 5.6 KB per lane) and the lockstep kernel is faster
  // (8 deployments 475 vs 307 ms, 12: 1039 vs 695 ms at 1e5 x 1440)
  int dmax, nmax;
  kernel_dims(w.n_deploy, w.max_nodes, &dmax, &nmax);
  if (dmax > 4) return false;
  if (k.nsub != 1 || k.hlen != 0 || !k.all_hours || (k.ablate & ~16) != 0) return false;  // 16: diagnostic counters
  if (w.disrupt_ext & (CCKA_DISRUPT_DRIFT | CCKA_DISRUPT_REPLACE | CCKA_DISRUPT_MULTI)) return false;
  for (int d = 0; d < w.n_deploy; ++d) {
    const int sc = w.deploy[d].scaler;
    if (sc != CCKA_SCALER_HPA && sc != CCKA_SCALER_STATIC) return false;
    if (sc != CCKA_SCALER_HPA) continue;
    // the quiet-step thresholds pack the tolerance band into 16-bit halves and
    // multiply replicas by the target in 32 bits (rollout_kernel.h, q_band):
    // targets and replica counts below 2^15, tolerance in [0, 1) as
    // d1_check_world asks; anything else keeps the lockstep kernel
    const ccka_deployment& dp = w.deploy[d];
    if (dp.target_util_pct <= 0 || dp.target_util_pct > kSkMax16) return false;
    if (!(dp.tolerance >= 0.0 && dp.tolerance < 1.0)) return false;
    if (dp.max_replicas > kSkMax16 || dp.replicas0 > kSkMax16) return false;
  }
  // the per-scenario overrides held in the context are bounded the same way
  if (c->sc_target_max > kSkMax16 || c->sc_maxr_max > kSkMax16) return false;
  return true;
}

extern "C" {

int ccka_rollout_async(ccka_ctx* c, int32_t trajectory) {
  if (!c) return CCKA_EINVAL;
  if (!c->have_world || !c->have_sc) return fail(c, CCKA_ESTATE, "world/scenarios not set");
  if (!c->have_load) return fail(c, CCKA_ESTATE, "no load traces (ccka_set_load / ccka_gen_load)");
  (void)hipSetDevice(c->device);
  const ccka_world& w = c->hw;
  int block = 256;
  size_t lds = 0;
  int rc;
  KParams k;
  if ((rc = setup_general(c, trajectory, k, &block, &lds)) != CCKA_OK) return rc;
  int32_t* const plan = c->last_plan;  // recorded for ccka_debug_last_plan, read by nothing here
  std::fill(plan, plan + PLAN_FIELDS, -1);
  plan[PLAN_TRACE_MOD] = k.trace_mod != 0;
  if (c->engine_mode == 0 && c->d1_world && !c->d1_ready && (rc = d1_prepare(c)) != CCKA_OK) return rc;
  if (c->engine_mode == 0 && c->d1_world && c->d1_ok && !c->detail_on) {
    // single-deployment engine: argmin tables for this rollout, then the rollout
    const TableParams tp = table_params(c, c->d_wc1000, c->NW, c->d_table, c->d_jtab);
    D1Params p = c->d1;  // the digest; this rollout's buffers and choices below
    p.load = c->d_load; p.price = c->d_price; p.ci_gpwmin = c->d_ci_gpwmin; p.acc = c->d_acc;
    p.table = c->d_table; p.jtab = c->d_jtab;
    p.region = c->d_region; p.target = c->d_target; p.maxr = c->d_maxr; p.down_stab = c->d_dstab;
    p.reset_ca = c->d_resetca; p.pswitch = c->d_pswitch; p.wci = c->d_wci; p.cap_sel = c->d_capsel;
    p.res = k.res; p.traj = k.traj;
    p.N = c->N;
    p.NL = k.NL;
    p.trace_mod = k.trace_mod;
    p.first_id = k.first_id;
    p.NW = c->NW;
    p.occ = c->occ > 0 ? c->occ : 2;  // higher targets spill (measured slower: tools/occ.py)
    p.lpw = d1_lpw(c);
    if (!c->trace_flat) {
      if ((rc = d1_trace_tile(c)) != CCKA_OK) return rc;
      if (c->load_w_lpw == p.lpw && c->d_load_w && p.trace_mod == 0) p.load_w = c->d_load_w;
    }
    p.ablate = k.ablate;
    // diagnostic phase stamps (single-deployment engine, 8 slots, 2 pools)
    if ((k.ablate & 16) && (rc = stamps_buffer(c, &p.stamps)) != CCKA_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_table(tp, c->stream));
    if (p.replace || p.multi) {  // the G2 / G3 offer table (price only)
      TableParams t2 = tp;
      t2.wc1000 = c->d_wc0;
      t2.NW = 1;
      t2.offer = 1;
      t2.table = c->d_table2;
      t2.jtab = c->d_jtab2;
      HIPCHK(c, launch_table(t2, c->stream));
      p.table2 = c->d_table2;
    }
    HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
    HIPCHK(c, launch_rollout_d1(p, c->stream, plan));
    plan[PLAN_D1_NW] = c->NW;
    plan[PLAN_D1_NZI] = p.NZI;
    plan[PLAN_D1_JT] = p.JT;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->last_engine = 2;
    c->traj_nt = true;
  } else {
    // (no ptable: the argmin-table launches are the policy loops', weights k / 16)
    // diagnostic phase stamps (read by ccka_debug_stamps; GK_STAMPS builds)
    if ((k.ablate & 16) && (rc = stamps_buffer(c, &k.stamps)) != CCKA_OK) return rc;
    const bool sk = sk_eligible(c, k);
    if (sk) {
      if ((rc = sk_trace(c)) != CCKA_OK) return rc;
      if (c->load_nt_dp) k.load_nt = c->d_load_nt;
      // lane-local provisioning for small catalogs: one LDS column of NodeClaims
      // per lane ([claim][field][lane] ints) when it fits beside the rest
      int dmax, nmax;
      kernel_dims(w.n_deploy, w.max_nodes, &dmax, &nmax);
      const size_t col = ((lds + 15) & ~(size_t)15), need = (size_t)nmax * (7 + dmax) * block * 4;
      if (!c->sk_coop_f2 && rollout_sk_lane_f2() && w.n_types <= 64 && col + need <= 160 * 1024) {
        k.lds_lclaims = (int32_t)col;
        lds = col + need;
      }
    }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
    if (sk) HIPCHK(c, launch_rollout_sk(k, block, lds, c->stream));
    else HIPCHK(c, launch_rollout(k, block, lds, c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    // (a copy of the general launchers' one-line grid rule, not read back from
    // them: one scenario per thread, launch_rollout / _multi / _sk / _sk416)
    plan[PLAN_GRID] = (int32_t)((c->N + block - 1) / block);
    plan[PLAN_SPAN] = k.span;
    plan[PLAN_ALL_HOURS] = k.all_hours;
    plan[PLAN_HLEN] = k.hlen;
    plan[PLAN_LDS] = (int32_t)lds;
    plan[PLAN_LCLAIMS] = k.lds_lclaims >= 0;
    c->last_engine = sk ? 5 : 1;
    c->traj_nt = sk;  // the skewed schedule writes scenario-major records
  }
  c->traj_valid = trajectory != 0;
  c->detail_valid = c->detail_on;
  c->ran = true;
  c->res_valid = true;
  return CCKA_OK;
}

int ccka_set_detail(ccka_ctx* c, int32_t on) {
  if (!c) return CCKA_EINVAL;
  c->detail_on = on != 0;
  return CCKA_OK;
}

int ccka_get_detail(ccka_ctx* c, ccka_detail* out, int64_t count) {
  if (!c || !out) return CCKA_EINVAL;
  if (!c->res_valid || !c->detail_valid) return fail(c, CCKA_ESTATE, "last rollout recorded no detail (ccka_set_detail)");
  if (count != c->N) return fail(c, CCKA_EINVAL, "detail count %lld != %lld scenarios", (long long)count, (long long)c->N);
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy2DAsync(out, sizeof(ccka_detail), c->d_detail, sizeof(DetailDev), sizeof(ccka_detail), (size_t)count,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_sync(ccka_ctx* c) {
  if (!c) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->ran) {
    float ms = 0.f, tab = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_mid, c->ev1));
    HIPCHK(c, hipEventElapsedTime(&tab, c->ev0, c->ev_mid));
    c->last_ms = ms;
    c->last_table_ms = tab;
  }
  return CCKA_OK;
}

int ccka_rollout(ccka_ctx* c, int32_t trajectory) {
  int rc = ccka_rollout_async(c, trajectory);
  if (rc != CCKA_OK) return rc;
  return ccka_sync(c);
}

int ccka_last_kernel_ms(ccka_ctx* c, double* ms) {
  if (!c || !ms) return CCKA_EINVAL;
  if (!c->ran) return fail(c, CCKA_ESTATE, "no rollout yet");
  *ms = c->last_ms;
  return CCKA_OK;
}

int ccka_get_results(ccka_ctx* c, ccka_results* o) {
  if (!c || !o) return CCKA_EINVAL;
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)c->N;
  const ResultPtrs& k = c->res;
  struct { void* dst; const void* src; size_t sz; } m[] = {
      {o->cost_uphmin, k.cost, 8}, {o->energy_wmin, k.energy, 8}, {o->gco2, k.gco2, 8},
      {o->slo_minutes, k.slo, 4}, {o->pending_pod_minutes, k.pend_min, 8},
      {o->node_min_spot, k.nmin_spot, 4}, {o->node_min_od, k.nmin_od, 4},
      {o->launches, k.launches, 4}, {o->deletions, k.deletions, 4}, {o->peak_nodes, k.peak_nodes, 4},
      {o->final_replicas, k.final_reps, 4}, {o->final_nodes, k.final_nodes, 4},
      {o->last_choice, k.last_choice, 4}, {o->choice_hash, k.hash, 4}};
  for (auto& x : m)
    if (x.dst) HIPCHK(c, hipMemcpyAsync(x.dst, x.src, n * x.sz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_get_trajectory(ccka_ctx* c, ccka_traj_rec* out, int64_t count) {
  if (!c || !out) return CCKA_EINVAL;
  if (!c->traj_valid) return fail(c, CCKA_ESTATE, "last rollout had no trajectory");
  if (count != c->d_traj.count()) return fail(c, CCKA_EINVAL, "trajectory count mismatch");
  (void)hipSetDevice(c->device);
  if (!c->traj_nt) {  // already [T][N]
    HIPCHK(c, hipMemcpyAsync(out, c->d_traj, (size_t)count * sizeof(ccka_traj_rec), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CCKA_OK;
  }
  // the single-deployment engine keeps [N][T] on the device: transpose tc
  // steps at a time into a bounded staging buffer (>= one step of N records,
  // else kTrajStageRecs) and copy each block of steps to its place in out.
  // tc comes from the capacity in force, not from the buffer's count(): the
  // buffer only grows (reserve), so a larger one left by an earlier read-back
  // would otherwise change the block size from call to call
  const int64_t N = c->N, T = count / N;
  const int64_t cap = traj_stage_cap(N, count, c->traj_stage);
  if (!c->d_traj_t.reserve(cap)) return fail(c, CCKA_ENOMEM, "trajectory staging alloc (%lld records)", (long long)cap);
  const int64_t tc = cap / N;
  for (int64_t t0 = 0; t0 < T; t0 += tc) {
    const int64_t n = std::min(tc, T - t0);
    HIPCHK(c, launch_traj_transpose(c->d_traj, c->d_traj_t, N, T, t0, n, c->stream));
    HIPCHK(c, hipMemcpyAsync(out + t0 * N, c->d_traj_t, (size_t)(n * N) * sizeof(ccka_traj_rec),
                             hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_trajectory_layout(ccka_ctx* c, int32_t* layout) {
  if (!c || !layout) return CCKA_EINVAL;
  if (!c->traj_valid) return fail(c, CCKA_ESTATE, "last rollout had no trajectory");
  *layout = c->traj_nt ? CCKA_TRAJ_NT : CCKA_TRAJ_TN;
  return CCKA_OK;
}

int ccka_get_trajectory_native(ccka_ctx* c, ccka_traj_rec* out, int64_t count, int32_t* layout) {
  if (!c || !out) return CCKA_EINVAL;
  if (!c->traj_valid) return fail(c, CCKA_ESTATE, "last rollout had no trajectory");
  if (count != c->d_traj.count()) return fail(c, CCKA_EINVAL, "trajectory count mismatch");
  (void)hipSetDevice(c->device);
  if (layout) *layout = c->traj_nt ? CCKA_TRAJ_NT : CCKA_TRAJ_TN;
  HIPCHK(c, hipMemcpyAsync(out, c->d_traj, (size_t)count * sizeof(ccka_traj_rec), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_get_totals(ccka_ctx* c, ccka_totals* out) {
  if (!c || !out) return CCKA_EINVAL;
  if (!c->res_valid) return fail(c, CCKA_ESTATE, "no rollout yet");
  (void)hipSetDevice(c->device);
  return totals_of(c, c->res, c->N, out);
}

}  // extern "C"

// the totals of N scenarios' result columns on the device (ccka_get_totals on
// the last rollout's, ccka_debug_totals on uploaded ones): up to 1024 block
// partials of >= 256 scenarios, the ordered final pass, the overflow word
int totals_of(ccka_ctx* c, const ResultPtrs& res, int64_t N, ccka_totals* out) {
  if (!all_or_none(c->d_parts.reserve(kTotalsParts * 11 + 1) && c->d_totals.reserve(1), c->d_parts, c->d_totals))
    return fail(c, CCKA_ENOMEM, "totals buffers");
  TotParams q{};
  q.res = res;
  q.parts = (Part*)c->d_parts.get();
  q.ovf = c->d_parts + kTotalsParts * 11;
  q.out = c->d_totals;
  q.N = N;
  const int nparts = (int)std::min<int64_t>(kTotalsParts, (N + 255) / 256);
  long long ovf = 0;
  HIPCHK(c, launch_totals(q, nparts, c->stream));
  HIPCHK(c, hipMemcpyAsync(out, c->d_totals, sizeof(ccka_totals), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&ovf, q.ovf, sizeof ovf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (ovf) return fail(c, CCKA_EOVERFLOW, "a fixed-point total exceeds int64 (ccka.h: ccka_totals)");
  return CCKA_OK;
}

extern "C" {

// ---- the totals exchange, host halves (ccka.h: ccka_totals_pack / _finish) ----
int ccka_totals_pack(const ccka_totals* in, int32_t nranks, int64_t* block, int32_t n) {
  if (!in || !block || n != CCKA_TOTALS_BLOCK || nranks < 1) return CCKA_EINVAL;
  const int64_t* f = &in->scenarios;  // the leading CCKA_TOTALS_INT64 int64 fields
  static_assert(offsetof(ccka_totals, gco2_ug) == (CCKA_TOTALS_INT64 - 1) * sizeof(int64_t), "int64 block");
  const int64_t lim = INT64_MAX / nranks;
  int64_t risk = 0;
  for (int k = 0; k < CCKA_TOTALS_INT64; ++k) {
    block[k] = f[k];
    risk |= (f[k] > lim || f[k] < -lim) ? 1 : 0;
  }
  block[CCKA_TOTALS_INT64] = risk;
  return CCKA_OK;
}

int ccka_totals_finish(const int64_t* block, int32_t n, ccka_totals* out) {
  if (!block || !out || n != CCKA_TOTALS_BLOCK) return CCKA_EINVAL;
  if (block[CCKA_TOTALS_INT64] != 0) return CCKA_EOVERFLOW;
  int64_t* f = &out->scenarios;
  for (int k = 0; k < CCKA_TOTALS_INT64; ++k) f[k] = block[k];
  out->energy_wmin = (double)out->energy_uwmin * 1e-6;
  out->gco2 = (double)out->gco2_ug * 1e-6;
  return CCKA_OK;
}

int ccka_comm_unique_id(uint8_t* id128) {
  if (!id128) return CCKA_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return CCKA_ERCCL;
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id size");
  std::memcpy(id128, &id, 128);
  return CCKA_OK;
}

int ccka_comm_init(ccka_ctx* c, const uint8_t* id128, int32_t nranks, int32_t rank) {
  if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  ncclUniqueId id;
  std::memcpy(&id, id128, 128);
  if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
  const ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
  if (r != ncclSuccess) return fail(c, CCKA_ERCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
  return CCKA_OK;
}

int ccka_allreduce_totals(ccka_ctx* c, ccka_totals* io) {
  if (!c || !io) return CCKA_EINVAL;
  if (!c->comm) return fail(c, CCKA_ESTATE, "ccka_comm_init first");
  (void)hipSetDevice(c->device);
  int nranks = 1;
  if (ncclCommCount(c->comm, &nranks) != ncclSuccess) return fail(c, CCKA_ERCCL, "ncclCommCount failed");
  int64_t block[CCKA_TOTALS_BLOCK];
  if (ccka_totals_pack(io, nranks, block, CCKA_TOTALS_BLOCK) != CCKA_OK) return fail(c, CCKA_EINVAL, "totals pack");
  // the block goes through the device totals buffer (96 B >= 88 B)
  static_assert(sizeof(ccka_totals) >= CCKA_TOTALS_BLOCK * sizeof(int64_t), "totals block fits");
  if (!c->d_totals.reserve(1)) return fail(c, CCKA_ENOMEM, "totals alloc");
  int64_t* d_block = (int64_t*)c->d_totals.get();
  HIPCHK(c, hipMemcpyAsync(d_block, block, sizeof block, hipMemcpyHostToDevice, c->stream));
  // one in-place all-reduce (exact, order-independent); the doubles are
  // re-derived from the sums, so every rank count gives the same bits
  const ncclResult_t r = ncclAllReduce(d_block, d_block, CCKA_TOTALS_BLOCK, ncclInt64, ncclSum, c->comm, c->stream);
  if (r != ncclSuccess) return fail(c, CCKA_ERCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
  HIPCHK(c, hipMemcpyAsync(block, d_block, sizeof block, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int st = ccka_totals_finish(block, CCKA_TOTALS_BLOCK, io);
  if (st != CCKA_OK) return fail(c, st, "a summed total exceeds int64 at %d ranks (ccka.h: ccka_totals)", nranks);
  return CCKA_OK;
}

int ccka_comm_info(ccka_ctx* c, int32_t* nranks, int32_t* rank) {
  if (!c) return CCKA_EINVAL;
  if (!c->comm) return fail(c, CCKA_ESTATE, "ccka_comm_init first");
  int n = 0, r = 0;
  if (ncclCommCount(c->comm, &n) != ncclSuccess || ncclCommUserRank(c->comm, &r) != ncclSuccess)
    return fail(c, CCKA_ERCCL, "ncclCommCount / ncclCommUserRank failed");
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  return CCKA_OK;
}

}  // extern "C"
