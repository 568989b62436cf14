// abi_ctx.cpp — the context of libccka.so's C ABI (include/ccka.h): open /
// close, the world (validated against the engine's limits), the scenario set
// and the load traces, and the single-deployment engine's eligibility and world
// digest. Multi-GPU: one context per GPU; totals are summed with RCCL over
// xGMI (the only cross-GPU exchange: scenarios are independent).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>

#include "ctx.h"
#include "host_rules.h"

using namespace ccka;

int fail(ccka_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

// ---------------------------------------------------------------------------
// Single-deployment engine: eligibility and world digest.
// Conditions (anything else runs the general kernel): one HPA Deployment, no
// NodePool CPU limits (the launch choice is then independent of pool usage),
// replica counts and records within int16, tolerance in [0, 1), PDB percent
// <= 100, at most 65535 steps, at most
// D1_MAX_ZI distinct zone masks and D1_MAX_WC distinct carbon weights.
// ---------------------------------------------------------------------------
static int pod_cap(const ccka_itype& t, int rc, int rm) {
  int f = t.max_pods;
  if (rc > 0) f = std::min(f, t.alloc_cpu_m / rc);
  if (rm > 0) f = std::min(f, t.alloc_mem_mi / rm);
  return f;
}

// decisions of the register history rings (8 entries at one decision per
// step) cover the rules: the fast paths; otherwise the HBM history
bool rules_fit_ring(const ccka_hpa_rules& r) {
  if (r.n_policies > 2 || r.stab_window_s > CCKA_HIST * CCKA_STEP_SECONDS) return false;
  for (int i = 0; i < r.n_policies; ++i)
    if (r.policies[i].period_s > CCKA_HIST * CCKA_STEP_SECONDS) return false;
  return true;
}

static D1Rule d1_rule(const ccka_hpa_rules& r, bool up) {
  auto wm = [](int w) {
    int m = 0;
    for (int k = 0; k < CCKA_HIST; ++k) m |= ((k + 1) * CCKA_STEP_SECONDS < w) ? (1 << k) : 0;
    return m;
  };
  D1Rule o{};
  o.sel = r.select;
  o.n = r.n_policies;
  o.stab_mask = wm(r.stab_window_s);
  for (int q = 0; q < 2; ++q) {
    o.type[q] = r.policies[q].type;
    o.value[q] = r.policies[q].value;
    o.pmask[q] = wm(r.policies[q].period_s);
    o.factor[q] = up ? (1.0 + (double)o.value[q] / 100.0) : (1.0 - (double)o.value[q] / 100.0);
  }
  for (int r = 0; r < 4; ++r) {
    auto bit = [](int m, int e) { return (m >> e) & 1; };
    o.stab16[r] = (bit(o.stab_mask, 2 * r) ? 0xFFFF : 0) | (bit(o.stab_mask, 2 * r + 1) ? (int32_t)0xFFFF0000 : 0);
    for (int q = 0; q < 2; ++q) {
      const int m = q < o.n ? o.pmask[q] : 0;
      o.pm16[q][r] = (bit(m, 2 * r) ? 1 : 0) | (bit(m, 2 * r + 1) ? 0x10000 : 0);
    }
  }
  return o;
}

// the rules as the kernel uses them equal the upstream default behavior
// (d1_default_rule; the down stabilisation window is per scenario, not here)
static bool d1_rule_is_default(const D1Rule& r, bool up) {
  const D1Rule d = d1_default_rule(up);
  if (r.sel != d.sel || r.n != d.n || (up && r.stab_mask != 0)) return false;
  for (int q = 0; q < r.n; ++q)
    if (r.type[q] != d.type[q] || r.value[q] != d.value[q] || r.pmask[q] != 0) return false;
  return true;
}

// longest down-stabilisation window the 15 s sync ring holds: 20 records,
// (W - 1) / 15 <= 20
constexpr int kD1Sync15MaxWindow = 315;

static int d1_check_world(ccka_ctx* c) {
  const ccka_world& w = c->hw;
  c->d1_world = false;
  c->d1_ready = false;
  const ccka_deployment& dp = w.deploy[0];
  // one HPA deployment, or one single-trigger KEDA ScaledObject (default
  // behavior, one decision per step: the KEDA instantiation)
  const bool keda = dp.scaler == CCKA_SCALER_KEDA;
  if (w.n_deploy != 1 || (dp.scaler != CCKA_SCALER_HPA && !keda)) return CCKA_OK;
  if (keda && (w.hpa_sync_s == 15 || w.max_nodes > 8 || w.n_pools > 2 || dp.keda_threshold < 1 || dp.keda_threshold >= (1 << 22) ||
               dp.keda_activation < INT32_MIN || dp.keda_activation >= INT32_MAX || dp.keda_min < 0 ||
               dp.keda_min > D1_REC_SAT || dp.keda_max < 0 || dp.keda_max > D1_REC_SAT))
    return CCKA_OK;
  // pool limits run on the general kernel; drift, replacement and multi-node
  // consolidation are checked per scenario set in d1_prepare (d1_disrupt_ok)
  for (int q = 0; q < w.n_pools; ++q)
    if (w.pools[q].limit_cpu_m >= 0 || w.pools[q].limit_mem_mi >= 0) return CCKA_OK;
  // one HPA decision per step over the 8-entry register rings, or the
  // Kubernetes default 15 s sync (four per step) with the default behavior
  // (checked below) over 20-entry rings
  const bool sync15 = w.hpa_sync_s == 15;
  if ((w.hpa_sync_s != 0 && w.hpa_sync_s != CCKA_STEP_SECONDS && !sync15) || !rules_fit_ring(dp.up) ||
      !rules_fit_ring(dp.down))
    return CCKA_OK;
  if (!(dp.tolerance >= 0.0 && dp.tolerance < 1.0) || dp.req_cpu_m < 1 || dp.req_cpu_m > 65535 ||
      dp.limit_cpu_m > 65535 ||
      dp.min_replicas < 0 || dp.max_replicas < 0 || dp.max_replicas > D1_REC_SAT || dp.replicas0 > D1_REC_SAT)
    return CCKA_OK;
  // 32-bit PDB arithmetic (pct x replicas) and pending-pod-minutes (pods x steps)
  if (w.pdb_min_available_pct > 100 || w.n_steps > 65535) return CCKA_OK;
  const int K = w.n_types;
  std::vector<int> cap1(K);
  int jmax = 0;
  for (int k = 0; k < K; ++k) {
    cap1[k] = std::max(0, pod_cap(w.types[k], dp.req_cpu_m, dp.req_mem_mi));
    if (cap1[k] > D1_REC_SAT || w.types[k].alloc_cpu_m >= (1 << 24) || w.types[k].idle_nw < 0 ||
        w.types[k].dyn_nw_per_m < 0 || w.types[k].dyn_nw_per_m > 0xFFFFFFFFLL)
      return CCKA_OK;
    jmax = std::max(jmax, cap1[k]);
  }
  // distinct zone masks of every patch that sets one
  std::vector<uint32_t> zm;
  auto zidx = [&](uint32_t m) -> int {
    if (!m) return -1;
    for (size_t i = 0; i < zm.size(); ++i) if (zm[i] == m) return (int)i;
    zm.push_back(m);
    return (int)zm.size() - 1;
  };
  D1Params& p = c->d1;
  p = D1Params{};
  for (int q = 0; q < w.n_pools; ++q) {
    const ccka_pool_patch* src[4] = {&w.pools[q].base, &w.pools[q].profile[CCKA_PROFILE_RESET],
                                     &w.pools[q].profile[CCKA_PROFILE_OFFPEAK], &w.pools[q].profile[CCKA_PROFILE_PEAK]};
    for (int s = 0; s < 4; ++s) {
      D1Patch& x = p.patch[q][s];
      x.policy = src[s]->policy;
      const int ca = src[s]->consolidate_after_s;
      x.cas = ca >= 0 ? (ca + CCKA_STEP_SECONDS - 1) / CCKA_STEP_SECONDS : -1;
      x.zi = zidx(src[s]->zone_mask & ((1u << w.n_zones) - 1u));
      x.cm = (int32_t)(src[s]->cap_mask & 3u);
    }
    p.budget[q] = w.pools[q].budget_pct;
  }
  if (zm.empty()) zm.push_back(1u);  // no pool ever selects a zone: J = 0 everywhere
  if ((int)zm.size() > D1_MAX_ZI) return CCKA_OK;
  // accounting coefficients and the catalog in pod-capacity-descending order
  std::vector<long long> acc((size_t)K * 3);
  std::vector<int32_t> order(K), cap1s(K);
  for (int k = 0; k < K; ++k) {
    acc[(size_t)k * 3 + 0] = w.types[k].idle_nw;
    acc[(size_t)k * 3 + 1] = w.types[k].dyn_nw_per_m;
    acc[(size_t)k * 3 + 2] = w.types[k].alloc_cpu_m;
    order[k] = k;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cap1[a] > cap1[b]; });
  for (int k = 0; k < K; ++k) cap1s[k] = cap1[order[k]];
  int rc;
  if ((rc = dupload(c, c->d_acc, acc.data(), acc.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_order, order.data(), order.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_cap1s, cap1s.data(), cap1s.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_cap1t, cap1.data(), cap1.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_zmasks, zm.data(), zm.size())) != CCKA_OK) return rc;
  c->zmasks = zm;
  for (size_t z = 0; z < 16; ++z) p.zml[z] = z < zm.size() ? zm[z] : 0u;
  c->JT = jmax + 1;
  p.T = w.n_steps; p.K = K; p.Z = w.n_zones; p.R = w.n_regions; p.NP = w.n_pools; p.maxn = w.max_nodes;
  p.NZI = (int)zm.size(); p.JT = c->JT;
  p.start_minute = w.start_minute; p.peak_start = w.peak_start_min; p.peak_end = w.peak_end_min;
  p.pswitch0 = w.peak_switch; p.delay = w.provision_delay_steps;
  p.base_nodes = w.base_nodes; p.base_type = w.base_type; p.slo_util = w.slo_util_pct;
  p.pdb_pct = w.pdb_min_available_pct; p.pdb_member = dp.pdb_member ? 1 : 0;
  p.replicas0 = dp.replicas0; p.minr = dp.min_replicas; p.maxr0 = dp.max_replicas;
  p.target0 = dp.target_util_pct; p.req_cpu = dp.req_cpu_m; p.limit = dp.limit_cpu_m;
  p.dstab0 = dp.down.stab_window_s; p.reset_ca0 = w.reset_ca_s; p.capsel0 = (int32_t)dp.cap_sel;
  p.tol_lo = 1.0 - dp.tolerance;
  p.tol_hi = 1.0 + dp.tolerance;
  const ccka_itype& bt = w.types[w.base_type];
  p.base_nw = (long long)w.base_nodes *
              (bt.idle_nw + bt.dyn_nw_per_m * (long long)(w.base_util * (double)bt.alloc_cpu_m));
  p.up = d1_rule(dp.up, true);
  p.dn = d1_rule(dp.down, false);
  p.bdef = d1_rule_is_default(p.up, true) && d1_rule_is_default(p.dn, false);
  p.nsub = sync15 ? 4 : 1;
  if (sync15 && (!p.bdef || dp.down.stab_window_s > kD1Sync15MaxWindow)) return CCKA_OK;
  if (keda) {
    if (!p.bdef || dp.down.stab_window_s > CCKA_HIST * CCKA_STEP_SECONDS) return CCKA_OK;
    p.keda = 1;
    p.k_thr = (int32_t)dp.keda_threshold;
    p.k_act = (int32_t)dp.keda_activation;
    p.k_cds = dp.keda_cooldown_s > 0 ? (int32_t)std::min<int64_t>(((int64_t)dp.keda_cooldown_s + 59) / 60, 1 << 20) : 0;
    p.k_min = dp.keda_min;
    p.k_max = dp.keda_max;
  }
  c->d1_world = true;
  return CCKA_OK;
}

// Drift never acts when no scenario switches profile or OFFPEAK and PEAK
// resolve to the same masks for every pool.
static bool d1_drift_inert(const ccka_ctx* c) {
  const ccka_world& w = c->hw;
  if (!(w.disrupt_ext & CCKA_DISRUPT_DRIFT)) return true;
  const bool switching = c->sc_pswitch_any >= 0 ? c->sc_pswitch_any != 0 : w.peak_switch != 0;
  bool same = true;
  for (int q = 0; q < w.n_pools; ++q) {
    uint32_t zm = 0, cm = 0;
    for (const ccka_pool_patch* x : {&w.pools[q].base, &w.pools[q].profile[CCKA_PROFILE_RESET]}) {
      if (x->zone_mask) zm = x->zone_mask;
      if (x->cap_mask) cm = x->cap_mask;
    }
    // masks after the first profile (t = 0, either one) must never change
    // over the alternations that follow (merge: 0 keeps the previous mask)
    const ccka_pool_patch* pr[2] = {&w.pools[q].profile[CCKA_PROFILE_OFFPEAK],
                                    &w.pools[q].profile[CCKA_PROFILE_PEAK]};
    for (int first = 0; first < 2; ++first) {
      uint32_t z = zm, k = cm, z1 = 0, k1 = 0;
      for (int j = 0; j < 4; ++j) {
        const ccka_pool_patch* x = pr[(first + j) & 1];
        if (x->zone_mask) z = x->zone_mask;
        if (x->cap_mask) k = x->cap_mask;
        if (j == 0) { z1 = z; k1 = k; }
        else if (z != z1 || k != k1) same = false;
      }
    }
  }
  return !switching || same;
}

// The single-deployment kernel runs drift (SEMANTICS 3.G0) and single-node
// replacement consolidation (3.G2) itself in its DRIFT instantiation (8
// slots, <= 2 pools); multi-node consolidation runs on the general kernel
// unless provably inert. Replacement needs an on-demand node in a
// WhenEmptyOrUnderutilized pool: inert when no pool profile uses that policy
// or no scenario's nodeSelector admits on-demand; multi-node consolidation
// needs a WhenEmptyOrUnderutilized pool and a budget of >= 2 nodes.
static bool d1_disrupt_ok(const ccka_ctx* c, bool* drift, bool* replace, bool* multi) {
  const ccka_world& w = c->hw;
  *drift = !d1_drift_inert(c);
  *replace = false;
  *multi = false;
  if (*drift && !(w.max_nodes <= 8 && w.n_pools <= 2)) return false;
  bool weou = false;
  for (int q = 0; q < w.n_pools; ++q) {
    weou |= w.pools[q].base.policy == CCKA_WHEN_EMPTY_OR_UNDERUTILIZED;
    for (int s = 0; s < 3; ++s) weou |= w.pools[q].profile[s].policy == CCKA_WHEN_EMPTY_OR_UNDERUTILIZED;
  }
  if (w.disrupt_ext & CCKA_DISRUPT_REPLACE) {
    const uint32_t sel = c->sc_capsel_or ? c->sc_capsel_or : w.deploy[0].cap_sel;
    if (weou && (sel & CCKA_CAP_OD)) {
      if (!(w.max_nodes <= 8 && w.n_pools <= 2)) return false;
      *replace = true;
    }
  }
  if ((w.disrupt_ext & CCKA_DISRUPT_MULTI) && weou) {
    // Multi-node consolidation moves >= 2 nodes of a pool in one step: its
    // firstN search tries prefixes of at most budget - deleted candidates
    // (SEMANTICS 3.G3). With every pool's disruption budget at <= 1 node for
    // any node count the world allows (ceil(pct * max_nodes / 100) <= 1: the
    // reference's 10 % at 8 nodes) there is no prefix to try, so it never acts
    // and is not evaluated; larger budgets run it in the DRIFT instantiation.
    bool two = false;
    for (int q = 0; q < w.n_pools; ++q) two |= (w.pools[q].budget_pct * w.max_nodes + 99) / 100 >= 2;
    if (two) {
      if (!(w.max_nodes <= 8 && w.n_pools <= 2)) return false;
      *multi = true;
    }
  }
  return true;
}

// scenario-dependent part: distinct carbon weights, per-scenario index, tables
int d1_prepare(ccka_ctx* c) {
  c->d1_ready = true;
  c->d1_ok = false;
  bool drift = false, replace = false, multi = false;
  // (a KEDA deployment ignores the per-scenario target / max / down-window
  // overrides: its bounds and rules are the ScaledObject's, SEMANTICS 3.C)
  const bool keda = c->d1.keda != 0;
  if (!c->d1_world || (!keda && !c->sc_maxr_ok) || !d1_disrupt_ok(c, &drift, &replace, &multi)) return CCKA_OK;
  if (keda && (drift || replace || multi)) return CCKA_OK;  // the KEDA instantiation has no DRIFT paths
  c->d1.drift = (drift || replace || multi) ? 1 : 0;  // the DRIFT instantiation carries all three
  c->d1.drift_on = drift ? 1 : 0;
  c->d1.replace = replace ? 1 : 0;
  c->d1.multi = multi ? 1 : 0;
  // beyond the register ring
  if (!keda && c->sc_dstab_max > (c->d1.nsub == 4 ? kD1Sync15MaxWindow : CCKA_HIST * CCKA_STEP_SECONDS))
    return CCKA_OK;
  // default behavior and no window beyond 300 s: the 4-record ring instantiation
  c->d1.he4 = (c->d1.nsub == 1 && c->d1.bdef && c->d1.dstab0 <= 300 && (keda || c->sc_dstab_max <= 300)) ? 1 : 0;
  const size_t n = (size_t)c->N;
  std::vector<double> wl;
  std::vector<uint8_t> wci;
  if (!c->h_cw.empty()) {
    std::map<uint64_t, int> seen;
    wci.resize(n);
    for (size_t i = 0; i < n; ++i) {
      uint64_t b;
      std::memcpy(&b, &c->h_cw[i], 8);
      auto it = seen.find(b);
      if (it == seen.end()) {
        if ((int)wl.size() >= D1_MAX_WC) return CCKA_OK;
        it = seen.emplace(b, (int)wl.size()).first;
        wl.push_back(c->h_cw[i]);
      }
      wci[i] = (uint8_t)it->second;
    }
  } else {
    wl.push_back(c->hw.carbon_weight);
  }
  std::vector<double> wc1000(wl.size());
  for (size_t k = 0; k < wl.size(); ++k) wc1000[k] = wl[k] * 1000.0;
  int rc;
  if ((rc = dupload(c, c->d_wc1000, wc1000.data(), wc1000.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_wci, wci.empty() ? nullptr : wci.data(), wci.size())) != CCKA_OK) return rc;
  c->NW = (int)wl.size();
  const ccka_world& w = c->hw;
  const int64_t keys = (int64_t)w.n_regions * 24 * (int64_t)c->zmasks.size() * 3;
  if (!all_or_none(c->d_table.resize(keys * c->NW * c->JT) && c->d_jtab.resize(keys), c->d_table, c->d_jtab))
    return fail(c, CCKA_ENOMEM, "argmin table alloc (%lld keys x %d weights x %d)", (long long)keys, c->NW, c->JT);
  // the G2 / G3 offer table: cheapest offering holding n pods, by price
  const int64_t keys2 = replace || multi ? keys : 0;
  if (keys2) {
    const double zero = 0.0;
    if ((rc = dupload(c, c->d_wc0, &zero, 1)) != CCKA_OK) return rc;
  }
  if (!all_or_none(c->d_table2.resize(keys2 * c->JT) && c->d_jtab2.resize(keys2), c->d_table2, c->d_jtab2))
    return fail(c, CCKA_ENOMEM, "offer table alloc (%lld keys x %d)", (long long)keys, c->JT);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->d1_ok = true;
  return CCKA_OK;
}

// the argmin-table builder's block over the world digest: NW carbon weights
// (x 1000) into table / jtab
TableParams table_params(const ccka_ctx* c, const double* wc1000, int NW, int2* table, int32_t* jtab) {
  const ccka_world& w = c->hw;
  TableParams tp{};
  tp.price = c->d_price; tp.ci_gpwh = c->d_ci_gpwh; tp.types = c->d_types;
  tp.order = c->d_order; tp.cap1s = c->d_cap1s; tp.cap1t = c->d_cap1t; tp.zmasks = c->d_zmasks; tp.wc1000 = wc1000;
  tp.table = table; tp.jtab = jtab;
  tp.K = w.n_types; tp.Z = w.n_zones; tp.R = w.n_regions; tp.NZI = (int)c->zmasks.size();
  tp.NW = NW; tp.JT = c->JT;
  return tp;
}

extern "C" {

int32_t ccka_abi_version(void) { return CCKA_ABI_VERSION; }

int32_t ccka_struct_sizes(int64_t* out, int32_t n) {
  const int64_t s[] = {sizeof(ccka_itype),    sizeof(ccka_pool),    sizeof(ccka_deployment),
                       sizeof(ccka_world),    sizeof(ccka_scenarios), sizeof(ccka_results),
                       sizeof(ccka_traj_rec), sizeof(ccka_totals),  sizeof(ccka_trace_gen),
                       sizeof(ccka_grid_stats), sizeof(ccka_detail), sizeof(ccka_sweep_stat),
                       sizeof(ccka_timeline_spec), sizeof(ccka_timeline_row)};
  const int32_t m = (int32_t)(sizeof s / sizeof s[0]);
  int32_t k = 0;
  for (; k < m && k < n; ++k) out[k] = s[k];
  return k;
}

const char* ccka_last_error(const ccka_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ccka_open(ccka_ctx** out, int device_ordinal) {
  if (!out) return CCKA_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CCKA_ENODEV;
  if (device_ordinal < 0 || device_ordinal >= ndev) return CCKA_ENODEV;
  if (hipSetDevice(device_ordinal) != hipSuccess) return CCKA_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return CCKA_ENODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CCKA_ENODEV;
  ccka_ctx* c = new (std::nothrow) ccka_ctx();
  if (!c) return CCKA_ENOMEM;
  c->device = device_ordinal;
  c->cus = prop.multiProcessorCount;
  std::snprintf(c->name, sizeof c->name, "%s (%s)", prop.name, prop.gcnArchName);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->ev_mid) != hipSuccess) {
    delete c;
    return CCKA_EHIP;
  }
  // sine table of the synthetic load generator (SEMANTICS.md §4)
  int32_t sinq[1440];
  for (int m = 0; m < 1440; ++m) sinq[m] = (int32_t)std::lround(65536.0 * std::sin(2.0 * M_PI * (double)m / 1440.0));
  if (dupload(c, c->d_sinq, sinq, 1440) != CCKA_OK || hipStreamSynchronize(c->stream) != hipSuccess) {
    ccka_close(c);
    return CCKA_EHIP;
  }
  *out = c;
  return CCKA_OK;
}

// no result of an earlier run is readable any more: the result columns, the
// trajectory, the detail, the closed loop's records and samples, the timing
static void end_results(ccka_ctx* c) {
  c->ran = false;
  c->res_valid = false;
  c->traj_valid = false;
  c->detail_valid = false;
  c->pol_rec_valid = false;
  c->pol_feat_valid = false;
  c->pg_valid = false;
}

static void free_results(ccka_ctx* c) {
  c->d_res.release();
  c->res = ResultPtrs{};
  c->d_traj.release();
  c->d_traj_t.release();
  c->d_parts.release();
  c->d_detail.release();
  c->traj_valid = false;
  c->detail_valid = false;
}

void ccka_close(ccka_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->pol_graph) (void)hipGraphExecDestroy(c->pol_graph);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // the device buffers go with it
}

// autoscaling/v2 ranges: stabilizationWindowSeconds 0..3600, periodSeconds
// 1..1800 (0 accepted: an empty period), up to CCKA_HPA_MAX_POLICIES policies
static bool rules_ok(const ccka_hpa_rules& r) {
  if (r.select < 0 || r.select > 2 || r.n_policies < 0 || r.n_policies > CCKA_HPA_MAX_POLICIES) return false;
  if (r.stab_window_s < 0 || r.stab_window_s > CCKA_HPA_MAX_WINDOW_S) return false;
  for (int i = 0; i < r.n_policies; ++i) {
    const ccka_hpa_policy& p = r.policies[i];
    if ((p.type != CCKA_HPA_PODS && p.type != CCKA_HPA_PERCENT) || p.value < 0 || p.period_s < 1 ||
        p.period_s > CCKA_HPA_MAX_PERIOD_S)
      return false;
  }
  return true;
}



int ccka_set_world(ccka_ctx* c, const ccka_world* w) {
  if (!c || !w) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  if (const char* why = world_timing_invalid(*w)) return fail(c, CCKA_EINVAL, "%s", why);
  if (w->max_nodes < 1 || w->max_nodes > CCKA_MAX_NODES) return fail(c, CCKA_EINVAL, "max_nodes out of range");
  if (w->n_types < 1 || w->n_types > CCKA_MAX_TYPES || !w->types) return fail(c, CCKA_EINVAL, "catalog invalid");
  if (w->n_zones < 1 || w->n_zones > CCKA_MAX_ZONES) return fail(c, CCKA_EINVAL, "n_zones out of range");
  if (w->n_regions < 1 || w->n_regions > CCKA_MAX_REGIONS) return fail(c, CCKA_EINVAL, "n_regions out of range");
  if (w->n_pools < 1 || w->n_pools > CCKA_MAX_POOLS) return fail(c, CCKA_EINVAL, "n_pools out of range");
  if (w->n_deploy < 1 || w->n_deploy > CCKA_MAX_DEPLOY) return fail(c, CCKA_EINVAL, "n_deploy out of range");
  if (!w->price_uph || !w->ci_gpwh || !w->ci_gpwmin) return fail(c, CCKA_EINVAL, "tiles missing");
  if (w->disrupt_ext & ~(CCKA_DISRUPT_DRIFT | CCKA_DISRUPT_REPLACE | CCKA_DISRUPT_MULTI))
    return fail(c, CCKA_EINVAL, "unknown disrupt_ext bits");
  if (w->base_type < 0 || w->base_type >= w->n_types) return fail(c, CCKA_EINVAL, "base_type out of range");
  for (int k = 0; k < w->n_types; ++k) {
    const ccka_itype& t = w->types[k];
    if (t.vcpu < 0 || t.alloc_cpu_m <= 0 || t.alloc_mem_mi < 0 || t.max_pods < 0)
      return fail(c, CCKA_EINVAL, "catalog entry %d invalid", k);
  }
  for (int d = 0; d < w->n_deploy; ++d) {
    const ccka_deployment& dp = w->deploy[d];
    if (dp.scaler < 0 || dp.scaler > 3 || dp.cap_sel == 0 || dp.cap_sel > 3 || dp.req_cpu_m < 0 ||
        dp.req_mem_mi < 0 || dp.replicas0 < 0)
      return fail(c, CCKA_EINVAL, "deployment %d invalid", d);
    if (dp.scaler == CCKA_SCALER_HPA && (dp.req_cpu_m <= 0 || dp.target_util_pct <= 0))
      return fail(c, CCKA_EINVAL, "HPA deployment %d needs cpu request and target", d);
    if ((dp.scaler == CCKA_SCALER_KEDA || dp.scaler == CCKA_SCALER_KEDA_TRIGGER) && dp.keda_threshold <= 0)
      return fail(c, CCKA_EINVAL, "KEDA deployment %d needs threshold", d);
    if (dp.scaler == CCKA_SCALER_KEDA_TRIGGER &&
        (d == 0 || dp.replicas0 != 0 || dp.pdb_member ||
         (w->deploy[d - 1].scaler != CCKA_SCALER_KEDA && w->deploy[d - 1].scaler != CCKA_SCALER_KEDA_TRIGGER)))
      return fail(c, CCKA_EINVAL, "KEDA trigger %d must follow a KEDA deployment and own no pods", d);
    if (!rules_ok(dp.up) || !rules_ok(dp.down))
      return fail(c, CCKA_EINVAL, "deployment %d behavior outside autoscaling/v2 ranges (window <= %d s, period <= %d s, "
                  "<= %d policies)", d, CCKA_HPA_MAX_WINDOW_S, CCKA_HPA_MAX_PERIOD_S, CCKA_HPA_MAX_POLICIES);
  }
  if (w->hpa_sync_s != 0 && w->hpa_sync_s != 10 && w->hpa_sync_s != 15 && w->hpa_sync_s != 20 &&
      w->hpa_sync_s != 30 && w->hpa_sync_s != 60)
    return fail(c, CCKA_EINVAL, "hpa_sync_s must be 0, 10, 15, 20, 30 or 60");
  for (int q = 0; q < w->n_pools; ++q)
    if (w->pools[q].limit_mem_mi < -1) return fail(c, CCKA_EINVAL, "pool %d limit_mem_mi invalid", q);
  // the world is accepted. Everything computed for the earlier one ends here,
  // before hw is replaced (ccka.h, "what ends what"), so that a failure below
  // (CCKA_ENOMEM, CCKA_EHIP) leaves no world rather than the new hw beside the
  // earlier set and results. The scenario set ends too: its region ids were
  // checked against the earlier n_regions, so the next step is ccka_set_scenarios
  c->have_world = false;
  c->have_sc = false;
  c->have_load = false;
  end_results(c);
  c->hw = *w;
  const int K = w->n_types, Z = w->n_zones, R = w->n_regions;
  int rc;
  if ((rc = dupload(c, c->d_types, w->types, (size_t)K)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_price, w->price_uph, (size_t)R * 24 * K * Z * 2)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_ci_gpwh, w->ci_gpwh, (size_t)R * 24)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_ci_gpwmin, w->ci_gpwmin, (size_t)R * 24)) != CCKA_OK) return rc;
  ccka_world dw = *w;
  dw.types = nullptr; dw.ci_gpwh = nullptr; dw.ci_gpwmin = nullptr; dw.price_uph = nullptr;
  if ((rc = dupload(c, c->d_world, &dw, 1)) != CCKA_OK) return rc;
  // provisioning order: req_cpu desc, req_mem desc, index asc
  const int D = w->n_deploy;
  for (int d = 0; d < D; ++d) c->prov[d] = d;
  std::stable_sort(c->prov, c->prov + D, [&](int a, int b) {
    const ccka_deployment &A = w->deploy[a], &B = w->deploy[b];
    if (A.req_cpu_m != B.req_cpu_m) return A.req_cpu_m > B.req_cpu_m;
    return A.req_mem_mi > B.req_mem_mi;
  });
  if ((rc = d1_check_world(c)) != CCKA_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_world = true;
  return CCKA_OK;
}

}  // extern "C"

// the result columns of N scenarios carved out of one allocation at p (the
// SoA the kernels write): returns its size in bytes; p == nullptr: the size alone
int64_t carve_results(char* p, int64_t N, ResultPtrs* out) {
  // 8-byte fields first, then 4-byte fields; each array 256-B aligned
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t b8 = up(N * 8), b4 = up(N * 4);
  const int64_t total = 4 * b8 + 10 * b4;
  if (!p) return total;
  ResultPtrs& k = *out;
  k.cost = (int64_t*)p; p += b8;
  k.energy = (double*)p; p += b8;
  k.gco2 = (double*)p; p += b8;
  k.pend_min = (int64_t*)p; p += b8;
  k.slo = (int32_t*)p; p += b4;
  k.nmin_spot = (int32_t*)p; p += b4;
  k.nmin_od = (int32_t*)p; p += b4;
  k.launches = (int32_t*)p; p += b4;
  k.deletions = (int32_t*)p; p += b4;
  k.peak_nodes = (int32_t*)p; p += b4;
  k.final_reps = (int32_t*)p; p += b4;
  k.final_nodes = (int32_t*)p; p += b4;
  k.last_choice = (uint32_t*)p; p += b4;
  k.hash = (uint32_t*)p;
  return total;
}

extern "C" {

static int alloc_results(ccka_ctx* c) {
  free_results(c);
  const int64_t N = c->N;
  if (!all_or_none(c->d_res.resize(carve_results(nullptr, N, nullptr)) &&
                       c->d_parts.resize(kTotalsParts * 11 + 1) && c->d_totals.reserve(1),
                   c->d_res, c->d_parts))
    return fail(c, CCKA_ENOMEM, "results alloc (%lld scenarios)", (long long)N);
  carve_results(c->d_res, N, &c->res);
  return CCKA_OK;
}

int ccka_set_scenarios(ccka_ctx* c, const ccka_scenarios* sc) {
  if (!c || !sc) return CCKA_EINVAL;
  if (!c->have_world) return fail(c, CCKA_ESTATE, "set_world first");
  // the previous set and its traces are gone from here on; the new set counts
  // only once every step below has succeeded
  c->have_sc = false;
  c->have_load = false;
  c->d_load.release();
  c->d_load_w.release();
  c->d_load_nt.release();
  c->load_w_lpw = 0;
  c->load_nt_dp = 0;
  if (sc->n < 1 || sc->n > (int64_t)1 << 31) return fail(c, CCKA_EINVAL, "scenario count out of range");
  if (sc->n_traces < 0 || sc->n_traces > (int64_t)1 << 31 || sc->first_id < 0)
    return fail(c, CCKA_EINVAL, "n_traces / first_id out of range");
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)sc->n;
  if (sc->region) {
    for (size_t i = 0; i < n; ++i)
      if (sc->region[i] >= c->hw.n_regions) return fail(c, CCKA_EINVAL, "region %u out of range", sc->region[i]);
    c->h_region.assign(sc->region, sc->region + n);
  } else {
    c->h_region.clear();
  }
  if (sc->cap_sel)
    for (size_t i = 0; i < n; ++i)
      if (sc->cap_sel[i] == 0 || sc->cap_sel[i] > 3) return fail(c, CCKA_EINVAL, "cap_sel invalid");
  c->sc_target_max = -1;
  if (sc->target_util_pct)
    for (size_t i = 0; i < n; ++i) {
      if (sc->target_util_pct[i] <= 0) return fail(c, CCKA_EINVAL, "target_util_pct must be > 0");
      c->sc_target_max = std::max<int>(c->sc_target_max, sc->target_util_pct[i]);
    }
  c->sc_dstab_max = -1;
  if (sc->down_stab_s)
    for (size_t i = 0; i < n; ++i) {
      if (sc->down_stab_s[i] < 0 || sc->down_stab_s[i] > CCKA_HPA_MAX_WINDOW_S)
        return fail(c, CCKA_EINVAL, "down_stab_s outside 0..%d s", CCKA_HPA_MAX_WINDOW_S);
      c->sc_dstab_max = std::max<int>(c->sc_dstab_max, sc->down_stab_s[i]);
    }
  int rc;
  if ((rc = dupload(c, c->d_region, sc->region, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_target, sc->target_util_pct, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_maxr, sc->max_replicas, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_dstab, sc->down_stab_s, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_resetca, sc->reset_ca_s, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_pswitch, sc->peak_switch, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_cw, sc->carbon_weight, n)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_capsel, sc->cap_sel, n)) != CCKA_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->h_cw.clear();
  if (sc->carbon_weight) c->h_cw.assign(sc->carbon_weight, sc->carbon_weight + n);
  c->sc_capsel_or = 0;
  if (sc->cap_sel)
    for (size_t i = 0; i < n; ++i) c->sc_capsel_or |= sc->cap_sel[i];
  c->sc_pswitch_any = -1;
  if (sc->peak_switch) {
    c->sc_pswitch_any = 0;
    for (size_t i = 0; i < n; ++i) c->sc_pswitch_any |= sc->peak_switch[i] != 0;
  }
  c->sc_maxr_ok = true;
  c->sc_maxr_max = -1;
  if (sc->max_replicas)
    for (size_t i = 0; i < n; ++i) {
      if (sc->max_replicas[i] < 0) c->sc_maxr_ok = false;
      c->sc_maxr_max = std::max<int>(c->sc_maxr_max, sc->max_replicas[i]);
    }
  c->d1_ready = false;
  c->N = sc->n;
  c->first_id = sc->first_id;
  c->n_traces = sc->n_traces;
  if ((rc = alloc_results(c)) != CCKA_OK) return rc;
  c->have_sc = true;
  end_results(c);
  return CCKA_OK;
}

// the trace buffer [T][D][NL] of the current world and scenario set
static int ensure_load(ccka_ctx* c) {
  const int64_t cnt = (int64_t)c->hw.n_steps * c->hw.n_deploy * load_cols(c);
  if (c->d_load.resize(cnt)) return CCKA_OK;
  c->have_load = false;
  return fail(c, CCKA_ENOMEM, "load alloc %lld ints", (long long)cnt);
}

int ccka_set_load(ccka_ctx* c, const int32_t* load, int64_t count) {
  if (!c || !load) return CCKA_EINVAL;
  if (!c->have_sc) return fail(c, CCKA_ESTATE, "set_scenarios first");
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = ensure_load(c)) != CCKA_OK) return rc;
  if (count != c->d_load.count())
    return fail(c, CCKA_EINVAL, "load count %lld != T*D*N %lld", (long long)count, (long long)c->d_load.count());
  c->load_w_lpw = 0;
  c->load_nt_dp = 0;
  HIPCHK(c, hipMemcpyAsync(c->d_load, load, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_load = true;
  return CCKA_OK;
}

int ccka_gen_load(ccka_ctx* c, const ccka_trace_gen* g) {
  if (!c || !g) return CCKA_EINVAL;
  if (!c->have_sc) return fail(c, CCKA_ESTATE, "set_scenarios first");
  if (const char* why = trace_gen_invalid(*g)) return fail(c, CCKA_EINVAL, "trace generator invalid: %s", why);
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = ensure_load(c)) != CCKA_OK) return rc;
  GenParams gp{};
  gp.out = c->d_load;
  gp.sinq = c->d_sinq;
  // shared traces are keyed by trace index, per-scenario traces by global id
  gp.n = load_cols(c);
  gp.first_id = c->n_traces > 0 ? 0 : c->first_id;
  gp.seed = g->seed;
  gp.T = c->hw.n_steps;
  gp.D = c->hw.n_deploy;
  gp.base_lo = g->base_lo; gp.base_hi = g->base_hi;
  gp.amp_lo = g->amp_lo_pm; gp.amp_hi = g->amp_hi_pm;
  gp.noise = g->noise_pm; gp.burst_prob = g->burst_prob_pm;
  gp.burst_mult = g->burst_mult_pm; gp.burst_len = g->burst_len;
  c->load_w_lpw = 0;
  c->load_nt_dp = 0;
  HIPCHK(c, launch_gen_load(gp, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_load = true;
  return CCKA_OK;
}

int ccka_get_load(ccka_ctx* c, int32_t* load, int64_t count) {
  if (!c || !load) return CCKA_EINVAL;
  if (!c->have_load) return fail(c, CCKA_ESTATE, "no load on device");
  if (count != c->d_load.count()) return fail(c, CCKA_EINVAL, "load count mismatch");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(load, c->d_load, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

}  // extern "C"
