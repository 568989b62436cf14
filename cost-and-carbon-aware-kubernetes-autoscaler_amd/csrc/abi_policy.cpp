// abi_policy.cpp — the learned control policy of libccka.so's C ABI (config 5):
// the closed loop (fused into one kernel, or launched step by step as a
// captured hipGraph), the recorded actions and features, and the differentiable
// control built on it (the score-function gradient and the MLP backward, pg.hip).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "host_rules.h"

using namespace ccka;

// ---- closed-loop learned control policy (config 5) ----

// The fused loop's Karpenter launches on a single-deployment world without
// pool limits (d1_check_world) read argmin tables instead of scanning the
// catalog: table_kernel over every carbon weight the policy can emit (k / 16,
// k = 0..64; the sampled policy's 0 and 1 are k = 0 and 16), rebuilt per loop
// on the stream (prices and carbon intensity are the world's). Leaves
// k.ptable null when the world does not qualify or there is no memory for the
// tables: the fused loop then scans the catalog (same choices).
static int policy_tables(ccka_ctx* c, KParams& k) {
  const ccka_world& w = c->hw;
  if (!c->d1_world || w.n_zones > 4 || c->zmasks.empty()) return CCKA_OK;
  constexpr int NWP = 65;
  const int64_t keys = (int64_t)w.n_regions * 24 * (int64_t)c->zmasks.size() * 3;
  if (!all_or_none(c->d_ptable.resize(keys * NWP * c->JT) && c->d_pjtab.resize(keys), c->d_ptable, c->d_pjtab))
    return CCKA_OK;
  if (!c->d_pwc) {
    double wc[NWP];
    for (int x = 0; x < NWP; ++x) wc[x] = (double)x / 16.0 * 1000.0;  // the kernel's c * 1000.0
    int rc;
    if ((rc = dupload(c, c->d_pwc, wc, (size_t)NWP)) != CCKA_OK) return rc;
  }
  const TableParams tp = table_params(c, c->d_pwc, NWP, c->d_ptable, c->d_pjtab);
  HIPCHK(c, launch_table(tp, c->stream));
  k.ptable = c->d_ptable;
  k.pjtab = c->d_pjtab;
  k.pNZI = tp.NZI;
  k.pJT = c->JT;
  k.pNW = NWP;
  const uint32_t zall = (1u << w.n_zones) - 1u;
  for (uint32_t m = 0; m < 16; ++m) {
    k.pzmi[m] = -1;
    for (size_t z = 0; z < c->zmasks.size(); ++z)
      if ((m & zall) && c->zmasks[z] == (m & zall)) k.pzmi[m] = (int32_t)z;
  }
  return CCKA_OK;
}

// a loop's launches are on the stream: what it left valid, then its timing
static int loop_done(ccka_ctx* c, int engine, int32_t trajectory, int32_t record, bool feat) {
  c->last_engine = engine;
  c->traj_nt = false;
  c->traj_valid = trajectory != 0;
  c->detail_valid = c->detail_on;
  c->pol_rec_valid = record != 0;
  c->pol_feat_valid = feat;
  c->ran = true;
  c->res_valid = true;
  return ccka_sync(c);
}

// The closed loop (SEMANTICS 5). pg == nullptr: the deterministic policy
// (policy_act_kernel); otherwise each step samples an action bin from
// softmax(y) (policy_sample_kernel) and the features and actions of every
// step are kept for the score-function gradient (ccka_policy_grad).
static int policy_loop(ccka_ctx* c, int32_t trajectory, int32_t record, const ccka_pg_params* pg) {
  if (!c) return CCKA_EINVAL;
  if (!c->have_world || !c->have_sc) return fail(c, CCKA_ESTATE, "world/scenarios not set");
  if (!c->have_load) return fail(c, CCKA_ESTATE, "no load traces (ccka_set_load / ccka_gen_load)");
  if (!c->mlp_have_w) return fail(c, CCKA_ESTATE, "MLP weights not set (ccka_mlp_set_weights)");
  (void)hipSetDevice(c->device);
  // the single-deployment kernel's tiled trace copy (N*T*4 bytes) and the
  // skewed schedule's scenario-major one are not read here: released for the
  // loop's own arrays, rebuilt by the next rollout
  c->d_load_w.release();
  c->load_w_lpw = 0;
  c->d_load_nt.release();
  c->load_nt_dp = 0;
  const ccka_world& w = c->hw;
  const int64_t N = c->N;
  const int T = w.n_steps;
  int block = 256;
  size_t lds = 0;
  int rc;
  KParams k;
  if ((rc = setup_general(c, trajectory, k, &block, &lds)) != CCKA_OK) return rc;
  int dmax, nmax;
  kernel_dims(w.n_deploy, w.max_nodes, &dmax, &nmax);
  const int64_t words = state_words(dmax, nmax);
  if (!c->d_pol_state.reserve(words * N))
    return fail(c, CCKA_ENOMEM, "policy state alloc (%lld words)", (long long)(words * N));
  if (!all_or_none(c->d_pol_target.reserve(N) && c->d_pol_cw.reserve(N), c->d_pol_target, c->d_pol_cw))
    return fail(c, CCKA_ENOMEM, "policy action alloc");
  // the recorded actions, features and samples are about to be overwritten
  c->pol_rec_valid = false;
  c->pol_feat_valid = false;
  c->pg_valid = false;
  const int64_t TN = (int64_t)T * N;
  if (record && !all_or_none(c->d_rec_target.reserve(TN) && c->d_rec_cw.reserve(TN), c->d_rec_target, c->d_rec_cw))
    return fail(c, CCKA_ENOMEM, "policy action record alloc");
  const bool feat_on = c->pol_feat_on || pg;
  if (pg && !c->d_pg_act.reserve(TN)) return fail(c, CCKA_ENOMEM, "policy-gradient action record alloc");
  if (feat_on && !c->d_feat_rec.reserve((int64_t)(T + 1) * N * 64))
    return fail(c, CCKA_ENOMEM, "policy feature record alloc");
  if ((rc = mlp_alloc(c, N)) != CCKA_OK) return rc;
  if (pg) {
    if (!c->d_pg_seed.reserve(1)) return fail(c, CCKA_ENOMEM, "seed alloc");
    // the seed is data, not part of a captured sequence: a new seed replays the graph
    c->pg_seed_host = pg->seed;
    HIPCHK(c, hipMemcpyAsync(c->d_pg_seed, &c->pg_seed_host, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  }
  // ---- the fused loop (rollout_kernel<1, 8, POL>): one deployment, <= 8 node
  // slots and the MLP's W2 fragments + biases beside the kernel's LDS ----
  {
    const size_t mlp_lds = (size_t)((MLP_HID / 32) * (MLP_HID / 16) + MLP_HID / 16) * 64 * 16 + (2 * MLP_HID + 32) * 4;
    const size_t off = (lds + 15) & ~(size_t)15;
    if (!c->pol_fused_off && dmax == 1 && nmax == 8 && off + mlp_lds <= 160 * 1024) {
      k.feat = c->d_mx;  // the last step's features become the MLP states
      k.w1f = c->d_w1f;
      k.w2f = c->d_w2f;
      k.w3f = c->d_w3f;
      k.mlp_b = c->d_mb;
      k.pol_seed = pg ? c->d_pg_seed.get() : nullptr;
      k.rec_target = record ? c->d_rec_target.get() : nullptr;
      k.rec_cw = record ? c->d_rec_cw.get() : nullptr;
      k.pol_act = pg ? c->d_pg_act.get() : nullptr;
      k.feat_rec = feat_on ? c->d_feat_rec.get() : nullptr;
      k.lds_off_mlp = (int32_t)off;
      // diagnostic phase stamps (GK_STAMPS builds; ccka_debug_stamps)
      if ((k.ablate & 16) && (rc = stamps_buffer(c, &k.stamps)) != CCKA_OK) return rc;
      HIPCHK(c, hipEventRecord(c->ev0, c->stream));
      if (!c->pol_table_off && (rc = policy_tables(c, k)) != CCKA_OK) return rc;
      HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
      HIPCHK(c, launch_rollout_policy(k, off + mlp_lds, pg ? 2 : 1, c->stream));
      HIPCHK(c, hipEventRecord(c->ev1, c->stream));
      return loop_done(c, 4, trajectory, record, feat_on);
    }
  }
  // ---- the launched loop: the general kernel one step per launch, the
  // standalone MLP (mlp_kernel) and the action kernel between the steps ----
  const MlpParams mp = mlp_params(c, N, 32);
  // the policy's actions replace the scenarios' target / carbon-weight overrides
  k.target = c->d_pol_target;
  k.cw = c->d_pol_cw;
  k.state = c->d_pol_state;
  k.feat = c->d_mx;
  auto keep_feat = [&](int t) -> int {
    if (!feat_on) return CCKA_OK;
    HIPCHK(c, hipMemcpyAsync(c->d_feat_rec + (size_t)t * N * 64, c->d_mx, (size_t)N * 64 * 2, hipMemcpyDeviceToDevice,
                             c->stream));
    return CCKA_OK;
  };
  PgSampleParams q0{};
  if (pg) {
    q0.y = c->d_my;
    q0.target = c->d_pol_target;
    q0.cw = c->d_pol_cw;
    q0.n = N;
    q0.first_id = c->first_id;
    q0.seed = c->d_pg_seed;
  }
  // the whole loop: state initialisation (t = 0, features of step 0), then
  // per step MLP -> actions -> one rollout step (+ the features kept)
  auto enqueue = [&]() -> int {
    k.t0 = 0;
    k.t1 = 0;
    k.state_load = 0;
    HIPCHK(c, launch_rollout(k, block, lds, c->stream));
    if ((rc = keep_feat(0)) != CCKA_OK) return rc;
    for (int t = 0; t < T; ++t) {
      HIPCHK(c, launch_mlp(mp, c->cus, c->stream));
      if (pg) {
        PgSampleParams q = q0;
        q.act = c->d_pg_act + (size_t)t * N;
        q.rec_target = record ? c->d_rec_target + (size_t)t * N : nullptr;
        q.rec_cw = record ? c->d_rec_cw + (size_t)t * N : nullptr;
        q.t = t;
        HIPCHK(c, launch_policy_sample(q, c->stream));
      } else {
        HIPCHK(c, launch_policy_act(c->d_my, c->d_pol_target, c->d_pol_cw,
                                    record ? c->d_rec_target + (size_t)t * N : nullptr,
                                    record ? c->d_rec_cw + (size_t)t * N : nullptr, N, c->stream));
      }
      k.t0 = t;
      k.t1 = t + 1;
      k.state_load = 1;
      HIPCHK(c, launch_rollout(k, block, lds, c->stream));
      if ((rc = keep_feat(t + 1)) != CCKA_OK) return rc;
    }
    return CCKA_OK;
  };
  // (launches by the wave-cooperative catalog scans, no ptable: the argmin-table
  // path is the fused kernel's, whose register budget has room for it)
  // graph key: every input of the sequence (parameter blocks by value: their
  // device pointers and sizes)
  std::vector<unsigned char> key;
  auto put = [&](const void* v, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(v);
    key.insert(key.end(), b, b + n);
  };
  {
    KParams k0;
    std::memcpy(&k0, &k, sizeof k0);  // setup_general's zeroed padding with it
    k0.t0 = k0.t1 = k0.state_load = 0;
    put(&k0, sizeof k0);
    put(&mp, sizeof mp);
    put(&q0, sizeof q0);
    const int64_t misc[10] = {N, T, block, (int64_t)lds, record, feat_on, pg != nullptr, c->cus,
                              (int64_t)(uintptr_t)c->d_feat_rec.get(), (int64_t)(uintptr_t)c->d_rec_target.get()};
    put(misc, sizeof misc);
    const void* ptrs[3] = {c->d_rec_cw.get(), c->d_pg_act.get(), c->stream};
    put(ptrs, sizeof ptrs);
  }
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
  if (c->pol_graph_off) {
    if ((rc = enqueue()) != CCKA_OK) return rc;
  } else {
    if (!c->pol_graph || key != c->pol_graph_key) {
      if (c->pol_graph) {
        (void)hipGraphExecDestroy(c->pol_graph);
        c->pol_graph = nullptr;
      }
      hipGraph_t g = nullptr;
      HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      const int erc = enqueue();
      const hipError_t ce = hipStreamEndCapture(c->stream, &g);
      if (erc != CCKA_OK) {
        if (g) (void)hipGraphDestroy(g);
        return erc;
      }
      HIPCHK(c, ce);
      const hipError_t ie = hipGraphInstantiate(&c->pol_graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPCHK(c, ie);
      c->pol_graph_key = key;
    }
    HIPCHK(c, hipGraphLaunch(c->pol_graph, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  return loop_done(c, 3, trajectory, record, feat_on);
}

extern "C" {

int ccka_policy_rollout(ccka_ctx* c, int32_t trajectory, int32_t record) {
  return policy_loop(c, trajectory, record, nullptr);
}

// ---- differentiable control: the MLP backward (pg.hip) ----
// rows m = 0..M-1 of x [M][64] bf16 / act [M] / coef[m % n_scen] -> d_pg_grad
// (dW1 | db1 | dW2 | db2 | dW3 | db3, fp32, the layouts of ccka_mlp_set_weights)
static constexpr int64_t kGradFloats = 64 * 256 + 256 + 256 * 256 + 256 + 256 * 8 + 8;
// Rows per backward chunk: the work arrays hold 1,096 bf16 units per row
// (2.2 KB), so all N*T rows of a large loop do not fit at once (1e7 x 60 would
// need 1.3 TB). Chunks of kPgChunkRows rows run one after another, each
// chunk's gradient added to the running sum in chunk order: the result depends
// only on M, never on the memory available (deterministic); M <= one chunk is
// the unchunked computation.
constexpr int64_t kPgChunkRows = 1LL << 23;
constexpr int64_t kPgSplits = 256;  // weight-gradient row splits per chunk (at most; 512 measured 21.8 -> 22.6 ms)
static int64_t pg_chunk_rows(const ccka_ctx* c) { return c->pg_chunk > 0 ? c->pg_chunk : kPgChunkRows; }

static int pg_backward(ccka_ctx* c, const uint16_t* x, const uint8_t* act, const float* coef, int64_t n_scen,
                       int64_t M) {
  if (!c->mlp_have_w) return fail(c, CCKA_ESTATE, "MLP weights not set (ccka_mlp_set_weights)");
  if (M < 1 || n_scen < 1) return fail(c, CCKA_EINVAL, "no rows");
  const int64_t rows = 64 + 4 * MLP_HID + 8;  // xT h1T h2T dh1T dh2T gyT
  const int64_t CH = pg_chunk_rows(c);
  const int64_t cap = (std::min(M, CH) + 31) / 32 * 32;
  if (!c->d_pg_work.reserve(rows * cap))
    return fail(c, CCKA_ENOMEM, "policy-gradient work alloc (%lld rows x %lld)", (long long)rows, (long long)cap);
  if (!c->d_pg_grad.reserve(kGradFloats)) return fail(c, CCKA_ENOMEM, "gradient alloc");
  // the three weight-gradient GEMMs over all rows, each with its bias gradient
  // (the row sums of its B operand) folded in: dW1 | db1, dW2 | db2, dW3 | db3
  const int64_t o_b1 = 64 * 256, o_w2 = o_b1 + 256, o_b2 = o_w2 + 256 * 256, o_w3 = o_b2 + 256, o_b3 = o_w3 + 256 * 8;
  for (int64_t r0 = 0; r0 < M; r0 += CH) {
    const int64_t Mc = std::min(CH, M - r0);
    const int64_t Mpad = (Mc + 31) / 32 * 32;
    c->pg_mpad = Mpad;
    uint16_t* xT = c->d_pg_work;
    uint16_t* h1T = xT + 64 * Mpad;
    uint16_t* h2T = h1T + MLP_HID * Mpad;
    uint16_t* dh1T = h2T + MLP_HID * Mpad;
    uint16_t* dh2T = dh1T + MLP_HID * Mpad;
    uint16_t* gyT = dh2T + MLP_HID * Mpad;
    PgRowsParams rp{};
    rp.x = x + r0 * MLP_IN;
    rp.act = act + r0;
    rp.coef = coef;
    rp.w1f = c->d_w1f;
    rp.w2f = c->d_w2f;
    rp.w3f = c->d_w3f;
    rp.w2b = c->d_w2b;
    rp.w3b = c->d_w3b;
    rp.bias = c->d_mb;
    rp.xT = xT; rp.h1T = h1T; rp.h2T = h2T; rp.dh1T = dh1T; rp.dh2T = dh2T; rp.gyT = gyT;
    rp.M = Mc;
    rp.Mpad = Mpad;
    rp.n_scen = n_scen;
    rp.row0 = r0;
    HIPCHK(c, launch_pg_rows(rp, c->cus, c->stream));
    struct G { const uint16_t* a; int ka; const uint16_t* b; int kb; int64_t off, boff; };
    const G gs[3] = {{xT, 64, dh1T, MLP_HID, 0, o_b1}, {h1T, MLP_HID, dh2T, MLP_HID, o_w2, o_b2},
                     {h2T, MLP_HID, gyT, MLP_OUT, o_w3, o_b3}};
    // one workgroup per split owns a share of the chunk's rows and the whole
    // output (pg.hip); the split count is a function of Mpad alone (256 = the
    // MI355X's CU count, not the device's), so the gradient's summation order
    // and bits do not depend on the GPU or its partition mode
    const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(kPgSplits, Mpad / 256));
    // each split's partials in the packed gradient order (w1 | b1 | w2 | b2 |
    // w3 | b3): one reduction for the three GEMMs
    const int64_t need = (int64_t)splits * kGradFloats;
    if (!c->d_pg_part.reserve(need)) return fail(c, CCKA_ENOMEM, "gradient partials alloc");
    for (const G& g : gs) {
      WgradParams q{};
      q.A = g.a;
      q.B = g.b;
      q.part = c->d_pg_part + g.off;
      q.bpart = c->d_pg_part + g.boff;
      q.Mpad = Mpad;
      q.pstride = kGradFloats;
      q.KA = g.ka;
      q.KB = g.kb;
      q.splits = splits;
      HIPCHK(c, launch_pg_wgrad(q, c->stream));
    }
    HIPCHK(c, launch_pg_reduce(c->d_pg_part, c->d_pg_grad, kGradFloats, splits, r0 > 0 ? 1 : 0, c->stream));
  }
  return CCKA_OK;
}

static int pg_copy_grads(ccka_ctx* c, ccka_mlp_grads* out) {
  if (!out) return CCKA_OK;
  const int64_t o_b1 = 64 * 256, o_w2 = o_b1 + 256, o_b2 = o_w2 + 256 * 256, o_w3 = o_b2 + 256, o_b3 = o_w3 + 256 * 8;
  const struct { float* dst; int64_t off, n; } m[6] = {{out->w1, 0, 64 * 256}, {out->b1, o_b1, 256},
                                                      {out->w2, o_w2, 256 * 256}, {out->b2, o_b2, 256},
                                                      {out->w3, o_w3, 256 * 8}, {out->b3, o_b3, 8}};
  for (const auto& x : m)
    if (x.dst) HIPCHK(c, hipMemcpyAsync(x.dst, c->d_pg_grad + x.off, (size_t)x.n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_mlp_backward(ccka_ctx* c, const uint16_t* x, const uint8_t* actions, const float* coef, int64_t m,
                      ccka_mlp_grads* out) {
  if (!c || !x || !actions || !coef || !out || m < 1) return CCKA_EINVAL;
  // every state and argument check before the first buffer is touched: the
  // rows go through the samples' buffers, and a failing call changes nothing
  if (!c->mlp_have_w) return fail(c, CCKA_ESTATE, "MLP weights not set (ccka_mlp_set_weights)");
  for (int64_t i = 0; i < m; ++i)
    if (actions[i] >= MLP_OUT) return fail(c, CCKA_EINVAL, "action %d of row %lld out of range", actions[i], (long long)i);
  (void)hipSetDevice(c->device);
  c->pg_valid = false;  // the recorded samples of ccka_policy_grad are gone
  if (!c->d_pg_x.reserve(m * MLP_IN)) return fail(c, CCKA_ENOMEM, "backward rows alloc");
  if (!c->d_pg_act.reserve(m)) return fail(c, CCKA_ENOMEM, "action alloc");
  if (!c->d_pg_coef.reserve(m)) return fail(c, CCKA_ENOMEM, "coef alloc");
  HIPCHK(c, hipMemcpyAsync(c->d_pg_x, x, (size_t)m * MLP_IN * 2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_pg_act, actions, (size_t)m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_pg_coef, coef, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  int rc;
  if ((rc = pg_backward(c, c->d_pg_x, c->d_pg_act, c->d_pg_coef, m, m)) != CCKA_OK) return rc;
  return pg_copy_grads(c, out);
}

int ccka_policy_grad(ccka_ctx* c, const ccka_pg_params* pg, ccka_mlp_grads* out, double* objective_mean) {
  if (!c || !pg) return CCKA_EINVAL;
  if (!(pg->w_carbon >= 0.0) || !(pg->w_slo >= 0.0)) return fail(c, CCKA_EINVAL, "objective weights must be >= 0");
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = policy_loop(c, 0, 1, pg)) != CCKA_OK) return rc;
  const int64_t N = c->N;
  const int64_t T = c->hw.n_steps;
  // J_i = cost $ + w_c gCO2 kg + w_s SLO minutes; coef_i = (J_i - b) / N
  std::vector<int64_t> cost((size_t)N);
  std::vector<double> g((size_t)N);
  std::vector<int32_t> slo((size_t)N);
  HIPCHK(c, hipMemcpyAsync(cost.data(), c->res.cost, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(g.data(), c->res.gco2, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(slo.data(), c->res.slo, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<double> J((size_t)N);
  double sum = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    J[(size_t)i] = (double)cost[(size_t)i] / 6e7 + pg->w_carbon * (g[(size_t)i] * 1e-3) + pg->w_slo * (double)slo[(size_t)i];
    sum += J[(size_t)i];
  }
  const double mean = sum / (double)N, b = pg->baseline ? mean : 0.0;
  std::vector<float> coef((size_t)N);
  for (int64_t i = 0; i < N; ++i) coef[(size_t)i] = (float)((J[(size_t)i] - b) / (double)N);
  if (objective_mean) *objective_mean = mean;
  if (!c->d_pg_coef.reserve(N)) return fail(c, CCKA_ENOMEM, "coef alloc");
  HIPCHK(c, hipMemcpyAsync(c->d_pg_coef, coef.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
  // rows (t, i) -> m = t N + i: the recorded features [T+1][N][64] (steps 0..T-1) and actions [T][N]
  if ((rc = pg_backward(c, c->d_feat_rec, c->d_pg_act, c->d_pg_coef, N, T * N)) != CCKA_OK) return rc;
  c->pg_valid = true;
  c->pg_T = T;
  return pg_copy_grads(c, out);
}

// Internal (tests): the backward's work arrays of the last ccka_mlp_backward /
// ccka_policy_grad (its last row chunk): xT | h1T | h2T | dh1T | dh2T | gyT,
// each row-blocked [Mpad/16][units][16] bf16, (64 + 4 * 256 + 8) * Mpad
// elements; *mpad receives that backward's Mpad (the buffer itself only grows,
// so its capacity does not locate the arrays after a smaller backward).
int ccka_debug_pg_work(ccka_ctx* c, uint16_t* out, int64_t count, int64_t* mpad) {
  if (!c || !out || !mpad || !c->d_pg_work || c->pg_mpad < 1) return CCKA_EINVAL;
  const int64_t rows = 64 + 4 * MLP_HID + 8;
  const int64_t have = rows * c->pg_mpad;
  if (have > c->d_pg_work.count()) return fail(c, CCKA_ESTATE, "work arrays released");
  if (count < have) return fail(c, CCKA_EINVAL, "need %lld", (long long)have);
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *mpad = c->pg_mpad;
  HIPCHK(c, hipMemcpy(out, c->d_pg_work, (size_t)have * 2, hipMemcpyDeviceToHost));
  return CCKA_OK;
}

int ccka_get_policy_samples(ccka_ctx* c, uint8_t* actions, float* coef, int64_t count) {
  if (!c || !actions || !coef) return CCKA_EINVAL;
  if (!c->pg_valid) return fail(c, CCKA_ESTATE, "no ccka_policy_grad samples");
  if (count != c->pg_T * c->N) return fail(c, CCKA_EINVAL, "sample count mismatch");
  if (!copy_fits(count, c->d_pg_act.count()) || !copy_fits(c->N, c->d_pg_coef.count()))
    return fail(c, CCKA_ESTATE, "sample records smaller than this batch");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(actions, c->d_pg_act, (size_t)count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(coef, c->d_pg_coef, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_get_policy_actions(ccka_ctx* c, int16_t* target, double* cw, int64_t count) {
  if (!c || !target || !cw) return CCKA_EINVAL;
  if (!c->pol_rec_valid) return fail(c, CCKA_ESTATE, "last run recorded no policy actions");
  if (count != (int64_t)c->hw.n_steps * c->N) return fail(c, CCKA_EINVAL, "action count != T x N");
  if (!copy_fits(count, c->d_rec_target.count()) || !copy_fits(count, c->d_rec_cw.count()))
    return fail(c, CCKA_ESTATE, "action records smaller than this batch");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(target, c->d_rec_target, (size_t)count * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cw, c->d_rec_cw, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

// Internal test hooks (not part of include/ccka.h): record the policy
// features of every step ([T + 1][N][64] bf16) and read them back.
int ccka_debug_policy_features(ccka_ctx* c, int32_t enable) {
  if (!c) return CCKA_EINVAL;
  c->pol_feat_on = enable != 0;
  return CCKA_OK;
}

int ccka_debug_get_policy_features(ccka_ctx* c, uint16_t* out, int64_t count) {
  if (!c || !out) return CCKA_EINVAL;
  if (!c->pol_feat_valid || !c->pol_rec_valid) return fail(c, CCKA_ESTATE, "no recorded features");
  if (count != (int64_t)(c->hw.n_steps + 1) * c->N * 64) return fail(c, CCKA_EINVAL, "feature count mismatch");
  if (!copy_fits(count, c->d_feat_rec.count())) return fail(c, CCKA_ESTATE, "feature records smaller than this batch");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(out, c->d_feat_rec, (size_t)count * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

}  // extern "C"
