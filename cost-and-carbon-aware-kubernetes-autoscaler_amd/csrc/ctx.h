// ctx.h — the context behind libccka.so's C ABI (include/ccka.h), shared by
// the abi_*.cpp units: its state and device buffers, error reporting, and the
// few helpers more than one unit calls.
//
// A context owns its device buffers as DevBufs (devbuf.h): each carries its own
// element count and is freed with the context. Kernel argument blocks
// (kparams.h) are built per call from this state, never kept here.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ccka.h"
#include "devbuf.h"
#include "kparams.h"

// internal to libccka.so: nothing below is an exported symbol
#pragma GCC visibility push(hidden)

struct ccka_ctx {
  template <class T>
  using Buf = ccka::DevBuf<T>;

  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev_mid = nullptr, ev1 = nullptr;  // ev_mid: after the argmin tables
  std::string err;
  int cus = 0;
  char name[128] = {0};
  // world
  bool have_world = false;
  ccka_world hw{};
  Buf<ccka_world> d_world;
  Buf<ccka_itype> d_types;
  Buf<int32_t> d_price;
  Buf<double> d_ci_gpwh;
  Buf<double> d_ci_gpwmin;
  int prov[CCKA_MAX_DEPLOY] = {0};
  // scenarios
  bool have_sc = false;
  int64_t N = 0, first_id = 0, n_traces = 0;
  std::vector<uint8_t> h_region;
  Buf<uint8_t> d_region;
  Buf<int16_t> d_target;
  Buf<int16_t> d_maxr;
  Buf<int16_t> d_dstab;
  Buf<int16_t> d_resetca;
  Buf<uint8_t> d_pswitch;
  Buf<double> d_cw;
  Buf<uint8_t> d_capsel;
  // traces / outputs
  Buf<int32_t> d_load;  // [T][D][NL]
  bool have_load = false;
  // wave-tiled copy of the trace for the single-deployment kernel (d1_trace_tile)
  Buf<int32_t> d_load_w;
  int32_t load_w_lpw = 0;  // lanes per wave it was tiled for (0: stale)
  // scenario-major copy [NL][T][DP] of the trace for the general kernel's
  // lane-skewed schedule (sk_trace); load_nt_dp = the DP it was built for (0: stale)
  Buf<int32_t> d_load_nt;
  int32_t load_nt_dp = 0;
  bool trace_flat = false;  // ccka_debug_trace_flat: read [T][N] (A/B of the layout)
  Buf<char> d_res;  // one allocation, SoA carve
  ccka::ResultPtrs res{};
  Buf<ccka_traj_rec> d_traj;  // [T][N] records (or [N][T]: traj_nt)
  bool traj_valid = false;
  bool traj_nt = false;          // device records are [N][T] (single-deployment engine)
  Buf<ccka_traj_rec> d_traj_t;  // [T][N] staging blocks for ccka_get_trajectory
  int64_t traj_stage = 0;       // their capacity in records (ccka_debug_traj_stage; 0: kTrajStageRecs)
  Buf<long long> d_parts;
  Buf<ccka_totals> d_totals;
  Buf<int32_t> d_sinq;
  ncclComm_t comm = nullptr;
  double last_ms = 0.0;        // rollout kernel (HIP events on the engine stream)
  double last_table_ms = 0.0;  // argmin-table kernel of the same rollout
  bool ran = false;        // a timed launch exists (ccka_sync / ccka_last_kernel_ms): rollout, loop or MLP forward
  bool res_valid = false;  // the result columns hold a run of this world and scenario set (every results getter)
  // single-deployment engine (rollout_d1.hip): world digest, argmin tables
  bool d1_world = false;     // the world qualifies (d1_check_world)
  bool d1_ready = false;     // scenario-dependent part prepared
  bool d1_ok = false;        // world + scenarios qualify
  bool sc_maxr_ok = true;
  int sc_dstab_max = -1;      // largest per-scenario down_stab_s override (-1: none given)
  int sc_target_max = -1;     // largest per-scenario target_util_pct override (-1: none given)
  int sc_maxr_max = -1;       // largest per-scenario max_replicas override (-1: none given)
  // HPA decision history in HBM for long windows / sub-steps (general kernel)
  Buf<int2> d_hist;
  uint32_t sc_capsel_or = 0;  // OR of the per-scenario cap_sel overrides (0: none given)
  int sc_pswitch_any = -1;    // any per-scenario peak_switch set (-1: none given)
  // the world / scenario digest of d1_check_world and d1_prepare; the buffers,
  // results and per-rollout choices are filled into a copy at the launch
  ccka::D1Params d1{};
  std::vector<uint32_t> zmasks;
  std::vector<double> h_cw;  // per-scenario carbon weights (empty: world default)
  Buf<long long> d_acc;
  Buf<int32_t> d_order;
  Buf<int32_t> d_cap1s;
  Buf<int32_t> d_cap1t;  // pod capacity per type (argmin-table entries)
  Buf<uint32_t> d_zmasks;
  Buf<double> d_wc1000;
  Buf<uint8_t> d_wci;
  Buf<int2> d_table;
  Buf<int32_t> d_jtab;
  Buf<int2> d_table2;   // G2 offer table (replacement consolidation in the single-deployment kernel)
  Buf<int32_t> d_jtab2;
  Buf<double> d_wc0;    // one zero carbon weight (the offer table's score is the price)
  int JT = 0, NW = 0;
  int engine_mode = 0;       // 0 auto, 1 general kernel only, 2 general kernel in lockstep (ccka_debug_engine)
  bool sk_coop_f2 = false;   // skewed schedule: keep the wave-cooperative provisioning (ccka_debug_engine 3)
  int32_t ablate = 0;        // profiling-only phase switches (ccka_debug_ablate; 0 in every real run)
  Buf<unsigned long long> d_stamps;
  int lpw = 0;               // scenarios per wave of the single-deployment kernel (0 = automatic)
  int occ = 0;               // its register-allocation occupancy target (0 = automatic)
  int mlp_stamps = 0;        // diagnostic MLP phase stamps (ccka_debug_mlp_stamps)
  // policy sweep (config 4)
  Buf<ccka_grid_stats> d_gstats;
  Buf<ccka_grid_stats> d_gcand;
  Buf<ccka_grid_stats> d_ggather;
  Buf<int64_t> d_gcounts;
  Buf<int32_t> d_gn;
  Buf<uint8_t> d_gflags;
  Buf<ccka_grid_stats> d_gfront;   // the frontier (local or global)
  // fleet timeline (SEMANTICS 7): the rows of the last ccka_get_timeline
  Buf<ccka_timeline_row> d_tlrows;
  // paired comparison (SEMANTICS 8): the snapshot [4][snap_n] of a batch's
  // integer vectors, kept across worlds, scenarios and rollouts (abi_paired.cpp)
  Buf<int64_t> d_snap;
  bool have_snap = false;
  int64_t snap_first = 0, snap_n = 0, snap_grid_size = 0, snap_traces = 0;
  Buf<ccka_paired_row> d_prows;  // the rows of the last ccka_get_paired
  Buf<uint32_t> d_pflag;         // its overflow word (and a capture's)
  // paired bootstrap (SEMANTICS 9, abi_boot.cpp): per pass of grids the deltas
  // [tiles][grid_size][K][4] and the replicate sums [grids][4][B]; the rows of
  // the last ccka_get_paired_bootstrap. The overflow word is d_pflag.
  Buf<int64_t> d_bdelta;
  Buf<int64_t> d_bsums;
  Buf<ccka_boot_row> d_brows;
  int64_t boot_max_sums = 0;  // ccka_debug_boot_workspace: sums per pass (0: kBootMaxSums)
  // learned MLP policy (config 5)
  bool mlp_have_w = false;
  Buf<ccka::mlp_bf16x8> d_w1f;
  Buf<ccka::mlp_bf16x8> d_w2f;
  Buf<ccka::mlp_bf16x8> d_w3f;
  // the standalone forward's fragments for v_mfma_f32_16x16x32_bf16 (mlp16_kernel)
  Buf<ccka::mlp_bf16x8> d_w1g;
  Buf<ccka::mlp_bf16x8> d_w2g;
  Buf<ccka::mlp_bf16x8> d_w3g;
  int mlp_tile = 16;         // standalone forward: 16 (mlp16_kernel) or 32 (mlp_kernel; ccka_debug_mlp_tile)
  Buf<float> d_mb;  // b1[256] b2[256] b3[8]
  Buf<uint16_t> d_mx;  // states [n][64] bf16 and actions [n][8]: sized together (mlp_alloc)
  Buf<float> d_my;
  int64_t mlp_n = 0;
  int last_engine = 0;       // 1 general, 2 single-deployment
  // launch plan of the last ccka_rollout_async (ccka_debug_last_plan): what
  // plan_launch, the engine choice and launch_rollout_d1 decided; -1 = the
  // field does not apply to the engine that ran. Recorded only, never read back.
  int32_t last_plan[ccka::PLAN_FIELDS] = {0};
  // closed-loop policy rollout (config 5)
  Buf<int32_t> d_pol_state;
  Buf<int16_t> d_pol_target;
  Buf<double> d_pol_cw;
  Buf<int16_t> d_rec_target;
  Buf<double> d_rec_cw;
  bool pol_rec_valid = false;
  bool pol_feat_valid = false;  // the last loop kept its features (the switch was on, or ccka_policy_grad)
  bool pol_feat_on = false;
  // the closed loop's launch sequence captured as one hipGraph, replayed while
  // its inputs (launch parameters, buffers, sizes) are unchanged
  hipGraphExec_t pol_graph = nullptr;
  std::vector<unsigned char> pol_graph_key;
  bool pol_graph_off = false;  // ccka_debug_policy_graph(0): launch the sequence directly
  bool pol_fused_off = false;  // ccka_debug_policy_fused(0): the launched loop even where the fused one applies
  bool pol_table_off = false;  // ccka_debug_policy_table(0): the fused loop's catalog scans instead of the tables
  int64_t pg_chunk = 0;        // ccka_debug_pg_chunk: rows per backward chunk (0: kPgChunkRows)
  int64_t pg_mpad = 0;         // Mpad of the last backward's last chunk: what d_pg_work holds (ccka_debug_pg_work)
  Buf<int2> d_ptable;          // the fused loop's argmin tables (65 policy carbon weights)
  Buf<int32_t> d_pjtab;
  Buf<double> d_pwc;
  Buf<uint16_t> d_feat_rec;
  // differentiable control (ccka_policy_grad / ccka_mlp_backward, pg.hip)
  Buf<ccka::mlp_bf16x8> d_w2b;   // A fragments of dH1^T = W2 dH2^T
  Buf<ccka::mlp_bf16x8> d_w3b;   // A fragments of dH2^T = W3 g_y^T
  Buf<uint8_t> d_pg_act;         // sampled actions [T][N] (or the rows of ccka_mlp_backward)
  Buf<float> d_pg_coef;          // per-scenario (J - b) / N (or per row)
  Buf<uint64_t> d_pg_seed;       // the sampling key of the stochastic loop (outside the graph key)
  uint64_t pg_seed_host = 0;
  Buf<uint16_t> d_pg_x;          // ccka_mlp_backward's rows [M][64]
  Buf<uint16_t> d_pg_work;       // xT | h1T | h2T | dh1T | dh2T | gyT, each row-blocked [Mpad/16][units][16]
  Buf<float> d_pg_part;          // weight-gradient row-split partials
  Buf<float> d_pg_grad;          // dW1 | db1 | dW2 | db2 | dW3 | db3
  bool pg_valid = false;
  int64_t pg_T = 0;
  // per-scenario summary breakdown (ccka_set_detail)
  bool detail_on = false;
  bool detail_valid = false;
  Buf<ccka::DetailDev> d_detail;
};

int fail(ccka_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIPCHK(c, x)                                                              \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess)                                                         \
      return fail((c), CCKA_EHIP, "%s: %s", #x, hipGetErrorString(e_));          \
  } while (0)

// dst = a device copy of src[count] (on the context's stream); empty for a null source
template <class T>
int dupload(ccka_ctx* c, ccka::DevBuf<T>& dst, const T* src, size_t count) {
  if (!src) count = 0;
  if (!dst.resize((int64_t)count)) return fail(c, CCKA_ENOMEM, "hipMalloc %zu bytes failed", sizeof(T) * count);
  if (count) HIPCHK(c, hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, c->stream));
  return CCKA_OK;
}

inline int64_t load_cols(const ccka_ctx* c) { return c->n_traces > 0 ? c->n_traces : c->N; }

// block partials of the totals reduction (d_parts: 11 words each, then the overflow word)
constexpr int kTotalsParts = 1024;

// abi_ctx.cpp
bool rules_fit_ring(const ccka_hpa_rules& r);
int d1_prepare(ccka_ctx* c);
int64_t carve_results(char* p, int64_t N, ccka::ResultPtrs* out);
ccka::TableParams table_params(const ccka_ctx* c, const double* wc1000, int NW, int2* table, int32_t* jtab);
// abi_rollout.cpp
int setup_general(ccka_ctx* c, int32_t trajectory, ccka::KParams& k, int* block_out, size_t* lds_out);
int totals_of(ccka_ctx* c, const ccka::ResultPtrs& res, int64_t N, ccka_totals* out);
// abi_sweep.cpp: the kinds and q_ppm of a statistic (CCKA_EINVAL, or for a null one)
int check_sweep_stat(ccka_ctx* c, const ccka_sweep_stat* st);
// abi_paired.cpp: the checks and helpers the paired comparison (SEMANTICS 8)
// shares with the paired bootstrap (abi_boot.cpp)
int paired_state(ccka_ctx* c);  // CCKA_ESTATE before a rollout or without a snapshot
// a batch (first_id, n) as whole grids of grid_size whose positions share traces
int paired_shape(ccka_ctx* c, int64_t grid_size, int64_t n_traces, int64_t first_id, int64_t n);
// paired_shape of the last rollout's batch, and grid_size / n_traces equal to the snapshot's
int paired_rollout_shape(ccka_ctx* c, int64_t grid_size);
ccka::GridSrc result_columns(const ccka::ResultPtrs& r, int64_t grid_size, int64_t first_id, int64_t n);
struct PairedBase {
  int64_t grid;  // global id of row 0's baseline grid
  int64_t step;  // added per row: 0, or grid_size (CCKA_PAIRED_SAME)
  int64_t off;   // snapshot index of position 0 of row 0's baseline grid
};
int paired_baseline(ccka_ctx* c, const ccka::GridSrc& cur, int64_t snap_n, int64_t snap_first_grid,
                    int64_t base_grid, PairedBase* out);
int read_flag(ccka_ctx* c, const uint32_t* flag, uint32_t* out);
int capture_into(ccka_ctx* c, const ccka::GridSrc& g, int64_t* snap);
// caller-supplied result columns on the device for the debug entry points: `n`
// current and `nb` baseline scenarios as whole grids of gs (grid ids from 0 on
// both sides), the baseline captured into a snapshot of its own. upload()
// synchronises unless it fails on its arguments; the owner synchronises the
// stream again before the columns go.
struct PairedDebugCols {
  ccka::DevBuf<int64_t> d_cost, d_bcost, d_snap;
  ccka::DevBuf<int32_t> d_slo, d_bslo;
  ccka::DevBuf<double> d_gco2, d_energy, d_bgco2, d_benergy;
  ccka::GridSrc cur{};
  int upload(ccka_ctx* c, const int64_t* cost, const int32_t* slo, const double* gco2, const double* energy,
             int64_t n, const int64_t* bcost, const int32_t* bslo, const double* bgco2, const double* benergy,
             int64_t nb, int64_t gs);
};
// abi_mlp.cpp
int mlp_alloc(ccka_ctx* c, int64_t n);
ccka::MlpParams mlp_params(const ccka_ctx* c, int64_t n, int tile);
// abi_debug.cpp
int stamps_buffer(ccka_ctx* c, unsigned long long** out);

#pragma GCC visibility pop
