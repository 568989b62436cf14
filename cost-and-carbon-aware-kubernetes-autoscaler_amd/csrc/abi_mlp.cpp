// abi_mlp.cpp — the learned MLP policy of libccka.so's C ABI (BASELINE config
// 5): packing the weights into MFMA fragment order, the states, the standalone
// forward (mlp.hip) and its measurement hook.
#include <cstring>
#include <vector>

#include "ctx.h"

using namespace ccka;

// MFMA fragment order of the weights (see mlp.hip). Lane l: r = l & 31, h = l >> 5.
// Layer 1 A operand (natural k): element j = W1[16s + 8h + j][32n + r].
// Layers 2/3 A operand, k-step kk, in the k order of the chained accumulator:
// element j <-> input unit 32(kk>>1) + 16(kk&1) + 8(j>>2) + 4h + (j&3).
static int kin(int kk, int j, int h) { return 32 * (kk >> 1) + 16 * (kk & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }
// 16x16x32 (mlp16_kernel), lane l: i = l & 15 (output row of the tile), g = l >> 4.
// Layer 1 A operand (natural k): element e = W1[32s + 8g + e][16o + i].
// Layers 2/3, k-step s, chained order: element e <-> input unit 32s + 16(e>>2) + 4g + (e&3).
static int kin16(int s, int e, int g) { return 32 * s + 16 * (e >> 2) + 4 * g + (e & 3); }

extern "C" {

int ccka_mlp_set_weights(ccka_ctx* c, int32_t in_dim, int32_t hidden, int32_t out_dim, const uint16_t* w1,
                         const float* b1, const uint16_t* w2, const float* b2, const uint16_t* w3, const float* b3) {
  if (!c || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return CCKA_EINVAL;
  if (in_dim != MLP_IN || hidden != MLP_HID || out_dim != MLP_OUT)
    return fail(c, CCKA_EINVAL, "MLP shape %dx%dx%d unsupported (64 -> 256 -> 256 -> 8)", in_dim, hidden, out_dim);
  (void)hipSetDevice(c->device);
  std::vector<uint16_t> f1((size_t)8 * 4 * 64 * 8), f2((size_t)8 * 16 * 64 * 8), f3((size_t)16 * 64 * 8, 0);
  for (int n = 0; n < 8; ++n)
    for (int st = 0; st < 4; ++st)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int r = l & 31, h = l >> 5;
          f1[(((size_t)n * 4 + st) * 64 + l) * 8 + j] = w1[(size_t)(16 * st + 8 * h + j) * MLP_HID + 32 * n + r];
        }
  for (int n = 0; n < 8; ++n)
    for (int kk = 0; kk < 16; ++kk)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int r = l & 31, h = l >> 5;
          f2[(((size_t)n * 16 + kk) * 64 + l) * 8 + j] = w2[(size_t)kin(kk, j, h) * MLP_HID + 32 * n + r];
        }
  for (int kk = 0; kk < 16; ++kk)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const int r = l & 31, h = l >> 5;
        if (r < MLP_OUT) f3[((size_t)kk * 64 + l) * 8 + j] = w3[(size_t)kin(kk, j, h) * MLP_OUT + r];
      }
  // backward (pg.hip): dH1^T = W2 dH2^T with dH2^T chained in the same permuted
  // k order (rows = H1 units), dH2^T = W3 g_y^T with k = action padded to 16
  std::vector<uint16_t> f2b((size_t)8 * 16 * 64 * 8), f3b((size_t)8 * 64 * 8, 0);
  for (int n = 0; n < 8; ++n)
    for (int kk = 0; kk < 16; ++kk)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int r = l & 31, h = l >> 5;
          f2b[(((size_t)n * 16 + kk) * 64 + l) * 8 + j] = w2[(size_t)(32 * n + r) * MLP_HID + kin(kk, j, h)];
        }
  for (int n = 0; n < 8; ++n)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const int r = l & 31, h = l >> 5;
        if (h == 0) f3b[((size_t)n * 64 + l) * 8 + j] = w3[(size_t)(32 * n + r) * MLP_OUT + j];
      }
  std::vector<uint16_t> g1((size_t)16 * 2 * 64 * 8), g2((size_t)16 * 8 * 64 * 8), g3((size_t)8 * 64 * 8, 0);
  for (int o = 0; o < 16; ++o)
    for (int st = 0; st < 2; ++st)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int i = l & 15, g = l >> 4;
          g1[(((size_t)o * 2 + st) * 64 + l) * 8 + e] = w1[(size_t)(32 * st + 8 * g + e) * MLP_HID + 16 * o + i];
        }
  for (int o = 0; o < 16; ++o)
    for (int st = 0; st < 8; ++st)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int i = l & 15, g = l >> 4;
          g2[(((size_t)o * 8 + st) * 64 + l) * 8 + e] = w2[(size_t)kin16(st, e, g) * MLP_HID + 16 * o + i];
        }
  for (int st = 0; st < 8; ++st)
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < 8; ++e) {
        const int i = l & 15, g = l >> 4;
        if (i < MLP_OUT) g3[((size_t)st * 64 + l) * 8 + e] = w3[(size_t)kin16(st, e, g) * MLP_OUT + i];
      }
  std::vector<float> bias(MLP_HID * 2 + 32);  // b3 zero-padded to one 32-row tile
  std::memcpy(bias.data(), b1, MLP_HID * 4);
  std::memcpy(bias.data() + MLP_HID, b2, MLP_HID * 4);
  std::memcpy(bias.data() + 2 * MLP_HID, b3, MLP_OUT * 4);
  int rc;
  if ((rc = dupload(c, c->d_w1f, (const mlp_bf16x8*)f1.data(), f1.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w2f, (const mlp_bf16x8*)f2.data(), f2.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w3f, (const mlp_bf16x8*)f3.data(), f3.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_mb, bias.data(), bias.size())) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w2b, (const mlp_bf16x8*)f2b.data(), f2b.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w3b, (const mlp_bf16x8*)f3b.data(), f3b.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w1g, (const mlp_bf16x8*)g1.data(), g1.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w2g, (const mlp_bf16x8*)g2.data(), g2.size() / 8)) != CCKA_OK) return rc;
  if ((rc = dupload(c, c->d_w3g, (const mlp_bf16x8*)g3.data(), g3.size() / 8)) != CCKA_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->mlp_have_w = true;
  return CCKA_OK;
}

}  // extern "C"

// states [n][64] and actions [n][8], sized together
int mlp_alloc(ccka_ctx* c, int64_t n) {
  if (n < 1 || n > ((int64_t)1 << 34)) return fail(c, CCKA_EINVAL, "state count out of range");
  c->mlp_n = 0;
  if (!all_or_none(c->d_mx.reserve(n * MLP_IN) && c->d_my.reserve(n * MLP_OUT), c->d_mx, c->d_my))
    return fail(c, CCKA_ENOMEM, "MLP state/action buffers (%lld states)", (long long)n);
  c->mlp_n = n;
  return CCKA_OK;
}

// the MLP kernels' block over n states: tile 16 = mlp16_kernel (its own
// fragment arrays set), 32 = mlp_kernel
MlpParams mlp_params(const ccka_ctx* c, int64_t n, int tile) {
  MlpParams p{};
  p.x = c->d_mx;
  p.y = c->d_my;
  p.w1f = c->d_w1f;
  p.w2f = c->d_w2f;
  p.w3f = c->d_w3f;
  p.b1 = c->d_mb;
  p.b2 = c->d_mb + MLP_HID;
  p.b3 = c->d_mb + 2 * MLP_HID;
  p.N = n;
  if (tile == 16) {
    p.w1g = c->d_w1g;
    p.w2g = c->d_w2g;
    p.w3g = c->d_w3g;
  }
  return p;
}

extern "C" {

int ccka_mlp_set_states(ccka_ctx* c, const uint16_t* x, int64_t n) {
  if (!c || !x) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = mlp_alloc(c, n)) != CCKA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_mx, x, (size_t)n * MLP_IN * 2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_mlp_gen_states(ccka_ctx* c, int64_t n, uint64_t seed) {
  if (!c) return CCKA_EINVAL;
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = mlp_alloc(c, n)) != CCKA_OK) return rc;
  HIPCHK(c, launch_mlp_gen_states(c->d_mx, n * MLP_IN, seed, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

int ccka_mlp_forward_async(ccka_ctx* c) {
  if (!c) return CCKA_EINVAL;
  if (!c->mlp_have_w || !c->mlp_n) return fail(c, CCKA_ESTATE, "MLP weights / states not set");
  (void)hipSetDevice(c->device);
  MlpParams p = mlp_params(c, c->mlp_n, c->mlp_tile);
  int rc;
  if (c->mlp_stamps && (rc = stamps_buffer(c, &p.stamps)) != CCKA_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
  HIPCHK(c, launch_mlp(p, c->cus, c->stream));
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  c->ran = true;
  return CCKA_OK;
}

// Internal measurement hook (bench.py config 5): `launches` back-to-back MLP
// launches with an event pair around each one; *avg_ms = the mean kernel
// duration (what rocprofv3 --kernel-trace averages), *span_ms = first start
// to last end (launch gaps included).
int ccka_debug_mlp_batch(ccka_ctx* c, int32_t launches, double* avg_ms, double* span_ms) {
  if (!c || !avg_ms || !span_ms || launches < 1 || launches > 4096) return CCKA_EINVAL;
  if (!c->mlp_have_w || !c->mlp_n) return fail(c, CCKA_ESTATE, "MLP weights / states not set");
  (void)hipSetDevice(c->device);
  struct Events {  // destroyed on every way out
    std::vector<hipEvent_t> v;
    ~Events() {
      for (hipEvent_t e : v)
        if (e) (void)hipEventDestroy(e);
    }
  } events{std::vector<hipEvent_t>((size_t)launches * 2, nullptr)};
  std::vector<hipEvent_t>& ev = events.v;
  for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
  const MlpParams p = mlp_params(c, c->mlp_n, c->mlp_tile);
  int rc = CCKA_OK;
  // the context's own pair spans the batch (ccka_sync / ccka_last_kernel_ms)
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_mid, c->stream));
  for (int k = 0; k < launches && rc == CCKA_OK; ++k) {
    if (hipEventRecord(ev[2 * k], c->stream) != hipSuccess || launch_mlp(p, c->cus, c->stream) != hipSuccess ||
        hipEventRecord(ev[2 * k + 1], c->stream) != hipSuccess)
      rc = fail(c, CCKA_EHIP, "MLP batch launch %d", k);
  }
  double sum = 0.0;
  float span = 0.f;
  if (rc == CCKA_OK && hipEventRecord(c->ev1, c->stream) != hipSuccess) rc = fail(c, CCKA_EHIP, "event record");
  if (rc == CCKA_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, CCKA_EHIP, "MLP batch sync");
  for (int k = 0; k < launches && rc == CCKA_OK; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) != hipSuccess) rc = fail(c, CCKA_EHIP, "event time");
    sum += ms;
  }
  if (rc == CCKA_OK && hipEventElapsedTime(&span, ev[0], ev[2 * launches - 1]) != hipSuccess)
    rc = fail(c, CCKA_EHIP, "event time");
  if (rc != CCKA_OK) return rc;
  *avg_ms = sum / launches;
  *span_ms = span;
  c->ran = true;
  return CCKA_OK;
}

int ccka_mlp_forward(ccka_ctx* c) {
  int rc = ccka_mlp_forward_async(c);
  if (rc != CCKA_OK) return rc;
  return ccka_sync(c);
}

int ccka_mlp_get_actions(ccka_ctx* c, float* y, int64_t n) {
  if (!c || !y) return CCKA_EINVAL;
  if (n != c->mlp_n) return fail(c, CCKA_EINVAL, "action count mismatch");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(y, c->d_my, (size_t)n * MLP_OUT * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CCKA_OK;
}

}  // extern "C"
