// mlp.hip — BASELINE config 5: the learned MLP control policy
// (state 64 -> 256 -> 256 -> 8, ReLU) batched over millions of cluster states
// with bf16 MFMA on gfx950 (v_mfma_f32_32x32x16_bf16, fp32 accumulation).
//
// Orientation: every layer computes the TRANSPOSED activation tile
// (hidden units on rows, 32 cluster states on columns = lanes):
//   H1^T = W1^T X^T,  H2^T = W2^T H1^T,  Y^T = W3^T H2^T.
// A 32x32 accumulator of one layer then IS the B operand of the next
// (column on the lane, rows in registers): registers 8s..8s+7, converted to
// bf16, are k-step s of the next product with the permuted k order
// k = 16s + 8(j>>2) + 4h + (j&3) (j = element, h = lane half). The host lays
// the weight fragments out in exactly that order (abi_mlp.cpp,
// ccka_mlp_set_weights), so no activation ever moves between lanes or through LDS.
//
// Residency and schedule (one persistent 4-wave workgroup per CU, one wave
// per SIMD): W1 fragments (32 KiB) in each wave's accumulation registers, W2
// and W3 fragments and the biases (146 KiB) in LDS; MFMA accumulators in
// architectural VGPRs (built with -amdgpu-mfma-vgpr-form) so the packed
// ReLU/bf16 epilogue reads them directly. Each wave evaluates two 32-state
// tiles per pass (every LDS fragment feeds two MFMAs); layer-1 row blocks and
// layer-2 row blocks are software-pipelined so each block's epilogue runs in
// the shadow of the next block's MFMAs. Measured (tools/mlp_stamps.py): 77 %
// of the MFMA-issue floor in cycles; under this kernel's power draw the shader
// clock settles near 1.8 GHz (tools/probe/clockprobe: 2.24 GHz for a
// low-toggle MFMA stream).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"
#include "mlp_dev.h"

namespace ccka {

// One persistent 4-wave workgroup per CU. W1 fragments (32 KiB) live in each
// wave's accumulation registers; W2 and W3 fragments and the biases
// (146 KiB) in LDS. Each wave evaluates TWO 32-state tiles per pass, so every
// W2 / W3 fragment and bias tile read from LDS feeds two MFMAs and the two
// tiles' dependency chains interleave.
// STAMPS: diagnostic build only: s_memtime cycle totals of layer 1 and of
// layers 2+3 summed over waves into p.stamps[0..1]
template <bool STAMPS>
__global__ void __launch_bounds__(256, 1) mlp_kernel(MlpParams p) {
  unsigned long long st[2] = {0, 0}, st_last = 0;
  const unsigned long long k0 = STAMPS ? __builtin_amdgcn_s_memtime() : 0, r0 = STAMPS ? __builtin_amdgcn_s_memrealtime() : 0;
  constexpr int KS1 = MLP_IN / 16, KS2 = MLP_HID / 16, NB = MLP_HID / 32;
  __shared__ __attribute__((aligned(16))) float s_b[2 * MLP_HID + 32];  // b1 | b2 | b3 (zero-padded)
  __shared__ bf16x8 s_w3[KS2 * WAVE];                                   // 16 KiB
  __shared__ bf16x8 s_w2[NB * KS2 * WAVE];                              // 128 KiB
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int r = lane & 31, h = lane >> 5;
  for (int x = tid; x < NB * KS2 * WAVE; x += blockDim.x) s_w2[x] = p.w2f[x];
  for (int x = tid; x < KS2 * WAVE; x += blockDim.x) s_w3[x] = p.w3f[x];
  for (int x = tid; x < 2 * MLP_HID + 32; x += blockDim.x) s_b[x] = p.b1[x];  // b1, b2, b3 are contiguous
  bf16x8 w1[NB][KS1];
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      w1[n][s] = p.w1f[(n * KS1 + s) * WAVE + lane];
      asm volatile("" : "+a"(w1[n][s]));  // accumulation registers: MFMA reads its A operand from them
    }
  __syncthreads();
  const float* const s_b1 = s_b;
  const float* const s_b2 = s_b + MLP_HID;
  const float* const s_b3 = s_b + 2 * MLP_HID;

  const int64_t ntiles = (p.N + 31) / 32, npairs = (ntiles + 1) / 2;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x / WAVE);
  int64_t pair = (int64_t)blockIdx.x * (blockDim.x / WAVE) + wave;
  // X^T fragments (B operand of layer 1): state r of the tile, features 16s + 8h .. +7
  auto load_x = [&](int64_t tl, bf16x8* xf) {
    const int64_t row = tl * 32 + r;
    const bool ok = tl < ntiles && row < p.N;
    const bf16x8* src = reinterpret_cast<const bf16x8*>(p.x + (ok ? row : 0) * MLP_IN + 8 * h);
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      const bf16x8 v = src[2 * s];
      xf[s] = ok ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  bf16x8 xa[KS1], xb[KS1];
  load_x(2 * pair, xa);
  load_x(2 * pair + 1, xb);
  for (; pair < npairs; pair += nw) {
    // scheduling fences at the phase boundaries (measured: the scheduler's
    // cross-phase interleaving is slower than the hand-placed order)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STAMPS) {
      st_last = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- layer 1: H1^T = relu(W1^T X^T + b1), both tiles ----
    // row blocks software-pipelined: block n+1's MFMAs are issued before
    // block n's ReLU/bf16 epilogue, which then runs in their shadow
    bf16x8 ha[KS2], hb[KS2];
    f32x16 ca, cb;
    {
      const f32x16 bias = bias_tile(s_b1, h);
      ca = mfma(w1[0][0], xa[0], bias);
      cb = mfma(w1[0][0], xb[0], bias);
#pragma unroll
      for (int s = 1; s < KS1; ++s) {
        ca = mfma(w1[0][s], xa[s], ca);
        cb = mfma(w1[0][s], xb[s], cb);
      }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      f32x16 na, nb;
      if (n + 1 < NB) {
        const f32x16 bias = bias_tile(s_b1 + 32 * (n + 1), h);
        na = mfma(w1[n + 1][0], xa[0], bias);
        nb = mfma(w1[n + 1][0], xb[0], bias);
#pragma unroll
        for (int s = 1; s < KS1; ++s) {
          na = mfma(w1[n + 1][s], xa[s], na);
          nb = mfma(w1[n + 1][s], xb[s], nb);
        }
      }
      ha[2 * n] = relu_pack(ca, 0);
      ha[2 * n + 1] = relu_pack(ca, 1);
      hb[2 * n] = relu_pack(cb, 0);
      hb[2 * n + 1] = relu_pack(cb, 1);
      if (n + 1 < NB) { ca = na; cb = nb; }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STAMPS) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
      st[0] += now - st_last;
      st_last = now;
    }
    // next pair's states in flight during layers 2 and 3
    load_x(2 * (pair + nw), xa);
    load_x(2 * (pair + nw) + 1, xb);
    // ---- layers 2 and 3: one 32-row block of H2 at a time, software-
    // pipelined: while block m+1's 16 k-steps run (2 MFMAs each, one W2
    // fragment read two k-steps ahead), block m's ReLU/bf16 epilogue and its
    // two layer-3 k-steps are spread over those k-steps ----
    f32x16 ya = bias_tile(s_b3, h), yb = ya;
    auto w2 = [&](int m, int kk) { return s_w2[(m * KS2 + kk) * WAVE + lane]; };
    {
      bf16x8 w0 = w2(0, 0), w1f = w2(0, 1);
      const f32x16 bias = bias_tile(s_b2, h);
#pragma unroll
      for (int kk = 0; kk < KS2; ++kk) {
        const bf16x8 wn = kk + 2 < KS2 ? w2(0, kk + 2) : w2(1, kk + 2 - KS2);
        asm volatile("" ::: "memory");
        ca = kk == 0 ? mfma(w0, ha[0], bias) : mfma(w0, ha[kk], ca);
        cb = kk == 0 ? mfma(w0, hb[0], bias) : mfma(w0, hb[kk], cb);
        w0 = w1f;
        w1f = wn;
      }
#pragma unroll
      for (int m = 0; m < NB; ++m) {
        f32x16 na, nb;
        bf16x8 ga0, ga1, gb0, gb1, w30, w31;
        if (m + 1 < NB) {
          const f32x16 bn = bias_tile(s_b2 + 32 * (m + 1), h);
#pragma unroll
          for (int kk = 0; kk < KS2; ++kk) {
            const int q = (m + 1) * KS2 + kk + 2;  // fragment two k-steps ahead (wraps into the next block)
            const bf16x8 wn = q < NB * KS2 ? s_w2[q * WAVE + lane] : w0;
            asm volatile("" ::: "memory");
            na = kk == 0 ? mfma(w0, ha[0], bn) : mfma(w0, ha[kk], na);
            nb = kk == 0 ? mfma(w0, hb[0], bn) : mfma(w0, hb[kk], nb);
            w0 = w1f;
            w1f = wn;
            if (kk == 1) ga0 = relu_pack(ca, 0);
            if (kk == 3) ga1 = relu_pack(ca, 1);
            if (kk == 5) gb0 = relu_pack(cb, 0);
            if (kk == 7) gb1 = relu_pack(cb, 1);
            if (kk == 7) { w30 = s_w3[(2 * m) * WAVE + lane]; w31 = s_w3[(2 * m + 1) * WAVE + lane]; }
            if (kk == 9) ya = mfma(w30, ga0, ya);
            if (kk == 11) yb = mfma(w30, gb0, yb);
            if (kk == 13) ya = mfma(w31, ga1, ya);
            if (kk == 15) yb = mfma(w31, gb1, yb);
          }
          ca = na;
          cb = nb;
        } else {
          w30 = s_w3[(2 * m) * WAVE + lane];
          w31 = s_w3[(2 * m + 1) * WAVE + lane];
          ya = mfma(w30, relu_pack(ca, 0), ya);
          yb = mfma(w30, relu_pack(cb, 0), yb);
          ya = mfma(w31, relu_pack(ca, 1), ya);
          yb = mfma(w31, relu_pack(cb, 1), yb);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STAMPS) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
      st[1] += now - st_last;
    }
    // registers 0..3 hold outputs 4h..4h+3 of state r
    const int64_t ra = (2 * pair) * 32 + r, rb = ra + 32;
    if (ra < p.N) *reinterpret_cast<f32x4*>(p.y + ra * MLP_OUT + 4 * h) = f32x4{ya[0], ya[1], ya[2], ya[3]};
    if (rb < p.N) *reinterpret_cast<f32x4*>(p.y + rb * MLP_OUT + 4 * h) = f32x4{yb[0], yb[1], yb[2], yb[3]};
  }
  if constexpr (STAMPS) {
    if (lane == 0) {
      atomicAdd(&p.stamps[0], st[0]);
      atomicAdd(&p.stamps[1], st[1]);
      // whole-wave shader cycles and 100 MHz real-time ticks: the clock the kernel ran at
      atomicAdd(&p.stamps[2], __builtin_amdgcn_s_memtime() - k0);
      atomicAdd(&p.stamps[3], __builtin_amdgcn_s_memrealtime() - r0);
    }
  }
}

// ---------------------------------------------------------------------------
// The same MLP on v_mfma_f32_16x16x32_bf16 (16-cycle issue; MI355X_MICROARCH.md
// measures its loops at 1.12-1.15x the FLOP/s of 32x32x16 on random data, and
// the 8-row output layer pads to 16 rows instead of 32). Transposed chaining as
// in mlp_kernel, with the 16x16 layouts: the accumulator of output tile o
// (16 units x 16 states) holds, in lane l, state l & 15 and units
// 16o + 4(l >> 4) + 0..3; the B operand of a k-step holds state l & 15 and
// k-slots 8(l >> 4) + e. Two consecutive accumulator tiles (2s, 2s+1), packed
// to bf16, are k-step s of the next layer with the permuted k order
// u = 32s + 16(e >> 2) + 4(l >> 4) + (e & 3) (mlp16 fragments on the host).
// One persistent 4-wave workgroup per CU; W1 fragments in accumulation
// registers, W2 / W3 fragments and the biases in LDS (138 KiB); each wave
// evaluates T16 16-state tiles per pass (every W2 fragment read feeds T16
// MFMAs), the next pass's states in flight during layers 2 and 3.
// ---------------------------------------------------------------------------
typedef float f32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4v mfma16(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// tiles (2s, 2s+1) -> one bf16 B fragment with ReLU (as relu_pack)
__device__ __forceinline__ bf16x8 relu_pack2(const f32x4v& a, const f32x4v& b) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    const bf16x2v x = __builtin_convertvector((f32x2){a[j], a[j + 1]}, bf16x2v);
    const short2v v = __builtin_elementwise_max(__builtin_bit_cast(short2v, x), (short2v){0, 0});
    r[j] = v.x;
    r[j + 1] = v.y;
    const bf16x2v y = __builtin_convertvector((f32x2){b[j], b[j + 1]}, bf16x2v);
    const short2v w = __builtin_elementwise_max(__builtin_bit_cast(short2v, y), (short2v){0, 0});
    r[4 + j] = w.x;
    r[4 + j + 1] = w.y;
  }
  return r;
}
#ifndef MLP16_T
#define MLP16_T 4
#endif
constexpr int T16 = MLP16_T;  // 16-state tiles per wave and pass
__global__ void __launch_bounds__(256, 1) mlp16_kernel(MlpParams p) {
  constexpr int NO = MLP_HID / 16;                      // output tiles of layers 1 and 2
  constexpr int KS1 = MLP_IN / 32, KS2 = MLP_HID / 32;  // k-steps
  constexpr int PF = 2;                                 // W2 fragments in flight
  // the output layer's k-step for tile t runs inside the W2 chain at s = t + 1
  // (s < KS2): more tiles per pass would drop layer-3 terms
  static_assert(T16 < KS2, "MLP16_T must stay below MLP_HID / 32");
  __shared__ __attribute__((aligned(16))) float s_b[2 * MLP_HID + 16];  // b1 | b2 | b3 (zero-padded to 16)
  __shared__ bf16x8 s_w3[KS2 * WAVE];                                   // 8 KiB
  __shared__ bf16x8 s_w2[NO * KS2 * WAVE];                              // 128 KiB
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int j = lane & 15, g = lane >> 4;
  for (int x = tid; x < NO * KS2 * WAVE; x += blockDim.x) s_w2[x] = p.w2g[x];
  for (int x = tid; x < KS2 * WAVE; x += blockDim.x) s_w3[x] = p.w3g[x];
  for (int x = tid; x < 2 * MLP_HID + 16; x += blockDim.x) s_b[x] = x < 2 * MLP_HID + MLP_OUT ? p.b1[x] : 0.f;
  bf16x8 w1[NO][KS1];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      w1[o][s] = p.w1g[(o * KS1 + s) * WAVE + lane];
      asm volatile("" : "+a"(w1[o][s]));  // accumulation registers: MFMA reads its A operand from them
    }
  __syncthreads();
  auto bias4 = [&](int off) { return *reinterpret_cast<const f32x4v*>(s_b + off + 4 * g); };
  const int64_t ntiles = (p.N + 15) / 16, npass = (ntiles + T16 - 1) / T16;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x / WAVE);
  int64_t pass = (int64_t)blockIdx.x * (blockDim.x / WAVE) + wave;
  // X^T fragments (B operand of layer 1): state j of the tile, features 32s + 8g .. +7
  auto load_x = [&](int64_t tl, bf16x8* xf) {
    const int64_t row = tl * 16 + j;
    const bool ok = row < p.N;
    const bf16x8* src = reinterpret_cast<const bf16x8*>(p.x + (ok ? row : 0) * MLP_IN + 8 * g);
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      const bf16x8 v = src[4 * s];
      xf[s] = ok ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  bf16x8 x[T16][KS1];
#pragma unroll
  for (int t = 0; t < T16; ++t) load_x(pass * T16 + t, x[t]);
  for (; pass < npass; pass += nw) {
    __builtin_amdgcn_sched_barrier(0);
    // ---- layer 1: H1^T = relu(W1^T X^T + b1). The tile pair (2m, 2m+1) is
    // packed to bf16 during tile 2m+2's MFMAs (its epilogue in their shadow) ----
    bf16x8 h1[T16][KS2];
    {
      f32x4v pa[T16], pb[T16], c[T16];
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const f32x4v b = bias4(16 * o);
#pragma unroll
        for (int s = 0; s < KS1; ++s) {
#pragma unroll
          for (int t = 0; t < T16; ++t) c[t] = mfma16(w1[o][s], x[t][s], s == 0 ? b : c[t]);
          if (o >= 2 && !(o & 1)) {  // the pending pair (o - 2, o - 1), half of its tiles per k-step
#pragma unroll
            for (int t = s * T16 / KS1; t < (s + 1) * T16 / KS1; ++t) h1[t][(o >> 1) - 1] = relu_pack2(pa[t], pb[t]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < T16; ++t) {
          if (o & 1) pb[t] = c[t];
          else pa[t] = c[t];
        }
      }
#pragma unroll
      for (int t = 0; t < T16; ++t) h1[t][KS2 - 1] = relu_pack2(pa[t], pb[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the next pass's states in flight during layers 2 and 3
#pragma unroll
    for (int t = 0; t < T16; ++t) load_x((pass + nw) * T16 + t, x[t]);
    // ---- layers 2 and 3: H2^T = relu(W2^T H1^T + b2) tile by tile, W2
    // fragments PF k-steps ahead; the pair (2m, 2m+1) is packed and multiplied
    // into Y^T = W3^T H2^T + b3 (k-step m) during tile 2m+2's MFMAs ----
    f32x4v y[T16];
    {
      const f32x4v b3 = bias4(2 * MLP_HID);
#pragma unroll
      for (int t = 0; t < T16; ++t) y[t] = b3;
    }
    {
      f32x4v pa[T16], pb[T16], c[T16];
      bf16x8 wq[PF + 1];
#pragma unroll
      for (int q = 0; q < PF; ++q) wq[q] = s_w2[q * WAVE + lane];
      bf16x8 w3 = s_w3[lane];
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const f32x4v b = bias4(MLP_HID + 16 * o);
        if (o >= 2 && !(o & 1)) w3 = s_w3[((o >> 1) - 1) * WAVE + lane];
#pragma unroll
        for (int s = 0; s < KS2; ++s) {
          const int q = o * KS2 + s;
          if (q + PF < NO * KS2) wq[(q + PF) % (PF + 1)] = s_w2[(q + PF) * WAVE + lane];
          const bf16x8 w = wq[q % (PF + 1)];
#pragma unroll
          for (int t = 0; t < T16; ++t) c[t] = mfma16(w, h1[t][s], s == 0 ? b : c[t]);
          if (o >= 2 && !(o & 1) && s >= 1 && s <= T16) {
            const int t = s - 1;
            y[t] = mfma16(w3, relu_pack2(pa[t], pb[t]), y[t]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < T16; ++t) {
          if (o & 1) pb[t] = c[t];
          else pa[t] = c[t];
        }
      }
      w3 = s_w3[(KS2 - 1) * WAVE + lane];
#pragma unroll
      for (int t = 0; t < T16; ++t) y[t] = mfma16(w3, relu_pack2(pa[t], pb[t]), y[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // rows 4g..4g+3 of Y^T = actions 4g..4g+3 of state j (g < 2)
#pragma unroll
    for (int t = 0; t < T16; ++t) {
      const int64_t row = (pass * T16 + t) * 16 + j;
      if (g < 2 && row < p.N) *reinterpret_cast<f32x4v*>(p.y + row * MLP_OUT + 4 * g) = y[t];
    }
  }
}

// Synthetic cluster states: Irwin-Hall sums of Philox words (~N(0,1)), bf16.
__global__ void __launch_bounds__(256) mlp_gen_states_kernel(uint16_t* x, int64_t count, uint64_t seed) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  uint32_t u[4];
  philox((uint32_t)e, (uint32_t)(e >> 32), 0x5EEDu, 0x57A7Eu, (uint32_t)seed, (uint32_t)(seed >> 32), u);
  const float v = ((float)(u[0] >> 16) + (float)(u[1] >> 16) + (float)(u[2] >> 16) + (float)(u[3] >> 16) - 131070.0f) *
                  (1.0f / 37837.0f);
  x[e] = __builtin_bit_cast(uint16_t, (__bf16)v);
}

hipError_t launch_mlp(const MlpParams& p, int cus, hipStream_t s) {
  if (p.stamps) hipLaunchKernelGGL(mlp_kernel<true>, dim3((unsigned)cus), dim3(256), 0, s, p);
  else if (p.w1g) hipLaunchKernelGGL(mlp16_kernel, dim3((unsigned)cus), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(mlp_kernel<false>, dim3((unsigned)cus), dim3(256), 0, s, p);
  return hipGetLastError();
}

// The policy's action -> this step's scaler parameters (policy_action, mlp_dev.h)
__global__ void __launch_bounds__(256) policy_act_kernel(const float* __restrict__ y, int16_t* target, double* cw,
                                                        int16_t* rec_target, double* rec_cw, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int t;
  double c;
  policy_action(y[i * 8 + 0], y[i * 8 + 1], t, c);
  const int16_t tg = (int16_t)t;
  target[i] = tg;
  cw[i] = c;
  if (rec_target) {
    rec_target[i] = tg;
    rec_cw[i] = c;
  }
}

hipError_t launch_policy_act(const float* y, int16_t* target, double* cw, int16_t* rec_target, double* rec_cw,
                             int64_t n, hipStream_t s) {
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(policy_act_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, target, cw, rec_target, rec_cw, n);
  return hipGetLastError();
}

hipError_t launch_mlp_gen_states(uint16_t* x, int64_t count, uint64_t seed, hipStream_t s) {
  hipLaunchKernelGGL(mlp_gen_states_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, x, count, seed);
  return hipGetLastError();
}

}  // namespace ccka
