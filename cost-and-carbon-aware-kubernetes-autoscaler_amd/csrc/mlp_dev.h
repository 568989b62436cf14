// mlp_dev.h — device helpers of the learned policy shared by mlp.hip, pg.hip
// and the fused closed loop (rollout_kernel.h): the MFMA operand types, the
// 32x32x16 wrapper, the bias tile, the ReLU/bf16 epilogue, and the policy's
// action rules (SEMANTICS 5), one definition each. Internal linkage: a
// translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "kparams.h"

namespace ccka {
namespace {

typedef mlp_bf16x8 bf16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short short2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// registers 8s..8s+7 as one bf16 operand fragment with ReLU: pairs rounded to
// nearest even (v_cvt_pk_bf16_f32), then ReLU on the bf16 bit patterns as
// packed int16 max with 0 (v_pk_max_i16: every negative value, -0 included,
// has the sign bit set) -- the same bits as rounding relu(x)
// (mlp_kernel and the fused loop's mlp_tile; pg_rows_kernel compiles differently with this text: relu_pack_dw)
__device__ __forceinline__ bf16x8 relu_pack(const f32x16& a, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const bf16x2v b = __builtin_convertvector((f32x2){a[8 * s + j], a[8 * s + j + 1]}, bf16x2v);
    const short2v v = __builtin_elementwise_max(__builtin_bit_cast(short2v, b), (short2v){0, 0});
    r[j] = v.x;
    r[j + 1] = v.y;
  }
  return r;
}
// the same bits built as four dwords (pg_rows_kernel; mlp_kernel compiles differently with this text)
__device__ __forceinline__ bf16x8 relu_pack_dw(const f32x16& a, int s) {
  u32x4_ o;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const bf16x2v b = __builtin_convertvector((f32x2){a[8 * s + 2 * w], a[8 * s + 2 * w + 1]}, bf16x2v);
    const short2v v = __builtin_elementwise_max(__builtin_bit_cast(short2v, b), (short2v){0, 0});
    o[w] = __builtin_bit_cast(uint32_t, v);
  }
  return __builtin_bit_cast(bf16x8, o);
}

// accumulator tile of the bias of rows 32 blocks: row = (reg&3) + 8(reg>>2) + 4h
// (four 16-byte loads, L1/L2-resident; used as the C operand of the first MFMA)
__device__ __forceinline__ f32x16 bias_tile(const float* b, int h) {
  f32x16 a;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(b + 8 * g + 4 * h);
    a[4 * g + 0] = v[0];
    a[4 * g + 1] = v[1];
    a[4 * g + 2] = v[2];
    a[4 * g + 3] = v[3];
  }
  return a;
}

// The policy's action -> this step's scaler parameters (SEMANTICS 5): the
// HPA target utilisation 60 + rint(16 y0) clamped to [20, 95] %, and the
// Karpenter carbon weight rint(16 y1) / 16 clamped to [0, 4] $/kgCO2. Scaling by
// 16 is exact in fp32 and rint rounds half to even, so the mapping is
// reproducible from y on any IEEE host.
__device__ __forceinline__ void policy_action(float y0, float y1, int& target, double& cw) {
  const float q0 = rintf(y0 * 16.0f), q1 = rintf(y1 * 16.0f);
  target = 60 + (int)fminf(fmaxf(q0, -40.0f), 35.0f);
  cw = (double)(int)fminf(fmaxf(q1, 0.0f), 64.0f) / 16.0;
}

// Stochastic policy step (SEMANTICS 5): p = softmax(y) in binary32 (max
// subtracted, expf); u = Philox(seed; global id g, step t) as a 24-bit uniform
// in [0, 1); the action is the first a with u * sum(p) < p_0 + ... + p_a (the
// last one if rounding leaves none). *seed is read here, at run time, so a
// captured loop replays with any seed.
__device__ __forceinline__ int policy_sample(const float* y, const uint64_t* seed_p, int64_t g, int t) {
  float p[MLP_OUT];
  float mx = y[0];
#pragma unroll
  for (int a = 1; a < MLP_OUT; ++a) mx = fmaxf(mx, y[a]);
  float sum = 0.f;
#pragma unroll
  for (int a = 0; a < MLP_OUT; ++a) {
    p[a] = expf(y[a] - mx);
    sum += p[a];
  }
  const uint64_t seed = *seed_p;
  uint32_t u4[4];
  philox((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)t, 0x5A3B1E7u, (uint32_t)seed, (uint32_t)(seed >> 32), u4);
  const float u = (float)(u4[0] >> 8) * (1.0f / 16777216.0f) * sum;
  int act = MLP_OUT - 1;  // the last action when rounding leaves u above every partial sum
  float acc = 0.f;
  bool found = false;
#pragma unroll
  for (int a = 0; a < MLP_OUT; ++a) {
    acc += p[a];
    if (!found && u < acc) { act = a; found = true; }
  }
  return act;
}
// action bin a -> the HPA target 40 + 10 (a & 3) % and the carbon weight (a >> 2) $/kgCO2
__device__ __forceinline__ void policy_bin_action(int a, int& target, double& cw) {
  target = 40 + 10 * (a & 3);
  cw = (double)(a >> 2);
}

}  // namespace
}  // namespace ccka
