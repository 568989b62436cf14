// host_rules.h — pure host arithmetic of libccka.so's C ABI that needs no
// device: which trace generators ccka_gen_load accepts, and the block of steps
// ccka_get_trajectory stages at a time. No HIP here, so the stand-alone host
// test (devbuf_test.cpp) covers it too.
#pragma once
#include <cstdint>

#include "../../include/ccka.h"

namespace ccka {

// nullptr when every intermediate of SEMANTICS.md §4 stays inside the
// arithmetic that evaluates it for every scenario, step and draw; else the
// rule that fails. Worst case of each signed 64-bit product, from the largest
// magnitudes of its factors (|SIN| <= 65536, |e| <= 131072):
//   B = max |base|, A = max |amp|
//   P1 = B * (65536000 + 65536 A)              V1 = P1 div 65536000
//   P2 = V1 * (37837000 + 131072 |noise_pm|)   V2 = P2 div 37837000
//   P3 = V2 * |burst_mult_pm|
// all three <= INT64_MAX. The two ranges' widths + 1 are moduli formed in
// int32 (<= INT32_MAX), and bstart + burst_len is an int32 sum with
// bstart <= 1439.
inline const char* trace_gen_invalid(const ccka_trace_gen& g) {
  typedef __int128 i128;
  const int64_t wb = (int64_t)g.base_hi - g.base_lo, wa = (int64_t)g.amp_hi_pm - g.amp_lo_pm;
  if (wb < 0 || wa < 0) return "a range has hi < lo";
  if (wb + 1 > INT32_MAX || wa + 1 > INT32_MAX) return "a range's width + 1 exceeds int32";
  if (g.burst_len < 0) return "burst_len < 0";
  if (g.burst_len > INT32_MAX - 1439) return "bstart + burst_len can exceed int32";
  auto mag = [](int32_t lo, int32_t hi) {
    const i128 a = lo < 0 ? -(i128)lo : (i128)lo, b = hi < 0 ? -(i128)hi : (i128)hi;
    return a > b ? a : b;
  };
  const i128 lim = INT64_MAX;
  const i128 B = mag(g.base_lo, g.base_hi), A = mag(g.amp_lo_pm, g.amp_hi_pm);
  const i128 P1 = B * (65536000 + 65536 * A);
  if (P1 > lim) return "base * (65536000 + amp * SIN) can leave int64";
  const i128 V1 = P1 / 65536000;
  const i128 P2 = V1 * (37837000 + 131072 * mag(g.noise_pm, g.noise_pm));
  if (P2 > lim) return "v * (37837000 + noise * e) can leave int64";
  const i128 V2 = P2 / 37837000;
  if (V2 * mag(g.burst_mult_pm, g.burst_mult_pm) > lim) return "v * burst_mult can leave int64";
  return nullptr;
}

// staging records of ccka_get_trajectory's [N][T] -> [T][N] transpose (64 MiB)
constexpr int64_t kTrajStageRecs = int64_t(4) << 20;

// Records the staging buffer of a read-back of `count` = N * T records must
// hold under the capacity `stage` (0: kTrajStageRecs): at least one step of N
// records, never more than the trajectory. The read-back moves
// traj_stage_cap / N steps at a time.
inline int64_t traj_stage_cap(int64_t N, int64_t count, int64_t stage) {
  const int64_t lim = stage > 0 ? stage : kTrajStageRecs;
  const int64_t cap = count < lim ? count : lim;
  return cap > N ? cap : N;
}

// element counts of the two trace copies (util.hip: trace_tile_kernel, trace_nt_kernel)
inline int64_t trace_tile_count(int64_t N, int64_t T, int64_t lpw) { return T * ((N + lpw - 1) / lpw * lpw); }
inline int64_t trace_nt_count(int64_t NL, int64_t T, int64_t DP) { return NL * T * DP; }

}  // namespace ccka
