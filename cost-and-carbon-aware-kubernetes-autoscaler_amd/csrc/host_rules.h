// host_rules.h — pure host arithmetic of libccka.so's C ABI that needs no
// device: which trace generators ccka_gen_load accepts, the timing fields
// ccka_set_world accepts, and the block of steps ccka_get_trajectory stages at
// a time. No HIP here, so the stand-alone host test (devbuf_test.cpp) covers
// it too.
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

// Largest start_minute and provision_delay_steps of a world (n_steps <= 65535).
//   start_minute: every engine forms start_minute + t in int32 before the
//     % 1440, for steps t <= n_steps (rollout_kernel.h `(gw->start_minute + t)
//     % 1440`, the policy features' lookahead `gw->start_minute + tq`, the
//     oracle's `w->start_minute + t1`), so start_minute + 65535 <= INT32_MAX.
//   provision_delay_steps: a node launched at step t <= n_steps - 1 <= 65534
//     is ready at the int32 step t + delay (`nready[n] = t + delay`,
//     `sready[n] = rs`, the oracle's `nd->ready_step`), and `next_ready` keeps
//     the least of them with 0x7fffffff for "none pending": t + delay <=
//     0x7ffffffe, so delay <= 0x7ffffffe - 65534. No kernel packs a ready step
//     into fewer than 32 bits.
// Both bounds are INT32_MAX - 65535.
constexpr int32_t kMaxStartMinute = INT32_MAX - 65535;
constexpr int32_t kMaxProvisionDelay = 0x7ffffffe - 65534;

// nullptr when the timing fields of a world stay inside the arithmetic above
// and the peak window is one of the day's: peak_start_min and peak_end_min in
// [0, 1440] (1440: "to the end of the day" under `minute >= ps && minute <
// pe`; the single-deployment kernel's next-edge distance `(ps % 1440 - minute
// + 1439) % 1440 + 1` is positive only for ps % 1440 >= 0). Else the rule
// that fails.
inline const char* world_timing_invalid(const ccka_world& w) {
  if (w.n_steps < 1 || w.n_steps > 65535) return "n_steps out of range";
  if (w.start_minute < 0 || w.provision_delay_steps < 0) return "negative timing";
  if (w.start_minute > kMaxStartMinute) return "start_minute + n_steps can leave int32";
  if (w.provision_delay_steps > kMaxProvisionDelay) return "a ready step t + provision_delay_steps can reach 0x7fffffff";
  if (w.peak_start_min < 0 || w.peak_start_min > 1440) return "peak_start_min outside [0, 1440]";
  if (w.peak_end_min < 0 || w.peak_end_min > 1440) return "peak_end_min outside [0, 1440]";
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

// A read-back of `want` elements from a buffer that holds `have`: the last
// check of every getter whose buffer only grows (the closed loop's records,
// the samples), after the validity flag and the caller's count. The flags end
// with the world and the scenario set, so this never fails today; it is what
// keeps a copy inside its allocation if a flag is ever left standing.
inline bool copy_fits(int64_t want, int64_t have) { return want >= 0 && want <= have; }

// element counts of the two trace copies (util.hip: trace_tile_kernel, trace_nt_kernel)
inline int64_t trace_tile_count(int64_t N, int64_t T, int64_t lpw) { return T * ((N + lpw - 1) / lpw * lpw); }
inline int64_t trace_nt_count(int64_t NL, int64_t T, int64_t DP) { return NL * T * DP; }

}  // namespace ccka
