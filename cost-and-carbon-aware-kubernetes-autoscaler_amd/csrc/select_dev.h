// select_dev.h — the wave-level MSB-first radix select over order-preserving
// 64-bit keys (SEMANTICS 6), shared by grid_select_kernel (sweep.hip) and
// paired_kernel (paired.hip): the key transforms, the pass loop (histogram
// with the kSelPeel step, 64-lane scan, digit pick) and the integer tail.
// Internal linkage, as dev_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ccka {
namespace {

constexpr int kSelLds = 1024;  // keys per objective a workgroup stages in LDS
constexpr int kSelPeel = 2;    // shared digits counted by one add each, per 64 keys
constexpr uint64_t kSignBit = 0x8000000000000000ull;

__device__ __forceinline__ uint64_t key_i64(int64_t v) { return (uint64_t)v ^ kSignBit; }
__device__ __forceinline__ int64_t unkey_i64(uint64_t k) { return (int64_t)(k ^ kSignBit); }

// LDS written by some lanes of this wave, read by others: LDS serves one
// wave's accesses in order, so only the compiler must not move them
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The key of rank `rank` (1-based, <= n) among key_at(0 .. n), found by one
// whole wave: 8 passes of 8 bits; each histograms the digit of the keys that
// match the prefix found so far into hist[256] (LDS counters private to the
// wave) and a 64-lane scan picks the digit that holds the rank. key_at(i) is
// called for i < n only, by every lane in wave-uniform trips.
template <class KeyAt>
__device__ __forceinline__ uint64_t wave_radix_select(int64_t n, uint64_t rank, uint32_t* hist, int lane,
                                                      KeyAt key_at) {
  // keys matching (prefix, mask) are the candidates; rank is 1-based among them
  uint64_t prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    // lane l owns counters 4l .. 4l+3: it clears the four it read last pass
    *(uint4*)&hist[4 * lane] = make_uint4(0, 0, 0, 0);
    wave_lds_sync();
    for (int64_t base = 0; base < n; base += 64) {  // wave-uniform trips: ballots inside
      const int64_t i = base + lane;
      uint64_t key = 0;
      if (i < n) key = key_at(i);
      const uint32_t digit = (uint32_t)(key >> shift) & 255;
      bool pending = i < n && (key & mask) == prefix;
      // Real columns share their high digits and tie heavily (SLO minutes are
      // mostly 0): 64 lanes adding to one counter serialise in the LDS. kSelPeel
      // times, the lanes that share the first pending lane's digit are counted
      // by one add of their number (register traffic only); what is left adds
      // lane by lane.
#pragma unroll
      for (int t = 0; t < kSelPeel; ++t) {
        if (pending) {
          const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)digit);
          const bool same = digit == d0;
          const uint64_t sm = __ballot(same);  // of the pending lanes
          if (lane == __ffsll((long long)sm) - 1) atomicAdd(&hist[d0], (uint32_t)__popcll(sm));
          pending = !same;
        }
      }
      if (pending) atomicAdd(&hist[digit], 1u);
    }
    wave_lds_sync();
    const uint4 c = *(const uint4*)&hist[4 * lane];
    const uint32_t own_sum = c.x + c.y + c.z + c.w;
    uint32_t incl = own_sum;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const uint32_t excl = incl - own_sum;
    // exactly one lane's counters hold the rank (the candidates number >= rank)
    const bool own = excl < rank && rank <= incl;
    uint32_t digit = 0, below = 0;
    if (own) {
      const uint32_t r = (uint32_t)rank - excl;  // 1 .. own_sum
      if (r <= c.x) { digit = 0; below = 0; }
      else if (r <= c.x + c.y) { digit = 1; below = c.x; }
      else if (r <= c.x + c.y + c.z) { digit = 2; below = c.x + c.y; }
      else { digit = 3; below = c.x + c.y + c.z; }
      digit += 4 * lane;
      below += excl;
    }
    const int owner = (__ffsll((long long)__ballot(own)) - 1) & 63;
    digit = __shfl(digit, owner);
    below = __shfl(below, owner);
    rank -= below;
    prefix |= (uint64_t)digit << shift;
    mask |= 0xffull << shift;
  }
  return prefix;  // the key of x(k)
}

// TAIL of int64 values behind key_i64 keys (SEMANTICS 6): the values above
// x(k) = unkey_i64(kx) in lane-strided order, a shuffle tree, and the ties with
// x(k) as one product; `terms` = n - k + 1. Wraps like int64; lane 0 holds it.
template <class KeyAt>
__device__ __forceinline__ int64_t wave_tail_i64(int64_t n, int64_t terms, uint64_t kx, int lane, KeyAt key_at) {
  uint64_t acc = 0;
  uint32_t gt = 0;
  for (int64_t i = lane; i < n; i += 64) {
    const uint64_t key = key_at(i);
    if (key > kx) { acc += (uint64_t)unkey_i64(key); ++gt; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    acc += __shfl_down(acc, d);
    gt += __shfl_down(gt, d);
  }
  return (int64_t)(acc + (uint64_t)(terms - (int64_t)gt) * (uint64_t)unkey_i64(kx));
}

}  // namespace
}  // namespace ccka
