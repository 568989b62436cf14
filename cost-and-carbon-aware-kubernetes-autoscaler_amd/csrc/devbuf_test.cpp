// devbuf_test.cpp — DevBuf (devbuf.h) over a malloc-backed allocator that counts
// its calls and can be told to fail the next k of them. Host only, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by `make devbuf-test`
// (tests/test_devbuf.py): a leak, a double free or a use after free aborts it.
// Also the pure host rules of host_rules.h (accepted trace generators, the
// timing rules of a world, the trajectory staging arithmetic), at the edge of
// every rule.
#define CCKA_DEVBUF_NO_HIP
#include "devbuf.h"
#include "host_rules.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

struct CountingAlloc {
  static inline long allocs = 0, frees = 0, calls = 0, fail_next = 0;
  static void* alloc(size_t bytes) {
    ++calls;
    if (fail_next > 0) {
      --fail_next;
      return nullptr;
    }
    ++allocs;
    return std::malloc(bytes);
  }
  static void free(void* p) {
    ++frees;
    std::free(p);
  }
};
using A = CountingAlloc;
template <class T>
using Buf = ccka::DevBuf<T, CountingAlloc>;

static_assert(!std::is_copy_constructible<Buf<int>>::value, "DevBuf must not be copyable");
static_assert(!std::is_copy_assignable<Buf<int>>::value, "DevBuf must not be copyable");
static_assert(std::is_nothrow_move_constructible<Buf<int>>::value, "DevBuf moves");
static_assert(std::is_nothrow_move_assignable<Buf<int>>::value, "DevBuf moves");

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

template <class T>
static bool empty(const Buf<T>& b) { return b.get() == nullptr && b.count() == 0; }

static void test_reserve() {
  Buf<int32_t> b;
  CHECK(empty(b));
  CHECK(b.reserve(0) && empty(b) && A::calls == 0);  // n == 0: empty, success, no allocation
  CHECK(b.reserve(100) && b.get() && b.count() == 100);
  int32_t* p = b.get();
  for (int i = 0; i < 100; ++i) p[i] = i;  // the whole extent is ours (ASan checks)
  CHECK(b.reserve(100) && b.get() == p && b.count() == 100);  // equal: kept
  CHECK(b.reserve(7) && b.get() == p && b.count() == 100);    // smaller: kept
  CHECK(b.reserve(0) && b.get() == p && b.count() == 100);
  const long a0 = A::allocs, f0 = A::frees;
  CHECK(b.reserve(101) && b.count() == 101);  // larger: a new allocation, the old one freed
  CHECK(A::allocs == a0 + 1 && A::frees == f0 + 1);
  b.get()[100] = 1;
  int32_t* q = b;  // implicit conversion
  CHECK(q == b.get());
}

static void test_resize() {
  Buf<double> b;
  CHECK(b.resize(0) && empty(b));
  CHECK(b.resize(64) && b.count() == 64);
  double* p = b.get();
  const long a0 = A::allocs, f0 = A::frees;
  CHECK(b.resize(64) && b.get() == p && A::allocs == a0);  // equal: kept
  CHECK(b.resize(63) && b.count() == 63 && A::allocs == a0 + 1 && A::frees == f0 + 1);  // smaller: reallocated
  b.get()[62] = 1.0;
  CHECK(b.resize(65) && b.count() == 65 && A::allocs == a0 + 2 && A::frees == f0 + 2);  // larger: reallocated
  b.get()[64] = 1.0;
  CHECK(b.resize(0) && empty(b) && A::frees == f0 + 3);  // n == 0: empty, success
}

static void test_overflow() {
  struct Wide { char c[4096]; };
  Buf<Wide> b;
  CHECK(b.reserve(4));
  const long c0 = A::calls;
  const int64_t big = INT64_MAX / 2;  // x 4096 bytes wraps size_t
  CHECK(!b.reserve(big) && empty(b) && A::calls == c0);
  CHECK(b.resize(4));
  CHECK(!b.resize(big) && empty(b) && A::calls == c0 + 1);
  CHECK(!b.resize(-1) && empty(b) && !b.reserve(-1) && A::calls == c0 + 1);
  Buf<char> bytes;  // one byte per element: no count overflows, the allocator decides
  A::fail_next = 1;
  CHECK(!bytes.reserve(INT64_MAX) && empty(bytes) && A::calls == c0 + 2);
}

static void test_failure_and_recovery() {
  Buf<int64_t> b;
  CHECK(b.reserve(10));
  A::fail_next = 1;
  CHECK(!b.reserve(20) && empty(b));  // the old allocation is gone too, never a stale count
  CHECK(b.reserve(5) && b.count() == 5);  // the next call recovers
  b.get()[4] = 1;
  A::fail_next = 1;
  CHECK(!b.resize(6) && empty(b));
  CHECK(b.resize(6) && b.count() == 6);
  b.get()[5] = 1;
  CHECK(A::fail_next == 0);
}

// buffers that are sized together, as the context's groups are
struct Group {
  Buf<int32_t> a;
  Buf<double> b;
  Buf<char> c;
  bool reserve(int64_t n) { return ccka::all_or_none(a.reserve(n) && b.reserve(2 * n) && c.reserve(n), a, b, c); }
};

static void test_group() {
  Group g;
  CHECK(g.reserve(8) && g.a.count() == 8 && g.b.count() == 16 && g.c.count() == 8);
  for (int second_fails = 0; second_fails < 2; ++second_fails) {
    // the first member grows, a later one fails: every member is empty afterwards
    A::fail_next = 0;
    CHECK(g.reserve(8));
    const long c0 = A::calls;
    if (second_fails) {
      CHECK(g.a.reserve(100));  // already large enough: the group call allocates b first
      A::fail_next = 1;
      CHECK(!g.reserve(100));
      CHECK(A::calls == c0 + 2);
    } else {
      A::fail_next = 1;
      CHECK(!g.reserve(100));
      CHECK(A::calls == c0 + 1);  // && stops at the first failure
    }
    CHECK(empty(g.a) && empty(g.b) && empty(g.c));
  }
  CHECK(g.reserve(3) && g.a.count() == 3 && g.b.count() == 6 && g.c.count() == 3);  // and recovers
}

static void test_release() {
  Buf<int> b;
  b.release();  // empty: harmless
  CHECK(b.reserve(3));
  const long f0 = A::frees;
  b.release();
  CHECK(empty(b) && A::frees == f0 + 1);
  b.release();  // twice: harmless
  CHECK(empty(b) && A::frees == f0 + 1);
}

static void test_move() {
  Buf<int> a;
  CHECK(a.reserve(4));
  int* pa = a.get();
  const long f0 = A::frees;
  Buf<int> b(std::move(a));  // construction: ownership moves, nothing freed
  CHECK(empty(a) && b.get() == pa && b.count() == 4 && A::frees == f0);
  Buf<int> c;
  CHECK(c.reserve(9));
  c = std::move(b);  // assignment: the overwritten target is freed
  CHECK(empty(b) && c.get() == pa && c.count() == 4 && A::frees == f0 + 1);
  Buf<int>& self = c;
  c = std::move(self);  // self-assignment keeps the buffer
  CHECK(c.get() == pa && c.count() == 4 && A::frees == f0 + 1);
  c.get()[3] = 1;
  Buf<int> d;
  d = std::move(a);  // moving an empty buffer
  CHECK(empty(d) && empty(a));
}

// host_rules.h: the accepted trace generators at the edge of every rule, and
// the staging arithmetic of the trajectory read-back (UBSan watches the sums)
static ccka_trace_gen gen(int32_t blo, int32_t bhi, int32_t alo, int32_t ahi, int32_t noise, int32_t mult, int32_t len) {
  ccka_trace_gen g{};
  g.base_lo = blo; g.base_hi = bhi; g.amp_lo_pm = alo; g.amp_hi_pm = ahi;
  g.noise_pm = noise; g.burst_prob_pm = 500; g.burst_mult_pm = mult; g.burst_len = len;
  return g;
}

static void test_host_rules() {
  using ccka::trace_gen_invalid;
  CHECK(!trace_gen_invalid(gen(500, 5000, 200, 800, 50, 3000, 30)));
  CHECK(!trace_gen_invalid(gen(0, 2000000000, 0, 3000, 1000, 3000, 30)));
  CHECK(!trace_gen_invalid(gen(0, 2000000000, 0, 3000, -1000, -3000, 700)));
  CHECK(!trace_gen_invalid(gen(7, 7, -5, -5, 0, 0, 0)));
  CHECK(trace_gen_invalid(gen(10, 9, 0, 0, 0, 0, 0)) && trace_gen_invalid(gen(0, 0, 1, 0, 0, 0, 0)));
  CHECK(!trace_gen_invalid(gen(-1, INT32_MAX - 2, 0, 0, 0, 0, 0)));  // width + 1 = INT32_MAX
  CHECK(trace_gen_invalid(gen(-1, INT32_MAX - 1, 0, 0, 0, 0, 0)));
  CHECK(trace_gen_invalid(gen(INT32_MIN, INT32_MAX, 0, 0, 0, 0, 0)));  // width + 1 = 2^32: a modulus of 0
  CHECK(trace_gen_invalid(gen(0, 1, INT32_MIN, INT32_MAX, 0, 0, 0)));
  CHECK(!trace_gen_invalid(gen(0, 1, 0, 0, 0, 0, INT32_MAX - 1439)) && trace_gen_invalid(gen(0, 1, 0, 0, 0, 0, INT32_MAX - 1438)));
  CHECK(trace_gen_invalid(gen(0, 1, 0, 0, 0, 0, -1)));
  // P1: 2^31 * (65536000 + 65536 A) <= 2^63 - 1  <=>  A <= 64536 (INT32_MIN as base: |base| = 2^31)
  CHECK(!trace_gen_invalid(gen(INT32_MIN, INT32_MIN + 1, 0, 64535, 0, 0, 0)));
  CHECK(trace_gen_invalid(gen(INT32_MIN, INT32_MIN + 1, 0, 64536, 0, 0, 0)));
  CHECK(trace_gen_invalid(gen(INT32_MIN, INT32_MIN + 1, -64536, 0, 0, 0, 0)));
  // P2: V1 = 8e9; 8e9 * (37837000 + 131072 n) <= 2^63 - 1  <=>  n <= 8507
  CHECK(!trace_gen_invalid(gen(0, 2000000000, 0, 3000, 8507, 0, 0)) && trace_gen_invalid(gen(0, 2000000000, 0, 3000, -8508, 0, 0)));
  CHECK(trace_gen_invalid(gen(0, 2000000000, 0, 3000, INT32_MIN, 0, 0)));
  // P3: V2 = 8e9 * 168909000 div 37837000 = 35712979358; * m <= 2^63 - 1  <=>  m <= 258263863
  CHECK(!trace_gen_invalid(gen(0, 2000000000, 0, 3000, 1000, 258263863, 0)));
  CHECK(trace_gen_invalid(gen(0, 2000000000, 0, 3000, 1000, -258263864, 0)));
  CHECK(trace_gen_invalid(gen(0, 2000000000, 0, 3000, 1000, INT32_MIN, 0)));

  // the timing rules of a world: the last accepted and the first rejected value of each
  auto timing = [](int32_t T, int32_t start, int32_t delay, int32_t ps, int32_t pe) {
    ccka_world w{};
    w.n_steps = T; w.start_minute = start; w.provision_delay_steps = delay;
    w.peak_start_min = ps; w.peak_end_min = pe;
    return ccka::world_timing_invalid(w);
  };
  const int32_t sm = ccka::kMaxStartMinute, dm = ccka::kMaxProvisionDelay;
  CHECK(sm == INT32_MAX - 65535 && dm == INT32_MAX - 65535);
  CHECK(!timing(1440, 0, 1, 960, 1260));
  CHECK(!timing(1, 0, 0, 0, 0) && timing(0, 0, 0, 0, 0));
  CHECK(!timing(65535, 0, 0, 0, 0) && timing(65536, 0, 0, 0, 0));
  CHECK(timing(10, -1, 0, 0, 0) && timing(10, 0, -1, 0, 0) && timing(10, INT32_MIN, 0, 0, 0) && timing(10, 0, INT32_MIN, 0, 0));
  CHECK(!timing(65535, sm, 0, 0, 0) && timing(65535, sm + 1, 0, 0, 0) && timing(1, INT32_MAX, 0, 0, 0));
  CHECK(!timing(65535, 0, dm, 0, 0) && timing(65535, 0, dm + 1, 0, 0) && timing(1, 0, INT32_MAX, 0, 0));
  {
    // what the bounds protect, formed as the kernels form it (UBSan watches the sums)
    volatile int32_t s = sm, d = dm, t = 65535;
    const int32_t minute = (s + t) % 1440, ready = (t - 1) + d;
    CHECK(minute == (int32_t)(((int64_t)sm + 65535) % 1440) && ready == 0x7ffffffe);
  }
  CHECK(!timing(10, 0, 0, 0, 1440) && !timing(10, 0, 0, 1440, 0) && !timing(10, 0, 0, 1440, 1440));
  CHECK(timing(10, 0, 0, -1, 0) && timing(10, 0, 0, 0, -1) && timing(10, 0, 0, 1441, 0) && timing(10, 0, 0, 0, 1441));
  CHECK(timing(10, 0, 0, -560, 100) && timing(10, 0, 0, INT32_MIN, 0) && timing(10, 0, 0, 0, INT32_MAX));

  using ccka::traj_stage_cap;
  const int64_t dflt = ccka::kTrajStageRecs;
  CHECK(traj_stage_cap(203, 203 * 71, 0) == 203 * 71);          // a small trajectory: all of it
  CHECK(traj_stage_cap(203, 203 * 71, 33 * 203) / 203 == 33);   // tc = 33
  CHECK(traj_stage_cap(203, 203 * 71, 33 * 203 + 202) / 203 == 33);
  CHECK(traj_stage_cap(203, 203 * 71, 5) == 203);               // never less than one step
  CHECK(traj_stage_cap(203, 203 * 71, 1 << 30) == 203 * 71);    // never more than the trajectory
  CHECK(traj_stage_cap(1000, dflt * 10, 0) == dflt && traj_stage_cap(dflt + 7, (dflt + 7) * 4, 0) == dflt + 7);
  CHECK(ccka::trace_tile_count(65, 5, 64) == 5 * 128 && ccka::trace_tile_count(64, 5, 64) == 5 * 64);
  CHECK(ccka::trace_nt_count(65, 5, 4) == 65 * 5 * 4);
  // a getter's copy against its grow-only buffer: all of it is the last
  // accepted count, one more the first rejected; nothing from an empty buffer
  using ccka::copy_fits;
  CHECK(copy_fits(120 * 64, 120 * 64) && copy_fits(40 * 64, 120 * 64) && copy_fits(0, 0));
  CHECK(!copy_fits(120 * 64 + 1, 120 * 64) && !copy_fits(1, 0) && !copy_fits(-1, 10));
  CHECK(copy_fits(INT64_MAX, INT64_MAX) && !copy_fits(INT64_MAX, INT64_MAX - 1));
}

int main() {
  test_host_rules();
  test_reserve();
  test_resize();
  test_overflow();
  test_failure_and_recovery();
  test_group();
  test_release();
  test_move();
  // every buffer above has left its scope: nothing outstanding
  CHECK(A::allocs > 0 && A::allocs == A::frees);
  std::printf("devbuf ok: %ld allocations, %ld frees\n", A::allocs, A::frees);
  return 0;
}
