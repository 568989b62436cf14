"""Plain references of the small kernels around a rollout (csrc/util.hip) and
of the per-grid sums (csrc/sweep.hip), restated from docs/SEMANTICS.md and
include/ccka.h in Python integers and numpy index arithmetic, no C: the
synthetic load generator (§4), the totals with their overflow flag, the two
summation orders of §6, and the two trace layouts. The checkers of
tests/test_util_ref.py and tests/test_gpu_util_kernels.py."""
from __future__ import annotations

import math

import numpy as np

from ccka import abi

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MAX = 0x7FFFFFFF
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------
# §4: the synthetic load generator
# ---------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on broadcastable counter words (uint64 arrays holding
    32-bit values; every product of two of them fits 64 bits): four words."""
    c = [np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & M32, (p0 >> s32) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def sin_table():
    """SIN[m] = lround(65536 sin(2 pi m / 1440)): half away from zero."""
    out = []
    for m in range(1440):
        x = 65536.0 * math.sin(2.0 * math.pi * m / 1440.0)
        out.append(int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1))
    return out


def _ints(a):
    """An object array of Python ints (unbounded: nothing wraps silently)."""
    return np.asarray(a).astype(object)


def _tdiv(a, b: int):
    """a / b truncated toward zero, as C divides (Python's // floors), b > 0."""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def _in_i64(name, a):
    lo, hi = a.min(), a.max()
    assert I64_MIN <= lo and hi <= I64_MAX, f"{name} leaves int64: [{lo}, {hi}]"


def gen_load(g: abi.TraceGen, T: int, D: int, n: int, first_id: int = 0):
    """(trace [T][D][n] int32, tallies) of the generator of §4 for scenario ids
    first_id .. first_id + n (shared traces: first_id = 0). Asserts that every
    intermediate stays inside int64 (so the case is defined for the C sides).
    tallies: samples, low / high (clamped to 0 / 0x7fffffff), interior, and
    flip1 / flip2: interior samples > 0 whose first / second product was
    negative and that a later negative factor turned positive (where a
    flooring division would differ from the truncating one)."""
    assert g.base_hi >= g.base_lo and g.amp_hi_pm >= g.amp_lo_pm
    assert g.base_hi - g.base_lo + 1 <= I32_MAX and g.amp_hi_pm - g.amp_lo_pm + 1 <= I32_MAX  # int32 moduli
    assert 0 <= g.burst_len <= I32_MAX - 1439
    SIN = _ints(sin_table())
    k0, k1 = g.seed & 0xFFFFFFFF, g.seed >> 32
    ids = np.arange(first_id, first_id + n, dtype=np.uint64)
    slo, shi = (ids & M32)[None, :], (ids >> np.uint64(32))[None, :]
    tt = np.arange(T, dtype=np.uint64)[:, None]
    out = np.zeros((T, D, n), np.int32)
    tally = dict(samples=0, low=0, high=0, interior=0, flip1=0, flip2=0)
    for d in range(D):
        u = philox(0xFFFFFFFF, slo, shi, d, k0, k1)
        v = philox(0xFFFFFFFE, slo, shi, d, k0, k1)
        base = g.base_lo + _ints(u[0] % np.uint64(g.base_hi - g.base_lo + 1))     # [1][n]
        amp = g.amp_lo_pm + _ints(u[1] % np.uint64(g.amp_hi_pm - g.amp_lo_pm + 1))
        phase = (u[2] % np.uint64(1440)).astype(np.int64)
        burst = (u[3] % np.uint64(1000)).astype(np.int64) < g.burst_prob_pm
        bstart = (v[0] % np.uint64(1440)).astype(np.int64)
        e4 = philox(tt, slo, shi, d, k0, k1)                                        # [T][n]
        e = _ints(sum(w >> np.uint64(16) for w in e4)) - 131072
        t = tt.astype(np.int64)
        f1 = 65536000 + amp * SIN[(t + phase) % 1440]
        p1 = base * f1
        v1 = _tdiv(p1, 65536000)
        f2 = 37837000 + int(g.noise_pm) * e
        p2 = v1 * f2
        val = _tdiv(p2, 37837000)
        inb = burst & (t >= bstart) & (t < bstart + g.burst_len)
        p3 = val * int(g.burst_mult_pm)
        for name, a in (("amp * SIN", f1), ("base * (...)", p1), ("noise * e", f2), ("v * (...)", p2)):
            _in_i64(name, a)
        if inb.any():
            _in_i64("v * burst_mult", p3[inb])
        val = np.where(inb, _tdiv(p3, 1000), val)
        low, high = val < 0, val > I32_MAX
        live = ~low & ~high & (val > 0)
        tally["samples"] += val.size
        tally["low"] += int(low.sum())
        tally["high"] += int(high.sum())
        tally["interior"] += int((~low & ~high).sum())
        tally["flip1"] += int((live & (p1 < 0)).sum())
        tally["flip2"] += int((live & (p2 < 0)).sum())
        out[:, d, :] = np.clip(val, 0, I32_MAX).astype(np.int64)
    return out, tally


def wide_gen(negative: bool = False, seed: int = 0xC0FFEE1234567) -> abi.TraceGen:
    """A generator at the edge of what ccka_gen_load accepts: base up to 2e9,
    amplitude up to 3 (the diurnal factor goes negative), noise sigma 1 (the
    noise factor goes negative), burst x3 for 30 steps at p = 0.5; `negative`:
    noise -1 and a burst of x(-3) for 700 steps (it turns negatives positive)."""
    g = abi.TraceGen()
    g.seed = seed
    g.base_lo, g.base_hi = 0, 2_000_000_000
    g.amp_lo_pm, g.amp_hi_pm = 0, 3000
    g.noise_pm = -1000 if negative else 1000
    g.burst_prob_pm, g.burst_mult_pm, g.burst_len = 500, (-3000 if negative else 3000), (700 if negative else 30)
    return g


# (T, D, n, first_id, n_traces): one step of one scenario; a high id word; t +
# phase beyond 2 * 1440 and a burst window past 1440; the id's high word
# changing inside the batch at 16 deployments; one shared-trace set (keyed
# from 0 whatever first_id is)
GEN_SHAPES = ((1, 1, 1, 0, 0), (97, 3, 321, (1 << 33) + 5, 0), (1500, 1, 65, 7, 0),
              (33, 16, 257, (1 << 32) - 100, 0), (50, 2, 48 * 3, 48 * 1000, 48))
_GEN_CACHE = {}


def gen_case(shape, negative: bool):
    """(trace, tallies) of GEN_SHAPES' `shape` under wide_gen(negative), computed once per process."""
    key = (shape, negative)
    if key not in _GEN_CACHE:
        T, D, n, first_id, n_traces = shape
        got = gen_load(wide_gen(negative), T, D, n_traces or n, 0 if n_traces else first_id)
        got[0].setflags(write=False)
        _GEN_CACHE[key] = got
    return _GEN_CACHE[key]


# ---------------------------------------------------------------------------
# totals (include/ccka.h: ccka_totals)
# ---------------------------------------------------------------------------
INT_TOTALS = (("cost_uphmin", "cost_uphmin"), ("slo_minutes", "slo_minutes"),
              ("pending_pod_minutes", "pending_pod_minutes"), ("node_min_spot", "node_min_spot"),
              ("node_min_od", "node_min_od"), ("launches", "launches"), ("deletions", "deletions"))
FIX_TOTALS = (("energy_uwmin", "energy_wmin"), ("gco2_ug", "gco2"))


def fix6(x: float):
    """(llrint(x * 1e6), flag): the binary64 product rounded once to the nearest
    integer, ties to even (Python's round on a float is exact and half-even);
    flagged, value 0, when the product is NaN or |product| >= 2^63."""
    y = float(x) * 1e6
    if not (-9.2233720368547758e18 < y < 9.2233720368547758e18):
        return 0, True
    return round(y), False


def totals(cols):
    """(fields dict, overflow flag) of result columns. Sums are Python ints; the
    flag is set when a per-scenario fixed-point value is not representable or
    a sum of one field leaves int64. Meant for non-negative columns, where the
    flag does not depend on the order of the additions (a prefix of a sum that
    fits also fits); the fields are what every order gives when unflagged."""
    n = len(cols["cost_uphmin"])
    out, ovf = {"scenarios": n}, False
    for f, col in INT_TOTALS:
        out[f] = sum(np.asarray(cols[col]).tolist())  # Python ints
    for f, col in FIX_TOTALS:
        # fix6 on the whole column: one binary64 product each, rint is to
        # nearest even and gives integer-valued floats, int() of those is exact
        y = np.asarray(cols[col], np.float64) * 1e6
        ok = (y > -9.2233720368547758e18) & (y < 9.2233720368547758e18)
        ovf = ovf or not ok.all()
        out[f] = sum(int(v) for v in np.rint(y[ok]).tolist())
    ovf = ovf or any(not (I64_MIN <= out[f] <= I64_MAX) for f in out)
    if not ovf:
        out["energy_wmin"] = float(out["energy_uwmin"]) * 1e-6  # int64 -> binary64 (nearest even), one product
        out["gco2"] = float(out["gco2_ug"]) * 1e-6
    return out, ovf


TOTALS_N = (1, 255, 256, 257, 511, 65537, 262144, 262145, 300001)


def random_columns(n: int, seed: int = 0):
    """Non-negative result columns of n scenarios in a rollout's ranges."""
    rng = np.random.default_rng([n, seed])
    return {"cost_uphmin": rng.integers(0, 1 << 40, n, dtype=np.int64),
            "slo_minutes": rng.integers(0, 1441, n, dtype=np.int32),
            "pending_pod_minutes": rng.integers(0, 1 << 33, n, dtype=np.int64),
            "node_min_spot": rng.integers(0, 1 << 20, n, dtype=np.int32),
            "node_min_od": rng.integers(0, 1 << 20, n, dtype=np.int32),
            "launches": rng.integers(0, I32_MAX, n, dtype=np.int32, endpoint=True),
            "deletions": rng.integers(0, 1 << 16, n, dtype=np.int32),
            "energy_wmin": rng.random(n) * 1e5,
            "gco2": rng.random(n) * 10.0 ** rng.integers(-9, 4, n)}


def zero_columns(n: int):
    return {k: np.zeros_like(v) for k, v in random_columns(n).items()}


def largest_fix6_input():
    """The largest double whose binary64 product with 1e6 is below 2^63: its
    successor's product is 2^63 or more (flagged). Near 9.22e12 one ulp of x
    moves the product by 1953.125, so the products step by 1024 or 2048 and
    2^63 - 1024 itself has no preimage: the product here is 2^63 - 2048."""
    x = 2.0 ** 63 / 1e6
    while x * 1e6 >= 2.0 ** 63:
        x = math.nextafter(x, 0.0)
    while math.nextafter(x, math.inf) * 1e6 < 2.0 ** 63:
        x = math.nextafter(x, math.inf)
    return x


def totals_edge_cases():
    """[(name, columns, flagged)]: 1000 scenarios (four partials of 250; 300001
    where two terms must meet in one thread), every column zero but the named one. Columns are non-negative, so `some partial
    overflows` and `the total overflows` coincide."""
    n, late = 1000, 900  # scenario 900 lies in the last partial
    cases = []

    def case(name, col, values, flagged, n=n):
        c = zero_columns(n)
        for i, v in values.items():
            c[col][i] = v
        cases.append((name, c, flagged))

    for col in ("cost_uphmin", "pending_pod_minutes"):
        case(f"{col} sums to INT64_MAX", col, {0: I64_MAX - 10, 3: 4, late: 6}, False)
        case(f"{col} sums to INT64_MAX + 1", col, {0: I64_MAX - 10, 3: 4, late: 7}, True)
    # 300001 scenarios: chunks of 293, so threads 0 .. 36 of a workgroup add two
    # scenarios (i and i + 256) before any tree: the excess meets the large
    # value in one thread's own run, in workgroup 1000
    big, i0 = 300001, 1000 * 293 + 5
    for col in ("cost_uphmin", "pending_pod_minutes"):
        case(f"{col} one thread's run sums to INT64_MAX", col, {i0: I64_MAX - 10, i0 + 256: 10}, False, big)
        case(f"{col} one thread's run sums to INT64_MAX + 1", col, {i0: I64_MAX - 10, i0 + 256: 11}, True, big)
    case("energy one thread's run leaves int64", "energy_wmin", {i0: 5e12, i0 + 256: 5e12}, True, big)
    case("energy 9.3e12", "energy_wmin", {late: 9.3e12}, True)
    case("energy product just below 2^63", "energy_wmin", {late: largest_fix6_input()}, False)
    case("gco2 NaN", "gco2", {5: math.nan}, True)
    case("gco2 +inf", "gco2", {late: math.inf}, True)
    # m / 128 * 1e6 = 7812.5 m exactly: ties, to even 7812 (m = 1), 23438 (m = 3), ...
    case("ties round to even", "gco2", {i: (2 * i + 1) / 128.0 for i in range(0, n, 7)}, False)
    return cases


# ---------------------------------------------------------------------------
# §6: the summation orders, and the bound that holds for any order
# ---------------------------------------------------------------------------
def _tree(s):
    """The halving tree over a power-of-two row of partials: s[j] += s[j + w]
    for w = len/2 .. 1 (one binary64 addition each)."""
    s = np.array(s, np.float64)
    w = len(s) // 2
    while w:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return s[0]


def _strided(x, lanes):
    """Lane j's partial: 0.0 + x[j] + x[j + lanes] + ... in index order."""
    acc = np.zeros(lanes, np.float64)
    for k in range(0, len(x), lanes):
        part = x[k:k + lanes]
        acc[:len(part)] = acc[:len(part)] + part
    return acc


def grid_sum(x) -> float:
    """SUM of one grid's doubles in the stated order: thread j of 256 adds
    elements j, j + 256, ... in index order, then the halving tree 128 .. 1."""
    return float(_tree(_strided(np.asarray(x, np.float64), 256)))


def tail_sum(x, k: int) -> float:
    """TAIL of one grid's doubles in the stated order: lane l of 64 adds the
    values above x(k) at l, l + 64, ... in index order, then the halving tree
    32 .. 1, then + ties * x(k) (one product, one addition)."""
    x = np.asarray(x, np.float64)
    xk = np.sort(x)[k - 1]
    above = x > xk
    m = (len(x) - k + 1) - int(above.sum())
    acc = _tree(_strided(np.where(above, x, 0.0), 64))  # + 0.0 leaves a partial's bits: it starts at +0.0
    return float(acc + np.float64(m) * xk)


def fsum_bound(terms) -> tuple:
    """(exact sum rounded once, bound): any order of n binary64 additions of
    `terms` lies within (n - 1) 2^-53 sum|x_i| of the exact sum, to first
    order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2)."""
    t = [float(v) for v in terms]
    return math.fsum(t), max(0, len(t) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


def tail_terms(x, k: int):
    """The n - k + 1 largest values of x, ascending (the TAIL's terms)."""
    return np.sort(np.asarray(x, np.float64))[k - 1:]


# ---------------------------------------------------------------------------
# trace layouts (csrc/util.hip)
# ---------------------------------------------------------------------------
def trace_nt(trace, dp: int):
    """[T][D][NL] -> [NL][T][DP], flat; deployments d >= D are zero."""
    T, D, NL = trace.shape
    out = np.zeros((NL, T, dp), np.int32)
    out[:, :, :D] = np.transpose(trace, (2, 0, 1))
    return out.ravel()


def trace_tile(trace, lpw: int, sentinel: int):
    """[T][1][N] -> [wave][T][lpw], flat: wave w holds scenarios w lpw ..
    (w + 1) lpw; the lanes of the last wave past N are not written (they keep
    `sentinel`): no kernel reads them."""
    T, D, N = trace.shape
    assert D == 1
    waves = (N + lpw - 1) // lpw
    out = np.full((waves, T, lpw), sentinel, np.int64)
    n = np.arange(N)
    out[n // lpw, :, n % lpw] = trace[:, 0, :].T
    return out.astype(np.int32).ravel()
