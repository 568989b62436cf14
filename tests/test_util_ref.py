"""CPU checks of tests/util_ref.py, the plain references behind
tests/test_gpu_util_kernels.py: that the wide generator cases are active (both
clamps, and negative dividends that survive to the output) and stay inside
int64, and that each restatement agrees with the CPU oracle or with a second,
independent statement of the same rule."""
import ctypes as C
import math

import numpy as np
import pytest

import pyoracle as po
import util_ref as ur
from ccka import abi, configs


# ---- generator ----------------------------------------------------------------
def test_philox_and_sine_table_match_the_oracle():
    out = (C.c_uint32 * 4)()
    rng = np.random.default_rng(3)
    for c0, c1, c2, c3, k0, k1 in rng.integers(0, 1 << 32, (50, 6)).tolist() + [[0] * 6, [0xFFFFFFFF] * 6]:
        po.lib().ccka_oracle_philox(c0, c1, c2, c3, k0, k1, out)
        assert [int(w) for w in ur.philox(c0, c1, c2, c3, k0, k1)] == list(out)
    tab = (C.c_int32 * 1440)()
    po.lib().ccka_oracle_sin_table(tab)
    assert ur.sin_table() == list(tab)


def test_division_truncates_toward_zero():
    a = ur._ints([-7, 7, -8, 8, -1, 0, 1, -(1 << 62) - 1])
    assert ur._tdiv(a, 4).tolist() == [-1, 1, -2, 2, 0, 0, 0, -(1 << 60)]
    assert (a // 4).tolist()[:2] == [-2, 1]  # what a bare // would have given


@pytest.mark.parametrize("negative", [False, True], ids=["wide", "negative"])
@pytest.mark.parametrize("shape", ur.GEN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wide_generator_cases_match_the_oracle(shape, negative):
    T, D, n, first_id, n_traces = shape
    want, _ = ur.gen_case(shape, negative)  # asserts every intermediate inside int64
    got = po.gen_load(ur.wide_gen(negative), T, D, n_traces or n, 0 if n_traces else first_id)
    assert np.array_equal(got, want)


def test_default_generator_matches_the_oracle():
    g = configs.trace_gen()
    want, tally = ur.gen_load(g, 200, 2, 50, first_id=123457)
    assert np.array_equal(po.gen_load(g, 200, 2, 50, first_id=123457), want)
    assert tally["low"] == tally["high"] == tally["flip1"] == tally["flip2"] == 0  # why the wide cases exist


def test_wide_generator_cases_are_active():
    tot = {}
    for negative in (False, True):
        for shape in ur.GEN_SHAPES:
            for k, v in ur.gen_case(shape, negative)[1].items():
                tot[k] = tot.get(k, 0) + v
    frac = {k: v / tot["samples"] for k, v in tot.items()}
    print(tot, frac)
    assert frac["low"] >= 0.05 and frac["high"] >= 0.05 and frac["interior"] >= 0.30
    # interior samples reached through a negative product that a later negative
    # factor turned positive: where floor and truncation differ
    assert frac["flip1"] + frac["flip2"] >= 0.01
    # each division on its own: the first through a negative noise factor, the
    # second through the negative burst multiplier
    assert tot["flip1"] >= 1000 and tot["flip2"] >= 1000


def test_intermediate_range_assertion_fires():
    g = ur.wide_gen()
    g.noise_pm = 2**30  # V1 * (37837000 + 131072 * 2^30) leaves int64
    with pytest.raises(AssertionError, match="leaves int64"):
        ur.gen_load(g, 8, 1, 64)


# ---- totals ---------------------------------------------------------------------
def _oracle(cols):
    n = len(cols["cost_uphmin"])
    full = {name: np.zeros(n, dt) for name, _, dt in abi.RESULT_FIELDS}
    for k, v in cols.items():
        full[k] = np.ascontiguousarray(v, full[k].dtype)
    try:
        return po.totals(full, n), False
    except OverflowError:
        return None, True


def _same(t, want):
    for f, _ in t._fields_:
        got = getattr(t, f)
        assert (got.hex() == float(want[f]).hex()) if isinstance(got, float) else got == want[f], f


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_totals_reference_matches_the_oracle(n):
    cols = ur.random_columns(n)
    want, flagged = ur.totals(cols)
    orc, oflag = _oracle(cols)
    assert not flagged and not oflag
    _same(orc, want)


def test_totals_edge_cases_match_the_oracle():
    cases = ur.totals_edge_cases()
    assert sum(f for _, _, f in cases) >= 5 and sum(not f for _, _, f in cases) >= 4
    for name, cols, flagged in cases:
        want, rflag = ur.totals(cols)
        orc, oflag = _oracle(cols)
        assert rflag == oflag == flagged, name
        if not flagged:
            _same(orc, want)


def test_fixed_point_rounding():
    assert ur.fix6(1 / 128) == (7812, False) and ur.fix6(3 / 128) == (23438, False)  # ties to even
    assert ur.fix6(-1 / 128) == (-7812, False)
    x = ur.largest_fix6_input()
    print("largest accepted energy", x.hex(), "product 2^63 -", (1 << 63) - ur.fix6(x)[0])
    assert ur.fix6(x)[1] is False and (1 << 63) - 2048 <= ur.fix6(x)[0] < 1 << 63
    assert ur.fix6(math.nextafter(x, math.inf)) == (0, True)
    for bad in (9.3e12, -9.3e12, math.nan, math.inf, -math.inf, 2.0 ** 63 / 1e6 * (1 + 1e-15)):
        assert ur.fix6(bad)[1], bad
    want, flagged = ur.totals({**ur.zero_columns(3), "gco2": np.array([1 / 128, 3 / 128, 5 / 128])})
    assert not flagged and want["gco2_ug"] == 7812 + 23438 + 39062


# ---- summation orders -------------------------------------------------------------
def _scalar_grid_sum(x, lanes):
    """The stated order, one Python float addition at a time."""
    acc = [0.0] * lanes
    for i, v in enumerate(x):
        acc[i % lanes] += float(v)  # lane i % lanes meets its elements in index order
    w = lanes // 2
    while w:
        for j in range(w):
            acc[j] += acc[j + w]
        w //= 2
    return acc[0]


@pytest.mark.parametrize("g", [1, 255, 256, 257, 513, 2500])
def test_sum_orders_against_scalar_restatement_and_fsum(g):
    rng = np.random.default_rng(g)
    x = rng.standard_normal(g) * 10.0 ** rng.integers(-5, 6, g)
    s = ur.grid_sum(x)
    assert s.hex() == _scalar_grid_sum(x, 256).hex()
    exact, bound = ur.fsum_bound(x)
    assert abs(s - exact) <= bound
    for k in sorted({1, max(1, g // 2), g}):
        t = ur.tail_sum(x, k)
        xs = np.sort(x)
        above = [v if v > xs[k - 1] else 0.0 for v in x]
        m = (g - k + 1) - sum(v > xs[k - 1] for v in x)
        assert t.hex() == (_scalar_grid_sum(above, 64) + float(m) * float(xs[k - 1])).hex()
        exact, bound = ur.fsum_bound(ur.tail_terms(x, k))
        assert abs(t - exact) <= bound
    if g > 256:  # the order matters: index order gives other bits somewhere
        assert any(ur.grid_sum(rng.permutation(x)).hex() != s.hex() for _ in range(4))


# ---- layouts ----------------------------------------------------------------------
def test_layout_references_against_loops():
    rng = np.random.default_rng(5)
    T, D, NL, dp = 5, 3, 9, 4
    tr = rng.integers(-2**31, 2**31, (T, D, NL)).astype(np.int32)
    nt = ur.trace_nt(tr, dp)
    assert nt.shape == (NL * T * dp,)
    for col in range(NL):
        for t in range(T):
            for d in range(dp):
                assert nt[(col * T + t) * dp + d] == (tr[t, d, col] if d < D else 0)
    N, lpw, s = 9, 4, 77
    tile = ur.trace_tile(tr[:, :1, :], lpw, s)
    assert tile.shape == (T * 12,)
    want = np.full(T * 12, s, np.int64)
    for n in range(N):
        for t in range(T):
            want[(n // lpw) * lpw * T + t * lpw + n % lpw] = tr[t, 0, n]
    assert np.array_equal(tile, want)
