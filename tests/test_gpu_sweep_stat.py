"""GPU checks of the sweep tail statistics (docs/SEMANTICS.md 6): per-grid
quantiles and tail sums from the device's radix select against the numpy
restatement (tests/sweep_stat_ref.py) on adversarial keys and on a sweep's
oracle results, SUM objectives against ccka_get_grid_stats bit for bit, the
sums and tail sums of doubles (signed ones included) bit for bit against the
summation order SEMANTICS 6 states (tests/util_ref.py) and within the bound
that holds for any order, and the frontier over the statistics, local and
through a one-rank communicator."""
import numpy as np
import pytest

import pyoracle as po
import sweep_stat_ref as ref
import util_ref as ur
from ccka import abi, configs
from ccka.engine import Engine
from parity import oracle, run_engine

pytestmark = pytest.mark.gpu
THREADS = 16
# two orders of n non-negative terms differ by <= 2 n 2^-53 relative: 2.3e-13 at
# n = 1024, 5.6e-13 at the largest grid here (2500)
TAIL_RTOL = 1e-12
I64 = np.iinfo(np.int64)
I32_MAX = np.iinfo(np.int32).max
N_GRIDS, N_TRACES = 24, 48


def _stat(kind, q):
    return abi.sweep_stat(*[(kind, q)] * 4)


MIXED = dict(slo=("quantile", 950000), energy=("tail", 900000))  # cost, gco2: SUM
MIXED_KINDS, MIXED_Q = (ref.SUM, ref.QUANTILE, ref.SUM, ref.TAIL), (0, 950000, 0, 900000)


def _check(got, want, kinds):
    for f in ("grid", "scenarios"):
        assert np.array_equal(got[f], want[f]), f
    for f, kind in zip(ref.FIELDS, kinds):
        if kind == ref.TAIL and got[f].dtype.kind == "f":
            print(f, "max rel", np.max(np.abs(got[f] - want[f]) / np.maximum(np.abs(want[f]), 1e-300)))
            assert np.allclose(got[f], want[f], rtol=TAIL_RTOL, atol=0), f
        elif kind != ref.SUM:
            assert np.array_equal(got[f], want[f]), (f, got[f], want[f])


# ---- 1. selection on adversarial keys (no rollout) -----------------------
def _columns(g, tail, signed=False):
    """Five grids of g scenarios whose keys stress every radix digit. signed
    (with tail): the doubles keep their signs (held to the stated summation
    order and the order-free bound below, not to TAIL_RTOL)."""
    rng = np.random.default_rng(1000 * g + tail)
    cost = np.empty((5, g), np.int64)
    cost[0] = np.array([I64.min, I64.max, 0, -1], np.int64)[rng.integers(0, 4, g)]
    cost[1] = 0x1234567890ABCD00 + rng.integers(0, 256, g)                        # lowest byte only
    cost[2] = (rng.integers(-128, 128, g).astype(np.int64) << 56) + 0x00FEDCBA98765432  # highest byte only
    cost[3] = -987654321012345                                                       # all equal
    cost[4] = rng.integers(I64.min, I64.max, g, dtype=np.int64, endpoint=True)
    slo = np.zeros((5, g), np.int32)                                                 # heavy ties
    u = rng.random((5, g))
    slo[u < 0.1] = I32_MAX
    slo[u > 0.9] = rng.integers(-3, 4, int((u > 0.9).sum()))
    pool = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, 1e300, -1e300, -1.5, 1.0, np.nextafter(1.0, 2.0),
                     -2.0, np.nextafter(-2.0, -3.0), 2.2250738585072014e-308])
    gco2 = pool[rng.integers(0, len(pool), (5, g))]
    energy = rng.standard_normal((5, g)) * 10.0 ** rng.integers(-5, 6, (5, g))
    h = g // 2
    energy[:, 1:2 * h:2] = np.nextafter(energy[:, 0:2 * h:2], np.inf)              # pairs one ulp apart
    if tail:  # sums must stay inside int64; the double tolerance is for non-negative terms
        cost = np.clip(cost, -(1 << 40), 1 << 40)
        if not signed:
            gco2, energy = np.abs(gco2), np.abs(energy)
    return {"cost_uphmin": cost.ravel(), "slo_minutes": slo.ravel(), "gco2": gco2.ravel(),
            "energy_wmin": energy.ravel()}


# up to 1024 the kernel keeps a grid's keys in LDS; 1025 and 2500 take its
# other path (every pass re-reads the columns)
@pytest.mark.parametrize("g", [1, 2, 63, 64, 65, 257, 700, 1024, 1025, 2500])
def test_selection_on_adversarial_keys(engine, g):
    for kind in (ref.QUANTILE, ref.TAIL):
        cols = _columns(g, kind == ref.TAIL)
        for q in (0, 1, 500000, 950000, 10**6):
            got = engine.debug_grid_stat(cols["cost_uphmin"], cols["slo_minutes"], cols["gco2"],
                                         cols["energy_wmin"], g, _stat(kind, q))
            assert len(got) == 5
            _check(got, ref.grid_stat(cols, g, [kind] * 4, [q] * 4), [kind] * 4)
            if kind == ref.QUANTILE:  # always an element of the input
                for f in ref.FIELDS:
                    assert all(v in cols[f].reshape(5, g)[i] for i, v in enumerate(got[f])), f


# ---- 1b. the sums' order (SEMANTICS 6), signed doubles included ------------
def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _within_fsum_bound(got, terms, what):
    """|got - fsum(terms)| <= (n - 1) 2^-53 sum|terms|: holds for any order of the additions."""
    exact, bound = ur.fsum_bound(terms)
    print(what, "err", abs(got - exact), "bound", bound)
    assert abs(got - exact) <= bound, (what, got, exact, bound)


# 255 / 256 / 257: the strided loop's first wrap; 513, 1024, 2500: 3, 4 and 10 trips
@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("g", [1, 255, 256, 257, 513, 1024, 2500])
def test_grid_sums_in_the_stated_order(engine, g, signed):
    cols = _columns(g, True, signed)
    got = engine.debug_grid_stat(cols["cost_uphmin"], cols["slo_minutes"], cols["gco2"], cols["energy_wmin"], g,
                                 abi.sweep_stat())
    assert len(got) == 5
    assert np.array_equal(got["grid"], np.arange(5)) and np.array_equal(got["scenarios"], np.full(5, g))
    for f in ("cost_uphmin", "slo_minutes"):  # Python ints: exact
        rows = cols[f].reshape(5, g)
        assert got[f].tolist() == [sum(r.tolist()) for r in rows], f
    for f in ("gco2", "energy_wmin"):
        rows = cols[f].reshape(5, g)
        want = [ur.grid_sum(r) for r in rows]
        assert np.array_equal(_bits(got[f]), _bits(want)), (f, got[f], want)  # bit for bit
        for i, r in enumerate(rows):
            _within_fsum_bound(float(got[f][i]), r, f"{f} sum g={g} grid {i}")


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("g", [1, 2, 63, 64, 65, 257, 700, 1024, 1025, 2500])
def test_tail_sums_in_the_stated_order(engine, g, signed):
    cols = _columns(g, True, signed)
    for q in (0, 1, 500000, 950000, 10**6):
        got = engine.debug_grid_stat(cols["cost_uphmin"], cols["slo_minutes"], cols["gco2"], cols["energy_wmin"], g,
                                     _stat(ref.TAIL, q))
        want = ref.grid_stat(cols, g, [ref.TAIL] * 4, [q] * 4)
        for f in ("grid", "scenarios", "cost_uphmin", "slo_minutes"):  # integers: exact
            assert np.array_equal(got[f], want[f]), (f, q)
        k = ref.rank(g, q)
        for f in ("gco2", "energy_wmin"):
            rows = cols[f].reshape(5, g)
            stated = [ur.tail_sum(r, k) for r in rows]
            assert np.array_equal(_bits(got[f]), _bits(stated)), (f, q, got[f], stated)  # bit for bit
            for i, r in enumerate(rows):
                _within_fsum_bound(float(got[f][i]), ur.tail_terms(r, k), f"{f} tail g={g} q={q} grid {i}")


# ---- 2.-4., 6., 7. on one sweep -------------------------------------------
@pytest.fixture(scope="module")
def sweep(engine):
    """One rollout of 24 grids x 48 shared traces on the engine, and the oracle's results."""
    T = 240
    spec = configs.config2_world(n_steps=T)
    sc = configs.config4_scenarios(37, N_GRIDS, N_TRACES)
    load = po.gen_load(configs.config4_trace_gen(), T, 1, N_TRACES)
    run_engine(engine, spec, sc, load=load)
    rc, _ = oracle(spec, sc, load, threads=THREADS)
    return sc, rc


@pytest.mark.parametrize("kind,q", [(ref.QUANTILE, 500000), (ref.QUANTILE, 950000), (ref.TAIL, 950000)])
def test_sweep_parity_with_oracle_statistics(engine, sweep, kind, q):
    sc, rc = sweep
    got = engine.grid_stat(N_TRACES, _stat(kind, q))
    assert len(got) == N_GRIDS
    _check(got, ref.grid_stat(rc, N_TRACES, [kind] * 4, [q] * 4, sc.first_id), [kind] * 4)


def test_sum_objectives_are_the_existing_sums(engine, sweep):
    sc, rc = sweep
    sums = engine.grid_stats(N_TRACES)
    got = engine.grid_stat(N_TRACES, abi.sweep_stat(**MIXED))
    assert np.array_equal(got["cost_uphmin"], sums["cost_uphmin"])
    assert np.array_equal(got["gco2"].view(np.int64), sums["gco2"].view(np.int64))  # bit for bit
    _check(got, ref.grid_stat(rc, N_TRACES, MIXED_KINDS, MIXED_Q, sc.first_id), MIXED_KINDS)
    # the tail from rank 1 is the whole sum
    got = engine.grid_stat(N_TRACES, _stat(ref.TAIL, 0))
    for f in ("grid", "scenarios", "cost_uphmin", "slo_minutes"):
        assert np.array_equal(got[f], sums[f]), f
    for f in ("gco2", "energy_wmin"):
        assert np.allclose(got[f], sums[f], rtol=TAIL_RTOL, atol=0), f


def test_frontier_over_statistics(engine, sweep):
    mixed = abi.sweep_stat(**MIXED)
    got = engine.grid_stat(N_TRACES, mixed)
    front = engine.pareto(N_TRACES, stat=mixed)
    assert np.array_equal(front, got[po.pareto({k: got[k] for k in got.dtype.names})])
    assert len(front) >= 1
    assert np.array_equal(engine.pareto(N_TRACES, stat=abi.sweep_stat()), engine.pareto(N_TRACES))


def test_deterministic_and_stateless(engine, sweep):
    st = _stat(ref.TAIL, 950000)
    a = engine.grid_stat(N_TRACES, st)
    sums = engine.grid_stats(N_TRACES)
    b = engine.grid_stat(N_TRACES, st)
    assert a.tobytes() == b.tobytes()
    assert sums.tobytes() == engine.grid_stats(N_TRACES).tobytes()
    q = engine.grid_stat(N_TRACES, _stat(ref.QUANTILE, 500000))
    assert q.tobytes() == engine.grid_stat(N_TRACES, _stat(ref.QUANTILE, 500000)).tobytes()


@pytest.mark.parametrize("bad", [abi.sweep_stat(cost=(3, 0)), abi.sweep_stat(slo=("quantile", -1)),
                                 abi.sweep_stat(energy=("tail", 1000001))])
def test_rejects_bad_statistics(engine, sweep, bad):
    with pytest.raises(abi.CckaError):
        engine.grid_stat(N_TRACES, bad)
    with pytest.raises(abi.CckaError):
        engine.pareto(N_TRACES, stat=bad)
    assert len(engine.grid_stat(N_TRACES, abi.sweep_stat(cost=("sum", -5)))) == N_GRIDS  # q_ppm ignored for SUM


# ---- 5. the communicator path, and partial grids --------------------------
@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_frontier_with_communicator_equals_local(eng):
    n_traces = 16
    spec = configs.config2_world(n_steps=360)
    sc = configs.config4_scenarios(40, 48, n_traces)
    load = po.gen_load(configs.config4_trace_gen(), 360, 1, n_traces)
    mixed = abi.sweep_stat(**MIXED)
    fresh = Engine(0)  # no communicator: the local frontier
    try:
        run_engine(fresh, spec, sc, load=load)
        want = fresh.pareto(n_traces, stat=mixed)
    finally:
        fresh.close()
    run_engine(eng, spec, sc, load=load)
    if not eng.lib.ccka_comm_info(eng.ctx, None, None) == 0:
        eng.comm_init()
    assert eng.comm_info() == (1, 0)
    got = eng.pareto(n_traces, stat=mixed)  # all-gather over the one-rank communicator + merge
    assert np.array_equal(got, want)
    assert len(got) >= 1


def test_rejects_partial_grids(eng):
    spec = configs.config2_world(n_steps=60)
    sc = configs.config4_scenarios(0, 4, 16)
    run_engine(eng, spec, sc, load=po.gen_load(configs.config4_trace_gen(), 60, 1, 16))
    st = _stat(ref.QUANTILE, 950000)
    assert len(eng.grid_stat(16, st)) == 4
    with pytest.raises(abi.CckaError):
        eng.grid_stat(24, st)
    with pytest.raises(abi.CckaError):
        eng.pareto(24, stat=st)
