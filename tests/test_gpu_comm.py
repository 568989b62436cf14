"""The RCCL exchange paths of libccka on one GPU: a one-rank
communicator through ccka_comm_unique_id / ccka_comm_init, the totals
all-reduce, the Pareto all-gather + merge, and the cross-rank merge itself on
synthetic multi-rank exchange buffers, each against the single-rank result or
the numpy restatement of the frontier (oracle/pyoracle.py)."""
import numpy as np
import pytest

import pyoracle as po
from ccka import abi, configs
from ccka.engine import GRID_DTYPE, Engine
from parity import run_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_comm_state_errors_before_init(eng):
    with pytest.raises(abi.CckaError):
        eng.comm_info()
    with pytest.raises(abi.CckaError):
        eng.allreduce_totals(abi.Totals())


def test_one_rank_allreduce_is_identity(eng):
    spec = configs.config2_world(n_steps=240)
    sc = configs.hpa_scenarios(3000, first_id=777)
    run_engine(eng, spec, sc, gen=configs.trace_gen())
    t = eng.totals()
    eng.comm_init()
    assert eng.comm_info() == (1, 0)
    got = eng.allreduce_totals(t)
    for f, _ in abi.Totals._fields_:
        assert getattr(got, f) == getattr(t, f), f
    assert got.scenarios == 3000


def test_pareto_with_communicator_equals_local(eng):
    n_traces = 16
    spec = configs.config2_world(n_steps=360)
    sc = configs.config4_scenarios(40, 48, n_traces)
    load = po.gen_load(configs.config4_trace_gen(), 360, 1, n_traces)
    fresh = Engine(0)  # no communicator: the local frontier
    try:
        run_engine(fresh, spec, sc, load=load)
        want = fresh.pareto(n_traces)
    finally:
        fresh.close()
    run_engine(eng, spec, sc, load=load)
    if not eng.lib.ccka_comm_info(eng.ctx, None, None) == 0:
        eng.comm_init()
    got = eng.pareto(n_traces)  # all-gather over the one-rank communicator + merge
    assert np.array_equal(got, want)
    stats = eng.grid_stats(n_traces)
    assert np.array_equal(got, stats[po.pareto({k: stats[k] for k in stats.dtype.names})])


def _random_grids(rng, g0, n):
    a = np.zeros(n, GRID_DTYPE)
    a["grid"] = np.arange(g0, g0 + n)
    a["scenarios"] = 16
    a["cost_uphmin"] = rng.integers(0, 40, n)
    a["slo_minutes"] = rng.integers(0, 40, n)
    a["gco2"] = rng.integers(0, 40, n).astype(np.float64) * 0.5
    a["energy_wmin"] = rng.random(n)
    return a


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_cross_rank_merge_equals_frontier_of_concatenation(eng, nranks):
    rng = np.random.default_rng(nranks)
    cap = 64
    rows = [_random_grids(rng, q * cap, cap) for q in range(nranks)]
    gathered = np.zeros((nranks, cap), GRID_DTYPE)
    counts = []
    for q, r in enumerate(rows):  # each rank contributes its local frontier
        loc = r[po.pareto({k: r[k] for k in r.dtype.names})]
        gathered[q, :len(loc)] = loc
        gathered[q, len(loc):]["grid"] = -1  # garbage beyond the count must be ignored
        counts.append(len(loc))
    got = eng.debug_pareto_merge(gathered, counts)
    allg = np.concatenate(rows)
    want = allg[po.pareto({k: allg[k] for k in allg.dtype.names})]
    assert np.array_equal(got, want)
    assert np.all(np.diff(got["grid"]) > 0)


def test_cross_rank_merge_keeps_all_when_nothing_dominates(eng):
    # every candidate of every rank survives: the frontier is larger than one
    # rank's grid count (the global buffer holds nranks x grids)
    nranks, cap = 4, 8
    g = np.zeros((nranks, cap), GRID_DTYPE)
    k = np.arange(nranks * cap)
    g["grid"] = k.reshape(nranks, cap)
    g["cost_uphmin"] = k.reshape(nranks, cap)
    g["slo_minutes"] = (nranks * cap - k).reshape(nranks, cap)
    got = eng.debug_pareto_merge(g, [cap] * nranks)
    assert len(got) == nranks * cap
    with pytest.raises(abi.CckaError):
        eng.debug_pareto_merge(g, [cap] * nranks, capacity=cap)


def _diagonal_grids(rng, n, noise):
    """n candidates along an anti-diagonal of (cost, SLO): with noise 0 none
    dominates another; with noise neighbours do, all along the diagonal."""
    a = _random_grids(rng, 0, n)
    k = np.arange(n)
    a["cost_uphmin"] = 4 * k + (rng.integers(0, noise, n) if noise else 0)
    a["slo_minutes"] = 4 * (n - k) + (rng.integers(0, noise, n) if noise else 0)
    a["gco2"] = rng.integers(0, 3, n).astype(np.float64) * 0.5 if noise else 1.0
    return a


# pareto_compact_kernel writes the survivors in chunks of 1024 candidates with
# a running base: one chunk exactly, one entry into the second, and three chunks
@pytest.mark.parametrize("case", ["all_2500", "random_2500", "n1024", "n1025", "duplicates"])
def test_merge_compaction_beyond_one_chunk(eng, case):
    rng = np.random.default_rng(len(case))
    if case == "all_2500":
        allg = _diagonal_grids(rng, 2500, 0)
    elif case == "random_2500":
        allg = _diagonal_grids(rng, 2500, 12)
    elif case == "duplicates":  # equal rows: neither dominates the other, both stay
        allg = _diagonal_grids(rng, 1300, 12)
        allg[1::2] = allg[0::2]
        allg["grid"] = np.arange(len(allg))
    else:
        allg = _diagonal_grids(rng, int(case[1:]), 12)
    n = len(allg)
    keep = po.pareto({k: allg[k] for k in allg.dtype.names})
    want = allg[keep]
    if case == "all_2500":
        assert len(want) == n
    else:  # survivors and casualties in every chunk of 1024 candidates
        for c0 in range(0, n, 1024):
            inside = int(((keep >= c0) & (keep < c0 + 1024)).sum())
            assert 0 < inside and (inside < min(1024, n - c0) or n - c0 == 1), (case, c0, inside)
    if case == "duplicates":
        assert np.all(np.isin(keep[keep % 2 == 0] + 1, keep))
    nranks = 2 if n % 2 == 0 else 1
    got = eng.debug_pareto_merge(allg.reshape(nranks, n // nranks), [n // nranks] * nranks)
    assert np.array_equal(got, want), (case, len(got), len(want))
    assert np.all(np.diff(got["grid"]) > 0)
