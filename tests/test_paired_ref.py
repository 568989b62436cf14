"""CPU-side checks of the paired comparison (docs/SEMANTICS.md 8): the worked
example of the text, the struct sizes behind ccka_paired_sizes, identities of
the restatement (tests/paired_ref.py) on its adversarial columns, and the
activity floors of the two sweeps tests/test_gpu_paired.py runs, computed with
the CPU oracle alone: every sign class of every objective and both dominance
counts are populated, so a device row that came out all zero could not pass."""
import ctypes as C

import numpy as np
import pytest

import paired_ref as ref
import pyoracle as po
from ccka import abi, configs
from sweep_stat_ref import QUANTILE, SUM, TAIL

N_GRIDS, N_TRACES, GRID_LO, BASE, T = 24, 48, 37, 37, 240
GS = (1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 2500)   # the GPU test's grid sizes


def _cols(cost):
    n = len(cost)
    return {"cost_uphmin": np.array(cost, np.int64), "slo_minutes": np.zeros(n, np.int32), "gco2": np.zeros(n),
            "energy_wmin": np.zeros(n)}


def test_worked_example_of_the_text():
    base, cur = _cols([10, 20, 30, 40]), _cols([8, 20, 35, 40])
    p = ref.Prepared(cur, base, 4)
    assert not p.ovf and p.d[0][0] == [-2, 0, 5, 0]
    assert abi.load_engine().ccka_sweep_rank(4, 500000) == 2
    r = p.rows((TAIL,) * 4, (500000,) * 4)[0]
    c = r["obj"][0]
    assert (c["sum"], c["min"], c["max"], c["n_less"], c["n_greater"], c["q_value"]) == (3, -2, 5, 1, 1, 5)
    assert p.rows((QUANTILE,) * 4, (500000,) * 4)[0]["obj"][0]["q_value"] == 0   # x(2)
    assert p.rows()[0]["obj"][0]["q_value"] == 0                                  # SUM: no selection
    assert (r["grid"], r["base"], r["pairs"], r["n_dominates"], r["n_dominated"]) == (0, 0, 4, 1, 1)
    for o in (1, 2, 3):
        assert r["obj"][o].tolist() == (0,) * 6


def test_struct_sizes_and_abi_version():
    assert [C.sizeof(s) for s in abi.PAIRED_STRUCTS] == [48, 48, 232]
    assert abi.paired_dtype().itemsize == 232 and abi.PAIRED_SAME == -1
    lib = abi.load_engine()
    buf = (C.c_int64 * 8)()
    assert lib.ccka_paired_sizes(buf, 8) == 3 and list(buf[:3]) == [48, 48, 232]
    assert lib.ccka_paired_sizes(buf, 2) == 2
    assert lib.ccka_abi_version() == 7 == abi.ABI_VERSION
    big = (C.c_int64 * 32)()
    assert lib.ccka_struct_sizes(big, 32) == 14 == len(abi.STRUCT_ORDER)
    abi.check_sizes(lib)
    sp = abi.paired_spec(48, 37, abi.sweep_stat(slo=("tail", 950000)))
    assert (sp.grid_size, sp.base_grid, list(sp.stat.kind), list(sp.stat.q_ppm)) == (48, 37, [0, 2, 0, 0],
                                                                                     [0, 950000, 0, 0])
    assert abi.paired_spec(7).base_grid == abi.PAIRED_SAME


@pytest.mark.parametrize("g", [1, 2, 65, 257])
def test_identities_of_the_restatement(g):
    cur, base = ref._columns(g, 6, 6)
    # a grid against itself: an all-zero row
    z = ref.Prepared(cur, cur, g).rows((TAIL, QUANTILE, TAIL, QUANTILE), (500000,) * 4)
    assert not z["obj"].view(np.int64).any() and not z["n_dominates"].any() and not z["n_dominated"].any()
    assert z["grid"].tolist() == z["base"].tolist() == list(range(6)) and (z["pairs"] == g).all()
    # swapping the roles negates the sums and swaps the counts
    a, b = ref.Prepared(cur, base, g), ref.Prepared(base, cur, g)
    ra, rb = a.rows(), b.rows()
    assert not a.ovf and not b.ovf
    assert np.array_equal(ra["obj"]["sum"], -rb["obj"]["sum"])
    assert np.array_equal(ra["obj"]["min"], -rb["obj"]["max"])
    assert np.array_equal(ra["obj"]["n_less"], rb["obj"]["n_greater"])
    assert np.array_equal(ra["obj"]["n_greater"], rb["obj"]["n_less"])
    assert np.array_equal(ra["n_dominates"], rb["n_dominated"]) and np.array_equal(ra["n_dominated"], rb["n_dominates"])
    # TAIL from rank 1 is the sum; QUANTILE at 0 and 1e6 are min and max
    assert np.array_equal(a.rows((TAIL,) * 4, (0,) * 4)["obj"]["q_value"], ra["obj"]["sum"])
    assert np.array_equal(a.rows((QUANTILE,) * 4, (0,) * 4)["obj"]["q_value"], ra["obj"]["min"])
    assert np.array_equal(a.rows((QUANTILE,) * 4, (10**6,) * 4)["obj"]["q_value"], ra["obj"]["max"])
    assert not a.rows((SUM,) * 4, (950000,) * 4)["obj"]["q_value"].any()


@pytest.mark.parametrize("g", GS)
def test_no_adversarial_case_overflows(g):
    cur, base = ref._columns(g, 6, 6)
    for base_grid in (0, 1, ref.SAME):
        p = ref.Prepared(cur, base, g, base_grid)
        assert not p.ovf, (g, base_grid)
    # every pattern is drawn, and the cost deltas reach both extremes
    d = ref.Prepared(cur, base, g).d
    assert set(d[3][0]) == {0} and set(d[5][0]) == {-987654321012345}
    assert all(abs(x) <= 1 << 62 for x in d[0][0] + d[4][0])
    if g >= 64:
        assert min(d[0][0]) == -(1 << 62) and max(d[0][0]) == 1 << 62


def test_overflow_is_flagged_by_the_restatement():
    base, cur = _cols([ref.I64_MAX, 0]), _cols([ref.I64_MIN, 0])
    assert ref.Prepared(cur, base, 2).ovf and not ref.Prepared(cur, cur, 2).ovf
    nan = _cols([0, 0])
    nan["gco2"] = np.array([0.0, np.nan])
    assert ref.Prepared(nan, cur, 2).ovf
    big = _cols([0, 0])
    big["energy_wmin"] = np.array([9.3e12, 0.0])
    assert ref.Prepared(cur, big, 2).ovf


# ---- the activity floors of the two GPU sweeps -------------------------------
def sweep_inputs():
    sc = configs.config4_scenarios(GRID_LO, N_GRIDS, N_TRACES)
    load = po.gen_load(configs.config4_trace_gen(), T, 1, N_TRACES)
    return sc, load


def cross_worlds():
    plain = configs.config2_world(n_steps=T)
    plain.start_minute = 900
    disrupt = configs.config2_world(n_steps=T)
    disrupt.start_minute = 900
    disrupt.drift, disrupt.replace = 1, 1
    return plain, disrupt


def _populated(rows, what):
    per, dom = ref.counts(rows)
    print(what, per, "dominates / dominated", dom)
    for f, classes in per.items():
        assert min(classes) >= 1, (what, f, classes)
    assert min(dom) >= 1, (what, dom)
    return per, dom


def test_same_world_sweep_populates_every_class():
    sc, load = sweep_inputs()
    res, _ = po.rollout(configs.config2_world(n_steps=T), sc, load, threads=8)
    rows, ovf = ref.paired(res, res, N_TRACES, BASE, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not ovf
    per, dom = _populated(rows, "same world, baseline grid 37")
    assert sum(per["cost"]) == N_GRIDS * N_TRACES
    assert not rows[BASE - GRID_LO]["obj"].view(np.int64).any()   # the baseline's own row


def test_cross_world_sweep_populates_every_class_and_grid():
    sc, load = sweep_inputs()
    plain, disrupt = cross_worlds()
    r0, _ = po.rollout(plain, sc, load, threads=8)
    r1, _ = po.rollout(disrupt, sc, load, threads=8)
    rows, ovf = ref.paired(r1, r0, N_TRACES, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not ovf and rows["base"].tolist() == rows["grid"].tolist() == list(range(GRID_LO, GRID_LO + N_GRIDS))
    _populated(rows, "drift + replace against plain, SAME")
    # every grid moves on every objective
    active = rows["obj"]["n_less"] + rows["obj"]["n_greater"]
    assert (active >= 1).all(), active
