"""GPU checks of the paired comparison (docs/SEMANTICS.md 8): the device rows
against the Python-int restatement (tests/paired_ref.py), every field equal.

1. ccka_debug_paired on adversarial columns (six grids, so every cost pattern of
   paired_ref._columns is drawn) at the wave edge, the workgroup stride, the LDS
   staging limit from both sides and several trips, for every kind, five
   quantiles and the three baseline modes.
2. A same-world sweep: rollout, capture, paired against global grid 37.
3. A cross-world SAME comparison: the snapshot survives set_world,
   set_scenarios, a new load and a rollout.
4. Export / import of one snapshot grid into a second context.
5. CCKA_ESTATE, every CCKA_EINVAL rule that is cheap to reach, CCKA_EOVERFLOW.
6. Determinism, and the sweep statistics untouched by a paired call.
tests/test_paired_ref.py shows on the CPU oracle that the sweeps of 2 and 3
populate every sign class, so an all-zero device row cannot pass."""
import ctypes as C

import numpy as np
import pytest

import paired_ref as ref
import pyoracle as po
from ccka import abi, configs
from ccka.engine import Engine
from parity import oracle, run_engine
from sweep_stat_ref import QUANTILE, SUM, TAIL
from test_paired_ref import BASE, GRID_LO, GS, N_GRIDS, N_TRACES, T, cross_worlds, sweep_inputs

pytestmark = pytest.mark.gpu
THREADS = 16
QS = (0, 1, 500000, 950000, 10**6)
MIXED = (SUM, QUANTILE, TAIL, SUM)
KINDS = {"quantile": (QUANTILE,) * 4, "tail": (TAIL,) * 4, "mixed": MIXED}
I64 = np.iinfo(np.int64)


def _stat(kinds, qs):
    return abi.sweep_stat(*zip(kinds, qs))


# ---- 1. adversarial columns --------------------------------------------------
@pytest.mark.parametrize("g", GS)
def test_debug_paired_on_adversarial_columns(engine, g):
    cur, base = ref._columns(g, 6, 6)
    for base_grid in (0, 1, ref.SAME):
        want = ref.Prepared(cur, base, g, base_grid)
        assert not want.ovf
        for name, kinds in KINDS.items():
            for q in QS:
                got = engine.debug_paired(cur, base, g, base_grid, _stat(kinds, (q,) * 4))
                ref.equal(got, want.rows(kinds, (q,) * 4), f"g {g} base {base_grid} {name} q {q}")
    sums = engine.debug_paired(cur, base, g)   # no statistic: every q_value is 0
    ref.equal(sums, ref.Prepared(cur, base, g).rows(), f"g {g} all SUM")


# ---- 2.-4., 6. on one sweep --------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
    """The scenarios, the load, the plain and disrupted worlds of the cross-world
    case and the oracle's results of all three rollouts, computed once."""
    sc, load = sweep_inputs()
    same = configs.config2_world(n_steps=T)
    plain, disrupt = cross_worlds()
    res = {k: oracle(w, sc, load, threads=THREADS)[0] for k, w in
           (("same", same), ("plain", plain), ("disrupt", disrupt))}
    for r in res.values():
        for a in r.values():
            a.setflags(write=False)
    return dict(sc=sc, load=load, same=same, plain=plain, disrupt=disrupt, res=res)


def _roll(eng, spec, w):
    run_engine(eng, spec, w["sc"], load=w["load"])


def _ref_rows(cur, base, base_grid, kinds, qs):
    rows, ovf = ref.paired(cur, base, N_TRACES, base_grid, kinds, qs, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not ovf
    return rows


@pytest.mark.parametrize("name", list(KINDS))
def test_same_world_sweep_against_grid_37(engine, worlds, name):
    _roll(engine, worlds["same"], worlds)
    engine.paired_capture(N_TRACES)
    kinds, qs = KINDS[name], (950000,) * 4
    got = engine.paired(N_TRACES, BASE, _stat(kinds, qs))
    rc = worlds["res"]["same"]
    ref.equal(got, _ref_rows(rc, rc, BASE, kinds, qs), f"same world {name}")
    own = got[BASE - GRID_LO]
    assert not own["obj"].view(np.int64).any() and own["n_dominates"] == 0 == own["n_dominated"]
    per, dom = ref.counts(got)
    assert min(min(c) for c in per.values()) >= 1 and min(dom) >= 1


def test_cross_world_same_and_the_snapshot_survives(engine, worlds):
    _roll(engine, worlds["plain"], worlds)
    engine.paired_capture(N_TRACES)
    _roll(engine, worlds["disrupt"], worlds)   # set_world, set_scenarios, set_load, rollout
    kinds, qs = MIXED, (500000,) * 4
    got = engine.paired(N_TRACES, stat=_stat(kinds, qs))
    res = worlds["res"]
    ref.equal(got, _ref_rows(res["disrupt"], res["plain"], ref.SAME, kinds, qs), "drift + replace against plain")
    assert ((got["obj"]["n_less"] + got["obj"]["n_greater"]) >= 1).all()
    # and a rollout with a trajectory, then the sweep statistics, leave it alone too
    engine.rollout(trajectory=True)
    engine.grid_stat(N_TRACES, _stat((QUANTILE,) * 4, (950000,) * 4))
    assert engine.paired(N_TRACES, stat=_stat(kinds, qs)).tobytes() == got.tobytes()


def test_export_and_import_into_a_second_context(engine, worlds):
    _roll(engine, worlds["same"], worlds)
    engine.paired_capture(N_TRACES)
    blk = engine.paired_export(40)
    assert blk.shape == (4, N_TRACES) and blk.dtype == np.int64
    assert np.array_equal(blk, ref.block(worlds["res"]["same"], N_TRACES, 40 - GRID_LO))
    st = _stat((TAIL,) * 4, (950000,) * 4)
    want = engine.paired(N_TRACES, 40, st)
    other = Engine(0)
    try:
        _roll(other, worlds["same"], worlds)
        other.paired_import(N_TRACES, N_TRACES, 40, blk)
        got = other.paired(N_TRACES, 40, st)
        assert np.array_equal(other.paired_export(40), blk)
    finally:
        other.close()
    assert got.tobytes() == want.tobytes()
    assert (got["base"] == 40).all() and not got[40 - GRID_LO]["obj"].view(np.int64).any()


def test_deterministic_and_leaves_the_sweep_statistics(engine, worlds):
    _roll(engine, worlds["same"], worlds)
    engine.paired_capture(N_TRACES)
    st = _stat((TAIL,) * 4, (950000,) * 4)
    sums = engine.grid_stats(N_TRACES)
    a = engine.paired(N_TRACES, BASE, st)
    assert engine.grid_stats(N_TRACES).tobytes() == sums.tobytes()
    b = engine.paired(N_TRACES, BASE, st)
    assert a.tobytes() == b.tobytes()
    res = engine.results()
    for k, v in worlds["res"]["same"].items():
        assert np.array_equal(res[k], v), k   # the results are untouched


# ---- 5. errors ----------------------------------------------------------------
@pytest.fixture
def eng():
    e = Engine(0)
    yield e
    e.close()


def _small(e, n_traces=16):
    """Grids 4..7 of 16 positions (also whole grids of 32 and 64) over 60 steps."""
    spec = configs.config2_world(n_steps=60)
    sc = configs.config4_scenarios(4, 4, n_traces) if n_traces else configs.hpa_scenarios(64, first_id=64)
    run_engine(e, spec, sc, load=po.gen_load(configs.config4_trace_gen(), 60, 1, n_traces or 64))


def _raises(code, fn, *a, **kw):
    with pytest.raises(abi.CckaError, match=code):
        fn(*a, **kw)


def test_estate(eng):
    _raises("ESTATE", eng.paired, 16)                 # before any rollout
    _raises("ESTATE", eng.paired_capture, 16)
    eng._paired_gs = 16
    _raises("ESTATE", eng.paired_export, 4)
    _small(eng)
    _raises("ESTATE", eng.paired, 16)                 # before any capture
    _raises("ESTATE", eng.paired_export, 4)
    eng.paired_capture(16)
    assert len(eng.paired(16)) == 4


def test_einval_rules(eng):
    _small(eng)
    eng.paired_capture(16)
    ok = eng.paired(16, 5, _stat((TAIL,) * 4, (500000,) * 4))
    lib, ctx = eng.lib, eng.ctx
    out = np.zeros(8, abi.paired_dtype())
    sp = abi.paired_spec(16, 5)
    assert lib.ccka_get_paired(ctx, None, out.ctypes.data, 4) == -1            # null arguments
    assert lib.ccka_get_paired(ctx, C.byref(sp), None, 4) == -1
    assert lib.ccka_get_paired(None, C.byref(sp), out.ctypes.data, 4) == -1
    assert lib.ccka_paired_capture(None, 16) == -1
    assert lib.ccka_paired_export(ctx, 5, None, 64) == -1
    assert lib.ccka_paired_import(ctx, 16, 16, 5, None, 64) == -1
    for n_rows in (0, 3, 5):                                                   # a wrong n_rows
        assert lib.ccka_get_paired(ctx, C.byref(sp), out.ctypes.data, n_rows) == -1
    assert lib.ccka_get_paired(ctx, C.byref(sp), out.ctypes.data, 4) == 0
    _raises("EINVAL", eng.paired, 32)                  # whole grids, but not the snapshot's grid_size
    _raises("EINVAL", eng.paired, 0)
    _raises("EINVAL", eng.paired, 24)                  # 24 mod n_traces != 0
    _raises("EINVAL", eng.paired, 48)                  # a batch without whole grids
    for bad in (3, 8, -2, 1 << 40):                    # base_grid outside the snapshot
        _raises("EINVAL", eng.paired, 16, bad)
    _raises("EINVAL", eng.paired, 16, 5, abi.sweep_stat(cost=(3, 0)))
    _raises("EINVAL", eng.paired, 16, 5, abi.sweep_stat(slo=(-1, 0)))
    _raises("EINVAL", eng.paired, 16, 5, abi.sweep_stat(gco2=("quantile", -1)))
    _raises("EINVAL", eng.paired, 16, 5, abi.sweep_stat(energy=("tail", 1000001)))
    assert len(eng.paired(16, 5, abi.sweep_stat(cost=("sum", -5)))) == 4   # q_ppm is ignored for SUM
    _raises("EINVAL", eng.paired_capture, 24)
    _raises("EINVAL", eng.paired_capture, 48)
    _raises("EINVAL", eng.paired_capture, 0)
    blk = eng.paired_export(5)
    for grid in (3, 8, -1):                            # export: a grid outside, a wrong count
        _raises("EINVAL", eng.paired_export, grid)
    assert lib.ccka_paired_export(ctx, 5, blk.ctypes.data, 63) == -1
    # argument errors left the snapshot alone
    assert eng.paired(16, 5, _stat((TAIL,) * 4, (500000,) * 4)).tobytes() == ok.tobytes()
    # import: its own rules, then a one-grid snapshot
    _raises("EINVAL", eng.paired_import, 16, 0, 5, blk)     # n_traces == 0
    _raises("EINVAL", eng.paired_import, 16, 5, 5, blk)     # 16 mod 5 != 0
    _raises("EINVAL", eng.paired_import, 16, 16, -1, blk)
    _raises("EINVAL", eng.paired_import, 16, 16, 5, blk[:3])  # a wrong count
    _raises("EINVAL", eng.paired_import, 0, 16, 5, blk)
    eng.paired_import(16, 16, 5, blk)
    assert eng.paired(16, 5, _stat((TAIL,) * 4, (500000,) * 4)).tobytes() == ok.tobytes()
    _raises("EINVAL", eng.paired, 16)                  # SAME: grids 4..7 are not all inside [5, 6)
    _raises("EINVAL", eng.paired, 16, 4)
    eng.paired_import(16, 8, 5, blk)                   # the snapshot's n_traces differs
    _raises("EINVAL", eng.paired, 16, 5)
    eng.paired_capture(16)
    assert eng.paired(16, 5, _stat((TAIL,) * 4, (500000,) * 4)).tobytes() == ok.tobytes()
    # per-scenario traces (n_traces == 0): no pairing
    _small(eng, n_traces=0)
    _raises("EINVAL", eng.paired_capture, 16)
    _raises("EINVAL", eng.paired, 16, 5)
    _small(eng)
    assert eng.paired(16, 5, _stat((TAIL,) * 4, (500000,) * 4)).tobytes() == ok.tobytes()   # the snapshot is still there


def _zero(n):
    return {"cost_uphmin": np.zeros(n, np.int64), "slo_minutes": np.zeros(n, np.int32), "gco2": np.zeros(n),
            "energy_wmin": np.zeros(n)}


@pytest.mark.parametrize("g", [65, 1025])
def test_eoverflow_is_an_error_return(engine, g):
    good_cur, good_base = ref._columns(g, 2, 2)
    st = _stat((QUANTILE,) * 4, (500000,) * 4)
    want = ref.Prepared(good_cur, good_base, g).rows((QUANTILE,) * 4, (500000,) * 4)
    cases = []
    cur, base = _zero(2 * g), _zero(2 * g)
    cur["gco2"][g + 3] = np.nan                    # NaN in the current columns
    cases.append(("nan", cur, base))
    cur, base = _zero(2 * g), _zero(2 * g)
    base["energy_wmin"][g - 1] = 9.3e12                # no fixed-point form in the baseline columns
    cases.append(("9.3e12", cur, base))
    cur, base = _zero(2 * g), _zero(2 * g)
    cur["cost_uphmin"][2 * g - 1], base["cost_uphmin"][2 * g - 1] = I64.min, I64.max   # the subtraction
    cases.append(("sub", cur, base))
    for what, cur, base in cases:
        assert ref.Prepared(cur, base, g).ovf, what
        _raises("EOVERFLOW", engine.debug_paired, cur, base, g, ref.SAME, st)
        ref.equal(engine.debug_paired(good_cur, good_base, g, ref.SAME, st), want, f"after {what}")
