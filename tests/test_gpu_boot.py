"""GPU checks of the paired bootstrap (docs/SEMANTICS.md 9): the device rows
against the restatement (tests/boot_ref.py), every field equal, then the bytes.

1. ccka_debug_boot on paired_ref._columns(g, 6, 6) (some replicate sums wrap)
   and on the scaled columns (none does), in the three baseline modes: grid
   sizes over the Philox four-word tail, the wave and workgroup edges and the
   staging limit L from both sides; replicate counts over the wave, the LDS key
   limit of the selection and the maximum; quantile pairs; seeds; grid counts
   around the tile width K. L and K come from ccka_debug_boot_limits.
2. A same-world sweep against grid 37: the activity floors of
   tests/test_boot_ref.py on the device rows; obj.sum equals ccka_get_paired's.
3. A cross-world SAME comparison; the snapshot survives.
4. Invariance, byte for byte: workspace passes of 1, 2 and 4 grids, two half
   batches, two calls; another seed moves lo / hi.
5. CCKA_ESTATE, each new CCKA_EINVAL rule, CCKA_EOVERFLOW; the paired rows, the
   sweep statistics and the results are the same bytes after a bootstrap call."""
import ctypes as C

import numpy as np
import pytest

import boot_ref as ref
import paired_ref
import pyoracle as po
from ccka import abi, configs
from ccka.engine import Engine
from parity import oracle, run_engine
from sweep_stat_ref import QUANTILE
from test_boot_ref import B_SWEEP, SEED, cross_world_floors, same_world_floors
from test_paired_ref import BASE, GRID_LO, N_GRIDS, N_TRACES, T, cross_worlds, sweep_inputs

pytestmark = pytest.mark.gpu
THREADS = 16
I64 = np.iinfo(np.int64)
PPM = ((0, 10**6), (25000, 975000), (500000, 500000), (1, 1))
SEEDS = (0, (1 << 64) - 1, SEED)
MODES = (0, 1, ref.SAME)


# sizes relative to the build's staging limit L and tile width K are named here
# and resolved when the test runs (ccka_debug_boot_limits), not at collection
GS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, "L-1", "L", "L+1", 2500)
BS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 2500)
GRID_COUNTS = (1, "K-1", "K", "K+1")


@pytest.fixture(scope="module")
def limits(engine):
    L, K = engine.debug_boot_limits()
    assert K in (1, 2, 4, 8) and 64 <= L <= 4096
    return {"L": L, "K": K}


def _size(v, limits):
    """An int as it is; "L-1", "K+1", ... from the limits (at least 1)."""
    if isinstance(v, int):
        return v
    return max(1, limits[v[0]] + int(v[1:] or 0))


def _both(g, grids=6):
    return (("wrapping", paired_ref._columns(g, grids, grids)), ("scaled", ref.scaled_columns(g, grids, grids)))


# ---- 1. adversarial columns --------------------------------------------------
@pytest.mark.parametrize("g", GS)
def test_grid_sizes(engine, limits, g):
    g = _size(g, limits)
    for name, (cur, base) in _both(g):
        for base_grid in MODES:
            want = ref.Boot(cur, base, g, base_grid)
            assert not want.ovf
            got = engine.debug_boot(cur, base, g, base_grid, 65, SEED)
            ref.equal(got, want.rows(65, SEED), f"{name} g {g} base {base_grid}")


@pytest.mark.parametrize("B", BS)
def test_replicate_counts(engine, B):
    for name, (cur, base) in _both(257):
        for base_grid in MODES:
            want = ref.Boot(cur, base, 257, base_grid).rows(B, SEED)
            got = engine.debug_boot(cur, base, 257, base_grid, B, SEED)
            ref.equal(got, want, f"{name} B {B} base {base_grid}")


def test_the_most_replicates(engine):
    B = abi.BOOT_MAX_REPLICATES
    cur, base = paired_ref._columns(3, 6, 6)
    ref.equal(engine.debug_boot(cur, base, 3, ref.SAME, B, SEED), ref.Boot(cur, base, 3).rows(B, SEED), "B 65536")


@pytest.mark.parametrize("g", [5, 257, 1025])
def test_quantile_pairs_and_seeds(engine, g):
    for name, (cur, base) in _both(g):
        want = ref.Boot(cur, base, g)
        for seed in SEEDS:
            for lo, hi in PPM:
                got = engine.debug_boot(cur, base, g, ref.SAME, 257, seed, lo, hi)
                ref.equal(got, want.rows(257, seed, lo, hi), f"{name} g {g} seed {seed:#x} ppm {lo} {hi}")


@pytest.mark.parametrize("grids", GRID_COUNTS)
def test_grid_counts_around_the_tile(engine, limits, grids):
    grids = _size(grids, limits)
    for g in (65, limits["L"] + 1):
        for name, (cur, base) in _both(g, grids):
            for base_grid in (0, ref.SAME):
                want = ref.Boot(cur, base, g, base_grid).rows(65, SEED)
                ref.equal(engine.debug_boot(cur, base, g, base_grid, 65, SEED), want, f"{name} {grids} grids of {g}")


# ---- 2.-4. on one sweep --------------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
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


def _ref(cur, base, base_grid):
    b = ref.Boot(cur, base, N_TRACES, base_grid, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not b.ovf
    return b


def test_same_world_sweep_against_grid_37(engine, worlds):
    _roll(engine, worlds["same"], worlds)
    engine.paired_capture(N_TRACES)
    got = engine.paired_bootstrap(N_TRACES, BASE, B_SWEEP, SEED)
    rc = worlds["res"]["same"]
    ref.equal(got, _ref(rc, rc, BASE).rows(B_SWEEP, SEED), "same world")
    same_world_floors(got, "device, same world, baseline grid 37")
    assert not got[BASE - GRID_LO]["obj"].view(np.int64).any()
    assert np.array_equal(got["obj"]["sum"], engine.paired(N_TRACES, BASE)["obj"]["sum"])


def test_cross_world_same_and_the_snapshot_survives(engine, worlds):
    _roll(engine, worlds["plain"], worlds)
    engine.paired_capture(N_TRACES)
    _roll(engine, worlds["disrupt"], worlds)   # set_world, set_scenarios, set_load, rollout
    got = engine.paired_bootstrap(N_TRACES, replicates=B_SWEEP, seed=SEED)
    res = worlds["res"]
    ref.equal(got, _ref(res["disrupt"], res["plain"], ref.SAME).rows(B_SWEEP, SEED), "drift + replace against plain")
    cross_world_floors(got, "device, drift + replace against plain, SAME")
    engine.rollout(trajectory=True)
    engine.grid_stat(N_TRACES, abi.sweep_stat(*[(QUANTILE, 950000)] * 4))
    assert engine.paired_bootstrap(N_TRACES, replicates=B_SWEEP, seed=SEED).tobytes() == got.tobytes()


def test_invariance(engine, worlds):
    _roll(engine, worlds["same"], worlds)
    engine.paired_capture(N_TRACES)
    args = (N_TRACES, BASE, B_SWEEP, SEED)
    whole = engine.paired_bootstrap(*args)
    assert engine.paired_bootstrap(*args).tobytes() == whole.tobytes()            # two calls
    try:
        for grids in (1, 2, 4):                                                   # passes of 1, 2, 4 grids
            engine.debug_boot_workspace(grids * 4 * B_SWEEP)
            assert engine.paired_bootstrap(*args).tobytes() == whole.tobytes(), grids
        same = engine.paired_bootstrap(N_TRACES, abi.PAIRED_SAME, B_SWEEP, SEED)
        engine.debug_boot_workspace(3 * 4 * B_SWEEP)
        assert engine.paired_bootstrap(N_TRACES, abi.PAIRED_SAME, B_SWEEP, SEED).tobytes() == same.tobytes()
    finally:
        engine.debug_boot_workspace(0)
    other = engine.paired_bootstrap(N_TRACES, BASE, B_SWEEP, SEED + 1)            # another seed
    assert (other["obj"]["lo"] != whole["obj"]["lo"]).any() or (other["obj"]["hi"] != whole["obj"]["hi"]).any()
    assert np.array_equal(other["obj"]["sum"], whole["obj"]["sum"])
    # two batches of half the grids against the whole batch (the snapshot stays the whole one)
    half = N_GRIDS // 2
    parts = []
    for first in (GRID_LO, GRID_LO + half):
        sc = configs.config4_scenarios(first, half, N_TRACES)
        run_engine(engine, worlds["same"], sc, load=worlds["load"])
        parts.append(engine.paired_bootstrap(*args))
    assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---- 5. errors ------------------------------------------------------------------
@pytest.fixture
def eng():
    e = Engine(0)
    yield e
    e.close()


def _small(e, n_traces=16):
    """Grids 4..7 of 16 positions over 60 steps."""
    spec = configs.config2_world(n_steps=60)
    sc = configs.config4_scenarios(4, 4, n_traces)
    run_engine(e, spec, sc, load=po.gen_load(configs.config4_trace_gen(), 60, 1, n_traces))


def _raises(code, fn, *a, **kw):
    with pytest.raises(abi.CckaError, match=code):
        fn(*a, **kw)


def test_estate(eng):
    _raises("ESTATE", eng.paired_bootstrap, 16)          # before any rollout
    _small(eng)
    _raises("ESTATE", eng.paired_bootstrap, 16)          # before any capture
    eng.paired_capture(16)
    assert len(eng.paired_bootstrap(16, replicates=8)) == 4


def test_einval_rules_and_nothing_else_is_touched(eng):
    _small(eng)
    eng.paired_capture(16)
    st = abi.sweep_stat(*[(QUANTILE, 950000)] * 4)
    paired, stats, res = eng.paired(16, 5, st), eng.grid_stat(16, st), eng.results()
    ok = eng.paired_bootstrap(16, 5, 65, SEED)
    lib, ctx = eng.lib, eng.ctx
    out = np.zeros(8, abi.boot_dtype())
    sp = abi.boot_spec(16, 5, 65, SEED)
    assert lib.ccka_get_paired_bootstrap(ctx, None, out.ctypes.data, 4) == -1   # null arguments
    assert lib.ccka_get_paired_bootstrap(ctx, C.byref(sp), None, 4) == -1
    assert lib.ccka_get_paired_bootstrap(None, C.byref(sp), out.ctypes.data, 4) == -1
    for n_rows in (0, 3, 5):
        assert lib.ccka_get_paired_bootstrap(ctx, C.byref(sp), out.ctypes.data, n_rows) == -1
    for field, bad in (("replicates", 0), ("replicates", -1), ("replicates", 65537), ("lo_ppm", -1),
                       ("hi_ppm", 1000001), ("lo_ppm", 1000001), ("hi_ppm", -1), ("_pad", 1), ("_pad", -1)):
        sp = abi.boot_spec(16, 5, 65, SEED)
        setattr(sp, field, bad)
        assert lib.ccka_get_paired_bootstrap(ctx, C.byref(sp), out.ctypes.data, 4) == -1, (field, bad)
    sp = abi.boot_spec(16, 5, 65, SEED, 500001, 500000)                         # lo_ppm > hi_ppm
    assert lib.ccka_get_paired_bootstrap(ctx, C.byref(sp), out.ctypes.data, 4) == -1
    assert not out.view(np.int64).any()                                         # nothing was written
    # the shape rules of the paired comparison
    for gs in (32, 0, 24, 48):
        _raises("EINVAL", eng.paired_bootstrap, gs, 5)
    for bad in (3, 8, -2, 1 << 40):
        _raises("EINVAL", eng.paired_bootstrap, 16, bad)
    assert len(eng.paired_bootstrap(16, 5, abi.BOOT_MAX_REPLICATES, SEED, 0, 10**6)) == 4
    assert eng.paired_bootstrap(16, 5, 65, SEED).tobytes() == ok.tobytes()
    # the paired rows, the sweep statistics and the results: the same bytes as before
    assert eng.paired(16, 5, st).tobytes() == paired.tobytes()
    assert eng.grid_stat(16, st).tobytes() == stats.tobytes()
    after = eng.results()
    for k, v in res.items():
        assert np.array_equal(after[k], v), k


def _zero(n):
    return {"cost_uphmin": np.zeros(n, np.int64), "slo_minutes": np.zeros(n, np.int32), "gco2": np.zeros(n),
            "energy_wmin": np.zeros(n)}


@pytest.mark.parametrize("g", [65, 1025])
def test_eoverflow_is_an_error_return(engine, g):
    good_cur, good_base = paired_ref._columns(g, 2, 2)
    want = ref.Boot(good_cur, good_base, g).rows(65, SEED)
    cases = []
    cur, base = _zero(2 * g), _zero(2 * g)
    cur["gco2"][g + 3] = np.nan                                                 # a NaN gCO2
    cases.append(("nan", cur, base))
    cur, base = _zero(2 * g), _zero(2 * g)
    cur["cost_uphmin"][2 * g - 1], base["cost_uphmin"][2 * g - 1] = I64.min, I64.max   # a delta that leaves int64
    cases.append(("sub", cur, base))
    for what, cur, base in cases:
        assert ref.Boot(cur, base, g).ovf, what
        _raises("EOVERFLOW", engine.debug_boot, cur, base, g, ref.SAME, 65, SEED)
        ref.equal(engine.debug_boot(good_cur, good_base, g, ref.SAME, 65, SEED), want, f"after {what}")
