"""GPU checks of the fleet timeline (docs/SEMANTICS.md 7): the device reduction
of trajectory records per (grid, step bucket) against the numpy restatement
(tests/timeline_ref.py).

1. Synthetic records through ccka_debug_timeline, every case in both device
   layouts on the same logical data: the rows equal the restatement field for
   field, and the two layouts' rows equal each other. The select kernel stages
   nothing on chip (every pass re-reads the records), so there is no staging
   limit to straddle and the issue's two cases for one are not drawn.
2. Real rollouts on every engine that writes records, the worlds of
   tests/test_gpu_random_worlds.py: the timeline equals the restatement of
   engine.trajectory(), and summed over the buckets it equals
   engine.results() through the five identities tests/test_timeline_ref.py
   asserts on the oracle for the same worlds (none is dropped: all hold
   there). The generator draws any first_id; timeline_ref.world moves each
   batch to a multiple of its size, a different one per seed. Config 2 runs
   588 scenarios, which 130, 65 and 13 do not divide; its specs are the same
   four shapes at grid sizes 588, 294, 12 and 1.
3. State: repeated and shrinking specs, the records untouched, CCKA_ESTATE and
   every CCKA_EINVAL rule a rollout can reach. The 2^31 bound and the 2^24-row
   cap need more scenarios than a test holds: tests/test_timeline_ref.py holds
   ccka_timeline_rows to them, the function ccka_get_timeline validates with."""
import numpy as np
import pytest

import random_worlds as rw
import timeline_ref as ref
from ccka import abi, configs
from ccka.world import TRAJ_DTYPE
from parity import oracle

pytestmark = pytest.mark.gpu
THREADS = 16
I32 = np.iinfo(np.int32)
QS = (0, 1, 500000, 950000, 999999, 10**6)
FIELDS = (ref.REPLICAS, ref.PENDING, ref.NODES)

# (N, T, G, B)
SHAPES = [(147, 61, 49, 1), (147, 61, 49, 7), (147, 61, 147, 61), (147, 61, 49, 100), (147, 61, 1, 1),
          (130, 129, 65, 64), (1, 1, 1, 1), (65539, 3, 65539, 3)]


def _random(rng, T, N):
    a = np.zeros((T, N), TRAJ_DTYPE)
    a["replicas"] = rng.integers(0, 5000, (T, N))
    a["pending"] = rng.integers(0, 300, (T, N))
    a["nodes_spot"] = rng.integers(0, 17, (T, N))
    a["nodes_od"] = rng.integers(0, 17, (T, N))
    a["last_type"] = rng.integers(0, 1 << 16, (T, N))
    a["flags"] = rng.integers(0, 128, (T, N))
    return a


def _ties(rng, T, N):
    a = _random(rng, T, N)
    a["pending"] = np.where(rng.random((T, N)) < 0.97, 0, a["pending"])
    a["replicas"] = rng.integers(3, 6, (T, N))
    a["nodes_od"] = 0
    return a


def _extreme(rng, T, N):
    a = np.zeros((T, N), TRAJ_DTYPE)
    pool = np.array([0, 1, I32.max], np.int32)
    a["replicas"] = pool[rng.integers(0, 3, (T, N))]
    a["pending"] = pool[rng.integers(0, 3, (T, N))]
    a["nodes_spot"] = 65535
    a["nodes_od"] = 65535
    a["last_type"] = rng.integers(0, 1 << 16, (T, N))
    a["flags"] = rng.integers(0, 1 << 16, (T, N))  # bits 8..15 must not be counted
    return a


def _signed(rng, T, N):
    a = _random(rng, T, N)
    a["replicas"] = np.array([I32.min, -1, 0, 5], np.int32)[rng.integers(0, 4, (T, N))]
    return a


DATA = {"random": _random, "ties": _ties, "extreme": _extreme, "signed": _signed}


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, f"{what}: {f} differs at (grid, bucket[, bit]) {bad[:5].tolist()}: " \
                              f"got {got[f][tuple(bad[0])]} want {want[f][tuple(bad[0])]}"


def _both_layouts(engine, recs, G, B, q_field=ref.NONE, q_ppm=0, what=""):
    """The rows of [T][N] records `recs` from both device layouts, checked
    against the restatement and each other."""
    tn = engine.debug_timeline(recs, abi.TRAJ_TN, G, B, q_field, q_ppm)
    nt = engine.debug_timeline(np.ascontiguousarray(recs.T), abi.TRAJ_NT, G, B, q_field, q_ppm)
    want = ref.timeline(recs, G, B, q_field, q_ppm)
    _equal(tn, want, f"{what} layout TN")
    _equal(nt, want, f"{what} layout NT")
    assert tn.tobytes() == nt.tobytes(), what
    return want


@pytest.mark.parametrize("kind", list(DATA))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_synthetic_records_in_both_layouts(engine, shape, kind):
    N, T, G, B = shape
    rng = np.random.default_rng([N, T, G, B, list(DATA).index(kind)])
    recs = DATA[kind](rng, T, N)
    what = f"{kind} {shape}"
    sums = _both_layouts(engine, recs, G, B, what=what)
    assert int(sums["samples"].sum()) == N * T
    big = N * T > 50000  # one quantile per field on the large shape, all six elsewhere
    for f in FIELDS:
        for q in (QS[3:4] if big else QS):
            got = _both_layouts(engine, recs, G, B, f, q, what=f"{what} field {f} q {q}")
            # always an input value, and the other fields are the sums-only rows
            vals = ref.field(recs, f)
            assert np.isin(got["q_value"], vals).all(), what
            for name in sums.dtype.names:
                if name != "q_value":
                    assert np.array_equal(got[name], sums[name]), (what, name)


def test_wrap_int32_max_in_every_sample(engine):
    """G * B = 2989 samples of replicas = INT32_MAX: a 32-bit partial wraps after two."""
    N, T, G, B = 61, 98, 61, 49
    recs = _random(np.random.default_rng(2989), T, N)
    recs["replicas"] = I32.max
    want = _both_layouts(engine, recs, G, B, ref.REPLICAS, 500000, what="wrap")
    assert G * B == 2989 and (want["sum_replicas"] == 2989 * I32.max).all() and (want["q_value"] == I32.max).all()


def test_extreme_nodes_reach_131070(engine):
    recs = _extreme(np.random.default_rng(7), 61, 147)
    got = _both_layouts(engine, recs, 49, 7, ref.NODES, 950000, what="extreme nodes")
    assert (got["max_nodes"] == 131070).all() and (got["min_nodes"] == 131070).all() and (got["q_value"] == 131070).all()
    assert (got["flag_count"] <= got["samples"][..., None]).all()


# ---- 2. real rollouts -------------------------------------------------------
def _identities(rows, res, G, what):
    """The rows, summed over the buckets (max_nodes: maxed), against the results per grid."""
    ng = rows.shape[0]
    per_grid = lambda f: res[f].astype(np.int64).reshape(ng, G).sum(axis=1)  # noqa: E731
    assert np.array_equal(rows["sum_pending"].sum(axis=1), per_grid("pending_pod_minutes")), what
    assert np.array_equal(rows["sum_nodes_spot"].sum(axis=1), per_grid("node_min_spot")), what
    assert np.array_equal(rows["sum_nodes_od"].sum(axis=1), per_grid("node_min_od")), what
    assert np.array_equal(rows["flag_count"][:, :, 3].sum(axis=1), per_grid("slo_minutes")), what
    # a grid's largest sample is its scenarios' largest peak (G = 1: the scenario's own)
    assert np.array_equal(rows["max_nodes"].max(axis=1), res["peak_nodes"].reshape(ng, G).max(axis=1)), what


def _check_rollout(engine, specs, first_id=0, what=""):
    res, tr = engine.results(), engine.trajectory()
    for G, B in specs:
        got = engine.timeline(G, B, ref.NODES, 950000)
        _equal(got, ref.timeline(tr, G, B, ref.NODES, 950000, first_id), f"{what} G {G} B {B}")
        _identities(got, res, G, f"{what} G {G} B {B}")
    return res, tr


def _specs(n, T):
    return [(n, 1), (n // 2, 60), (13 if n % 13 == 0 else 12, 7), (1, T)]


# profile -> (ccka_debug_engine mode, engine that must run, layout)
ROLLOUTS = {"d1_default": (0, 2, abi.TRAJ_NT), "d1_disrupt": (0, 2, abi.TRAJ_NT), "gk_multi": (0, 1, abi.TRAJ_TN),
            "sk": (0, 5, abi.TRAJ_NT)}


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("profile", list(ROLLOUTS))
def test_rollout_timeline_matches_trajectory_and_results(engine, profile, seed):
    mode, want_engine, want_layout = ROLLOUTS[profile]
    spec, sc, load = ref.world(profile, seed)
    engine.set_engine(mode)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.rollout(trajectory=True)
    what = f"profile {profile} seed {seed}"
    assert engine.last_engine()[0] == want_engine, what
    assert engine.trajectory_native()[1] == want_layout, what
    _, tr = _check_rollout(engine, _specs(sc.n, spec.n_steps), sc.first_id, what=what)
    # the records are untouched: still the oracle's
    _, tc = oracle(spec, sc, load, traj=True, threads=THREADS)
    assert np.array_equal(engine.trajectory(), tc) and np.array_equal(tr, tc), what


@pytest.mark.parametrize("seed", [0, 1])
def test_closed_loop_timeline(engine, seed):
    spec, sc, load = ref.world("loop", seed)
    ws, bs = configs.mlp_weights(seed)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
    engine.policy_rollout(trajectory=True)
    assert engine.last_engine()[0] == 4
    assert engine.trajectory_native()[1] == abi.TRAJ_TN
    _check_rollout(engine, _specs(sc.n, spec.n_steps), sc.first_id, what=f"loop seed {seed}")


def test_config2_day_with_peak_window(engine):
    spec = configs.config2_world(n_steps=1440)
    sc = configs.hpa_scenarios(588)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.gen_load(configs.trace_gen())
    engine.rollout(trajectory=True)
    assert engine.last_engine()[0] == 2 and engine.trajectory_native()[1] == abi.TRAJ_NT
    _check_rollout(engine, _specs(588, 1440), what="config 2")
    hourly = engine.timeline(588, 60)
    peak = hourly["flag_count"][0, :, 0]
    assert peak.max() > 0 and peak.min() == 0  # the PEAK bit shows up in some hours only


def test_first_id_offsets_the_grid_ids(engine):
    spec, sc, load = rw.draw("d1_default", 0)
    G = 65
    sc.first_id = 3 * G
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.rollout(trajectory=True)
    got = engine.timeline(G, 60, ref.NODES, 950000)
    assert got["grid"][:, 0].tolist() == [3, 4]
    _equal(got, ref.timeline(engine.trajectory(), G, 60, ref.NODES, 950000, first_id=3 * G), "first_id")
    with pytest.raises(abi.CckaError, match="EINVAL"):
        engine.timeline(2 * G, 60)  # first_id = 3 G holds no whole grid of 2 G


# ---- 3. state ---------------------------------------------------------------
@pytest.fixture
def small_run(engine):
    spec, sc, load = ref.world("d1_default", 1)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.rollout(trajectory=True)
    return spec, sc, load


def test_repeated_and_shrinking_specs(engine, small_run):
    spec, sc, load = small_run
    tr = engine.trajectory()
    a = engine.timeline(1, 1, ref.PENDING, 999999)       # the largest row buffer
    b = engine.timeline(1, 1, ref.PENDING, 999999)
    assert a.tobytes() == b.tobytes()
    small = engine.timeline(sc.n, spec.n_steps)           # one row in the same buffer: no stale sums
    _equal(small, ref.timeline(tr, sc.n, spec.n_steps, first_id=sc.first_id), "after a larger spec")
    _equal(engine.timeline(65, 7, ref.REPLICAS, 0), ref.timeline(tr, 65, 7, ref.REPLICAS, 0, sc.first_id),
           "then a quantile")
    _equal(engine.timeline(65, 7), ref.timeline(tr, 65, 7, first_id=sc.first_id), "then none: q_value is 0 again")
    _, tc = oracle(spec, sc, load, traj=True, threads=THREADS)
    assert np.array_equal(engine.trajectory(), tc)


def test_estate_without_a_trajectory(engine, small_run):
    from ccka.engine import Engine
    fresh = Engine(0)
    try:
        with pytest.raises(abi.CckaError, match="ESTATE"):
            fresh.timeline(1)
    finally:
        fresh.close()
    engine.rollout(trajectory=False)
    with pytest.raises(abi.CckaError, match="ESTATE"):
        engine.timeline(small_run[1].n)
    with pytest.raises(abi.CckaError, match="ESTATE"):
        engine.trajectory()


def test_einval_rules(engine, small_run):
    import ctypes as C
    spec, sc, _ = small_run
    n, T = sc.n, spec.n_steps
    bad = [dict(grid_size=7), dict(grid_size=0), dict(grid_size=n, step_bucket=0),
           dict(grid_size=n, q_field=4), dict(grid_size=n, q_field=-1),
           dict(grid_size=n, q_field=ref.NODES, q_ppm=-1), dict(grid_size=n, q_field=ref.NODES, q_ppm=1000001)]
    for kw in bad:
        with pytest.raises(abi.CckaError, match="EINVAL"):
            engine.timeline(**kw)
    assert engine.timeline(n, T, ref.NONE, -5).shape == (1, 1)  # q_ppm is ignored for NONE
    out = np.zeros(4, abi.timeline_dtype())
    ok = abi.timeline_spec(n, T)
    lib = engine.lib
    assert lib.ccka_get_timeline(engine.ctx, None, out.ctypes.data, 1) == -1          # null spec
    assert lib.ccka_get_timeline(engine.ctx, C.byref(ok), out.ctypes.data, 2) == -1   # another n_rows
    assert lib.ccka_get_timeline(engine.ctx, C.byref(ok), out.ctypes.data, 0) == -1
    assert lib.ccka_get_timeline(engine.ctx, C.byref(ok), out.ctypes.data, 1) == 0
    assert out["samples"][0] == n * T and (out["samples"][1:] == 0).all()
