"""CPU-side checks of the fleet timeline (docs/SEMANTICS.md 7): the numpy
restatement (tests/timeline_ref.py) against a plain-Python triple loop; the
five identities that tie a timeline to the rollout results, on the CPU
oracle's own trajectories of the worlds tests/test_gpu_timeline.py runs (all
five hold on every one of them, so the GPU test drops none); and
ccka_timeline_rows with the struct sizes, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
import timeline_ref as ref
from ccka import abi, configs
from ccka.world import TRAJ_DTYPE
from sweep_stat_ref import rank

WORLDS = [(p, s) for p in ("d1_default", "d1_disrupt", "gk_multi", "sk") for s in (0, 1)]


def _loops(recs, G, B, q_field, q_ppm, first_id=0):
    """SEMANTICS 7 word for word, one sample at a time."""
    T, N = recs.shape
    rows = []
    for g in range(N // G):
        for b in range(-(-T // B)):
            r = dict(grid=first_id // G + g, t0=b * B, samples=0, sum_replicas=0, sum_pending=0, sum_nodes_spot=0,
                     sum_nodes_od=0, flag_count=[0] * 8, max_replicas=None, max_pending=None, max_nodes=None,
                     min_nodes=None, q_value=0)
            vals = []
            for t in range(b * B, min((b + 1) * B, T)):
                for i in range(g * G, (g + 1) * G):
                    x = recs[t, i]
                    rep, pend, sp, od, fl = int(x["replicas"]), int(x["pending"]), int(x["nodes_spot"]), \
                        int(x["nodes_od"]), int(x["flags"])
                    r["samples"] += 1
                    r["sum_replicas"] += rep
                    r["sum_pending"] += pend
                    r["sum_nodes_spot"] += sp
                    r["sum_nodes_od"] += od
                    for bit in range(8):
                        r["flag_count"][bit] += (fl >> bit) & 1
                    r["max_replicas"] = rep if r["max_replicas"] is None else max(r["max_replicas"], rep)
                    r["max_pending"] = pend if r["max_pending"] is None else max(r["max_pending"], pend)
                    r["max_nodes"] = sp + od if r["max_nodes"] is None else max(r["max_nodes"], sp + od)
                    r["min_nodes"] = sp + od if r["min_nodes"] is None else min(r["min_nodes"], sp + od)
                    vals.append({ref.REPLICAS: rep, ref.PENDING: pend, ref.NODES: sp + od}.get(q_field, 0))
            if q_field != ref.NONE:
                k = max(1, -(-q_ppm * len(vals) // 10**6))  # ceil in integers
                r["q_value"] = sorted(vals)[k - 1]
            rows.append(r)
    return rows


def _tiny(seed, T, N, ties=False):
    rng = np.random.default_rng(seed)
    a = np.zeros((T, N), TRAJ_DTYPE)
    a["replicas"] = rng.integers(-3, 4, (T, N)) if ties else rng.integers(-2**31, 2**31, (T, N))
    a["pending"] = rng.integers(0, 2, (T, N)) if ties else rng.integers(0, 2**31, (T, N))
    a["nodes_spot"] = rng.integers(0, 3 if ties else 65536, (T, N))
    a["nodes_od"] = rng.integers(0, 3 if ties else 65536, (T, N))
    a["last_type"] = rng.integers(0, 65536, (T, N))
    a["flags"] = rng.integers(0, 65536, (T, N))
    return a


# (T, N, G, B): B not dividing T, B > T, G = 1, one row, one sample
@pytest.mark.parametrize("shape", [(7, 6, 3, 3), (7, 6, 2, 100), (5, 4, 1, 2), (5, 4, 4, 5), (1, 1, 1, 1), (9, 3, 3, 4)])
@pytest.mark.parametrize("ties", [False, True])
def test_restatement_equals_the_plain_loops(shape, ties):
    T, N, G, B = shape
    recs = _tiny(sum(shape) + ties, T, N, ties)
    for q_field in (ref.NONE, ref.REPLICAS, ref.PENDING, ref.NODES):
        for q in (0, 1, 500000, 1000000):
            got = ref.timeline(recs, G, B, q_field, q, first_id=2 * G)
            want = _loops(recs, G, B, q_field, q, first_id=2 * G)
            assert got.shape == (N // G, -(-T // B))
            for o, w in zip(got.ravel(), want):
                for f in ref.ROW_DTYPE.names:
                    assert np.array_equal(o[f], w[f]), (shape, q_field, q, f, o[f], w[f])
            if q_field == ref.NONE:
                assert (got["q_value"] == 0).all()
                break


def test_rank_is_the_sweep_rank():
    lib = abi.load_engine()
    for n in (1, 2, 49, 2989, 1 << 31):
        for q in (0, 1, 500000, 950000, 999999, 10**6):
            assert lib.ccka_sweep_rank(n, q) == rank(n, q)


def _oracle_identities(spec, sc, load, what):
    res, tr = po.rollout(spec, sc, load, traj=True, threads=8)
    i64 = lambda a: a.astype(np.int64)  # noqa: E731
    assert np.array_equal(i64(tr["pending"]).sum(axis=0), res["pending_pod_minutes"]), what
    assert np.array_equal(i64(tr["nodes_spot"]).sum(axis=0), res["node_min_spot"]), what
    assert np.array_equal(i64(tr["nodes_od"]).sum(axis=0), res["node_min_od"]), what
    assert np.array_equal(i64((tr["flags"] >> 3) & 1).sum(axis=0), res["slo_minutes"]), what
    assert np.array_equal((i64(tr["nodes_spot"]) + tr["nodes_od"]).max(axis=0), res["peak_nodes"]), what
    assert tr["replicas"].min() >= 0 and tr["pending"].min() >= 0, what
    # and so through the restatement, per scenario and per whole batch
    per = ref.timeline(tr, 1, spec.n_steps)
    assert np.array_equal(per["sum_pending"][:, 0], res["pending_pod_minutes"]), what
    assert np.array_equal(per["max_nodes"][:, 0], res["peak_nodes"]), what
    hourly = ref.timeline(tr, sc.n, 60)
    assert hourly["flag_count"][0, :, 3].sum() == i64(res["slo_minutes"]).sum(), what
    return tr


@pytest.mark.parametrize("profile,seed", WORLDS)
def test_identities_hold_on_the_oracle(profile, seed):
    spec, sc, load = ref.world(profile, seed)
    _oracle_identities(spec, sc, load, f"profile {profile} seed {seed}")


def test_identities_hold_on_config2_with_the_peak_bit():
    spec = configs.config2_world(n_steps=1440)
    sc = configs.hpa_scenarios(588)
    load = po.gen_load(configs.trace_gen(), spec.n_steps, 1, sc.n)
    tr = _oracle_identities(spec, sc, load, "config 2")
    peak = (tr["flags"] & 1).sum(axis=1)
    assert peak.max() > 0 and peak.min() == 0  # the peak window covers part of the day


def _rows(lib, n, T, **kw):
    sp = abi.timeline_spec(**kw)
    return lib.ccka_timeline_rows(n, T, C.byref(sp))


def test_timeline_rows_and_its_rules():
    lib = abi.load_engine()
    for n, T, G, B in [(147, 61, 49, 1), (147, 61, 49, 7), (147, 61, 147, 61), (147, 61, 49, 100), (147, 61, 1, 1),
                       (130, 129, 65, 64), (1, 1, 1, 1), (65539, 3, 65539, 3), (100000, 1440, 1000, 60)]:
        assert _rows(lib, n, T, grid_size=G, step_bucket=B) == n // G * -(-T // B) == ref.n_rows(n, T, G, B)
    assert lib.ccka_timeline_rows(130, 60, None) == -1                              # null spec
    bad = [dict(grid_size=7), dict(grid_size=0), dict(grid_size=-130), dict(grid_size=130, step_bucket=0),
           dict(grid_size=130, step_bucket=-1), dict(grid_size=130, q_field=4), dict(grid_size=130, q_field=-1),
           dict(grid_size=130, q_field=abi.TL_NODES, q_ppm=-1),
           dict(grid_size=130, q_field=abi.TL_PENDING, q_ppm=1000001)]
    for kw in bad:
        assert _rows(lib, 130, 60, **kw) == -1 == ref.n_rows(130, 60, kw["grid_size"], kw.get("step_bucket", 1),
                                                             kw.get("q_field", 0), kw.get("q_ppm", 0)), kw
    assert _rows(lib, 130, 60, grid_size=130, q_ppm=-7) == 60                       # q_ppm is ignored for NONE
    assert _rows(lib, 0, 60, grid_size=1) == -1 and _rows(lib, 130, 0, grid_size=130) == -1
    # G * min(B, T) <= 2^31: the bound itself is allowed, one scenario more is not; B > T counts as T
    big = 1 << 31
    assert _rows(lib, big, 1, grid_size=big) == 1
    assert _rows(lib, big // 64, 64, grid_size=big // 64, step_bucket=64) == 1
    assert _rows(lib, big // 64 + 1, 64, grid_size=big // 64 + 1, step_bucket=64) == -1
    assert _rows(lib, big // 64 + 1, 64, grid_size=big // 64 + 1, step_bucket=63) == 2
    assert _rows(lib, big + 1, 1, grid_size=big + 1, step_bucket=1 << 30) == -1
    assert _rows(lib, big, 1, grid_size=big, step_bucket=1 << 30) == 1
    # at most 2^24 rows
    assert _rows(lib, 1 << 24, 1, grid_size=1) == 1 << 24
    assert _rows(lib, (1 << 24) + 1, 1, grid_size=1) == -1
    assert _rows(lib, 1 << 12, 1 << 12, grid_size=1) == 1 << 24
    assert _rows(lib, 1 << 12, (1 << 12) + 1, grid_size=1) == -1
    assert ref.n_rows(1 << 12, (1 << 12) + 1, 1, 1) == -1 and ref.n_rows(big // 64 + 1, 64, big // 64 + 1, 64) == -1


def test_struct_sizes_and_dtype():
    assert C.sizeof(abi.TimelineSpec) == 24 and C.sizeof(abi.TimelineRow) == 144
    assert abi.timeline_dtype() == ref.ROW_DTYPE and ref.ROW_DTYPE.itemsize == 144
    lib = abi.load_engine()
    buf = (C.c_int64 * 16)()
    n = lib.ccka_struct_sizes(buf, 16)
    assert n == len(abi.STRUCT_ORDER) == 14 and list(buf[12:14]) == [24, 144]
    assert lib.ccka_abi_version() == 7 == abi.ABI_VERSION
    assert (abi.TL_NONE, abi.TL_REPLICAS, abi.TL_PENDING, abi.TL_NODES) == (0, 1, 2, 3)
    sp = abi.timeline_spec(1000, 60, "nodes", 950000)
    assert (sp.grid_size, sp.step_bucket, sp.q_field, sp.q_ppm) == (1000, 60, 3, 950000)
