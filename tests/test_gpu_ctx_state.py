"""The context behind the C ABI against its restated model (tests/ctx_model.py,
held to include/ccka.h's "What ends what" by tests/test_ctx_model.py).

1. Sequences (seeds 0-23): every call's raw return code equals the model's, and
   every payload a getter returns equals what the model says must come back:
   the run of that station, kind and load, from the CPU references the other
   GPU files use, through their helpers and tolerances (parity.compare,
   pyoracle.rollout / rollout_policy / grid_stats / pareto / totals,
   loop_check.compare_detail, sweep_stat_ref, timeline_ref, paired_ref,
   boot_ref, mlp_ref.exact_case). The closed loops' payloads come from a fresh
   context in the canonical order, itself checked against the oracle's replay
   of its recorded actions; a sequence's loop must equal it byte for byte.
2. One named case per finding of the context-state work, and for the two rules
   on failing calls.
3. History independence at the equal-count pair: 120 x 64, then 40 x 192 (the
   trajectory allocation stays, the layout changes), then 120 x 64 again, on
   the single-deployment engine ([N][T] records through the staging
   transpose), the general kernel ([T][N]) and the lane-skewed schedule.

Each case opens its own Engine, so the order of the calls is the test."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import boot_ref
import ctx_model as cm
import mlp_ref
import paired_ref
import pyoracle as po
import sweep_stat_ref
import timeline_ref
from ccka import abi, configs
from ccka.engine import Engine, _grid_array
from ccka.world import TRAJ_DTYPE, alloc_results
from ctx_model import EINVAL, ESTATE, GS, OK, STATIONS
from loop_check import compare_detail
from parity import compare

pytestmark = pytest.mark.gpu
THREADS = 16
LIB = os.environ.get("CCKA_TEST_LIB") or None   # the build under test, as the session's engine
W_CARBON, W_SLO = 0.05, 0.01
STAT_KINDS, STAT_Q = (sweep_stat_ref.TAIL, sweep_stat_ref.QUANTILE, sweep_stat_ref.SUM, sweep_stat_ref.SUM), (900000, 950000, 0, 0)
STAT = abi.sweep_stat(cost=("tail", 900000), slo=("quantile", 950000))
TL = (7, timeline_ref.NODES, 950000)   # step bucket, quantile field, q_ppm
BOOT_SEED = 5
TAIL_RTOL = 1e-12                      # tests/test_gpu_sweep_stat.py


def _ro(x):
    for a in (x.values() if isinstance(x, dict) else [x]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


# ---------------------------------------------------------------------------
# the library, call by call: raw return codes
# ---------------------------------------------------------------------------
class Rig:
    def __init__(self):
        self.e = Engine(0, lib_path=LIB)
        self.lib, self.ctx = self.e.lib, self.e.ctx
        self.station = "A"     # the station whose set stands (drive); its load serves a set_load that must fail too

    def close(self):
        self.e.close()

    def set_world(self, name, valid=True):
        w = cm.build(name)[0].to_c()
        if not valid:
            w.n_steps = 0
        return self.lib.ccka_set_world(self.ctx, C.byref(w)), None

    def set_scenarios(self, name, valid=True):
        s = cm.build(name)[1].to_c()
        if not valid:
            s.n = 0
        return self.lib.ccka_set_scenarios(self.ctx, C.byref(s)), None

    def set_load(self, variant):
        _, _, loads, gens = cm.build(self.station)
        if variant == 1:
            return self.lib.ccka_gen_load(self.ctx, C.byref(gens[1])), None
        a = np.ascontiguousarray(loads[0])
        return self.lib.ccka_set_load(self.ctx, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size), None

    def set_weights(self, which):
        ws, bs = configs.mlp_weights() if which == "cfg" else mlp_ref.exact_weights(0)
        self.e.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
        return OK, None

    def switch(self, name, on):
        if name == "detail_on":
            return self.lib.ccka_set_detail(self.ctx, int(on)), None
        fn = self.lib.ccka_debug_policy_fused if name == "fused_off" else self.lib.ccka_debug_policy_features
        fn.argtypes = [C.c_void_p, C.c_int32]
        return fn(self.ctx, int(not on) if name == "fused_off" else int(on)), None

    def rollout(self, traj):
        return self.lib.ccka_rollout(self.ctx, int(traj)), None

    def policy_rollout(self, traj, record):
        return self.lib.ccka_policy_rollout(self.ctx, int(traj), int(record)), None

    def policy_grad(self):
        g, s = Engine._grads()
        prm = abi.PgParams(STATIONS[self.station].seed, W_CARBON, W_SLO, 1, 0)
        obj = C.c_double()
        rc = self.lib.ccka_policy_grad(self.ctx, C.byref(prm), C.byref(s), C.byref(obj))
        return rc, (g, obj.value)

    def mlp_backward(self, rows=cm.MLP_ROWS):
        c = mlp_ref.exact_case(0, rows)
        x = np.ascontiguousarray(configs.to_bf16_bits(c["x"]), np.uint16)
        a, cf = np.ascontiguousarray(c["act"], np.uint8), np.ascontiguousarray(c["coef"], np.float32)
        g, s = Engine._grads()
        rc = self.lib.ccka_mlp_backward(self.ctx, x.ctypes.data_as(C.POINTER(C.c_uint16)),
                                        a.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        cf.ctypes.data_as(C.POINTER(C.c_float)), rows, C.byref(s))
        return rc, g

    def mlp_set_states(self):
        self.e.mlp_set_states(configs.to_bf16_bits(mlp_ref.exact_case(0, cm.MLP_ROWS)["x"]))
        return OK, None

    def mlp_forward(self):
        return self.lib.ccka_mlp_forward(self.ctx), None

    def mlp_actions(self):
        return OK, self.e.mlp_actions()

    def kernel_ms(self):
        return self.lib.ccka_last_kernel_ms(self.ctx, C.byref(C.c_double())), None

    def last_engine(self):
        return OK, self.e.last_engine()[0]

    def get(self, getter, T, N, base=None):
        """A getter with the counts of the shape (T, N), the current one."""
        lib, ctx = self.lib, self.ctx
        ng = N // GS
        bg = abi.PAIRED_SAME if base is None else base
        if getter == "results":
            arrays, r = alloc_results(max(N, 1))
            return lib.ccka_get_results(ctx, C.byref(r)), arrays
        if getter == "totals":
            t = abi.Totals()
            return lib.ccka_get_totals(ctx, C.byref(t)), t
        if getter in ("grid_stats", "grid_stat"):
            a = (abi.GridStats * max(ng, 1))()
            if getter == "grid_stats":
                rc = lib.ccka_get_grid_stats(ctx, C.c_int64(GS), a, C.c_int64(ng))
            else:
                rc = lib.ccka_get_grid_stat(ctx, C.c_int64(GS), C.byref(STAT), a, C.c_int64(ng))
            return rc, _grid_array(a, ng)
        if getter == "pareto":
            a, n = (abi.GridStats * max(ng, 1))(), C.c_int32()
            rc = lib.ccka_pareto_frontier(ctx, C.c_int64(GS), a, max(ng, 1), C.byref(n))
            return rc, _grid_array(a, n.value if rc == OK else 0)
        if getter == "capture":
            return lib.ccka_paired_capture(ctx, C.c_int64(GS)), None
        if getter == "paired":
            spec, out = abi.paired_spec(GS, bg, STAT), np.zeros(max(ng, 1), abi.paired_dtype())
            return lib.ccka_get_paired(ctx, C.byref(spec), out.ctypes.data, C.c_int64(ng)), out[:ng]
        if getter == "boot":
            spec, out = abi.boot_spec(GS, bg, cm.BOOT_B, BOOT_SEED), np.zeros(max(ng, 1), abi.boot_dtype())
            return lib.ccka_get_paired_bootstrap(ctx, C.byref(spec), out.ctypes.data, C.c_int64(ng)), out[:ng]
        if getter == "timeline":
            spec = abi.timeline_spec(GS, *TL)
            rows = max(lib.ccka_timeline_rows(N, T, C.byref(spec)), 0)
            out = np.zeros(max(rows, 1), abi.timeline_dtype())
            return lib.ccka_get_timeline(ctx, C.byref(spec), out.ctypes.data, rows), out[:rows].reshape(max(ng, 1), -1)
        if getter == "trajectory":
            a = np.zeros((T, N), TRAJ_DTYPE)
            return lib.ccka_get_trajectory(ctx, a.ctypes.data_as(C.POINTER(abi.TrajRec)), a.size), a
        if getter == "detail":
            a = np.zeros(N, abi.detail_dtype())
            return lib.ccka_get_detail(ctx, a.ctypes.data, a.size), a
        if getter == "actions":
            tg, cw = np.zeros((T, N), np.int16), np.zeros((T, N), np.float64)
            return lib.ccka_get_policy_actions(ctx, tg.ctypes.data, cw.ctypes.data, tg.size), (tg, cw)
        if getter == "features":
            fn = lib.ccka_debug_get_policy_features
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
            a = np.zeros((T + 1, N, 64), np.uint16)
            return fn(ctx, a.ctypes.data, a.size), a
        assert getter == "samples"
        a, cf = np.zeros((T, N), np.uint8), np.zeros(N, np.float32)
        return lib.ccka_get_policy_samples(ctx, a.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           cf.ctypes.data_as(C.POINTER(C.c_float)), a.size), (a, cf)


# ---------------------------------------------------------------------------
# what must come back: computed once per run, shared and read-only
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(run):
    """The payloads of a run (station, kind, load variant)."""
    name, kind, lv = run
    spec, sc, loads, _ = cm.build(name)
    load = loads[lv]
    if kind == "roll":
        res, traj, det = po.rollout(spec, sc, load, traj=True, threads=THREADS, detail=True)
        return dict(res=_ro(res), traj=_ro(traj), detail=_ro(det))
    # a closed loop: a fresh context in the canonical order, checked against the oracle's replay of its actions
    r = Rig()
    r.station = name
    try:
        for c in (("set_world", name), ("set_scenarios", name), ("set_load", lv), ("set_weights", "cfg"),
                  ("switch", "feat_on", True), ("switch", "detail_on", True)):
            assert getattr(r, c[0])(*c[1:])[0] == OK, c
        out = {}
        if kind == "loop":
            r.e.n, r.e.T = sc.n, spec.n_steps
            r.e.policy_rollout(trajectory=True, record=True)
            out["traj"] = r.e.trajectory()
        else:
            rc, (g, obj) = r.policy_grad()
            assert rc == OK
            out["grads"], out["obj"] = {k: v.copy() for k, v in g.items()}, obj
            rc, out["samples"] = r.get("samples", spec.n_steps, sc.n)
            assert rc == OK
        T, N = spec.n_steps, sc.n
        for key, getter in (("res", "results"), ("actions", "actions"), ("features", "features"), ("detail", "detail")):
            rc, out[key] = r.get(getter, T, N)
            assert rc == OK, (run, getter, rc)
    finally:
        r.close()
    tg, cw = out["actions"]
    rep = po.rollout_policy(spec, sc, load, tg, cw, traj=True, threads=THREADS, features=True, detail=True)
    compare(out["res"], rep[0], out.get("traj"), rep[1] if "traj" in out else None)
    assert np.array_equal(out["features"], rep[2]), f"{run}: features differ from the oracle's replay"
    compare_detail(out["detail"], rep[3])
    if kind == "grad":
        act, coef = out["samples"]
        assert np.array_equal(tg, 40 + 10 * (act.astype(np.int16) & 3)) and np.array_equal(cw, (act >> 2).astype(np.float64))
        res = out["res"]
        J = res["cost_uphmin"] / 6e7 + W_CARBON * res["gco2"] * 1e-3 + W_SLO * res["slo_minutes"]
        assert out["obj"] == pytest.approx(J.mean(), rel=1e-12)
        assert np.allclose(coef, ((J - J.mean()) / sc.n).astype(np.float32), rtol=1e-6, atol=1e-12)
    for v in out.values():
        for a in (v if isinstance(v, tuple) else [v]):
            _ro(a)
    return out


@functools.lru_cache(maxsize=None)
def expected_rows(getter, run, snap=None, base=None):
    """The rows of a grid call on a run's results or trajectory."""
    s = STATIONS[run[0]]
    res = expected(run)["res"]
    if getter == "grid_stats":
        return po.grid_stats(res, GS, s.first_id)
    if getter == "grid_stat":
        return sweep_stat_ref.grid_stat(res, GS, STAT_KINDS, STAT_Q, s.first_id)
    if getter == "timeline":
        return timeline_ref.timeline(expected(run)["traj"], GS, *TL, first_id=s.first_id)
    b = STATIONS[snap[0]]
    args = (res, expected(snap)["res"], GS, paired_ref.SAME if base is None else base, s.first_id // GS, b.first_id // GS)
    if getter == "paired":
        rows, ovf = paired_ref.paired(*args[:4], STAT_KINDS, STAT_Q, *args[4:])
        assert not ovf
        return rows
    boot = boot_ref.Boot(*args)
    assert not boot.ovf
    return boot.rows(cm.BOOT_B, BOOT_SEED)


def check(call, key, got, what):
    """A successful call's payload against the run the model names."""
    op = call[0]
    if op == "last_engine":
        assert got == key, f"{what}: ran on engine {got}, the model says {key}"
    elif op == "mlp_actions":
        assert np.array_equal(got, mlp_ref.exact_case(0, cm.MLP_ROWS)["ref"]["y"].astype(np.float32)), what
    elif op == "mlp_backward":
        ref = mlp_ref.exact_case(0, key)["ref"]
        for k in mlp_ref.GRADS:
            assert np.array_equal(got[k], ref[k].astype(np.float32)), f"{what}: d{k}"
    elif op == "policy_grad":
        want = expected(key)
        assert got[1] == want["obj"], f"{what}: objective"
        for k in mlp_ref.GRADS:
            assert np.array_equal(got[0][k], want["grads"][k]), f"{what}: d{k} differs from a fresh context's"
    elif op == "get":
        check_get(call[1], key, got, what)


def check_get(getter, key, got, what):
    if getter == "capture":
        return
    if getter in ("paired", "boot"):
        run, snap, base = key
        (paired_ref if getter == "paired" else boot_ref).equal(got, expected_rows(getter, run, snap, base), what)
        return
    want = expected(key)
    s = STATIONS[key[0]]
    if getter == "results":
        compare(got, want["res"])
    elif getter == "totals":
        ref = po.totals(want["res"], s.N)
        for f, _ in got._fields_:
            a, b = getattr(got, f), getattr(ref, f)
            assert (a.hex() == b.hex()) if isinstance(a, float) else a == b, (what, f, a, b)
    elif getter == "grid_stats":
        ref = expected_rows(getter, key)
        for f in ("grid", "scenarios", "cost_uphmin", "slo_minutes"):
            assert np.array_equal(got[f], ref[f]), (what, f)
        for f in ("gco2", "energy_wmin"):
            assert np.allclose(got[f], ref[f], rtol=1e-12, atol=0), (what, f)
    elif getter == "grid_stat":
        ref = expected_rows(getter, key)
        for f in ("grid", "scenarios"):
            assert np.array_equal(got[f], ref[f]), (what, f)
        for f, kind in zip(sweep_stat_ref.FIELDS, STAT_KINDS):
            if got[f].dtype.kind == "f":
                assert np.allclose(got[f], ref[f], rtol=TAIL_RTOL, atol=0), (what, f)
            else:
                assert np.array_equal(got[f], ref[f]), (what, f, got[f], ref[f])
    elif getter == "pareto":
        ref = expected_rows("grid_stats", key)
        assert np.array_equal(got["grid"], ref["grid"][po.pareto(ref)]), what
    elif getter == "timeline":
        ref = expected_rows(getter, key)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        for f in ref.dtype.names:
            assert np.array_equal(got[f], ref[f]), (what, f)
    elif getter == "trajectory":
        for f in got.dtype.names:
            bad = np.argwhere(got[f] != want["traj"][f])
            assert bad.size == 0, f"{what}: traj.{f} differs at (t, i) {bad[:5].tolist()}"
    elif getter == "detail":
        compare_detail(got, want["detail"])
    elif getter == "actions":
        assert np.array_equal(got[0], want["actions"][0]) and np.array_equal(got[1], want["actions"][1]), what
    elif getter == "features":
        assert np.array_equal(got, want["features"]), what
    elif getter == "samples":
        assert np.array_equal(got[0], want["samples"][0]) and np.array_equal(got[1], want["samples"][1]), what


def drive(rig, model, calls, seed=None):
    """Every call on the model, then on the library: the status, then the payload.
    The first wrong status ends the case: what follows assumed the state it denies."""
    for i, c in enumerate(calls):
        want, key = getattr(model, c[0])(*c[1:])
        rig.station = model.sc or rig.station
        args = (c[1], model.T, model.N) + tuple(c[2:]) if c[0] == "get" else c[1:]
        got, payload = getattr(rig, c[0])(*args)
        what = f"seed {seed} call {i} {c} after {calls[max(0, i - 6):i]}"
        assert got == want, f"{what}: returned {abi.STATUS.get(got, got)}, the contract says {abi.STATUS[want]}"
        if want == OK:
            check(c, key, payload, what)


@pytest.fixture
def rig():
    r = Rig()
    try:
        yield r
    finally:
        r.close()


# ---- 1. sequences ---------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_sequence(rig, seed):
    drive(rig, cm.Ctx(), cm.sequence(seed), seed)


# ---- 2. named cases ---------------------------------------------------------
def canonical(name, lv=0):
    return [("set_weights", "cfg"), ("set_world", name), ("set_scenarios", name), ("set_load", lv)]


def statuses(rig, model, getters):
    return [rig.get(g, model.T, model.N)[0] for g in getters]


FORWARD = [("set_weights", "exact"), ("mlp_set_states",), ("mlp_forward",), ("mlp_actions",)]
RESULTS = ("results", "totals", "grid_stats", "grid_stat", "pareto", "capture", "timeline", "detail", "trajectory")


@pytest.mark.parametrize("ending", ["set_scenarios", "set_world"])
def test_finding_1_an_mlp_forward_makes_no_results_readable(rig, ending):
    """ccka_mlp_forward is a timed launch only. After ccka_set_scenarios the
    result columns are a fresh allocation no kernel has written; after a lone
    ccka_set_world they hold the earlier world's run. Neither is readable
    after the forward, and the forward's time is."""
    m = cm.Ctx()
    drive(rig, m, canonical("E") + [("switch", "detail_on", True), ("rollout", True), ("get", "capture"), ("get", "detail")])
    # (the lone world keeps the horizon at 30 steps: every count stays inside what the run wrote)
    drive(rig, m, [("set_scenarios", "E")] if ending == "set_scenarios" else [("set_world", "G")])
    drive(rig, m, FORWARD + [("kernel_ms",)])
    assert m.kernel_ms()[0] == OK and (ending == "set_scenarios" or all(m.in_bounds(g) for g in RESULTS))
    got = statuses(rig, m, RESULTS)
    assert got == [ESTATE] * len(RESULTS), dict(zip(RESULTS, (abi.STATUS.get(x, x) for x in got)))


def test_finding_1_kernel_time_of_a_context_that_ran_only_a_forward(rig):
    m = cm.Ctx()
    drive(rig, m, [("kernel_ms",)] + FORWARD + [("kernel_ms",)])
    assert m.timed and m.obj["res"] is None


RECORDS = ("actions", "features", "samples")


@pytest.mark.parametrize("ending", [("set_scenarios", "B"), ("set_scenarios", "C"), ("set_world", "E")],
                         ids=["equal N", "smaller N", "a shorter horizon"])
def test_finding_2_the_loops_records_end_with_the_world_and_the_set(rig, ending):
    """The recorded actions, features and samples of a loop on 40 x 192 are not
    readable under another batch or world: the getters' counts then come from
    the new shape, the buffers' contents from the earlier loop."""
    m = cm.Ctx()
    drive(rig, m, canonical("B") + [("policy_grad",)] + [("get", g) for g in RECORDS])
    drive(rig, m, [ending])
    assert all(m.in_bounds(g) for g in RECORDS)      # what a wrong library would copy stays inside the loop's buffers
    got = statuses(rig, m, RECORDS)
    assert got == [ESTATE] * 3, dict(zip(RECORDS, (abi.STATUS.get(x, x) for x in got)))


def test_finding_2_a_rollout_and_a_new_load_keep_the_records(rig):
    m = cm.Ctx()
    drive(rig, m, canonical("B") + [("policy_grad",)])
    first = [rig.get(g, m.T, m.N) for g in RECORDS]
    drive(rig, m, [("rollout", True), ("get", "results")] + [("get", g) for g in RECORDS])
    drive(rig, m, [("set_load", 1)] + [("get", g) for g in RECORDS] + [("rollout", False), ("get", "results")])
    for g, (st0, a), (st1, b) in zip(RECORDS, first, [rig.get(g, m.T, m.N) for g in RECORDS]):
        assert st0 == st1 == OK
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert x.tobytes() == y.tobytes(), g


def test_finding_3_set_world_ends_the_scenario_set(rig):
    """From two regions (the batch's second half in region 1) to a one-region
    world: the kept set would index the new price and carbon tiles by region 1.
    ccka_set_load returns ESTATE and nothing runs until the new set is in."""
    m = cm.Ctx()
    drive(rig, m, canonical("G") + [("rollout", True), ("get", "results"), ("get", "trajectory")])
    drive(rig, m, [("set_world", "A"), ("set_load", 0), ("set_load", 1)])
    assert m.sc is None and m.set_load(0)[0] == ESTATE
    drive(rig, m, [("set_scenarios", "A"), ("set_load", 0), ("rollout", True), ("last_engine",), ("get", "results"),
                   ("get", "trajectory")])


def test_a_set_world_that_fails_validation_changes_nothing(rig):
    m = cm.Ctx()
    drive(rig, m, canonical("C") + [("policy_rollout", False, True), ("rollout", True)])
    kept = ("results", "trajectory", "actions")
    first = [rig.get(g, m.T, m.N) for g in kept]
    drive(rig, m, [("set_world", "D", False)] + [("get", g) for g in kept])
    again = [rig.get(g, m.T, m.N) for g in kept]
    drive(rig, m, [("rollout", True), ("get", "results"), ("get", "trajectory")])
    after = [rig.get(g, m.T, m.N) for g in kept]      # the rollout afterwards: equal to the first, byte for byte
    for g, (st0, a), (st1, b), (st2, c) in zip(kept, first, again, after):
        assert st0 == st1 == st2 == OK
        parts = [list(v.values()) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else [v] for v in (a, b, c)]
        for x, y, z in zip(*parts):
            assert x.tobytes() == y.tobytes() == z.tobytes(), g


@pytest.mark.parametrize("name", ["A", "D", "H"])
def test_a_new_load_is_what_the_next_rollout_reads(rig, name):
    """rollout, ccka_set_load, rollout on one scenario set: the second run reads
    the new trace, not the wave-tiled (A) or scenario-major (D) copy derived
    from the first, and starts from an empty HBM decision history (H), not from
    the decisions the first run left there. Then the first load again."""
    m = cm.Ctx()
    drive(rig, m, canonical(name, 1) + [("rollout", True), ("last_engine",), ("get", "results"), ("get", "trajectory")])
    for lv in (0, 1, 0):
        drive(rig, m, [("set_load", lv), ("get", "results"), ("rollout", True), ("last_engine",), ("get", "results"),
                       ("get", "trajectory")])


def test_a_failing_set_scenarios_ends_the_set(rig):
    m = cm.Ctx()
    drive(rig, m, canonical("H") + [("rollout", True), ("set_scenarios", "H", False), ("rollout", False),
                                    ("policy_rollout", False, False), ("set_load", 0), ("get", "results"),
                                    ("set_scenarios", "H"), ("set_load", 1), ("rollout", True), ("last_engine",),
                                    ("get", "results"), ("get", "trajectory")])


# ---- 3. history independence at the equal-count pair ------------------------
def _two_deployments(spec):
    from ccka.world import deployment
    spec.deploys = [deployment(abi.SCALER_HPA, cap_sel=abi.CAP_SPOT),
                    deployment(abi.SCALER_HPA, cap_sel=abi.CAP_OD, req_cpu=400, target=60)]
    return spec


@pytest.mark.parametrize("engine_id", [2, 1, 5])
def test_equal_count_pair_is_history_independent(engine_id):
    """120 x 64, 40 x 192, 120 x 64 with a trajectory each: d_traj keeps its
    7,680 records while the layout changes. Each read-back equals the oracle,
    the third the first byte for byte."""
    e = Engine(0, lib_path=LIB)
    try:
        e.set_engine(1 if engine_id == 1 else 0)
        reads = []
        for T, n, first in ((120, 64, 0), (40, 192, 7), (120, 64, 0)):
            spec = configs.config2_world(n_steps=T)
            if engine_id == 5:
                spec = _two_deployments(spec)
            sc = configs.hpa_scenarios(n, first)
            load = po.gen_load(configs.trace_gen(71), T, len(spec.deploys), n, first_id=first)
            e.set_world(spec)
            e.set_scenarios(sc)
            e.set_load(load)
            e.rollout(trajectory=True)
            assert e.last_engine()[0] == engine_id
            res, tr = e.results(), e.trajectory()
            rc, tc = po.rollout(spec, sc, load, traj=True, threads=THREADS)
            compare(res, rc, tr, tc)
            reads.append((res, tr))
        assert reads[2][1].tobytes() == reads[0][1].tobytes()
        assert all(reads[2][0][k].tobytes() == reads[0][0][k].tobytes() for k in reads[0][0])
    finally:
        e.close()
