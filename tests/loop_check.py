"""TEST INFRASTRUCTURE: the closed-loop checker shared by the GPU parity files
(tests/test_gpu_random_worlds.py, tests/test_gpu_time_axis.py,
tests/test_gpu_loop_worlds.py) and its CPU guard (tests/test_loop_worlds.py).

loop_plan / loop_engine restate in plain Python which closed loop
ccka_policy_rollout takes for a world (abi_policy.cpp policy_loop over
abi_rollout.cpp plan_launch / setup_general): the fused loop (engine 4) for
one deployment on <= 8 slots whose general-kernel LDS leaves room for the
MLP's 149,632 B, the launched loop (engine 3) otherwise. check_loop runs a
world on the loop the rule predicts (and on the launched loop too where it
fuses) against the oracle's replay of the recorded actions; check_sampled does
the same for the sampled policy of ccka_policy_grad. Every run is tallied
(TALLY) by (engine, dmax, nmax) and by the launch flags the world has; a
tallied world's restated plan is asserted against ccka_debug_last_plan of a
lockstep general-kernel run of the same world (_device_plan)."""
import ctypes as C

import numpy as np

import mlp_ref
import pyoracle as po
from ccka import abi, configs
from parity import compare
from test_detail import FP_DETAIL, INT_DETAIL

THREADS = 16
MLP_LDS = ((256 // 32) * (256 // 16) + 256 // 16) * 64 * 16 + (2 * 256 + 32) * 4  # W2 + W3 fragments, biases
LDS_BYTES = 160 * 1024
# (name, seed) -> what ran: filled by check_loop / check_sampled, read by the tally test
TALLY = {}


def kernel_dims(n_deploy, max_nodes):
    """kparams.h kernel_dims: the DMAX x MAXN instantiation of a world."""
    dmax = next(d for d in (1, 2, 4, 8, 12, 16) if n_deploy <= d)
    return dmax, 8 if max_nodes <= 8 and dmax <= 4 else 16


def _up16(x):
    return (x + 15) & ~15


def _hist_entries(window_s, sync_s):
    return (window_s - 1) // sync_s if window_s > sync_s else 0


def _fits_ring(r):
    """abi_ctx.cpp rules_fit_ring: the 8-decision register rings hold the rules."""
    lim = abi.HIST * abi.STEP_SECONDS
    return r.n_policies <= 2 and r.stab_window_s <= lim and all(r.policies[q].period_s <= lim
                                                                for q in range(r.n_policies))


def general_lds(K, Z, span, dmax, nmax):
    """(all_hours, dynamic LDS bytes) of the general kernel for K types over Z
    zones, `span` regions per block and the DMAX x MAXN instantiation
    (abi_rollout.cpp plan_launch; sizeof(ccka_itype) from the abi struct)."""
    B = 256
    itype = C.sizeof(abi.ItType)
    assert itype == 48  # rollout_kernel.h stages a catalog entry as three 16-byte words
    off = _up16(K * itype)
    off = _up16(off + K * 4)
    tile = span * K * Z * 2 * 4
    all_hours = int(off + 24 * tile + 8 * 1024 <= 64 * 1024)
    off = _up16(off + (24 if all_hours else 1) * tile)
    off = _up16(off + (B // 64) * nmax * (7 + dmax) * 4)
    off += 16
    off = _up16(off + span * 24 * 2 * 8)
    return all_hours, off


def fuses(K, Z, span, dmax, nmax):
    """abi_policy.cpp policy_loop: one deployment, <= 8 slots and the MLP's LDS beside the kernel's."""
    return dmax == 1 and nmax == 8 and _up16(general_lds(K, Z, span, dmax, nmax)[1]) + MLP_LDS <= LDS_BYTES


def loop_plan(spec, sc):
    """The general kernel's launch plan of a world and a scenario set, as
    plan_launch and setup_general decide it: dmax, nmax, the region span per
    block of 256 scenarios, all_hours, the dynamic LDS bytes, the HBM history
    length, the HPA decisions per step and the shared-trace flag."""
    B = 256
    span = 1
    if sc.region is not None:
        reg = np.asarray(sc.region, np.int64)
        span = max(int(reg[b:b + B].max() - reg[b:b + B].min()) + 1 for b in range(0, sc.n, B))
    dmax, nmax = kernel_dims(len(spec.deploys), spec.max_nodes)
    all_hours, off = general_lds(spec.catalog.k, spec.n_zones, span, dmax, nmax)
    assert off <= LDS_BYTES, f"ccka_policy_rollout refuses the world: {off} B of LDS"
    sync_s = spec.hpa_sync_s if spec.hpa_sync_s > 0 else abi.STEP_SECONDS
    nsub = abi.STEP_SECONDS // sync_s
    dstab_max = -1 if sc.down_stab_s is None else int(np.max(sc.down_stab_s))
    fit = nsub == 1 and dstab_max <= abi.HIST * abi.STEP_SECONDS
    hl = 0
    for d in spec.deploys:
        if d.scaler not in (abi.SCALER_HPA, abi.SCALER_KEDA):
            continue
        fit = fit and _fits_ring(d.up) and _fits_ring(d.down)
        dstab = d.down.stab_window_s
        if d.scaler == abi.SCALER_HPA and dstab_max >= 0:
            dstab = max(dstab, dstab_max)
        hl = max(hl, _hist_entries(d.up.stab_window_s, sync_s), _hist_entries(dstab, sync_s))
        for r in (d.up, d.down):
            for q in range(r.n_policies):
                hl = max(hl, _hist_entries(r.policies[q].period_s, sync_s))
    return dict(dmax=dmax, nmax=nmax, span=span, all_hours=all_hours, lds=off, hlen=0 if fit else max(hl, 1),
                nsub=nsub, trace_mod=int(sc.n_traces > 0))


def loop_engine(spec, sc):
    """The engine ccka_policy_rollout reports for the world: 4 (fused) or 3 (launched)."""
    p = loop_plan(spec, sc)
    return 4 if fuses(spec.catalog.k, spec.n_zones, p["span"], p["dmax"], p["nmax"]) else 3


def _fused(engine, on):
    fn = engine.lib.ccka_debug_policy_fused
    fn.argtypes = [C.c_void_p, C.c_int32]
    fn(engine.ctx, on)


def _named(what, fn):
    try:
        return fn()
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _setup(engine, world, weights_seed):
    spec, sc, load = world
    ws, bs = configs.mlp_weights(weights_seed)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)


def _device_plan(engine, spec, sc, what):
    """loop_plan against the library: the same world on the general kernel in
    lockstep (ccka_debug_engine(2); setup_general is the closed loops' too, and
    they record no plan of their own), its launch plan field for field."""
    want = loop_plan(spec, sc)
    try:
        engine.set_engine(2)
        engine.rollout()
        got, ran = engine.last_plan(), engine.last_engine()[0]
    finally:
        engine.set_engine(0)
    assert ran == 1, f"{what}: the lockstep run reports engine {ran}"
    for f in ("span", "all_hours", "hlen", "lds", "trace_mod"):
        assert got[f] == want[f], f"{what}: plan field {f} is {got[f]} on the device, restated {want[f]}"
    assert got["grid"] == (sc.n + 255) // 256 and got["lclaims"] == 0, f"{what}: plan {got}"
    return want


def _tally(key, engine, spec, sc, what, engines, varying):
    if key is not None:
        TALLY[key] = dict(_device_plan(engine, spec, sc, what), engines=tuple(engines), varying=bool(varying))


def _modes(want, launched):
    """(fused switch, engine the run must report) of a world's runs: the loop
    the rule predicts, then the launched loop where the world fuses."""
    if want == 3:
        return [(1, 3)]
    return [(1, 4), (0, 3)] if launched else [(1, 4)]


def compare_detail(dg, dc):
    for f in INT_DETAIL:
        bad = np.argwhere(dg[f] != dc[f])
        assert bad.size == 0, f"detail.{f}: {len(bad)} mismatches, first {bad[:5].tolist()}"
    for f in FP_DETAIL:
        bad = np.argwhere(dg[f] != dc[f])
        assert bad.size == 0, f"detail.{f}: {len(bad)} not bit-exact, first {bad[:5].tolist()}"


def check_loop(engine, world, weights_seed, what, launched=True, detail=False, key=None, want=None):
    """One world through ccka_policy_rollout under configs.mlp_weights(weights_seed).

    The engine of every run is asserted against loop_engine (`want` overrides
    the expectation of the first run only to state it twice, never to relax
    it). Results, every trajectory record and every feature word equal the
    oracle's replay of the recorded actions; where the world fuses and
    `launched` is set, the launched loop's results, trajectory, actions and
    features equal the fused run's. detail: each loop runs once more with
    ccka_set_detail(1); its records equal the oracle's replay detail field for
    field and its results those of the run without detail.
    Returns the first run's (results, trajectory, (targets, weights), features)."""
    spec, sc, load = world
    predicted = loop_engine(spec, sc)
    assert want in (None, predicted), f"{what}: the rule predicts engine {predicted}, the case expects {want}"
    _setup(engine, world, weights_seed)
    runs, details = [], []
    modes = _modes(predicted, launched)
    engine.debug_policy_features(True)
    try:
        for fused, eng in modes:
            _fused(engine, fused)
            engine.policy_rollout(trajectory=True, record=True)
            got = engine.last_engine()[0]
            assert got == eng, f"{what} fused {fused}: ran on engine {got}, expected {eng}"
            runs.append((engine.results(), engine.trajectory(), engine.policy_actions(),
                         engine.debug_get_policy_features()))
            if detail:
                engine.set_detail(True)
                try:
                    engine.policy_rollout(trajectory=True, record=True)
                    got = engine.last_engine()[0]
                    assert got == eng, f"{what} fused {fused} with detail: ran on engine {got}, expected {eng}"
                    details.append((engine.results(), engine.trajectory(), engine.policy_actions(), engine.detail()))
                finally:
                    engine.set_detail(False)
    finally:
        _fused(engine, 1)
        engine.debug_policy_features(False)
    rg, tg, (at, ac), fg = runs[0]
    first = f"{what} engine {modes[0][1]} ({'fused' if modes[0][1] == 4 else 'launched'})"
    out = po.rollout_policy(spec, sc, load, at, ac, traj=True, threads=THREADS, features=True, detail=detail)
    rc, tc, fc = out[:3]
    _named(f"{first} vs oracle replay", lambda: compare(rg, rc, tg, tc))
    bad = np.argwhere(fg != fc)
    assert bad.size == 0, f"{first} vs oracle replay: features differ at (t, i, f) {bad[:5].tolist()}"
    if len(runs) > 1:
        rl, tl, (atl, acl), fl = runs[1]
        w2 = f"{what} engine 3 (launched) vs engine 4 (fused)"
        _named(w2, lambda: compare(rl, rg, tl, tg))
        assert np.array_equal(atl, at) and np.array_equal(acl, ac), f"{w2}: actions differ"
        assert np.array_equal(fl, fg), f"{w2}: features differ"
    for (fused, eng), (rd, td, (atd, acd), dg) in zip(modes, details):
        w3 = f"{what} engine {eng} with detail"
        _named(f"{w3} vs the run without", lambda: compare(rd, rg, td, tg))
        assert np.array_equal(atd, at) and np.array_equal(acd, ac), f"{w3}: actions differ from the run without"
        _named(f"{w3} vs oracle replay detail", lambda: compare_detail(dg, out[3]))
    varying = max(len(np.unique(at)), len(np.unique(ac))) >= 2
    _tally(key, engine, spec, sc, what, [m[1] for m in modes], varying)
    return runs[0]


def check_sampled(engine, world, seed, what, key=None, w_carbon=0.05, w_slo=0.01):
    """One world through ccka_policy_grad(seed) under configs.mlp_weights(seed):
    the bin table, results and features against the oracle's replay of the
    sampled actions, the objective and the factors from the results, the
    gradient against ccka_mlp_backward of the recorded rows (bit for bit),
    every sampled bin against mlp_ref.sample_bins on mlp_kernel's logits and
    the oracle's Philox uniforms (bins within 1e-6 relative of an edge exempt;
    returns (samples, exempt) for the caller's 0.1 % bound), and where the
    world fuses the launched loop's bins, factors, objective, results and
    gradient against the fused run's."""
    import pytest
    from test_gpu_mlp import run_forward
    spec, sc, load = world
    predicted = loop_engine(spec, sc)
    _setup(engine, world, seed)
    T, n = spec.n_steps, sc.n
    runs = []
    try:
        for fused, eng in _modes(predicted, True):
            _fused(engine, fused)
            g, obj = engine.policy_grad(seed=seed, w_carbon=w_carbon, w_slo=w_slo)
            got = engine.last_engine()[0]
            assert got == eng, f"{what} fused {fused}: ran on engine {got}, expected {eng}"
            act, coef = engine.policy_samples()
            runs.append(dict(g={k: v.copy() for k, v in g.items()}, obj=obj, act=act, coef=coef,
                             feats=engine.debug_get_policy_features(), actions=engine.policy_actions(),
                             res=engine.results(), eng=eng))
    finally:
        _fused(engine, 1)
    r0 = runs[0]
    act, coef, feats, (tg, cw), rg = r0["act"], r0["coef"], r0["feats"], r0["actions"], r0["res"]
    first = f"{what} engine {r0['eng']}"
    assert np.array_equal(tg, 40 + 10 * (act.astype(np.int16) & 3)), f"{first}: target bin table"
    assert np.array_equal(cw, (act >> 2).astype(np.float64)), f"{first}: carbon-weight bin table"
    rc, _, fc = po.rollout_policy(spec, sc, load, tg, cw, threads=THREADS, features=True)
    _named(f"{first} vs oracle replay", lambda: compare(rg, rc))
    bad = np.argwhere(feats != fc)
    assert bad.size == 0, f"{first} vs oracle replay: features differ at (t, i, f) {bad[:5].tolist()}"
    J = rg["cost_uphmin"] / 6e7 + w_carbon * rg["gco2"] * 1e-3 + w_slo * rg["slo_minutes"]
    assert r0["obj"] == pytest.approx(J.mean(), rel=1e-12), f"{first}: objective"
    assert np.allclose(coef, ((J - J.mean()) / n).astype(np.float32), rtol=1e-6, atol=1e-12), f"{first}: factors"
    rows_x = feats[:T].reshape(T * n, 64)
    g2 = engine.mlp_backward(rows_x, act.reshape(-1), np.tile(coef, T))
    for k in r0["g"]:
        assert np.array_equal(r0["g"][k], g2[k]), f"{first}: d{k} is not the backward of the recorded rows"
    # every bin: mlp_kernel's logits of all T x n recorded rows in one forward (rows are independent)
    y = run_forward(engine, rows_x, 32).reshape(T, n, 8)
    ids = sc.first_id + np.arange(n)
    n_near = 0
    for t in range(T):
        want, near = mlp_ref.sample_bins(y[t], po.policy_uniform(seed, ids, t))
        wrong = (want != act[t]) & ~near
        assert not wrong.any(), f"{first} step {t}: scenarios {np.nonzero(wrong)[0][:8].tolist()} sampled another bin"
        n_near += int(near.sum())
    if len(runs) > 1:
        r1 = runs[1]
        w2 = f"{what} engine 3 (launched) vs engine 4 (fused)"
        assert np.array_equal(r1["act"], act), f"{w2}: sampled bins differ"
        assert np.array_equal(r1["coef"], coef) and r1["obj"] == r0["obj"], f"{w2}: factors / objective differ"
        _named(w2, lambda: compare(r1["res"], rg))
        assert np.array_equal(r1["feats"], feats), f"{w2}: features differ"
        for k in r0["g"]:
            assert np.array_equal(r1["g"][k], r0["g"][k]), f"{w2}: d{k} differs"
    _tally(key, engine, spec, sc, what, [r["eng"] for r in runs], len(np.unique(act)) >= 2)
    return act.size, n_near


# ---------------------------------------------------------------------------
# The worlds of tests/test_gpu_loop_worlds.py (tests/test_loop_worlds.py holds
# what they reach from the generator alone)
# ---------------------------------------------------------------------------
PER_CASE = 10
FAMILIES = ("d1_rules", "d1_sync15", "d1_keda", "d1_disrupt", "gk_single", "gk_multi", "sk")
FAMILY_SEEDS = 40
WIDE = ("d1_wide", "gk_wide", "sk_wide")
WIDE_SEEDS = 20
NAMED = ("layout12", "layout16", "lds_fits", "lds_over")
DETAIL = ("d1_disrupt", "gk_single", "gk_multi")   # seeds 0-9, and layout12
SAMPLED = ("d1_rules", "d1_keda", "gk_single", "gk_multi", "sk")  # seeds 0-9
LAYOUTS = ((1, 8), (1, 16), (2, 8), (2, 16), (4, 8), (4, 16), (8, 16), (12, 16), (16, 16))
FLAGS = {"hlen > 0": lambda v: v["hlen"] > 0, "nsub > 1": lambda v: v["nsub"] > 1,
         "shared traces": lambda v: v["trace_mod"] == 1, "all_hours 0": lambda v: v["all_hours"] == 0}


def world(name, seed=0):
    import random_worlds as rw
    if name in NAMED:
        return {"layout12": lambda: rw.loop_layout_world(12), "layout16": lambda: rw.loop_layout_world(16),
                "lds_fits": lambda: rw.loop_lds_world(True), "lds_over": lambda: rw.loop_lds_world(False)}[name]()
    return rw.draw(name, seed)


def tally_keys():
    """Every (name, seed) the deterministic-policy cases run: the tally's worlds."""
    return ([(p, s) for p in FAMILIES for s in range(FAMILY_SEEDS)] + [(p, s) for p in WIDE for s in range(WIDE_SEEDS)]
            + [(n, 0) for n in NAMED])


def predicted_row(spec, sc):
    """What a world's run must tally, from the generator alone (no `varying`)."""
    eng = loop_engine(spec, sc)
    return dict(loop_plan(spec, sc), engines=(4, 3) if eng == 4 else (3,))


def tally_counts(rows):
    """rows: {(name, seed): row} -> the counts the floors are set on."""
    out = {}
    for e in (4, 3):
        out[f"engine {e}"] = sum(e in v["engines"] for v in rows.values())
    for e, d, n in sorted({(e, v["dmax"], v["nmax"]) for v in rows.values() for e in v["engines"]}):
        out[f"engine {e} <{d},{n}>"] = sum(e in v["engines"] and (v["dmax"], v["nmax"]) == (d, n) for v in rows.values())
    for name, pred in FLAGS.items():
        out[name] = sum(bool(pred(v)) for v in rows.values())
        out[name + ", launched only"] = sum(bool(pred(v)) and 4 not in v["engines"] for v in rows.values())
    return out


def assert_floors(counts):
    assert counts["engine 4"] >= 10 and counts["engine 3"] >= 10, counts
    missing = [lay for lay in LAYOUTS if counts.get("engine 3 <%d,%d>" % lay, 0) < 1]
    assert not missing, f"register layouts the launched loop never ran: {missing}; {counts}"
    assert counts.get("engine 4 <1,8>", 0) >= 1, counts
    short = {k: counts[k] for k in FLAGS if counts[k] < 5}
    assert not short, f"flags in fewer than 5 worlds: {short}"
