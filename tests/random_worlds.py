"""TEST INFRASTRUCTURE: seeded random worlds for the GPU-vs-oracle parity suite
(tests/test_gpu_random_worlds.py) and its CPU guard (tests/test_random_worlds.py).

draw(profile, seed) -> (spec, scenarios, load) is a pure function of its
arguments (np.random.default_rng keyed by both), so a failure names the world
that reproduces it. Every draw stays inside what ccka_set_world and
ccka_set_scenarios document as valid; each profile is shaped to land on one
engine by construction (the eligibility rules of abi_ctx.cpp d1_check_world /
d1_prepare, abi_rollout.cpp sk_eligible, abi_policy.cpp policy_loop), see
PROFILES.

Common shape, the smallest at which the kernels can still go wrong: 130
scenarios (two full waves and a ragged one), 90-240 steps from a random start
minute with one peak-window boundary and at least one hour boundary inside,
2-6 instance types over 1-2 regions and 2-4 zones, 0 / 10 / 30 % of the
offerings missing, 1-2 pools (up to 3 on the general kernel) with random base
and profile patches, per-scenario overrides, and a per-scenario piecewise
constant burst load (levels 0, hi/8, hi/2, hi held 10-40 steps, 5 % noise;
in one world of four 1 % of the samples are -5000, 2e9 or 2^31 - 1).
The worlds are tuned for activity (launches, deletions, drift, replacement):
tests/test_random_worlds.py holds the floors.
"""
from __future__ import annotations

import numpy as np

from ccka import abi
from ccka.world import (Catalog, ScenarioSet, WorldSpec, default_down, default_up, deployment, hpa_rules,
                        keda_trigger, patch)

N_SCEN = 130
WEOU, WE = abi.WHEN_EMPTY_OR_UNDERUTILIZED, abi.WHEN_EMPTY
SPOT, OD = abi.CAP_SPOT, abi.CAP_OD

# profile -> the engine an automatic rollout must report (ccka_debug_last_engine)
PROFILES = {
    "d1_default": 2,   # one HPA deployment, default behavior, windows <= 300 s: 4-record ring
    "d1_rules": 2,     # ring-sized random behavior rules: the generic instantiation
    "d1_sync15": 2,    # 15 s sync, default behavior, windows <= 315 s: NSUB 4
    "d1_keda": 2,      # one single-trigger KEDA ScaledObject, scale to / from zero
    "d1_disrupt": 2,   # drift / replacement / multi-node consolidation: DRIFT instantiation
    "gk_single": 1,    # one deployment the single-deployment engine must refuse
    "gk_multi": 1,     # 2-6 deployments mixing HPA, static and KEDA with 1-3 triggers
    "sk": 5,           # 2-4 HPA / static deployments on the lane-skewed schedule
    "loop": 4,         # closed-loop worlds (fused loop; 3 when the fused loop is switched off)
}
_PIDX = {p: i for i, p in enumerate(PROFILES)}


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


# ---------------------------------------------------------------------------
# catalog, prices, carbon
# ---------------------------------------------------------------------------
def _catalog(rng):
    K = int(rng.integers(2, 7))
    vcpu = [2] + [pick(rng, [2, 4, 8, 16, 32]) for _ in range(K - 1)]
    mem = [8.0] + [float(v * pick(rng, [2, 4, 8])) for v in vcpu[1:]]
    pods = [29] + [pick(rng, [8, 17, 29, 58, 110]) for _ in range(K - 1)]
    od = [int(v * rng.integers(35000, 60001)) for v in vcpu]
    names = ["m6i.large"] + [f"t{k}.x" for k in range(1, K)]  # index 0: the base node group's type
    return Catalog(names, np.array(vcpu, np.int32), np.array(mem, np.float64), np.array(pods, np.int32),
                   np.array(od, np.int64))


def _prices(rng, cat, R, Z):
    K = cat.k
    od = cat.od_uph[None, :] * (1.0 + 0.08 * np.arange(R))[:, None]                      # [R][K]
    odz = od[:, None, :, None] * (1.0 + 0.02 * rng.uniform(-1, 1, size=(R, 1, K, Z)))    # per-zone jitter
    disc = rng.uniform(0.25, 0.7, size=(R, 1, K, Z))
    spot = odz * disc * (1.0 + 0.1 * rng.normal(size=(R, 24, K, Z)))
    spot = np.clip(spot, 0.2 * odz, 0.95 * odz)
    tile = np.zeros((R, 24, K, Z, 2), np.int32)
    tile[..., 0] = np.rint(spot)
    tile[..., 1] = np.rint(np.broadcast_to(odz, spot.shape))
    # in one world of four the largest type is the cheapest offer for any claim:
    # a node's pod capacity is its type's, not the claim's bracket (SEMANTICS 3.F)
    if rng.integers(4) == 0:
        big = int(np.argmax(cat.vcpu))
        tile[:, :, big] = np.maximum(tile[:, :, big] // 20, 1)
    miss = pick(rng, [0.0, 0.1, 0.3])
    if miss > 0:
        gone = rng.random(size=(R, 1, K, Z, 2)) < miss             # an offering absent all day
        if rng.integers(2):
            gone = gone | (rng.random(size=tile.shape) < miss / 3)  # and hour by hour
        gone[:, :, 0, 0, 1] = False                                 # the base group's own offering stays
        tile[np.broadcast_to(gone, tile.shape)] = 0
    return tile


# ---------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------
def _mask(rng, Z):
    return int(rng.integers(1, 1 << Z))


def _pools(rng, Z, n_pools, disrupt=False, limits=False):
    pools = []
    for q in range(n_pools):
        p = abi.Pool()
        p.limit_cpu_m, p.limit_mem_mi = -1, -1
        if limits and (q == 0 or rng.integers(2)):
            if rng.integers(2):
                p.limit_cpu_m = pick(rng, [8000, 16000, 48000])
            else:
                p.limit_mem_mi = pick(rng, [32768, 131072])
        p.budget_pct = pick(rng, [34, 50, 100] if disrupt and q == 0 else [10, 34, 50, 100])
        last = q == n_pools - 1
        if disrupt:
            # WhenEmptyOrUnderutilized, on-demand admitted, OFFPEAK and PEAK zones differ
            caps = SPOT | OD if last else pick(rng, [OD, SPOT | OD])
            p.base = patch(WEOU, pick(rng, [0, 30, 60]), _mask(rng, Z), caps)
            p.profile[abi.PROFILE_RESET] = patch(pick(rng, [0, WEOU]), pick(rng, [-1, 0, 30]), 0, 0)
            zo = _mask(rng, Z)
            zp = _mask(rng, Z)
            while zp == zo:
                zp = _mask(rng, Z)
            if rng.integers(2) and (zo & ~zp):  # disjoint: every node of the old profile drifts
                zo &= ~zp
            p.profile[abi.PROFILE_OFFPEAK] = patch(pick(rng, [0, WEOU]), pick(rng, [-1, 0, 30, 60]), zo, 0)
            p.profile[abi.PROFILE_PEAK] = patch(pick(rng, [0, WEOU, WEOU, WE]), pick(rng, [-1, 0, 60, 120]), zp, 0)
        else:
            caps = SPOT | OD if last else int(rng.integers(1, 4))
            p.base = patch(pick(rng, [WE, WEOU]), pick(rng, [0, 30, 60, 120]), _mask(rng, Z), caps)
            for prof in range(3):
                p.profile[prof] = patch(pick(rng, [0, WE, WEOU, WEOU]), pick(rng, [-1, -1, 0, 30, 60, 120, 300]),
                                        pick(rng, [0, _mask(rng, Z)]), pick(rng, [0, 0, caps]))
        pools.append(p)
    return pools


# ---------------------------------------------------------------------------
# deployments
# ---------------------------------------------------------------------------
def _ring_rules(rng, up):
    """Behavior rules the 8-decision register rings hold: <= 2 policies, periods and windows <= 480 s."""
    sel = pick(rng, [abi.SELECT_MAX] * 4 + [abi.SELECT_MIN] * 3 + [abi.SELECT_DISABLED])
    pols = [(pick(rng, [abi.HPA_PODS, abi.HPA_PERCENT]), int(rng.integers(1, 151)),
             pick(rng, [15, 60, 120, 240, 420, 480])) for _ in range(int(rng.integers(1, 3)))]
    stab = pick(rng, [0, 0, 60, 120] if up else [0, 60, 180, 300, 450, 480])
    return hpa_rules(sel, pols, stab)


def _hpa(rng, rules="default", stab_set=(0, 60, 120, 300), tol_set=(0.1,), cap_set=(1, 2, 3), big=False):
    if rules == "ring":
        up, down = _ring_rules(rng, True), _ring_rules(rng, False)
    else:
        up, down = default_up(), default_down(pick(rng, list(stab_set)))
    return deployment(abi.SCALER_HPA, replicas0=int(rng.integers(1, 7)), min_r=int(rng.integers(0, 3)),
                      max_r=int(rng.integers(10, 61)), target=int(rng.integers(40, 91)),
                      req_cpu=pick(rng, [250, 500, 900] if big else [100, 200, 250, 500]),
                      req_mem=pick(rng, [64, 128, 512]), limit_cpu=pick(rng, [0, 500, 1000]),
                      cap_sel=pick(rng, list(cap_set)), pdb=int(rng.integers(2)), tol=pick(rng, list(tol_set)),
                      up=up, down=down)


def _keda(rng, hi, cap_set=(1, 2, 3)):
    return deployment(abi.SCALER_KEDA, replicas0=pick(rng, [0, 0, 1, 3]), keda_min=pick(rng, [0, 0, 0, 1]),
                      keda_max=int(rng.integers(6, 41)), keda_threshold=pick(rng, [100, 300, 700, 2000]),
                      keda_activation=pick(rng, [0, 200, hi // 8 + hi // 20]), keda_cooldown=pick(rng, [0, 60, 120, 300]),
                      req_cpu=pick(rng, [200, 250, 500, 900]), req_mem=pick(rng, [64, 128, 512, 2048]),
                      limit_cpu=pick(rng, [0, 500, 1000]), cap_sel=pick(rng, list(cap_set)), pdb=int(rng.integers(2)),
                      tol=pick(rng, [0.1, 0.1, 0.0, 0.25]), down=default_down(pick(rng, [0, 60, 300, 480])))


def _static(rng):
    n = int(rng.integers(1, 7))
    return deployment(abi.SCALER_STATIC, n, n, n, req_cpu=pick(rng, [100, 200, 400]), req_mem=pick(rng, [64, 256]),
                      cap_sel=int(rng.integers(1, 4)), pdb=int(rng.integers(2)))


# ---------------------------------------------------------------------------
# time, scenarios, load
# ---------------------------------------------------------------------------
def _timing(rng):
    """(n_steps, start_minute, peak_start, peak_end): exactly one edge of the
    peak window falls inside the horizon (T >= 90 puts an hour boundary there too)."""
    T = int(rng.integers(90, 241))
    start = int(rng.integers(0, 1440))
    edge = (start + int(rng.integers(20, T - 19))) % 1440
    other = (start + T + int(rng.integers(30, 1440 - T - 30))) % 1440  # outside [start, start + T)
    return (T, start, edge, other) if rng.integers(2) else (T, start, other, edge)


def _scenarios(rng, R, stab_set, cap_set=(1, 2, 3), switch_p=0.85):
    n = N_SCEN
    kw = {}
    if rng.random() < 0.6:
        kw["target_util_pct"] = rng.integers(30, 96, size=n).astype(np.int16)
    if rng.random() < 0.6:
        kw["max_replicas"] = rng.integers(5, 61, size=n).astype(np.int16)
    if rng.random() < 0.75:
        kw["cap_sel"] = rng.choice(np.array(cap_set, np.uint8), size=n)
    if rng.random() < 0.6:
        kw["down_stab_s"] = rng.choice(np.array(stab_set, np.int16), size=n)
    if R > 1 and rng.random() < 0.8:
        kw["region"] = rng.integers(0, R, size=n).astype(np.uint8)
    if rng.random() < 0.6:  # at most 3 distinct weights (the single-deployment engine holds 8)
        ws = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 3.0]), size=int(rng.integers(1, 4)), replace=False)
        kw["carbon_weight"] = rng.choice(ws, size=n)
    if rng.random() < 0.6:
        kw["reset_ca_s"] = rng.choice(np.array([0, 30, 60, 200], np.int16), size=n)
    if rng.random() < 0.6:
        kw["peak_switch"] = (rng.random(size=n) < switch_p).astype(np.uint8)
    return ScenarioSet(n, int(rng.integers(0, 1001)), **kw)


def _load(rng, T, his):
    """[T][D][n] piecewise-constant bursts, one column per (deployment, scenario)."""
    D, n = len(his), N_SCEN
    S = T // 10 + 1
    ends = np.cumsum(rng.integers(10, 41, size=(D, n, S)), axis=2)
    seg = (ends[None] <= np.arange(T)[:, None, None, None]).sum(axis=3)          # [T][D][n]
    frac = rng.choice(np.array([0.0, 0.125, 0.5, 1.0]), size=(D, n, S))
    lvl = np.take_along_axis(np.broadcast_to(frac[None], (T, D, n, S)), seg[..., None], axis=3)[..., 0]
    lvl = lvl * np.asarray(his, np.float64)[None, :, None]
    load = np.rint(lvl * (1.0 + 0.05 * rng.uniform(-1, 1, size=lvl.shape))).astype(np.int32)
    if rng.integers(4) == 0:  # the int64 utilisation path and negative samples
        edge = rng.random(size=load.shape) < 0.01
        vals = rng.choice(np.array([-5000, 2_000_000_000, 2**31 - 1], np.int32), size=load.shape)
        load = np.where(edge, vals, load)
    return np.ascontiguousarray(load, np.int32)


def _world(rng, deploys, pools, cat, R, Z, max_nodes, **kw):
    T, start, ps, pe = _timing(rng)
    return WorldSpec(catalog=cat, ci=rng.uniform(50.0, 700.0, size=(R, 24)), price=_prices(rng, cat, R, Z),
                     pools=pools, deploys=deploys, n_steps=T, start_minute=start,
                     provision_delay_steps=pick(rng, [0, 1, 1, 1, 2, 3]), max_nodes=max_nodes,
                     base_nodes=int(rng.integers(0, 4)), base_util=pick(rng, [0.0, 0.25]),
                     slo_util_pct=pick(rng, [100, 150]), pdb_pct=pick(rng, [-1, -1, 0, 50, 50, 80]),
                     peak_start=ps, peak_end=pe, peak_switch=1, reset_ca_s=pick(rng, [0, 30, 90]),
                     carbon_weight=pick(rng, [0.0, 0.5, 2.0]), **kw)


def _geo(rng):
    return _catalog(rng), int(rng.integers(1, 3)), int(rng.integers(2, 5))


HIS = [3000, 9000, 20000]


# ---------------------------------------------------------------------------
# profiles
# ---------------------------------------------------------------------------
def _d1(rng, kind):
    cat, R, Z = _geo(rng)
    hi = pick(rng, HIS)
    kw = {}
    stab_set = (0, 60, 120, 300)
    cap_set = (1, 2, 3)
    disrupt = kind == "d1_disrupt" or kind == "loop_drift"
    if kind == "d1_default":
        dep = _hpa(rng, tol_set=(0.1, 0.1, 0.0, 0.25))
        kw["hpa_sync_s"] = pick(rng, [0, 60])
    elif kind == "d1_rules":
        stab_set = (0, 60, 300, 450, 480)
        dep = _hpa(rng, rules="ring", tol_set=(0.0, 0.1, 0.25))
    elif kind == "d1_sync15":
        stab_set = (0, 60, 300, 315)
        dep = _hpa(rng, stab_set=stab_set)
        kw["hpa_sync_s"] = 15
    elif kind == "d1_keda":
        dep = _keda(rng, hi)
    else:
        cap_set = (2, 3, 3)  # on-demand admitted
        dep = _hpa(rng, cap_set=(2, 3), big=True)
        on = int(rng.integers(1, 8)) if kind == "d1_disrupt" else 1
        kw.update(drift=on & 1, replace=(on >> 1) & 1, multi=(on >> 2) & 1)
    pools = _pools(rng, Z, int(rng.integers(1, 3)), disrupt=disrupt)
    spec = _world(rng, [dep], pools, cat, R, Z, int(rng.integers(3, 9)), **kw)
    sc = _scenarios(rng, R, stab_set, cap_set, switch_p=0.95 if disrupt else 0.85)
    return spec, sc, _load(rng, spec.n_steps, [hi])


def _gk_single(rng):
    cat, R, Z = _geo(rng)
    hi = pick(rng, HIS)
    why = pick(rng, ["pool_limit", "slots_drift", "policies3", "window", "sync30"])
    kw = {}
    stab_set = (0, 60, 300, 480)
    dep = _hpa(rng, rules=pick(rng, ["default", "ring"]), tol_set=(0.1, 0.0, 0.25))
    slots = int(rng.integers(3, 9))
    if why == "slots_drift":  # drift that can act, beyond the DRIFT instantiation's 8 slots
        slots = int(rng.integers(9, 17))
        kw["drift"] = 1
        hi = 20000
    elif why == "policies3":
        r = dep.up if rng.integers(2) else dep.down
        r.n_policies = 3
        for q in range(3):
            r.policies[q].type = pick(rng, [abi.HPA_PODS, abi.HPA_PERCENT])
            r.policies[q].value = int(rng.integers(1, 151))
            r.policies[q].period_s = pick(rng, [15, 60, 240])
    elif why == "window":  # beyond the register rings: the HBM history
        dep.down.stab_window_s = pick(rng, [540, 900, 1800])
        stab_set = (0, 300, 600, 1200)
    elif why == "sync30":
        kw["hpa_sync_s"] = 30
    if why != "slots_drift" and rng.integers(3) == 0:
        on = int(rng.integers(1, 8))
        kw.update(drift=on & 1, replace=(on >> 1) & 1, multi=(on >> 2) & 1)
    disrupt = bool(kw.get("drift") or kw.get("replace") or kw.get("multi"))
    pools = _pools(rng, Z, int(rng.integers(1, 4)), disrupt=disrupt, limits=why == "pool_limit")
    spec = _world(rng, [dep], pools, cat, R, Z, slots, **kw)
    sc = _scenarios(rng, R, stab_set)
    if why == "slots_drift" and sc.peak_switch is not None:
        sc.peak_switch[0] = 1  # one switching scenario: drift is not inert
    return spec, sc, _load(rng, spec.n_steps, [hi])


def _gk_multi(rng):
    cat, R, Z = _geo(rng)
    on = int(rng.integers(0, 8))
    kw = dict(drift=on & 1, replace=(on >> 1) & 1, multi=(on >> 2) & 1)
    disrupt = on != 0
    n_dep = int(rng.integers(2, 7))
    kinds = [pick(rng, ["hpa", "hpa", "static", "keda"]) for _ in range(n_dep)]
    if "hpa" not in kinds:
        kinds[0] = "hpa"
    if not disrupt and n_dep <= 4 and "keda" not in kinds:
        kinds[int(rng.integers(1, n_dep))] = "keda"  # HPA / static alone would take the skewed schedule
    deploys, his = [], []
    cap_set = (2, 3) if disrupt else (1, 2, 3)
    for k in kinds:
        hi = pick(rng, HIS)
        if k == "hpa":
            deploys.append(_hpa(rng, rules=pick(rng, ["default", "ring"]), tol_set=(0.1, 0.0, 0.25), cap_set=cap_set,
                                big=disrupt))
            his.append(hi)
        elif k == "static":
            deploys.append(_static(rng))
            his.append(hi)
        else:
            deploys.append(_keda(rng, hi, cap_set))
            his.append(hi)
            for _ in range(int(rng.integers(0, 3))):  # 1-3 triggers in all
                deploys.append(keda_trigger(pick(rng, [300, 700, 2000]), pick(rng, [0, 200, hi // 8 + hi // 20])))
                his.append(hi)
    pools = _pools(rng, Z, int(rng.integers(1, 4)), disrupt=disrupt, limits=rng.integers(3) == 0)
    spec = _world(rng, deploys, pools, cat, R, Z, int(rng.integers(8, 17)), **kw)
    sc = _scenarios(rng, R, (0, 60, 300, 480), (2, 3, 3) if disrupt else (1, 2, 3), switch_p=0.95 if disrupt else 0.85)
    return spec, sc, _load(rng, spec.n_steps, his)


def _sk(rng):
    cat, R, Z = _geo(rng)
    n_dep = int(rng.integers(2, 5))
    kinds = ["hpa", "hpa"] + [pick(rng, ["hpa", "static"]) for _ in range(n_dep - 2)]
    deploys = [_hpa(rng, rules=pick(rng, ["default", "ring"]), stab_set=(0, 60, 300, 480), tol_set=(0.1, 0.0, 0.25, 0.05))
               if k == "hpa" else _static(rng) for k in (kinds[i] for i in rng.permutation(n_dep))]
    pools = _pools(rng, Z, int(rng.integers(1, 3)), limits=rng.integers(3) == 0)
    spec = _world(rng, deploys, pools, cat, R, Z, pick(rng, [8, 16]), hpa_sync_s=pick(rng, [0, 60]))
    sc = _scenarios(rng, R, (0, 60, 300, 480))
    return spec, sc, _load(rng, spec.n_steps, [pick(rng, HIS) for _ in deploys])


def draw(profile: str, seed: int):
    """(WorldSpec, ScenarioSet, load [T][D][130] int32) of a profile's world number `seed`."""
    rng = np.random.default_rng([20251205, _PIDX[profile], seed])
    if profile.startswith("d1_"):
        return _d1(rng, profile)
    if profile == "gk_single":
        return _gk_single(rng)
    if profile == "gk_multi":
        return _gk_multi(rng)
    if profile == "sk":
        return _sk(rng)
    if profile == "loop":
        return _d1(rng, "d1_default" if seed % 2 == 0 else "loop_drift")
    raise KeyError(profile)


def boundary_world(which: str):
    """The two worlds at the edge of the skewed schedule's packed tolerance band
    (16-bit halves: targets < 2^15, tolerance < 1): two HPA deployments, no
    per-scenario target override, world target 40000 % or tolerance 1.5."""
    rng = np.random.default_rng([20251205, 99, {"target40000": 0, "tolerance1_5": 1}[which]])
    cat, R, Z = _geo(rng)
    deploys = [_hpa(rng), _hpa(rng)]
    if which == "target40000":
        deploys[0].target_util_pct = 40000
    else:
        deploys[1].tolerance = 1.5
    spec = _world(rng, deploys, _pools(rng, Z, 2), cat, R, Z, 8)
    sc = _scenarios(rng, R, (0, 60, 300))
    sc.target_util_pct = None
    return spec, sc, _load(rng, spec.n_steps, [9000, 9000])
