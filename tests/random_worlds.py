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

The wide profiles (WIDE_PROFILES, 100 worlds each) leave that shape on purpose:
catalogs of 63-200 types, 1-8 regions laid out over three workgroups of 600
scenarios, 3-4 pools, 9-16 slots, shared traces, 8 carbon weights / zone
masks. Their sub-kinds are chosen by the seed (seed % 3, seed % 4, ...), so
how many worlds take each kernel path is fixed, not a matter of luck.

The time-axis kinds (TIMINGS; draw(profile, seed, timing=kind), seeds from
timing_seeds) keep a profile's builders and replace the time axis: horizons of
1-61, 1500-3000 and 65535 steps, every shape of the peak window, delays up to
the last value ccka_set_world accepts, consolidateAfter beyond the horizon
(_timing_kind, _timing_post). They draw from a stream of their own, so the
worlds of draw(profile, seed) are what they were before the kinds existed
(world_digest; tests/test_random_worlds.py freezes a few).

The closed-loop suite (tests/test_gpu_loop_worlds.py) reuses draw() and adds
named worlds on streams of their own: loop_layout_world (12 and 16 deployment
columns) and loop_lds_world (the two catalogs on either side of the fused
loop's LDS rule).
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
# the wide profiles (100 worlds each): catalogs of 63-200 types, 3-8 regions,
# 600 scenarios in three workgroups, shared traces, the slot / pool limits
WIDE_PROFILES = {
    "d1_wide": 2,      # one HPA deployment: 3-4 pools, 9-16 slots, 63-200 types, up to 8 weights / zone masks
    "gk_wide": 1,      # gk_single / gk_multi worlds, 600 scenarios over 3-8 regions, 65-200 types
    "sk_wide": 5,      # sk worlds, 600 scenarios over 3-8 regions, 64-130 types, 8 / 16 slots
}
WIDE_SEEDS = 100
_PIDX = {p: i for i, p in enumerate(list(PROFILES) + list(WIDE_PROFILES))}


def pod_cap1(spec):
    """Pod capacity per type for deployment 0 (abi_ctx.cpp pod_cap, floored at 0)."""
    ac, am = spec.catalog.alloc()
    d = spec.deploys[0]
    cap = spec.catalog.max_pods.astype(np.int64)
    if d.req_cpu_m > 0:
        cap = np.minimum(cap, ac // d.req_cpu_m)
    if d.req_mem_mi > 0:
        cap = np.minimum(cap, am // d.req_mem_mi)
    return np.maximum(cap, 0)


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
            while zp == zo and Z > 1:  # (one zone: both profiles name it)
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


# the time-axis kinds (draw(profile, seed, timing=kind)): what _timing never draws
TIMINGS = ("days", "window", "short", "delay", "max")
TIMING_PROFILES = ("d1_default", "d1_rules", "d1_sync15", "d1_keda", "d1_disrupt", "gk_single", "gk_multi", "sk", "loop")
SHORT_T = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 59, 60, 61)
# the last values ccka_set_world accepts (csrc/host_rules.h world_timing_invalid)
MAX_START = 2**31 - 1 - 65535
MAX_DELAY = 2**31 - 1 - 65535
WINDOW_CHANGES = (0, 0, 2, 2, 0, 1, 0, 2, 2, 2)  # PEAK-flag changes of a switching scenario, by sub-kind
CA_BEYOND_T = 4_000_000  # seconds: 66667 steps, more than any horizon (and than 0xFFFF)


# days: per profile the first seeds from 0 upward (four for loop) whose oracle
# run shows at a step >= 1440 a launch (flags bit 1), a deletion (bit 2) and a
# change of the PEAK flag in a switching scenario (tests/test_random_worlds.py
# asserts it; a generator change that moves these worlds fails there). Among
# the eight of d1_disrupt (1, 22) and gk_multi (2, 5) two also show a drift
# record (bit 4) that late.
DAYS_SEEDS = {
    "d1_default": (2, 3, 8, 10, 13, 18, 19, 21),
    "d1_rules": (1, 3, 5, 7, 10, 16, 18, 23),
    "d1_sync15": (1, 2, 6, 8, 9, 10, 12, 17),
    "d1_keda": (0, 1, 2, 3, 4, 5, 6, 7),
    "d1_disrupt": (1, 3, 8, 10, 13, 21, 22, 26),
    "gk_single": (1, 6, 12, 13, 14, 15, 18, 19),
    "gk_multi": (1, 2, 5, 8, 9, 10, 11, 12),
    "sk": (1, 2, 3, 6, 7, 9, 10, 12),
    "loop": (13, 14, 36, 48),
}
MAX_PROFILES = ("d1_default", "d1_sync15", "gk_single", "sk")


def timing_seeds(profile, kind):
    """The worlds of a time-axis kind: draw(profile, seed, timing=kind) for these seeds."""
    if kind == "days":
        return DAYS_SEEDS[profile]
    if kind == "max":
        return (0,) if profile in MAX_PROFILES else ()
    return range({"window": 20, "short": len(SHORT_T), "delay": 16}[kind])


def pend_limit_world(n=N_SCEN):
    """One HPA deployment pinned at 32767 replicas for 65535 steps, no node
    ever ready (delay = T): pending_pod_minutes = 32767 x 65535 =
    2 147 385 345 in every scenario, 98 303 below 2^31, the most the
    single-deployment engine admits (D1_REC_SAT pods, n_steps <= 65535)."""
    rng = np.random.default_rng([20251205, 97, 0])
    cat, R, Z = _geo(rng)
    dep = deployment(abi.SCALER_HPA, replicas0=32767, min_r=32767, max_r=32767, target=70, req_cpu=100, req_mem=64,
                     limit_cpu=0, cap_sel=3, pdb=0)
    spec = _world(rng, [dep], _pools(rng, Z, 2), cat, R, Z, 8, timing=("max", 0, False))
    spec.base_nodes, spec.provision_delay_steps = 0, spec.n_steps
    sc = _scenarios(rng, R, (0, 60, 300), n=n)
    sc.max_replicas = None
    return spec, sc, np.zeros((spec.n_steps, 1, n), np.int32)


def ca_limit_world(ca_s=CA_BEYOND_T, n=N_SCEN):
    """The d1_default world of the last accepted horizon with ca_s as every
    pool's consolidateAfter under every profile and no load after step 64:
    the nodes of the first burst stand empty for the remaining 65470 steps.
    At CA_BEYOND_T (66667 steps; the single-deployment kernel clamps its
    copy to 65535, which no node launched at t >= 0 reaches before T) none is
    ever deleted; at 32767 steps they all are (the CPU guard asserts both)."""
    spec, sc, load = draw("d1_default", 0, timing="max")
    for p in spec.pools:
        p.base.consolidate_after_s = ca_s
        for prof in range(3):
            p.profile[prof].consolidate_after_s = -1
    load = load.copy()
    load[64:] = 0
    return spec, sc, load


def _outside(rng, start, T):
    """A minute outside [start, start + T] (T <= 400)."""
    return (start + T + int(rng.integers(30, 1440 - T - 30))) % 1440


def _timing_kind(rng, kind, seed, loop=False):
    """(n_steps, start_minute, peak_start, peak_end, delay or None) of a
    time-axis kind; delay None keeps the profile's own draw (0-3 steps).

    days    1500-3000 steps (loop: 1500-1800) from any minute, any window of
            30-1410 minutes: 2-4 edges, half of the windows wrap midnight
    window  150-400 steps, the window's shape by seed % 10 (WINDOW_CHANGES)
    short   SHORT_T[seed] steps, a clock hour at t = 1 (even seeds) or t = T - 1
            (odd), delay in {0, 1, T - 1, T, T + 1}
    delay   200-300 steps, delay = (5, 59, 60, 61, T - 1, T, T + 1, MAX_DELAY)[seed % 8]
    max     65535 steps from start minute MAX_START"""
    if kind == "days":
        T = int(rng.integers(1500, 1801 if loop else 3001))
        start, ps = int(rng.integers(0, 1440)), int(rng.integers(0, 1440))
        return T, start, ps, (ps + int(rng.integers(30, 1411))) % 1440, None
    if kind == "max":
        ps = int(rng.integers(0, 1440))
        return 65535, MAX_START, ps, (ps + int(rng.integers(30, 1411))) % 1440, None
    if kind == "short":
        T = SHORT_T[seed]
        hour = 60 * int(rng.integers(0, 24))
        start = (hour - (1 if seed % 2 == 0 else T - 1)) % 1440
        edge = (start + int(rng.integers(0, T + 1))) % 1440
        other = int(rng.integers(0, 1440))
        ps, pe = (edge, other) if rng.integers(2) else (other, edge)
        return T, start, ps, pe, pick(rng, [0, 1, T - 1, T, T + 1])
    if kind == "delay":
        T = int(rng.integers(200, 301))
        start = int(rng.integers(0, 1440))
        edge, other = (start + int(rng.integers(20, T - 19))) % 1440, _outside(rng, start, T)
        ps, pe = (edge, other) if rng.integers(2) else (other, edge)
        return T, start, ps, pe, (5, 59, 60, 61, T - 1, T, T + 1, MAX_DELAY)[seed % 8]
    assert kind == "window", kind
    T = int(rng.integers(150, 401))
    start = int(rng.integers(0, 1440))
    sub = seed % 10
    at = lambda t: (start + t) % 1440  # the minute of step t
    if sub == 0:
        ps = pe = int(rng.integers(0, 1441))
    elif sub == 1:
        ps, pe = 0, 1440
    elif sub in (2, 3):  # midnight at step a, the window opens at step b < a
        a = int(rng.integers(40, T - 39))
        start = 1440 - a
        ps = start + int(rng.integers(10, a - 9))
        pe = 1440 if sub == 2 else int(rng.integers(5, T - a - 4))  # closes at step a + pe < T
    elif sub == 4:
        ps, pe = (start, _outside(rng, start, T)) if rng.integers(2) else (_outside(rng, start, T), start)
    elif sub in (5, 6):
        edge = at(T - 1 if sub == 5 else T)
        ps, pe = (edge, _outside(rng, start, T)) if rng.integers(2) else (_outside(rng, start, T), edge)
    elif sub == 7:  # two of the clock hours inside the horizon
        first = 60 - start % 60
        j = rng.choice((T - 1 - first) // 60 + 1, size=2, replace=False)
        ps, pe = at(first + 60 * int(j[0])), at(first + 60 * int(j[1]))
    elif sub == 8:
        ps = at(int(rng.integers(5, T - 5)))
        pe = ps + 1  # (1439 -> 1440: the end of the day)
    else:
        b = int(rng.integers(5, T - 124))
        ps, pe = at(b), at(b + int(rng.integers(61, 121)))
        if rng.integers(2):
            ps, pe = pe, ps
        start += 1440 * int(rng.integers(1, 1001))
    return T, start, ps, pe, None


def _timing_post(spec, sc, kind, seed, profile):
    """consolidateAfter beyond the horizon. delay, seeds 8-15: 3600 s or
    86400 s in pool 0's PEAK or OFFPEAK patch (odd seeds: as the world's
    reset_ca_s, no per-scenario override); seeds 8 and 11 (small delays, so
    nodes get ready and idle): CA_BEYOND_T, more than 65535 steps. max,
    d1_default: pool 0 keeps CA_BEYOND_T under every profile, so a node idle
    for 32768 steps and more stays."""
    p0 = spec.pools[0]
    if kind == "delay" and seed >= 8:
        ca = CA_BEYOND_T if seed in (8, 11) else (3600, 86400)[(seed // 2) % 2]
        if seed % 2:
            spec.reset_ca_s, sc.reset_ca_s = ca, None
            if p0.profile[abi.PROFILE_RESET].consolidate_after_s < 0:
                p0.profile[abi.PROFILE_RESET].consolidate_after_s = 0  # RESET sets it: reset_ca_s applies
        else:
            p0.profile[(abi.PROFILE_PEAK, abi.PROFILE_OFFPEAK)[(seed // 4) % 2]].consolidate_after_s = ca
    if kind == "max" and profile == "d1_default":
        p0.base.consolidate_after_s = CA_BEYOND_T
        for prof in range(3):
            p0.profile[prof].consolidate_after_s = -1


def _scenarios(rng, R, stab_set, cap_set=(1, 2, 3), switch_p=0.85, n=N_SCEN):
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


def _load(rng, T, his, n=N_SCEN):
    """[T][D][n] piecewise-constant bursts, one column per (deployment, scenario).
    O(T D n) in memory: the segment of step t is the number of segment ends
    <= t, found per column by a binary search (a horizon of 65535 steps fits)."""
    D = len(his)
    S = T // 10 + 1
    ends = np.cumsum(rng.integers(10, 41, size=(D, n, S)), axis=2)
    steps = np.arange(T)
    seg = np.empty((D, n, T), np.int64)                                          # < S: ends[..., S - 1] >= 10 S > T
    for d in range(D):
        for i in range(n):
            seg[d, i] = np.searchsorted(ends[d, i], steps, side="right")
    frac = rng.choice(np.array([0.0, 0.125, 0.5, 1.0]), size=(D, n, S))
    lvl = np.ascontiguousarray(np.take_along_axis(frac, seg, axis=2).transpose(2, 0, 1))  # [T][D][n]
    del seg
    lvl *= np.asarray(his, np.float64)[None, :, None]
    load = np.rint(lvl * (1.0 + 0.05 * rng.uniform(-1, 1, size=lvl.shape))).astype(np.int32)
    del lvl
    if rng.integers(4) == 0:  # the int64 utilisation path and negative samples
        edge = rng.random(size=load.shape) < 0.01
        vals = rng.choice(np.array([-5000, 2_000_000_000, 2**31 - 1], np.int32), size=load.shape)
        load = np.where(edge, vals, load)
    return np.ascontiguousarray(load, np.int32)


def _world(rng, deploys, pools, cat, R, Z, max_nodes, timing=None, **kw):
    T, start, ps, pe, delay = _timing(rng) + (None,) if timing is None else _timing_kind(rng, *timing)
    prices = _prices_wide if cat.k > 6 else _prices
    spec = WorldSpec(catalog=cat, ci=rng.uniform(50.0, 700.0, size=(R, 24)), price=prices(rng, cat, R, Z),
                     pools=pools, deploys=deploys, n_steps=T, start_minute=start,
                     provision_delay_steps=pick(rng, [0, 1, 1, 1, 2, 3]), max_nodes=max_nodes,
                     base_nodes=int(rng.integers(0, 4)), base_util=pick(rng, [0.0, 0.25]),
                     slo_util_pct=pick(rng, [100, 150]), pdb_pct=pick(rng, [-1, -1, 0, 50, 50, 80]),
                     peak_start=ps, peak_end=pe, peak_switch=1, reset_ca_s=pick(rng, [0, 30, 90]),
                     carbon_weight=pick(rng, [0.0, 0.5, 2.0]), **kw)
    if delay is not None:
        spec.provision_delay_steps = delay
    return spec


def _geo(rng):
    return _catalog(rng), int(rng.integers(1, 3)), int(rng.integers(2, 5))


HIS = [3000, 9000, 20000]


# ---------------------------------------------------------------------------
# profiles
# ---------------------------------------------------------------------------
def _d1(rng, kind, n=N_SCEN, timing=None):
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
    spec = _world(rng, [dep], pools, cat, R, Z, int(rng.integers(3, 9)), timing=timing, **kw)
    sc = _scenarios(rng, R, stab_set, cap_set, switch_p=0.95 if disrupt else 0.85, n=n)
    return spec, sc, _load(rng, spec.n_steps, [hi], n)


def _gk_single(rng, geo=None, n=N_SCEN, timing=None):
    cat, R, Z = geo or _geo(rng)
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
    spec = _world(rng, [dep], pools, cat, R, Z, slots, timing=timing, **kw)
    sc = _scenarios(rng, R, stab_set, n=n)
    if why == "slots_drift" and sc.peak_switch is not None:
        sc.peak_switch[0] = 1  # one switching scenario: drift is not inert
    return spec, sc, _load(rng, spec.n_steps, [hi], n)


def _gk_multi(rng, geo=None, n=N_SCEN, timing=None):
    cat, R, Z = geo or _geo(rng)
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
    spec = _world(rng, deploys, pools, cat, R, Z, int(rng.integers(8, 17)), timing=timing, **kw)
    sc = _scenarios(rng, R, (0, 60, 300, 480), (2, 3, 3) if disrupt else (1, 2, 3), switch_p=0.95 if disrupt else 0.85,
                    n=n)
    return spec, sc, _load(rng, spec.n_steps, his, n)


def _sk(rng, geo=None, n=N_SCEN, slots=None, timing=None):
    cat, R, Z = geo or _geo(rng)
    n_dep = int(rng.integers(2, 5))
    kinds = ["hpa", "hpa"] + [pick(rng, ["hpa", "static"]) for _ in range(n_dep - 2)]
    deploys = [_hpa(rng, rules=pick(rng, ["default", "ring"]), stab_set=(0, 60, 300, 480), tol_set=(0.1, 0.0, 0.25, 0.05))
               if k == "hpa" else _static(rng) for k in (kinds[i] for i in rng.permutation(n_dep))]
    pools = _pools(rng, Z, int(rng.integers(1, 3)), limits=rng.integers(3) == 0)
    spec = _world(rng, deploys, pools, cat, R, Z, slots or pick(rng, [8, 16]), timing=timing, hpa_sync_s=pick(rng, [0, 60]))
    sc = _scenarios(rng, R, (0, 60, 300, 480), n=n)
    return spec, sc, _load(rng, spec.n_steps, [pick(rng, HIS) for _ in deploys], n)


# ---------------------------------------------------------------------------
# wide profiles: catalogs beyond one wave, 3-8 regions, several workgroups,
# shared traces, the slot / pool / weight / mask limits of the engines
# ---------------------------------------------------------------------------
N_WIDE = 600  # two full 256-thread workgroups and a ragged third
D1_KS = (63, 64, 65, 127, 128, 129, 200)


def _catalog_wide(rng, K, zero_cap=True):
    """K types of few distinct shapes, so many share a pod capacity and the
    runs of equal capacity are long (they straddle positions 63 / 64 and
    127 / 128 of the capacity-sorted order); catalog order is random, so a
    type's index says nothing about its capacity. Index 0 is the base group's
    type; the last index is a type of the smallest shape (2 vCPU, 4 GiB, 8
    pods), so (ties keep catalog order) it is last in the capacity order among
    the types that hold a pod, at a price that wins small claims.
    With zero_cap some types hold no pod at all (max_pods 0)."""
    vcpu = np.array([2] + [pick(rng, [2, 2, 4, 4, 8, 16, 32]) for _ in range(K - 1)], np.int32)
    mem = np.array([8.0] + [float(v * pick(rng, [2, 4, 8])) for v in vcpu[1:]], np.float64)
    pods = np.array([29] + [pick(rng, [8, 17, 29, 58, 110]) for _ in range(K - 1)], np.int32)
    if zero_cap:
        none = 1 + rng.choice(K - 2, size=max(1, K // 25), replace=False)
        pods[none] = 0
    vcpu[K - 1], mem[K - 1], pods[K - 1] = 2, 4.0, 8
    od = np.array([int(v * rng.integers(35000, 60001)) for v in vcpu], np.int64)
    od[K - 1] = 2 * 20000  # and the cheapest for the small claims it holds
    names = ["m6i.large"] + [f"t{k}.x" for k in range(1, K)]
    return Catalog(names, vcpu, mem, pods, od)


def _prices_wide(rng, cat, R, Z):
    """Prices of a wide catalog: per-type discounts by region and zone with
    20 % hour-by-hour noise, so among the many types of one shape the
    cheapest changes with the hour, the region and the zone mask, and (price
    following the vCPU count) with the size of the claim. Types that hold no
    pod are the cheapest of all: a scan that admitted one would choose it."""
    K = cat.k
    od = cat.od_uph[None, :] * (1.0 + 0.08 * np.arange(R))[:, None]
    odz = od[:, None, :, None] * (1.0 + 0.02 * rng.uniform(-1, 1, size=(R, 1, K, Z)))
    disc = rng.uniform(0.3, 0.7, size=(R, 1, K, Z))
    spot = odz * disc * (1.0 + 0.2 * rng.normal(size=(R, 24, K, Z)))
    spot = np.clip(spot, 0.2 * odz, 0.95 * odz)
    odh = odz * (1.0 + 0.05 * rng.uniform(-1, 1, size=(R, 24, K, Z)))
    tile = np.zeros((R, 24, K, Z, 2), np.int32)
    tile[..., 0] = np.rint(spot)
    tile[..., 1] = np.rint(odh)
    tile[:, :, cat.max_pods == 0] //= 8
    miss = pick(rng, [0.0, 0.1, 0.3])
    if miss > 0:
        gone = rng.random(size=(R, 1, K, Z, 2)) < miss
        if rng.integers(2):
            gone = gone | (rng.random(size=tile.shape) < miss / 3)
        gone[:, :, 0, 0, 1] = False
        tile[np.broadcast_to(gone, tile.shape)] = 0
    return tile


def _regions(rng, layout, R, n=N_WIDE, B=256):
    """The region column of n scenarios over workgroups of B.
    sorted: ascending, equal shares (each block spans a few regions, every
      block's lowest region differs);
    shuffled: every block spans all R regions;
    sorted_last: ascending over the full blocks (boundaries off the block
      edges: the first block spans two regions or more), the ragged last block
      holds the highest region alone (its lowest region + span runs past R);
    aligned: one region per block (span 1), three distinct regions."""
    i = np.arange(n)
    if layout == "sorted":
        reg = i * R // n
    elif layout == "shuffled":
        reg = rng.permutation(i % R)
    elif layout == "sorted_last":
        full = n // B * B
        reg = np.where(i < full, np.minimum((i + B // 4) * (R - 1) // full, R - 2), R - 1)
    else:
        reg = np.sort(rng.choice(R, size=3, replace=False))[np.minimum(i // B, 2)]
    return reg.astype(np.uint8)


LAYOUTS = ("sorted", "shuffled", "sorted_last", "aligned")


def layout_span(layout, R, n=N_WIDE, B=256):
    """The largest number of regions one workgroup of B scenarios spans."""
    reg = _regions(np.random.default_rng(0), layout, R, n, B).astype(int)
    return max(int(reg[b:b + B].max() - reg[b:b + B].min()) + 1 for b in range(0, n, B))


def _share_traces(rng, sc, load, seed):
    """Every third world reads shared traces: n_traces in {7, 64, 130} (no
    divisor of 600) with a first_id that is no multiple of it, and per-scenario
    target and replica-bound overrides, so scenarios on one trace differ. One
    world in four has first_id = 2^33 + a draw."""
    n = sc.n
    if (seed // 4) % 4 == 0:
        sc.first_id += 1 << 33
    if seed % 3 != 0:
        return load
    nt = (7, 64, 130)[(seed // 3) % 3]
    if sc.first_id % nt == 0:
        sc.first_id += 1 + int(rng.integers(nt - 1))
    sc.n_traces = nt
    sc.target_util_pct = rng.integers(30, 96, size=n).astype(np.int16)
    sc.max_replicas = rng.integers(5, 61, size=n).astype(np.int16)
    return np.ascontiguousarray(load[:, :, :nt])


def _cap_masks(pools, Z, limit):
    """At most `limit` distinct non-zero zone masks over every patch of the
    pools (the single-deployment engine holds D1_MAX_ZI = 8): later ones are
    folded onto the first `limit`."""
    seen = []
    for p in pools:
        for x in [p.base] + [p.profile[s] for s in range(3)]:
            m = x.zone_mask & ((1 << Z) - 1)
            if m and m not in seen:
                if len(seen) < limit:
                    seen.append(m)
                else:
                    x.zone_mask = seen[m % limit]
    return len(seen)


def _d1_wide(rng, seed, n=N_SCEN, n_weights=None, n_masks=None):
    """kind 0: 3-4 pools, <= 8 slots; kind 1: 9-16 slots, <= 2 pools; kind 2:
    9-16 slots, 3-4 pools and exactly 8 distinct carbon weights. n_weights /
    n_masks: the boundary worlds' exact counts of distinct carbon weights and
    zone masks (4 pools over 4 zones)."""
    kind = seed % 3
    K = D1_KS[(seed // 3) % len(D1_KS)]
    R = pick(rng, [1, 1, 2, 3, 5, 8])
    Z = int(rng.integers(2, 5))
    n_pools = int(rng.integers(3, 5)) if kind != 1 else int(rng.integers(1, 3))
    slots = int(rng.integers(9, 17)) if kind != 0 else int(rng.integers(3, 9))
    if n_masks:
        Z, n_pools = 4, 4
    elif K <= 65 and seed % 2 == 0:
        # the kernel's four 16 KiB rings leave 15 KiB for prices, ci and J under its
        # 80 KiB bound: at 63 types and more only one region of one zone fits (lds_tab 1)
        R, Z = 1, 1
    cat = _catalog_wide(rng, K, zero_cap=K != 65 and rng.integers(3) > 0)
    hi = pick(rng, HIS)
    rules = pick(rng, ["default", "ring"])
    stab_set = (0, 60, 300, 450, 480) if rules == "ring" else (0, 60, 120, 300)
    dep = _hpa(rng, rules=rules, stab_set=stab_set, tol_set=(0.1, 0.0, 0.25))
    pools = _pools(rng, Z, n_pools)
    if n_masks:
        masks = [int(m) for m in 1 + rng.permutation(15)[:n_masks]]
        patches = [x for p in pools for x in [p.base] + [p.profile[s] for s in range(3)]]
        for j, x in enumerate(patches):
            x.zone_mask = masks[j] if j < n_masks else pick(rng, [0] + masks)
    else:
        _cap_masks(pools, Z, 8)
    spec = _world(rng, [dep], pools, cat, R, Z, slots, hpa_sync_s=pick(rng, [0, 60]))
    spec.base_nodes = int(rng.integers(0, 2))
    sc = _scenarios(rng, R, stab_set, n=n)
    if R > 1:
        sc.region = rng.integers(0, R, size=n).astype(np.uint8)
    n_weights = n_weights or (8 if kind == 2 else None)
    if n_weights:
        ws = np.arange(n_weights) * 0.25 + rng.uniform(0.0, 0.2)
        sc.carbon_weight = ws[rng.permutation(np.arange(n) % n_weights)]
    return spec, sc, _load(rng, spec.n_steps, [hi], n)


def _wide_geo(rng, seed, Ks, need_all_hours):
    """(catalog, R, Z, layout) of a gk_wide / sk_wide world. The layout cycles
    with the seed; where all 24 hourly tiles must fit in LDS beside the
    catalog (plan_launch: span x Z <= 4 up to 65 types, <= 2 at 130, never at
    200) the catalog, the zones and R are drawn inside that bound (a span of
    R >= 3 then has one zone), otherwise outside it."""
    layout = LAYOUTS[seed % 4]
    R = int(rng.integers(3, 9))
    if need_all_hours:
        small = [k for k in Ks if k <= 65]
        if layout == "aligned":        # span 1
            K = pick(rng, [k for k in Ks if k <= 130])
            Z = 2 if K > 65 else int(rng.integers(2, 5))
        elif layout == "shuffled":     # span R
            K, Z, R = pick(rng, small), 1, int(rng.integers(3, 5))
        elif layout == "sorted":       # span 2 of R = 3
            K, Z, R = pick(rng, small), 2, 3
        else:                          # sorted_last: span 2 of R = 3 (one region per full block, +1)
            K, Z, R = pick(rng, small), 2, 3
    else:
        K = pick(rng, [k for k in Ks if k > 65])
        Z = int(rng.integers(3, 5)) if K <= 130 else int(rng.integers(2, 5))
        if layout == "aligned":        # span 1 stages all hours up to 130 types
            K = max(Ks)
    return _catalog_wide(rng, K, zero_cap=K != 65), R, Z, layout


def _finish_wide(rng, seed, world, R, layout):
    spec, sc, load = world
    spec.base_nodes = int(rng.integers(0, 2))
    sc.region = _regions(rng, layout, R)
    return spec, sc, _share_traces(rng, sc, load, seed)


def _gk_wide(rng, seed):
    """seed % 4: the region layout; (seed // 4) % 2: all 24 hourly tiles
    staged or one hour at a time; seed % 3 == 0: shared traces; every other
    world has one deployment (as gk_single), the rest several (as gk_multi)."""
    cat, R, Z, layout = _wide_geo(rng, seed, (65, 130, 200), need_all_hours=(seed // 4) % 2 == 0)
    # (one zone leaves drift inert, and with it one of gk_single's reasons: several deployments there)
    draw1 = _gk_single if (seed // 2) % 2 == 0 and Z > 1 else _gk_multi
    return _finish_wide(rng, seed, draw1(rng, geo=(cat, R, Z), n=N_WIDE), R, layout)


def _sk_wide(rng, seed):
    """seed % 4: the region layout; (seed // 4) % 2: 8 or 16 node slots; K = 64
    where (seed // 8) % 4 == 0, so 64 types meet both slot counts; seed % 3 == 0:
    shared traces. Every world stages all 24 hours (sk_eligible)."""
    Ks = (64,) if (seed // 8) % 4 == 0 else (65, 130)
    cat, R, Z, layout = _wide_geo(rng, seed, Ks, need_all_hours=True)
    return _finish_wide(rng, seed, _sk(rng, geo=(cat, R, Z), n=N_WIDE, slots=(8, 16)[(seed // 4) % 2]), R, layout)


def draw(profile: str, seed: int, n: int = N_SCEN, timing: str | None = None):
    """(WorldSpec, ScenarioSet, load [T][D][n] int32) of a profile's world
    number `seed`. n: the scenario count of the `loop` profile's worlds (130;
    600 for several workgroups); the wide profiles fix their own. timing: one
    of TIMINGS in place of _timing's draw (a world stream of its own: the
    profile's builders, another time axis; TIMING_PROFILES only)."""
    if timing is None:
        rng, tm = np.random.default_rng([20251205, _PIDX[profile], seed]), None
    else:
        assert profile in TIMING_PROFILES and timing in TIMINGS, (profile, timing)
        rng = np.random.default_rng([20251205, _PIDX[profile], seed, 1 + TIMINGS.index(timing)])
        tm = (timing, seed, profile == "loop")
    if profile == "d1_wide":
        return _d1_wide(rng, seed)
    if profile == "gk_wide":
        return _gk_wide(rng, seed)
    if profile == "sk_wide":
        return _sk_wide(rng, seed)
    if profile.startswith("d1_"):
        world = _d1(rng, profile, timing=tm)
    elif profile == "gk_single":
        world = _gk_single(rng, timing=tm)
    elif profile == "gk_multi":
        world = _gk_multi(rng, timing=tm)
    elif profile == "sk":
        world = _sk(rng, timing=tm)
    elif profile == "loop":
        world = _d1(rng, "d1_default" if seed % 2 == 0 else "loop_drift", n, timing=tm)
    else:
        raise KeyError(profile)
    if tm:
        _timing_post(world[0], world[1], timing, seed, profile)
    return world


def world_digest(world) -> str:
    """sha256 over everything of a world that reaches an engine: the spec's
    scalar fields, catalog, tiles, pools and deployments, every scenario
    array, and the load bytes."""
    import dataclasses
    import hashlib
    spec, sc, load = world
    h = hashlib.sha256()
    for f in dataclasses.fields(spec):
        v = getattr(spec, f.name)
        if isinstance(v, (int, float, str)):
            h.update(f"{f.name}={v!r};".encode())
    cat = spec.catalog
    h.update(",".join(cat.names).encode())
    for a in (cat.vcpu, cat.mem_gib, cat.max_pods, cat.od_uph, spec.ci, spec.price):
        h.update(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    for x in list(spec.pools) + list(spec.deploys):
        h.update(bytes(x))
    h.update(f"{sc.n},{sc.first_id},{sc.n_traces};".encode())
    for name in sc._DT:
        a = getattr(sc, name)
        h.update(name.encode() + (b"-" if a is None else str(a.dtype).encode() + np.ascontiguousarray(a).tobytes()))
    h.update(str(load.dtype).encode() + str(load.shape).encode() + np.ascontiguousarray(load).tobytes())
    return h.hexdigest()


def limit_world(which: str):
    """The d1_wide worlds at the single-deployment engine's limits: 8 distinct
    carbon weights or zone masks stay on it (engine 2), 9 go to the general
    kernel (D1_MAX_WC, D1_MAX_ZI)."""
    what, count = {"weights8": ("w", 8), "weights9": ("w", 9), "masks8": ("m", 8), "masks9": ("m", 9)}[which]
    seed = 4 if what == "w" else 5  # kinds 1 (two pools) and 2 (four pools)
    rng = np.random.default_rng([20251205, 98, seed])
    return _d1_wide(rng, seed, n_weights=count if what == "w" else None, n_masks=count if what == "m" else None)


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


def loop_layout_world(n_deploy: int):
    """The closed-loop worlds of the two widest register layouts (kernel_dims:
    12 and 16 deployment columns on 16 slots): n_deploy in (12, 16) columns
    mixing HPA, static and KEDA deployments, one KEDA ScaledObject with two
    triggers among them, 3 pools with limits, 130 scenarios, 90-120 steps with
    an hour boundary and one edge of the peak window inside."""
    assert n_deploy in (12, 16), n_deploy
    rng = np.random.default_rng([20251205, 96, n_deploy])
    cat, R, Z = _geo(rng)
    on = int(rng.integers(0, 8))
    disrupt = on != 0
    cap_set = (2, 3) if disrupt else (1, 2, 3)
    groups = [["hpa"], ["keda", "trigger"], ["static"]]
    while sum(len(g) for g in groups) < n_deploy:
        groups.append([pick(rng, ["hpa", "hpa", "static", "keda"])])
    deploys, his = [], []
    for j in rng.permutation(len(groups)):
        hi = pick(rng, [3000, 9000])
        for k in groups[j]:
            if k == "hpa":
                deploys.append(_hpa(rng, rules=pick(rng, ["default", "ring"]), tol_set=(0.1, 0.0, 0.25), cap_set=cap_set,
                                    big=disrupt))
            elif k == "static":
                deploys.append(_static(rng))
            elif k == "keda":
                deploys.append(_keda(rng, hi, cap_set))
            else:
                deploys.append(keda_trigger(pick(rng, [300, 700, 2000]), pick(rng, [0, 200, hi // 8 + hi // 20])))
            his.append(hi)
    assert len(deploys) == n_deploy
    pools = _pools(rng, Z, 3, disrupt=disrupt, limits=True)
    spec = _world(rng, deploys, pools, cat, R, Z, 16, drift=on & 1, replace=(on >> 1) & 1, multi=(on >> 2) & 1)
    T = int(rng.integers(90, 121))  # >= 60: a clock hour inside
    start = int(rng.integers(0, 1440))
    edge, other = (start + int(rng.integers(20, T - 19))) % 1440, _outside(rng, start, T)
    spec.n_steps, spec.start_minute = T, start
    spec.peak_start, spec.peak_end = (edge, other) if rng.integers(2) else (other, edge)
    sc = _scenarios(rng, R, (0, 60, 300, 480), (2, 3, 3) if disrupt else (1, 2, 3), switch_p=0.95 if disrupt else 0.85)
    return spec, sc, _load(rng, T, his)


def loop_lds_world(fits: bool):
    """The two worlds on either side of the fused closed loop's LDS rule
    (abi_policy.cpp policy_loop: the general kernel's LDS, rounded up to 16,
    plus the MLP's 149,632 B within 160 KiB): one HPA deployment on 8 slots,
    two zones, two regions in the one block of 130 scenarios (span 2), and a
    catalog of K types (fits) or K + 1, K the largest count for which the
    restated rule (loop_check.fuses) admits the fused loop. The K-type world
    is the other one without catalog entry (K + 1) // 2: same stream, same
    prices, scenarios and load."""
    from loop_check import fuses
    R = Z = 2
    K = max(k for k in range(1, abi.MAX_TYPES) if fuses(k, Z, R, 1, 8))
    assert not fuses(K + 1, Z, R, 1, 8)
    rng = np.random.default_rng([20251205, 95, 0])
    cat = _catalog_wide(rng, K + 1, zero_cap=False)
    hi = pick(rng, HIS)
    dep = _hpa(rng, tol_set=(0.1, 0.0, 0.25))
    spec = _world(rng, [dep], _pools(rng, Z, 2), cat, R, Z, 8)
    sc = _scenarios(rng, R, (0, 60, 120, 300))
    sc.region = (rng.permutation(N_SCEN) % R).astype(np.uint8)
    load = _load(rng, spec.n_steps, [hi])
    if fits:
        keep = np.arange(K + 1) != (K + 1) // 2
        spec.catalog = Catalog([n for n, k in zip(cat.names, keep) if k], cat.vcpu[keep], cat.mem_gib[keep],
                               cat.max_pods[keep], cat.od_uph[keep])
        spec.price = np.ascontiguousarray(spec.price[:, :, keep])
    return spec, sc, load
