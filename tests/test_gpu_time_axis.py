"""The time axis of every rollout engine against the CPU oracle: multi-day
horizons, every shape of the peak window, horizons of 1-61 steps, provisioning
delays up to the last accepted value, consolidateAfter beyond the horizon, and
the last accepted horizon (65535 steps from start minute INT32_MAX - 65535).

The worlds are random_worlds.draw(profile, seed, timing=kind) for the seeds of
random_worlds.timing_seeds (tests/test_random_worlds.py holds, on the CPU,
what each kind is drawn for). Every world runs on every mode its profile runs
in (test_gpu_random_worlds.MODES, check_world / check_loop: the engine that
ran is asserted, odd seeds draw the lanes per wave; every loop world runs the
fused and the launched loop) and is compared bit for bit, fp64 included, with
its trajectory.

A failure names (profile:kind, seed, engine mode):
random_worlds.draw(profile, seed, timing=kind) reproduces the world."""
import ctypes as C

import numpy as np
import pytest

import random_worlds as rw
from ccka import abi
from parity import compare, oracle, run_engine
from test_gpu_random_worlds import MODES, THREADS, check_loop, check_world

pytestmark = pytest.mark.gpu
ROLLOUT_PROFILES = [p for p in rw.TIMING_PROFILES if p != "loop"]
# worlds per case, so that a case stays within a few seconds
PER_CASE = {"days": 2, "window": 10, "short": 17, "delay": 8, "max": 1}


def run(engine, profile, kind, seed):
    """A loop world runs fused (engine 4, against the oracle's replay) and
    launched (engine 3, equal to the fused run): every loop world of this
    file, where the earlier suite launches seeds 0-49 of 200."""
    world = rw.draw(profile, seed, timing=kind)
    if profile == "loop":
        check_loop(engine, seed, launched=True, world=world)
    else:
        check_world(engine, f"{profile}:{kind}", seed, world=world, modes=MODES[profile])


def cases(kind, profiles=rw.TIMING_PROFILES):
    out = []
    for p in profiles:
        seeds = list(rw.timing_seeds(p, kind))
        out += [pytest.param(p, seeds[i:i + PER_CASE[kind]], id=f"{p}-{seeds[i]}") for i in range(0, len(seeds), PER_CASE[kind])]
    return out


@pytest.mark.parametrize("profile,seeds", cases("days"))
def test_multi_day_horizons(engine, profile, seeds):
    """1500-3000 steps: midnight, the hour carry 23 -> 0 and 2-4 window edges,
    with launches, deletions and PEAK-flag changes after step 1440. The loop
    worlds run fused and launched (engine 3: the resumed launches cross
    midnight with the saved hour)."""
    for seed in seeds:
        run(engine, profile, "days", seed)


@pytest.mark.parametrize("profile,seeds", cases("window"))
def test_peak_window_shapes(engine, profile, seeds):
    """Empty, whole-day, to-midnight and wrapping windows, an edge at t = 0,
    T - 1 and T, edges on clock hours, a one-minute window, a start minute of
    1440 k + m (random_worlds.WINDOW_CHANGES, by seed % 10)."""
    for seed in seeds:
        run(engine, profile, "window", seed)


@pytest.mark.parametrize("profile,seeds", cases("short"))
def test_short_horizons(engine, profile, seeds):
    """1-61 steps with a clock hour at t = 1 or t = T - 1 and delays around T."""
    for seed in seeds:
        run(engine, profile, "short", seed)


@pytest.mark.parametrize("profile,seeds", cases("delay"))
def test_delays_and_consolidate_after(engine, profile, seeds):
    """Delays of 5, 59-61, T - 1, T, T + 1 steps and the last accepted value;
    consolidateAfter of 3600 s, 86400 s and 4e6 s (more than 65535 steps)."""
    for seed in seeds:
        run(engine, profile, "delay", seed)


@pytest.mark.parametrize("profile,seeds", cases("max", rw.MAX_PROFILES))
def test_last_accepted_horizon(engine, profile, seeds):
    """65535 steps from start minute INT32_MAX - 65535, trajectory on."""
    run(engine, profile, "max", seeds[0])


def test_pending_pod_minutes_at_the_32_bit_limit(engine):
    """32767 pods pending for 65535 steps: 2 147 385 345 pod-minutes in every
    scenario (98 303 below 2^31), on the single-deployment engine and on the
    general kernel, equal to the oracle."""
    spec, sc, load = rw.pend_limit_world()
    rc, _ = oracle(spec, sc, load, threads=THREADS)
    assert (rc["pending_pod_minutes"] == 2_147_385_345).all()
    for mode, want in ((0, 2), (1, 1)):
        try:
            engine.set_engine(mode)
            rg, _ = run_engine(engine, spec, sc, load=load)
            got = engine.last_engine()[0]
        finally:
            engine.set_engine(0)
        assert got == want, f"engine mode {mode}: ran on engine {got}, expected {want}"
        assert (rg["pending_pod_minutes"] == 2_147_385_345).all(), rg["pending_pod_minutes"][:4]
        compare(rg, rc)


def test_consolidate_after_beyond_the_horizon(engine):
    """Empty nodes standing for 65470 steps under a consolidateAfter of 66667
    steps are never deleted (the single-deployment kernel keeps min(ca, 0xFFFF)
    steps; at 0x7FFF it would delete them): equal to the oracle on both engines."""
    check_world(engine, "ca_limit", 0, world=rw.ca_limit_world(), modes=MODES["d1_default"])


# Worlds that diverged when this file first ran, frozen by name.
REGRESSIONS = {
    # single-deployment kernel, replacement consolidation (3.G2): the launch of a
    # pre-spun replacement taints its source, but the source's free space stayed in
    # the running sum of free capacity until the replacement was ready. With a
    # delay of 60 / 61 steps a node that became ready meanwhile was evaluated
    # against that sum: an under-utilised node was deleted though its pods did not
    # fit, and the pods were lost (pending went negative). Delays <= 3 hid it.
    "replacement_source_free_space_delay61": ("d1_disrupt", "delay", 11),
}


@pytest.mark.parametrize("name", list(REGRESSIONS))
def test_frozen_time_axis_regressions(engine, name):
    profile, kind, seed = REGRESSIONS[name]
    run(engine, profile, kind, seed)


def test_frozen_regression_without_drift(engine):
    """The same world with drift off: three other scenarios left the oracle."""
    spec, sc, load = rw.draw("d1_disrupt", 11, timing="delay")
    spec.drift = 0
    check_world(engine, "d1_disrupt:delay:no_drift", 11, world=(spec, sc, load), modes=MODES["d1_disrupt"])


METAMORPHIC = ([(p, "window", s) for p in ("d1_default", "d1_disrupt", "gk_single", "gk_multi", "sk") for s in (9, 19)] +
               [(p, "days", rw.DAYS_SEEDS[p][0]) for p in ("d1_default", "d1_disrupt", "gk_multi", "sk")])


@pytest.mark.parametrize("profile,kind,seed", METAMORPHIC)
def test_start_minute_counts_modulo_a_day(engine, profile, kind, seed):
    """The run from start minute 1440 k + m equals the run from m byte for
    byte, results and trajectory (automatic engine, and the forced general
    kernel for the d1 profiles)."""
    spec, sc, load = rw.draw(profile, seed, timing=kind)
    if kind == "days":
        spec.start_minute += 1440 * (1 + seed % 1000)
    assert spec.start_minute >= 1440
    runs = {}
    for start in (spec.start_minute, spec.start_minute % 1440):
        spec.start_minute = start
        for mode, label, want in MODES[profile][:2]:
            if label == "cooperative":
                continue
            try:
                engine.set_engine(mode)
                runs[start >= 1440, mode] = run_engine(engine, spec, sc, load=load, traj=True)
                assert engine.last_engine()[0] == want
            finally:
                engine.set_engine(0)
    for (late, mode), (res, tr) in runs.items():
        if late:
            r0, t0 = runs[False, mode]
            compare(res, r0, tr, t0)
            assert tr.tobytes() == t0.tobytes() and all(res[k].tobytes() == r0[k].tobytes() for k in res), (profile, seed, mode)


REJECTED = {"start_minute": rw.MAX_START + 1, "provision_delay_steps": rw.MAX_DELAY + 1,
            "peak_start_min": 1441, "peak_end_min": -1}
ACCEPTED = {"start_minute": rw.MAX_START, "provision_delay_steps": rw.MAX_DELAY, "peak_start_min": 1440, "peak_end_min": 0}


@pytest.mark.parametrize("field", list(REJECTED))
def test_timing_rules_reject_and_leave_the_context_usable(engine, field):
    """One world past each timing rule gives CCKA_EINVAL (-1); the context
    then takes the rule's last value and runs that world equal to the oracle."""
    spec, sc, load = rw.draw("d1_default", 0, timing="short")
    w = spec.to_c()
    setattr(w, field, REJECTED[field])
    rc = engine.lib.ccka_set_world(engine.ctx, C.byref(w))
    assert rc == -1 and abi.STATUS[rc] == "EINVAL", (field, REJECTED[field], rc)
    setattr(spec, {"peak_start_min": "peak_start", "peak_end_min": "peak_end"}.get(field, field), ACCEPTED[field])
    assert getattr(spec.to_c(), field) == ACCEPTED[field]
    check_world(engine, f"d1_default:short:{field}", 0, world=(spec, sc, load), modes=MODES["d1_default"])


@pytest.mark.parametrize("profile", ["d1_default", "d1_disrupt", "gk_multi", "sk"])
@pytest.mark.parametrize("seed", [3, 13])
def test_window_from_minute_1440(engine, profile, seed):
    """peak_start_min = 1440 with peak_end_min > 0 (the wrapping window of
    sub-kind 3, its start moved to the end of the day): the window is [0, pe),
    in_window compares the raw 1440 (never reached) and the next-edge distance
    of the single-deployment kernel uses 1440 % 1440 = 0: PEAK from midnight
    to pe inside the horizon, equal to the oracle."""
    spec, sc, load = rw.draw(profile, seed, timing="window")
    assert spec.peak_start > spec.peak_end > 0 and spec.start_minute + spec.n_steps > 1440 + spec.peak_end
    spec.peak_start = 1440
    rc, tc = oracle(spec, sc, load, traj=True, threads=THREADS)
    sw = np.ones(sc.n, bool) if sc.peak_switch is None else sc.peak_switch != 0
    pk = (tc["flags"] & 1)[:, sw].astype(np.int8)
    a = 1440 - spec.start_minute  # midnight's step
    assert not pk[:a].any() and pk[a:a + spec.peak_end].all() and not pk[a + spec.peak_end:].any()
    check_world(engine, f"{profile}:window:ps1440", seed, world=(spec, sc, load), modes=MODES[profile])
