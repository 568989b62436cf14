"""The random-world generator (tests/random_worlds.py) is not vacuous, and the
two CPU restatements agree on its worlds.

1. Activity floors: seeds 0-199 of every profile through the C oracle alone.
   A parity suite over inert worlds proves nothing (hypothesis' worlds() of
   test_spec_model.py: a drift record in 0 % of the worlds, one distinct
   choice hash per world in the median), so the floors below are conditions:
   a generator change that makes the worlds quiet fails here, on the CPU.
2. tests/spec_model.py against the oracle on seeds 0-39 (first 3 scenarios)
   of every world inside spec_model's stated scope (no multi-node
   consolidation, no extra KEDA triggers): every result field and trajectory
   record, fp64 included, with drift and replacement really acting.
3. The wide profiles (random_worlds.WIDE_PROFILES, 100 worlds each): the same
   activity floors, the conditions on the inputs that make the wide shapes
   matter (a launched type beyond position 63 of the capacity order,
   launches in three regions, shared-trace worlds whose scenarios differ on
   one trace), and the spec model on seeds 0-9, first and last 8 scenarios.

4. The time-axis kinds (random_worlds.TIMINGS; run on the GPU by
   tests/test_gpu_time_axis.py): the oracle shows what each kind is drawn
   for. days: a launch, a deletion and a PEAK-flag change at a step >= 1440 in
   every frozen world, 2-4 window edges, late drift in two worlds of
   d1_disrupt and gk_multi; window: the exact number of PEAK-flag changes of
   every switching scenario by sub-kind; short: the clock hour where the start
   minute puts it; delay: no pod ever runs where the delay is >= T; the
   activity floors over the window and delay worlds; spec_model on the first
   three scenarios of every days, window and short world inside its scope
   (the days worlds one case each).
   A few digests of the earlier profiles' worlds are frozen: the generator's
   time-axis argument and its O(T D n) load construction moved none of them.

Run time of this file (8 oracle threads): 30 s before the wide profiles, 51 s
with them, about 7 min with the time-axis kinds (290 s of it
tests/spec_model.py on the 56 days worlds inside its scope)."""
import functools

import numpy as np
import pytest

import pyoracle as po
import random_worlds as rw
from ccka import abi
from test_spec_model import compare_model

SEEDS = range(200)
THREADS = 8


@functools.lru_cache(maxsize=None)
def activity(profile):
    """Per-world activity of a profile's 200 worlds (computed once, read-only)."""
    rows = []
    for seed in SEEDS:
        spec, sc, load = rw.draw(profile, seed)
        res, tr, det = po.rollout(spec, sc, load, traj=True, threads=THREADS, detail=True)
        f, r = tr["flags"], tr["replicas"]
        D = len(spec.deploys)
        r0 = np.array([d.replicas0 for d in spec.deploys])
        rows.append(dict(
            seed=seed, drift_on=bool(spec.drift), replace_on=bool(spec.replace),
            launch=bool(res["launches"].sum() > 0), delete=bool(res["deletions"].sum() > 0),
            hashes=len(np.unique(res["choice_hash"])),
            drift=bool((f & 16).any()), prespun=bool(((f & 48) == 48).any()), evict=bool(((f & 20) == 20).any()),
            repl=bool((f & 32).any()),
            from_zero=bool(((r[:-1] == 0) & (r[1:] > 0)).any()), to_zero=bool(((r[:-1] > 0) & (r[1:] == 0)).any()),
            # deployments whose final replica count left replicas0, most in any scenario
            moved=int((det["desired"][:, :D] != r0[None, :]).sum(axis=1).max())))
    return rows


def share(rows, key, among=None):
    rows = [r for r in rows if among is None or r[among]]
    assert rows, f"no world with {among}"
    return sum(bool(r[key]) for r in rows) / len(rows)


@pytest.mark.parametrize("profile", list(rw.PROFILES))
def test_worlds_are_active(profile):
    rows = activity(profile)
    got = {"launch": share(rows, "launch"), "delete": share(rows, "delete"),
           "hashes": float(np.median([r["hashes"] for r in rows]))}
    print(profile, got)
    assert got["launch"] >= 0.70, got
    assert got["delete"] >= 0.60, got
    assert got["hashes"] >= 16, got


@pytest.mark.parametrize("profile", ["d1_disrupt", "gk_multi"])
def test_disruption_really_acts(profile):
    rows = activity(profile)
    got = {"drift": share(rows, "drift", "drift_on"), "prespun": share(rows, "prespun", "drift_on"),
           "evict": share(rows, "evict", "drift_on"), "repl": share(rows, "repl", "replace_on")}
    print(profile, got)
    assert got["drift"] >= 0.40, got      # a drift record (flags & 16)
    assert got["prespun"] >= 0.30, got    # pre-spun replacement (flags 16 | 32)
    assert got["evict"] >= 0.30, got      # eviction fallback (flags 16 | 4)
    assert got["repl"] >= 0.40, got       # a replacement launched, worlds with replacement on


def test_keda_scales_through_zero():
    rows = activity("d1_keda")
    got = {"from_zero": share(rows, "from_zero"), "to_zero": share(rows, "to_zero")}
    print(got)
    assert got["from_zero"] >= 0.30 and got["to_zero"] >= 0.30, got


def test_skewed_worlds_move_two_deployments():
    got = share([dict(r, two=r["moved"] >= 2) for r in activity("sk")], "two")
    print(got)
    assert got >= 0.60, got


def test_draw_is_a_function_of_profile_and_seed():
    a, b = rw.draw("gk_multi", 7), rw.draw("gk_multi", 7)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0].price, b[0].price)
    assert bytes(a[0].to_c().deploy[0]) == bytes(b[0].to_c().deploy[0])
    assert not np.array_equal(a[2], rw.draw("gk_multi", 8)[2])


def in_model_scope(spec):
    return not spec.multi and all(d.scaler != abi.SCALER_KEDA_TRIGGER for d in spec.deploys)


@pytest.mark.parametrize("profile", list(rw.PROFILES))
def test_spec_model_equals_oracle(profile):
    ran = 0
    for seed in range(40):
        spec, sc, load = rw.draw(profile, seed)
        if not in_model_scope(spec):
            continue
        try:
            compare_model(spec, sc.slice(0, 3), np.ascontiguousarray(load[:, :, :3]))
        except AssertionError as e:
            raise AssertionError(f"{profile} seed {seed}: {e}") from None
        ran += 1
    assert ran >= 10, f"{profile}: only {ran} of 40 worlds inside spec_model's scope"


# ---------------------------------------------------------------------------
# wide profiles
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_activity(profile):
    """Per-world activity of a wide profile's worlds on the oracle (computed once, read-only)."""
    rows = []
    for seed in range(rw.WIDE_SEEDS):
        spec, sc, load = rw.draw(profile, seed)
        res, tr = po.rollout(spec, sc, load, traj=True, threads=THREADS)
        # position of every type in the capacity-descending stable order (d1_check_world)
        pos = np.empty(spec.catalog.k, np.int64)
        pos[np.argsort(-rw.pod_cap1(spec), kind="stable")] = np.arange(spec.catalog.k)
        launched = (tr["flags"] & 2 != 0) & (tr["last_type"] != 0xFFFF)  # a launch this step: last_type is its type
        types = np.unique(tr["last_type"][launched])
        reg = sc.region if sc.region is not None else np.zeros(sc.n, np.uint8)
        row = dict(seed=seed, launch=bool(res["launches"].sum() > 0), delete=bool(res["deletions"].sum() > 0),
                   hashes=len(np.unique(res["choice_hash"])), R=spec.n_regions, traces=sc.n_traces,
                   beyond=bool(types.size and pos[types].max() >= 64), index64=bool(types.size and types.max() >= 64),
                   regions=len(np.unique(reg[res["launches"] > 0])))
        if sc.n_traces:
            col = (sc.first_id + np.arange(sc.n)) % sc.n_traces
            key = np.stack([res["cost_uphmin"], res["choice_hash"].astype(np.int64)], axis=1)
            row["differ"] = any(len(np.unique(key[col == c], axis=0)) > 1 for c in np.unique(col))
        rows.append(row)
    return rows


@pytest.mark.parametrize("profile", list(rw.WIDE_PROFILES))
def test_wide_worlds_are_active(profile):
    rows = wide_activity(profile)
    got = {"launch": share(rows, "launch"), "delete": share(rows, "delete"),
           "hashes": float(np.median([r["hashes"] for r in rows]))}
    print(profile, got)
    assert got["launch"] >= 0.70, got
    assert got["delete"] >= 0.60, got
    assert got["hashes"] >= 16, got


@pytest.mark.parametrize("profile", list(rw.WIDE_PROFILES))
def test_wide_shapes_matter(profile):
    rows = wide_activity(profile)
    multi = [dict(r, three=r["regions"] >= 3) for r in rows if r["R"] >= 3]
    traced = [r for r in rows if r["traces"]]
    got = {"beyond": share(rows, "beyond"), "three_regions": share(multi, "three") if multi else None,
           "index64": share(rows, "index64"), "traced": len(traced)}
    print(profile, got)
    # a launched type at position >= 64 of the capacity-sorted order (the argmin
    # tables' second chunk); on the general kernel the catalog index counts
    # (lane k % 64 on trip k / 64 of the cooperative scans)
    assert got["beyond"] >= 0.60, got
    if profile != "d1_wide":
        assert got["index64"] >= 0.60, got
        assert len(traced) >= 30, got
    assert multi and got["three_regions"] >= 0.50, got
    bad = [r["seed"] for r in traced if not r["differ"]]
    assert not bad, f"{profile}: shared-trace worlds whose scenarios agree on every trace: seeds {bad}"


@pytest.mark.parametrize("profile", list(rw.WIDE_PROFILES))
def test_wide_spec_model_equals_oracle(profile):
    ran = 0
    for seed in range(10):
        spec, sc, load = rw.draw(profile, seed)
        if not in_model_scope(spec):
            continue
        for lo in (0, sc.n - 8):
            cols = load if sc.n_traces else np.ascontiguousarray(load[:, :, lo:lo + 8])
            try:
                compare_model(spec, sc.slice(lo, lo + 8), cols)
            except AssertionError as e:
                raise AssertionError(f"{profile} seed {seed} scenarios {lo}..{lo + 7}: {e}") from None
        ran += 1
    assert ran >= 3, f"{profile}: only {ran} of 10 worlds inside spec_model's scope"


def test_limit_worlds_are_at_the_limits():
    for which, nw, nm in (("weights8", 8, None), ("weights9", 9, None), ("masks8", None, 8), ("masks9", None, 9)):
        spec, sc, _ = rw.limit_world(which)
        if nw:
            assert len(np.unique(sc.carbon_weight)) == nw
        masks = {x.zone_mask for p in spec.pools for x in [p.base] + [p.profile[s] for s in range(3)]} - {0}
        if nm:
            assert len(masks) == nm, (which, masks)
            assert len(np.unique(sc.carbon_weight)) == 8, which  # kind 2: at the weight limit as well
        else:
            assert len(masks) <= 8, (which, masks)


# ---------------------------------------------------------------------------
# time-axis kinds
# ---------------------------------------------------------------------------
def test_earlier_worlds_did_not_move():
    """sha256 of six worlds as the generator drew them before it had a timing
    argument (spec, scenario arrays, load bytes)."""
    want = {("d1_default", 0): "8ce8be91c1760da79acd515e817e450d24eb8320611d4b35dc0d1eabd897e0b9",
            ("gk_multi", 7): "8113649f0d55704102f2e623055a3b5357e02a0403484d030ff248da80eb5625",
            ("sk", 9): "2fac21d1c8d51e7b9d99f0f5cb29c0e4245fd8a0a7f0bfed93685b2a4c006205",
            ("loop", 1): "17c15b453ae5e15f858f4b0217a026c34754c5e4fc66ff73c22f7dd497a4a236",
            ("sk_wide", 3): "19b35ce4ddf99fd0ccf24b964dfaa9cca9c34f45ddaa8f06ed9f036072dc9824",
            ("d1_wide", 4): "fe1792a5892c515f8f9d2807cfa0937bbc0b5aa1cc6fceda366486f6ba903680"}
    got = {k: rw.world_digest(rw.draw(*k)) for k in want}
    assert got == want


def in_window(spec, minute):
    ps, pe = spec.peak_start, spec.peak_end
    return ps <= minute < pe if ps <= pe else (minute >= ps or minute < pe)


@functools.lru_cache(maxsize=None)
def timing_rows(profile, kind):
    """The oracle's view of a kind's worlds of one profile (computed once, read-only)."""
    rows = []
    for seed in rw.timing_seeds(profile, kind):
        spec, sc, load = rw.draw(profile, seed, timing=kind)
        res, tr, det = po.rollout(spec, sc, load, traj=True, threads=THREADS, detail=True)
        f = tr["flags"]
        sw = np.ones(sc.n, bool) if sc.peak_switch is None else sc.peak_switch != 0
        pk = (f & 1)[:, sw].astype(np.int8)
        late = f[1440:]
        rows.append(dict(
            seed=seed, spec=spec, T=spec.n_steps, switching=int(sw.sum()),
            launch=bool(res["launches"].sum() > 0), delete=bool(res["deletions"].sum() > 0),
            changes=np.abs(np.diff(pk, axis=0)).sum(axis=0), pk_any=bool(pk.any()), pk_all=bool(pk.all()),
            pk0=pk[0], pk_quiet=bool((f & 1)[:, ~sw].any()),
            late_launch=bool((late & 2).any()), late_delete=bool((late & 4).any()), late_drift=bool((late & 16).any()),
            late_change=bool(np.diff(pk[1439:], axis=0).any()) if spec.n_steps > 1440 else False,
            running=int((tr["replicas"] - tr["pending"]).sum()), ready=int(det["ready"].sum()),
            pend_min=int(res["pending_pod_minutes"].sum()), deletions=int(res["deletions"].sum())))
    return rows


@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_days_worlds_are_active_after_a_day(profile):
    rows = timing_rows(profile, "days")
    assert len(rows) == (4 if profile == "loop" else 8)
    for r in rows:
        what = f"{profile} days seed {r['seed']}"
        assert 1500 <= r["T"] <= (1800 if profile == "loop" else 3000), what
        assert r["late_launch"] and r["late_delete"] and r["late_change"], f"{what}: {r}"
        assert r["switching"] and 2 <= r["changes"].min() and r["changes"].max() <= 4, f"{what}: {r['changes']}"
        assert not r["pk_quiet"], what  # a scenario that does not switch never shows PEAK
    if profile in ("d1_disrupt", "gk_multi"):
        assert sum(r["late_drift"] for r in rows) >= 2, [r["late_drift"] for r in rows]
    # half of the windows wrap midnight (over all profiles: test below)


def test_days_windows_wrap_midnight_in_half_the_worlds():
    wraps = [r["spec"].peak_start > r["spec"].peak_end for p in rw.TIMING_PROFILES for r in timing_rows(p, "days")]
    assert 0.3 <= sum(wraps) / len(wraps) <= 0.7, sum(wraps)


@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_window_shapes_change_the_peak_flag_as_stated(profile):
    rows = timing_rows(profile, "window")
    assert len(rows) == 20
    for r in rows:
        sub, spec = r["seed"] % 10, r["spec"]
        what = f"{profile} window seed {r['seed']} (sub-kind {sub}, start {spec.start_minute}, window {spec.peak_start}..{spec.peak_end}, T {r['T']})"
        assert 150 <= r["T"] <= 400 and r["switching"], what
        assert (r["changes"] == rw.WINDOW_CHANGES[sub]).all(), f"{what}: {r['changes']}"
        assert not r["pk_quiet"], what
        if sub == 0:
            assert spec.peak_start == spec.peak_end and not r["pk_any"], what
        if sub == 1:
            assert (spec.peak_start, spec.peak_end) == (0, 1440) and r["pk_all"], what
        if sub == 2:
            assert spec.peak_end == 1440 and spec.start_minute + r["T"] > 1440, what
        if sub == 3:
            assert spec.peak_start > spec.peak_end and spec.start_minute + r["T"] > 1440 + spec.peak_end, what
        if sub == 4:
            assert spec.start_minute in (spec.peak_start, spec.peak_end), what
            assert (r["pk0"] == int(in_window(spec, spec.start_minute))).all(), what
            assert (r["pk0"] == int(spec.start_minute == spec.peak_start)).all(), what
        if sub in (5, 6):
            assert (spec.start_minute + r["T"] - (1 if sub == 5 else 0)) % 1440 in (spec.peak_start, spec.peak_end), what
        if sub == 7:
            assert spec.peak_start % 60 == 0 and spec.peak_end % 60 == 0, what
        if sub == 8:
            assert spec.peak_end == spec.peak_start + 1, what
        if sub == 9:
            assert 1440 <= spec.start_minute <= 1440 * 1001 and (spec.peak_end - spec.peak_start) % 1440 in (
                *range(61, 121), *range(1320, 1380)), what
    assert sum(r["spec"].peak_end == 1440 for r in rows) >= 4


@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_short_worlds_hold_their_hour_boundary(profile):
    rows = timing_rows(profile, "short")
    assert [r["T"] for r in rows] == list(rw.SHORT_T)
    for r in rows:
        spec, T = r["spec"], r["T"]
        assert spec.provision_delay_steps in (0, 1, T - 1, T, T + 1)
        if T >= 2:
            at = 1 if r["seed"] % 2 == 0 else T - 1
            assert (spec.start_minute + at) % 60 == 0, (profile, r["seed"])
    assert len({r["spec"].provision_delay_steps >= r["T"] for r in rows}) == 2  # both sides of delay = T


@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_delay_worlds_never_ready_from_t_on(profile):
    rows = timing_rows(profile, "delay")
    assert len(rows) == 16
    big = 0
    for r in rows:
        spec, T = r["spec"], r["T"]
        assert 200 <= T <= 300
        assert spec.provision_delay_steps == (5, 59, 60, 61, T - 1, T, T + 1, rw.MAX_DELAY)[r["seed"] % 8]
        cas = [spec.reset_ca_s] + [x.consolidate_after_s for p in spec.pools for x in [p.base] + [p.profile[q] for q in range(3)]]
        assert (max(cas) >= 3600) == (r["seed"] >= 8), (profile, r["seed"], cas)
        big += max(cas) > 65535 * 60
        if spec.provision_delay_steps >= T:
            # no node ever becomes ready: no pod runs, none is ready at the end, pods wait, nothing is deleted
            assert r["running"] == 0 and r["ready"] == 0 and r["pend_min"] > 0 and r["deletions"] == 0, (profile, r)
    assert big == 2


@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_window_and_delay_worlds_are_active(profile):
    """The floors of the earlier profiles (launches in >= 70 %, deletions in
    >= 60 % of the worlds) hold over each kind where the kind can reach them,
    and over both kinds together. Of the delay kind's 16 worlds, six have a
    delay >= T by construction (no node is ever ready, so none is deleted) and
    two have delay = T - 1 (a node launched at t = 0 is ready for the last
    step alone): no draw lifts the whole kind to 60 % deletions. Its floor is
    therefore set over the eight worlds with a delay < T - 1 (5, 59, 60, 61
    steps), and its launch floor over all sixteen."""
    window, delay = timing_rows(profile, "window"), timing_rows(profile, "delay")
    can = [r for r in delay if r["spec"].provision_delay_steps < r["T"] - 1]
    assert len(can) == 8
    got = {"launch": share(window + delay, "launch"), "delete": share(window + delay, "delete"),
           "window launch": share(window, "launch"), "window delete": share(window, "delete"),
           "delay launch": share(delay, "launch"), "delay delete, delay < T - 1": share(can, "delete")}
    print(profile, got)
    for k, v in got.items():
        assert v >= (0.70 if "launch" in k else 0.60), got


def test_max_and_pending_limit_worlds_are_at_the_limits():
    for profile in rw.MAX_PROFILES:
        spec = rw.draw(profile, 0, timing="max")[0]
        assert (spec.n_steps, spec.start_minute) == (65535, rw.MAX_START) and rw.MAX_START + 65535 == 2**31 - 1
    spec, sc, load = rw.pend_limit_world()
    res, _ = po.rollout(spec, sc, load, threads=THREADS)
    assert spec.provision_delay_steps == spec.n_steps == 65535 and spec.base_nodes == 0
    assert (res["pending_pod_minutes"] == 2_147_385_345).all() and 32767 * 65535 == 2_147_385_345 == 2**31 - 98_303


def test_consolidate_after_limit_world_tells_the_clamp():
    """Empty nodes stand for 65470 steps: never deleted at 66667 steps of
    consolidateAfter, deleted at 32767 (a kernel that clamped its copy at
    0x7FFF would delete them at the first value too)."""
    spec, sc, load = rw.ca_limit_world()
    res, _ = po.rollout(spec, sc, load, threads=THREADS)
    assert rw.CA_BEYOND_T > 65535 * 60 and (res["deletions"] == 0).all()
    assert (res["final_nodes"] >= 2).sum() >= sc.n // 2, res["final_nodes"]
    res, _ = po.rollout(*rw.ca_limit_world(32767 * 60), threads=THREADS)
    assert (res["deletions"] > 0).sum() >= sc.n // 2, res["deletions"]


def model_case(profile, kind, seed):
    """spec_model against the oracle on a time-axis world's first three scenarios; False outside its scope."""
    spec, sc, load = rw.draw(profile, seed, timing=kind)
    if not in_model_scope(spec):
        return False
    try:
        compare_model(spec, sc.slice(0, 3), np.ascontiguousarray(load[:, :, :3]))
    except AssertionError as e:
        raise AssertionError(f"{profile} {kind} seed {seed}: {e}") from None
    return True


@pytest.mark.parametrize("kind", ["window", "short"])
@pytest.mark.parametrize("profile", rw.TIMING_PROFILES)
def test_time_axis_spec_model_equals_oracle(profile, kind):
    ran = sum(model_case(profile, kind, seed) for seed in rw.timing_seeds(profile, kind))
    assert ran >= 1, f"{profile} {kind}: no world inside spec_model's scope"


@pytest.mark.parametrize("profile,seed", [(p, s) for p in rw.TIMING_PROFILES for s in rw.DAYS_SEEDS[p]])
def test_days_spec_model_equals_oracle(profile, seed):
    """Every days world inside spec_model's scope, one case per world (the
    Python model needs 0.4-8 s for a world, 13-34 s for a d1_sync15 one: four
    decisions per step). A world outside the scope (multi-node consolidation,
    extra KEDA triggers) has nothing to compare; the case below holds the count."""
    model_case(profile, "days", seed)


def test_days_spec_model_covers_every_profile():
    """56 of the 68 days worlds are inside the model's scope, at least one of every profile."""
    n = {p: sum(in_model_scope(rw.draw(p, s, timing="days")[0]) for s in rw.DAYS_SEEDS[p]) for p in rw.TIMING_PROFILES}
    assert min(n.values()) >= 1 and sum(n.values()) == 56, n
