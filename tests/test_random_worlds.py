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

Run time of this file: 30 s before the wide profiles, 51 s with them (8 oracle threads)."""
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
