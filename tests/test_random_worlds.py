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
   record, fp64 included, with drift and replacement really acting."""
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
