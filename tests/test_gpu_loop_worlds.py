"""Closed-loop parity on every world family: ccka_policy_rollout and
ccka_policy_grad against the oracle's replay of their recorded actions, on the
loop the restated rule predicts (loop_check.loop_engine; a world on the other
loop is a failure) and, where a world fuses, on the launched loop as well.

  families   seeds 0-39 of d1_rules, d1_sync15, d1_keda, d1_disrupt (all fused:
             the HBM history, the 15 s sub-steps, KEDA and full disruption
             inside rollout_kernel<1, 8, POL>, then launched), gk_single (fused
             or launched), gk_multi and sk (launched: state_io of the <2,8>
             <2,16> <4,8> <4,16> <8,16> layouts)
  wide       seeds 0-19 of d1_wide, gk_wide, sk_wide: 600 scenarios in three
             workgroups, shared traces, one-hour staging with span > 1 (the
             restage of a resumed launch)
  named      loop_layout_world(12 | 16): the <12,16> and <16,16> layouts;
             loop_lds_world: the largest catalog that fuses and one type more
  detail     ccka_detail out of both loops against the replay's detail
  sampled    ccka_policy_grad: bin table, replay, objective, factors, gradient,
             every sampled bin
  context    several worlds through one context of the test's own: graph
             replay, a new graph, a fused run in between
  tally      what ran, with floors (tests/test_loop_worlds.py holds the same
             floors from the generator alone)

10 worlds per case, each under configs.mlp_weights(seed). A failure names the
world: loop_check.world(name, seed) reproduces it."""
import os

import pytest

import loop_check as lc
import random_worlds as rw
from ccka.engine import Engine
from parity import compare

pytestmark = pytest.mark.gpu
# (samples, exempt) of the sampled-policy cases, for the 0.1 % bound over all of them
NEAR = {}


def run_world(engine, name, seed, **kw):
    return lc.check_loop(engine, lc.world(name, seed), seed, f"{name} seed {seed}", key=(name, seed), **kw)


@pytest.mark.parametrize("chunk", range(lc.FAMILY_SEEDS // lc.PER_CASE))
@pytest.mark.parametrize("profile", lc.FAMILIES)
def test_family_loops_match_oracle(engine, profile, chunk):
    for seed in range(chunk * lc.PER_CASE, (chunk + 1) * lc.PER_CASE):
        run_world(engine, profile, seed)


@pytest.mark.parametrize("chunk", range(lc.WIDE_SEEDS // lc.PER_CASE))
@pytest.mark.parametrize("profile", lc.WIDE)
def test_wide_loops_match_oracle(engine, profile, chunk):
    for seed in range(chunk * lc.PER_CASE, (chunk + 1) * lc.PER_CASE):
        run_world(engine, profile, seed)


@pytest.mark.parametrize("name", lc.NAMED)
def test_named_loops_match_oracle(engine, name):
    """The <12,16> and <16,16> layouts on the launched loop; the largest catalog
    beside which the MLP's LDS fits on the fused loop (and launched), one type
    more on the launched loop alone."""
    want = {"layout12": 3, "layout16": 3, "lds_fits": 4, "lds_over": 3}[name]
    run_world(engine, name, 0, want=want)


@pytest.mark.parametrize("profile", lc.DETAIL + ("layout12",))
def test_loop_detail_matches_oracle_replay(engine, profile):
    for seed in range(1 if profile in lc.NAMED else 10):
        lc.check_loop(engine, lc.world(profile, seed), seed, f"{profile} seed {seed} (detail)", detail=True)


@pytest.mark.parametrize("profile", lc.SAMPLED)
def test_sampled_policy_loops(engine, profile):
    samples = near = 0
    for seed in range(10):
        s, n = lc.check_sampled(engine, rw.draw(profile, seed), seed, f"{profile} seed {seed} (sampled)")
        samples, near = samples + s, near + n
    NEAR[profile] = (samples, near)
    print(f"{profile}: samples within 1e-6 of a bin edge: {near} of {samples}")
    assert near <= 1e-3 * samples


def test_one_context_several_worlds():
    """A gk_multi world launched, again (graph replay), a gk_multi world of
    another horizon and deployment count (a new graph), a fused d1_rules world,
    then the first world once more: every run equals the oracle, the first and
    the last byte for byte."""
    first = rw.draw("gk_multi", 0)
    other = next(w for w in (rw.draw("gk_multi", s) for s in range(1, 40))
                 if w[0].n_steps != first[0].n_steps and len(w[0].deploys) != len(first[0].deploys))
    e = Engine(0, lib_path=os.environ.get("CCKA_TEST_LIB") or None)  # the build under test, as the session's engine
    try:
        runs = [lc.check_loop(e, w, ws, f"one context, run {j}", want=want)
                for j, (w, ws, want) in enumerate([(first, 0, 3), (first, 0, 3), (other, 1, 3),
                                                   (rw.draw("d1_rules", 0), 2, 4), (first, 0, 3)])]
    finally:
        e.close()
    (r0, t0, (a0, c0), f0), (r4, t4, (a4, c4), f4) = runs[0], runs[4]
    for f in r0:
        assert r0[f].tobytes() == r4[f].tobytes(), f
    assert t0.tobytes() == t4.tobytes() and a0.tobytes() == a4.tobytes() and c0.tobytes() == c4.tobytes()
    assert f0.tobytes() == f4.tobytes()
    compare(runs[1][0], r0, runs[1][1], t0)


def test_tally(engine):
    """What the cases above ran (a world this process has not run yet is run
    here): worlds per (engine, DMAX, MAXN), worlds with the HBM history, HPA
    sub-steps, shared traces or one-hour staging, and per profile the worlds
    whose recorded actions take at least two values. Floors: both loops in >=
    10 worlds, every layout on the launched loop, every flag in >= 5 worlds,
    varying actions in >= 1 world of 10 per profile (an activity floor: parity
    holds whether or not the policy steers). The counts equal what
    tests/test_loop_worlds.py derives from the generator alone."""
    for name, seed in lc.tally_keys():
        if (name, seed) not in lc.TALLY:
            run_world(engine, name, seed)
    rows = {k: lc.TALLY[k] for k in lc.tally_keys()}
    counts = lc.tally_counts(rows)
    varying = {p: (sum(v["varying"] for (n, _), v in rows.items() if n == p), sum(n == p for n, _ in rows))
               for p in lc.FAMILIES + lc.WIDE + lc.NAMED}
    print("tally:", counts)
    print("worlds with varying actions (of):", varying)
    lc.assert_floors(counts)
    want = lc.tally_counts({k: lc.predicted_row(*lc.world(*k)[:2]) for k in rows})
    assert counts == want, (counts, want)
    quiet = {p: v for p, v in varying.items() if p not in lc.NAMED and 10 * v[0] < v[1]}
    assert not quiet, f"profiles whose policy varies its actions in fewer than 1 world of 10: {quiet}"
