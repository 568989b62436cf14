"""CPU guards of the closed-loop parity suite (tests/test_gpu_loop_worlds.py).

1. Which loop and which register layout every world of the GPU file takes,
   from the generator and the restated rule alone (loop_check.loop_engine /
   loop_plan): the floors of the GPU file's tally (both loops in >= 10 worlds,
   every DMAX x MAXN layout on the launched loop, each launch flag in >= 5
   worlds) hold before a GPU is involved; only "the policy's actions vary" needs
   the device's MLP.
2. The oracle's replay (ccka_oracle_rollout_policy) on seeds 0-9 of every
   profile under seeded random actions (targets 20-95 %, weights k / 16) with
   detail: the detail adds up to the totals, the replay of constant actions
   equal to the scenarios' overrides is the plain rollout, and random actions
   change the results, so a parity test of the loops' actions is not vacuous.
3. The named worlds: loop_lds_world's two catalogs differ by one type and sit
   on either side of the fused loop's LDS rule; loop_layout_world(12 | 16)
   give 12 and 16 deployment columns."""
import dataclasses
import functools

import numpy as np
import pytest

import loop_check as lc
import pyoracle as po
import random_worlds as rw
from ccka import abi
from test_detail import _check_consistent

THREADS = 8


@functools.lru_cache(maxsize=None)
def predicted():
    return {key: lc.predicted_row(*lc.world(*key)[:2]) for key in lc.tally_keys()}


def test_tally_floors_hold_from_the_generator():
    counts = lc.tally_counts(predicted())
    print(counts)
    lc.assert_floors(counts)


def test_every_family_world_runs_on_the_loop_its_profile_is_drawn_for():
    """d1_* worlds (<= 6 types, <= 8 slots) all fuse; several-deployment worlds never do."""
    rows = predicted()
    for (name, seed), v in rows.items():
        if name.startswith("d1_") and name != "d1_wide":
            assert v["engines"] == (4, 3), (name, seed, v)
        if name in ("gk_multi", "sk", "sk_wide", "layout12", "layout16"):
            assert v["engines"] == (3,) and v["dmax"] >= 2, (name, seed, v)
    # the wide worlds: one-hour staging with span > 1, and shared traces on seeds divisible by 3
    wide = {k: v for k, v in rows.items() if k[0] in lc.WIDE}
    assert sum(v["all_hours"] == 0 and v["span"] > 1 for v in wide.values()) >= 5
    assert all((v["trace_mod"] == 1) == (seed % 3 == 0) for (name, seed), v in wide.items() if name != "d1_wide")


def _filled(spec, sc):
    """The scenario set with the target and carbon-weight overrides present (a
    missing one filled with the world's own value), so a constant action equals them."""
    tgt = sc.target_util_pct
    if tgt is None:
        first = next(d for d in spec.deploys if d.scaler == abi.SCALER_HPA) if any(
            d.scaler == abi.SCALER_HPA for d in spec.deploys) else spec.deploys[0]
        tgt = np.full(sc.n, first.target_util_pct, np.int16)
    cw = sc.carbon_weight if sc.carbon_weight is not None else np.full(sc.n, spec.carbon_weight, np.float64)
    return dataclasses.replace(sc, target_util_pct=np.asarray(tgt, np.int16), carbon_weight=np.asarray(cw, np.float64))


@pytest.mark.parametrize("profile", lc.FAMILIES + lc.WIDE)
def test_oracle_replay_of_random_actions(profile):
    differ = total = 0
    for seed in range(10):
        spec, sc, load = rw.draw(profile, seed)
        what = f"{profile} seed {seed}"
        T, n = spec.n_steps, sc.n
        rng = np.random.default_rng([20251205, 94, rw._PIDX[profile], seed])
        at = rng.integers(20, 96, size=(T, n)).astype(np.int16)
        ac = rng.integers(0, 65, size=(T, n)).astype(np.float64) / 16.0
        res, traj, _, det = po.rollout_policy(spec, sc, load, at, ac, traj=True, threads=THREADS, detail=True)
        try:
            _check_consistent(spec, res, traj, det)
        except AssertionError as e:
            raise AssertionError(f"{what}: replay detail does not add up: {e}") from None
        plain, ptraj = po.rollout(spec, sc, load, traj=True, threads=THREADS)
        differ += int(np.any([res[f] != plain[f] for f in res], axis=0).sum())
        total += n
        # constant actions equal to the overrides: the plain rollout of the same scenario set
        sc2 = _filled(spec, sc)
        same, straj, _ = po.rollout_policy(spec, sc2, load, np.broadcast_to(sc2.target_util_pct, (T, n)),
                                           np.broadcast_to(sc2.carbon_weight, (T, n)), traj=True, threads=THREADS)
        plain2, ptraj2 = po.rollout(spec, sc2, load, traj=True, threads=THREADS)
        for f in same:
            assert np.array_equal(same[f], plain2[f]), f"{what}: constant-action replay differs in {f}"
        assert np.array_equal(straj, ptraj2), f"{what}: constant-action replay trajectory differs"
    print(f"{profile}: random actions change {differ} of {total} scenarios")
    assert differ >= 1, f"{profile}: random actions change no scenario of {total}"


def test_lds_worlds_straddle_the_fused_rule():
    fit, over = rw.loop_lds_world(True), rw.loop_lds_world(False)
    K = fit[0].catalog.k
    assert over[0].catalog.k == K + 1
    assert lc.loop_engine(*fit[:2]) == 4 and lc.loop_engine(*over[:2]) == 3
    pf, po_ = lc.loop_plan(*fit[:2]), lc.loop_plan(*over[:2])
    assert (pf["dmax"], pf["nmax"], pf["span"]) == (1, 8, 2) == (po_["dmax"], po_["nmax"], po_["span"])
    # K is the largest fusing catalog of that shape, not merely a boundary of the non-monotonic rule
    assert not any(lc.fuses(k, 2, 2, 1, 8) for k in range(K + 1, abi.MAX_TYPES + 1))
    assert lc._up16(pf["lds"]) + lc.MLP_LDS <= lc.LDS_BYTES < lc._up16(po_["lds"]) + lc.MLP_LDS
    # one type apart, everything else equal
    gone = [i for i, nm in enumerate(over[0].catalog.names) if nm not in fit[0].catalog.names]
    assert len(gone) == 1 and gone[0] not in (0, K)
    keep = np.arange(K + 1) != gone[0]
    for a in ("vcpu", "mem_gib", "max_pods", "od_uph"):
        assert np.array_equal(getattr(over[0].catalog, a)[keep], getattr(fit[0].catalog, a)), a
    assert np.array_equal(over[0].price[:, :, keep], fit[0].price) and np.array_equal(over[0].ci, fit[0].ci)
    assert np.array_equal(over[2], fit[2]) and np.array_equal(over[1].region, fit[1].region)
    assert bytes(over[0].deploys[0]) == bytes(fit[0].deploys[0])
    assert (over[0].n_steps, over[0].start_minute) == (fit[0].n_steps, fit[0].start_minute)
    assert len(np.unique(fit[1].region)) == 2 and fit[1].n == rw.N_SCEN


@pytest.mark.parametrize("n_deploy", [12, 16])
def test_layout_worlds_have_the_widest_layouts(n_deploy):
    spec, sc, load = rw.loop_layout_world(n_deploy)
    assert lc.kernel_dims(len(spec.deploys), spec.max_nodes) == (n_deploy, 16)
    assert len(spec.deploys) == n_deploy and spec.max_nodes == 16 and len(spec.pools) == 3 and sc.n == rw.N_SCEN
    kinds = [d.scaler for d in spec.deploys]
    assert {abi.SCALER_HPA, abi.SCALER_STATIC, abi.SCALER_KEDA, abi.SCALER_KEDA_TRIGGER} <= set(kinds)
    assert any(a == abi.SCALER_KEDA and b == abi.SCALER_KEDA_TRIGGER for a, b in zip(kinds, kinds[1:]))
    T, start = spec.n_steps, spec.start_minute
    assert 90 <= T <= 120 and load.shape == (T, n_deploy, sc.n)
    inside = [(m - start) % 1440 for m in (spec.peak_start, spec.peak_end)]
    assert sum(0 < x < T for x in inside) == 1, inside  # one edge of the peak window
    assert lc.loop_engine(spec, sc) == 3
    # the world is alive on the oracle, and its detail adds up
    res, traj, det = po.rollout(spec, sc, load, traj=True, threads=THREADS, detail=True)
    _check_consistent(spec, res, traj, det)
    assert res["launches"].sum() > 0 and len(np.unique(res["choice_hash"])) >= 16
