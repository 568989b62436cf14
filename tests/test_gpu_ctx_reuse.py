"""One context through a sequence of worlds, batch sizes and engines: every
device buffer it owns is grown, shrunk, released and rebuilt along the way
(results, trajectory and its transpose staging, both trace copies, the policy
loop's arrays, the detail records), and every rollout still equals the CPU
oracle bit for bit. The engine is the test's own, not the session's, so the
order of the steps is the test."""
import numpy as np
import pytest

import pyoracle as po
from ccka import abi, configs
from ccka.engine import Engine
from ccka.world import ScenarioSet, deployment
from parity import compare, oracle

pytestmark = pytest.mark.gpu
THREADS = 16


def _load(spec, sc, seed):
    return po.gen_load(configs.trace_gen(seed), spec.n_steps, len(spec.deploys), sc.n, first_id=sc.first_id)


def _rollout(eng, spec, sc, load, traj, engine):
    """Rollout on what the context holds now (world, scenarios and load are set
    by the caller, in the order the step wants) against the oracle."""
    eng.rollout(trajectory=traj)
    assert eng.last_engine()[0] == engine
    rg = eng.results()
    tg = eng.trajectory() if traj else None
    rc, tc = oracle(spec, sc, load, traj=traj, threads=THREADS)
    compare(rg, rc, tg, tc)


def _policy_step(eng, spec, sc, load, wb, bs):
    eng.set_world(spec)
    eng.set_scenarios(sc)
    eng.set_load(load)
    eng.mlp_set_weights(wb, bs)
    out = []
    for _ in range(2):
        eng.policy_rollout(record=True)
        assert eng.last_engine()[0] == 4  # the fused loop
        out.append((eng.results(), eng.policy_actions()))
    return out


def _same_policy_run(a, b):
    (ra, (ta, ca)), (rb, (tb, cb)) = a, b
    for f in ra:
        assert np.array_equal(ra[f], rb[f]), f
    assert np.array_equal(ta, tb) and np.array_equal(ca, cb)


def test_one_context_through_worlds_sizes_and_engines():
    eng = Engine(0)
    try:
        # 1. single-deployment engine with a trajectory (the [N][T] records go
        # through the transpose staging buffer)
        spec = configs.config2_world(n_steps=120)
        sc = configs.hpa_scenarios(192)
        load = _load(spec, sc, 41)
        eng.set_world(spec)
        eng.set_scenarios(sc)
        eng.set_load(load)
        _rollout(eng, spec, sc, load, True, 2)
        # 2. shrink: fewer scenarios, another first id, a new load
        sc = configs.hpa_scenarios(64, first_id=7)
        load = _load(spec, sc, 43)
        eng.set_scenarios(sc)
        eng.set_load(load)
        _rollout(eng, spec, sc, load, True, 2)
        # 3. grow, without a trajectory: none to read afterwards
        sc = configs.hpa_scenarios(320)
        load = _load(spec, sc, 47)
        eng.set_scenarios(sc)
        eng.set_load(load)
        _rollout(eng, spec, sc, load, False, 2)
        with pytest.raises(abi.CckaError):
            eng.trajectory()
        # 4. two HPA deployments: the general kernel on the lane-skewed schedule
        # (test_gpu_skew.py's d2_n8) and its scenario-major trace copy
        spec = configs.config2_world(n_steps=120)
        spec.deploys = [deployment(abi.SCALER_HPA, cap_sel=abi.CAP_SPOT),
                        deployment(abi.SCALER_HPA, cap_sel=abi.CAP_OD, req_cpu=400, target=60)]
        sc = ScenarioSet(256, 5)
        load = _load(spec, sc, 53)
        eng.set_world(spec)
        eng.set_scenarios(sc)
        eng.set_load(load)
        _rollout(eng, spec, sc, load, True, 5)
        # 5. the policy loop twice (it releases both trace copies), equal to each
        # other and to a fresh context's; then plain rollouts again
        spec = configs.config2_world(n_steps=30)
        sc = configs.hpa_scenarios(128)
        load = _load(spec, sc, 59)
        ws, bs = configs.mlp_weights()
        wb = [configs.to_bf16_bits(x) for x in ws]
        runs = _policy_step(eng, spec, sc, load, wb, bs)
        _same_policy_run(runs[0], runs[1])
        fresh = Engine(0)
        try:
            _same_policy_run(runs[0], _policy_step(fresh, spec, sc, load, wb, bs)[0])
        finally:
            fresh.close()
        _rollout(eng, spec, sc, load, False, 2)
        # 6. the detail breakdown runs on the general kernel; off again, the
        # single-deployment engine is back
        eng.set_detail(True)
        _rollout(eng, spec, sc, load, False, 1)
        eng.set_detail(False)
        _rollout(eng, spec, sc, load, False, 2)
    finally:
        eng.close()
