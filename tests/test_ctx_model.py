"""CPU guard of tests/ctx_model.py: the model gives the statuses include/ccka.h
states ("What ends what") on hand-written sequences, one per finding of the
context-state work and per row of the table, and the sequences the GPU file
runs (seeds 0-23) reach what they are meant to reach. The floors are printed
(pytest -s) and asserted; where one is missed the draw changes, not the floor."""
import collections

import pytest

import ctx_model as cm
from ctx_model import EINVAL, ESTATE, OK, STATIONS

SEEDS = range(24)


def play(calls):
    """Statuses of a hand-written sequence; a call is (method, args...)."""
    m = cm.Ctx()
    return [getattr(m, c[0])(*c[1:])[0] for c in calls], m


def gets(m, *getters):
    return [m.get_status(g) for g in getters]


def canonical(name, weights=True):
    return ([("set_weights", "cfg")] if weights else []) + [("set_world", name), ("set_scenarios", name), ("set_load", 0)]


# ---- the three findings ----
def test_finding_1_an_mlp_forward_makes_no_results_readable():
    pre = canonical("A") + [("rollout", True), ("switch", "detail_on", True), ("rollout", True)]
    fwd = [("set_weights", "exact"), ("mlp_set_states",), ("mlp_forward",)]
    for ending in ([("set_scenarios", "A")], [("set_world", "C")]):
        st, m = play(pre + ending + fwd)
        assert st == [OK] * len(st)
        assert set(gets(m, *cm.RESULT_GETTERS, "timeline", "trajectory", "detail")) == {ESTATE}
        assert m.kernel_ms()[0] == OK   # the forward is a timed launch
    st, m = play(fwd)                   # a context that has run nothing else
    assert st == [OK] * 3 and m.kernel_ms()[0] == OK and m.get_status("results") == ESTATE


def test_finding_2_the_loops_records_end_with_the_world_and_the_set():
    rec = ("actions", "features", "samples")
    pre = canonical("B") + [("policy_grad",)]
    for ending in ([("set_scenarios", "B")], [("set_scenarios", "C")], [("set_world", "E")]):
        _, m = play(pre)
        assert gets(m, *rec) == [OK] * 3
        st, m = play(pre + ending)
        assert st[-1] == OK and gets(m, *rec) == [ESTATE] * 3
    # a plain rollout and a new load keep them: no rollout touches their buffers
    _, m = play(pre + [("rollout", True), ("set_load", 1), ("rollout", False)])
    assert gets(m, *rec) == [OK] * 3 and m.obj["actions"] == ("B", "grad", 0) and m.obj["res"] == ("B", "roll", 1)


def test_finding_3_set_world_ends_the_scenario_set():
    st, m = play(canonical("G") + [("rollout", False), ("set_world", "A"), ("set_load", 0), ("rollout", False),
                                   ("policy_rollout", False, False), ("policy_grad",)])
    assert st[-5:] == [OK, ESTATE, ESTATE, ESTATE, ESTATE]
    st, m = play(canonical("G") + [("set_world", "A"), ("set_scenarios", "A"), ("set_load", 0), ("rollout", True)])
    assert st[-3:] == [OK, OK, OK] and m.obj["res"] == ("A", "roll", 0)


# ---- the table, row by row ----
def test_set_world_row():
    pre = canonical("E") + [("switch", "detail_on", True), ("switch", "feat_on", True), ("policy_grad",),
                            ("get", "capture"), ("policy_rollout", True, True)]
    _, m = play(pre)
    assert set(gets(m, *[g for g in cm.GETTERS if g != "samples"])) == {OK}
    _, m = play(pre + [("set_world", "A")])
    assert set(gets(m, *cm.GETTERS)) == {ESTATE} and m.kernel_ms()[0] == ESTATE
    # kept: the snapshot, the weights, the switches
    assert m.snap == (("E", "grad", 0), "E") and m.weights == "cfg" and m.detail_on and m.feat_on
    st, m = play(pre + [("set_world", "F"), ("set_scenarios", "F"), ("set_load", 0), ("rollout", False), ("get", "paired", 7)])
    assert st[-1] == OK


def test_set_scenarios_row():
    pre = canonical("B") + [("switch", "detail_on", True), ("policy_grad",)]
    st, m = play(pre + [("set_scenarios", "C"), ("set_load", 1), ("rollout", False)])
    assert st[-3:] == [OK, OK, OK]          # the world stands
    st, m = play(pre + [("set_scenarios", "C")])
    assert set(gets(m, *cm.GETTERS)) == {ESTATE} and m.set_load(0)[0] == OK and m.rollout(False)[0] == OK
    st, m = play([("set_scenarios", "A")])
    assert st == [ESTATE]


def test_set_load_row_keeps_everything_readable():
    st, m = play(canonical("A") + [("rollout", True), ("set_load", 1)])
    assert m.get("results") == (OK, ("A", "roll", 0)) and m.get("trajectory") == (OK, ("A", "roll", 0))
    st, m = play(canonical("A") + [("rollout", True), ("set_load", 1), ("rollout", False)])
    assert m.get("results") == (OK, ("A", "roll", 1)) and m.get_status("trajectory") == ESTATE


def test_rollout_row():
    pre = canonical("C") + [("switch", "detail_on", True), ("policy_rollout", True, True)]
    _, m = play(pre + [("rollout", True)])
    assert gets(m, "trajectory", "detail", "actions") == [OK, OK, OK] and m.engine == 1
    _, m = play(pre + [("switch", "detail_on", False), ("rollout", False)])
    assert gets(m, "trajectory", "timeline", "detail", "actions") == [ESTATE, ESTATE, ESTATE, OK] and m.engine == 2
    assert m.ended_by["traj"] == "rollout" and m.obj["actions"] == ("C", "loop", 0)


def test_loop_rows():
    pre = canonical("A") + [("policy_grad",)]
    _, m = play(pre)
    assert gets(m, "samples", "actions", "features", "trajectory") == [OK, OK, OK, ESTATE] and m.engine == 4
    _, m = play(pre + [("policy_rollout", True, False)])
    assert gets(m, "samples", "actions", "features", "trajectory") == [ESTATE, ESTATE, ESTATE, OK]
    _, m = play(pre + [("switch", "feat_on", True), ("switch", "fused_off", True), ("policy_rollout", False, True)])
    assert gets(m, "samples", "actions", "features", "trajectory") == [ESTATE, OK, OK, ESTATE] and m.engine == 3
    _, m = play(pre + [("set_weights", "exact"), ("mlp_backward",)])
    assert gets(m, "samples", "actions", "features") == [ESTATE, OK, OK]
    st, _ = play(canonical("A", weights=False) + [("policy_rollout", False, False), ("policy_grad",), ("mlp_backward",)])
    assert st[-3:] == [ESTATE] * 3


def test_mlp_forward_row_ends_nothing():
    pre = canonical("A") + [("rollout", True)]
    _, m = play(pre + [("set_weights", "exact"), ("mlp_set_states",), ("mlp_forward",)])
    assert m.get("results") == (OK, ("A", "roll", 0)) and m.get_status("trajectory") == OK and m.mlp_actions() == (OK, "exact")
    st, _ = play([("mlp_forward",), ("set_weights", "exact"), ("mlp_forward",)])
    assert st == [ESTATE, OK, ESTATE]     # no weights; no states


def test_failing_calls():
    pre = canonical("A") + [("policy_grad",), ("rollout", True)]
    _, m = play(pre + [("set_world", "D", False)])
    assert set(gets(m, "results", "trajectory", "actions", "samples")) == {OK} and m.rollout(True)[0] == OK
    st, m = play(pre + [("set_scenarios", "A", False)])
    assert st[-1] == EINVAL and m.rollout(False)[0] == ESTATE and m.set_load(0)[0] == ESTATE
    assert set(gets(m, "results", "trajectory", "actions", "samples")) == {OK}   # the last run's, still
    st, m = play(pre + [("set_scenarios", "A", False), ("set_scenarios", "A"), ("set_load", 0), ("rollout", False)])
    assert st[-3:] == [OK, OK, OK]


def test_grid_and_paired_shape_rules_come_after_the_state():
    _, m = play(canonical("B") + [("rollout", True)])        # first id 7: no whole grids
    assert gets(m, "grid_stats", "timeline", "capture", "results") == [EINVAL, EINVAL, EINVAL, OK]
    _, m = play(canonical("B") + [("rollout", True), ("set_world", "A")])
    assert gets(m, "grid_stats", "timeline", "capture") == [ESTATE] * 3  # never EINVAL on an ended object
    pre = canonical("E") + [("rollout", False), ("get", "capture"), ("set_scenarios", "F"), ("set_load", 0), ("rollout", False)]
    _, m = play(pre)   # F holds grids 6..9, the snapshot 0..7
    assert [m.get("paired")[0], m.get("paired", 3)[0], m.get("boot", 8)[0], m.get("boot", 7)[0]] == [EINVAL, OK, EINVAL, OK]
    _, m = play(pre + [("get", "capture"), ("set_scenarios", "E"), ("set_load", 0), ("rollout", False)])
    assert [m.get("paired")[0], m.get("paired", 6)[0]] == [EINVAL, OK]   # now the snapshot is 6..9, the batch 0..7


def test_stations_hold_what_the_sequences_need():
    S = STATIONS
    assert all(s.N <= 320 and s.T <= 120 for s in S.values())
    assert S["A"].T * S["A"].N == S["B"].T * S["B"].N and S["A"].N != S["B"].N
    assert S["A"].N == S["C"].N and S["A"].T != S["C"].T
    assert S["D"].T > S["C"].T and S["D"].N > S["C"].N
    assert S["G"].regions == 2 and cm.build("G")[1].region.max() == 1 and S["A"].regions == 1
    assert S["E"].paired_ok and S["F"].paired_ok and S["E"].world == S["F"].world
    assert S["H"].T * S["H"].N < S["D"].T * S["D"].N
    import loop_check
    spec, sc, _, _ = cm.build("H")
    assert loop_check.loop_plan(spec, sc)["hlen"] > 0      # the HBM history
    assert {cm.loop_engine(n) for n in S} == {3, 4} and cm.loop_engine("D") == 3
    assert {s.roll_engine for s in S.values()} == {1, 2, 5}


# ---- the sequences of the GPU file ----
def _written_counts(rows):
    """The in-bounds rule recomputed from the station shapes and the statuses
    alone: per ESTATE probe (getter, elements it would copy, elements written)."""
    T = N = 0
    sc = None
    detail = feat = False
    w = collections.Counter()
    out = []
    for (c, st, key, facts) in rows:
        op = c[0]
        if op == "switch":
            detail, feat = (c[2] if c[1] == "detail_on" else detail), (c[2] if c[1] == "feat_on" else feat)
        if st != OK:
            if op == "get" and st == ESTATE:
                g = c[1]
                need = {"trajectory": [("traj", T * N)], "timeline": [("traj", T * N)], "detail": [("detail", N)],
                        "actions": [("actions", T * N)], "features": [("features", (T + 1) * N * 64), ("actions", T * N)],
                        "samples": [("samples", T * N), ("coef", N)]}.get(g, [("res", N)])
                out.append((g, need, {k: w[k] for k, _ in need}))
            continue
        if op == "set_world":
            T = STATIONS[c[1]].T
        elif op == "set_scenarios":
            sc, N = c[1], STATIONS[c[1]].N
            w["res"], w["traj"], w["detail"] = N, 0, 0
        elif op in ("rollout", "policy_rollout", "policy_grad"):
            traj = op != "policy_grad" and c[1]
            if traj:
                w["traj"] = T * N
            if detail:
                w["detail"] = N
            if op == "policy_grad" or (op == "policy_rollout" and c[2]):
                w["actions"] = T * N
            if op == "policy_grad" or (op == "policy_rollout" and feat):
                w["features"] = (T + 1) * N * 64
            if op == "policy_grad":
                w["samples"], w["coef"] = T * N, N
        elif op == "mlp_backward":
            w["samples"] = w["coef"] = c[1] if len(c) > 1 else cm.MLP_ROWS
    return out


@pytest.fixture(scope="module")
def replays():
    return {s: cm.replay(cm.sequence(s)) for s in SEEDS}


def test_sequences_are_deterministic_and_sized(replays):
    for s in SEEDS:
        calls = cm.sequence(s)
        assert calls == cm.sequence(s) and 40 <= len(calls) <= 60, (s, len(calls))
        assert all(st in (OK, EINVAL, ESTATE) for _, st, _, _ in replays[s])


def test_every_estate_probe_is_in_bounds(replays):
    n = 0
    for s in SEEDS:
        for g, need, have in _written_counts(replays[s]):
            for k, cnt in need:
                assert 1 <= cnt <= have[k], f"seed {s}: {g} would copy {cnt} of {k}, written with {have[k]}"
            n += 1
    print(f"\nESTATE probes, all in bounds: {n}")
    assert n >= 140


def test_no_launch_after_a_lone_set_world(replays):
    for s in SEEDS:
        lone = False
        for (c, st, _, _) in replays[s]:
            if c[0] == "set_world" and st == OK:
                lone = True
            elif c[0] == "set_scenarios":
                lone = False
            assert not (lone and c[0] in ("rollout", "policy_rollout", "policy_grad")), (s, c)


def test_floors(replays):
    pairs, ok, estate, engines, moves = (collections.Counter() for _ in range(5))
    for s in SEEDS:
        rows = replays[s]
        shape = None
        for i, (c, st, key, facts) in enumerate(rows):
            if c[0] == "get":
                (ok if st == OK else estate if st == ESTATE else collections.Counter())[c[1]] += 1
                if st == ESTATE and facts["ended_by"]:
                    pairs[facts["ended_by"], c[1]] += 1
            if "engine" in facts:
                engines[facts["engine"]] += 1
            if c[0] == "set_world" and st == OK:
                nxt = rows[i + 1][0] if i + 1 < len(rows) else None
                moves["canonical" if nxt and nxt[0] == "set_scenarios" else "broken: set_world alone"] += 1
            if c[0] == "set_scenarios" and st == OK:
                later = [r[0][0] for r in rows[i + 1:]]
                first = next((x for x in later if x in ("set_load", "rollout", "policy_rollout", "policy_grad")), None)
                if first and first != "set_load":
                    moves["broken: no load"] += 1
                new = (rows[i][0][1], STATIONS[c[1]].T, STATIONS[c[1]].N)
                if shape and shape[0] != new[0]:
                    a, b = shape[1] * shape[2], new[1] * new[2]
                    moves["growing" if b > a else "shrinking" if b < a else "equal count, another shape"] += 1
                shape = new
    print("\npairs (ending call x getter -> ESTATE):", dict(sorted(pairs.items())))
    print("getter OK:", dict(ok), "\ngetter ESTATE:", dict(estate))
    print("engines:", dict(engines), "\nmoves:", dict(moves))
    # cm.PAIRS is the table's pairs less three: (set_scenarios x trajectory / timeline / detail).
    # That is a narrowing of "every pair of the table", forced by the in-bounds rule: set_scenarios
    # frees the trajectory and detail allocations, so the count the ended object was written with is
    # 0 and no admissible ESTATE probe of them exists. tests/test_gpu_ctx_state.py's finding-1 case
    # probes the three once, after set_scenarios + an MLP forward.
    assert len(cm.PAIRS) == 36 and not [p for p in cm.PAIRS if p[0] == "set_scenarios" and cm.OBJECT[p[1]] in ("traj", "detail")]
    short = {p: pairs[p] for p in cm.PAIRS if pairs[p] < 3}
    assert not short, f"(ending call, getter) pairs in fewer than 3 probes: {short}"
    assert not {g: (ok[g], estate[g]) for g in cm.GETTERS if ok[g] < 10 or estate[g] < 10}
    assert not {e: engines[e] for e in (1, 2, 3, 4, 5) if engines[e] < 10}
    kinds = ("growing", "shrinking", "equal count, another shape", "canonical", "broken: set_world alone",
             "broken: no load")
    assert not {k: moves[k] for k in kinds if moves[k] < 20}
