"""TEST INFRASTRUCTURE: a restated model of the context behind the C ABI, written
from the comment block "What ends what" of include/ccka.h and from nothing in
csrc/. One method per ABI call: each returns the status the library must
return and, for a getter that succeeds, WHICH RUN's payload must come back.

A run is (station, kind, load variant): a station is a fixed (world, scenario
set) pair with two loads (variant 0 is uploaded with ccka_set_load, variant 1
generated on the device with ccka_gen_load), the kind is "roll" (ccka_rollout),
"loop" (ccka_policy_rollout under configs.mlp_weights) or "grad"
(ccka_policy_grad under the station's seed). tests/test_ctx_model.py holds the
model to the contract on the CPU; tests/test_gpu_ctx_state.py holds the
library to the model.

sequence(seed) draws a call sequence. One rule keeps a wrong library inside
its allocations: a getter that must return ESTATE is drawn only when the
element count it would copy under the current shape is at most the count the
ended object was last written with (`written`; the result columns count the
scenarios they were allocated for). After a lone set_world the sequence probes
set_load and the getters, and never launches."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

OK, EINVAL, ESTATE = 0, -1, -6
GS = 16            # grid size of every grid call (the sweep stations' n_traces)
BOOT_B = 65        # replicates of a bootstrap call
MLP_ROWS = 33      # rows of an MLP forward / backward (mlp_ref.exact_case(0, 33))


@dataclasses.dataclass(frozen=True)
class Station:
    name: str
    world: str       # stations of one world differ in their scenario sets only
    T: int
    N: int
    first_id: int
    traces: int      # shared traces (0: one trace per scenario)
    regions: int
    roll_engine: int  # engine of a plain rollout without detail (with detail: 1)
    seed: int         # load seeds seed / seed + 1, policy-gradient seed

    @property
    def grids_ok(self):
        return self.N % GS == 0 and self.first_id % GS == 0

    @property
    def paired_ok(self):
        return self.traces > 0 and GS % self.traces == 0 and self.grids_ok


# Together: every rollout engine (2: A B C C2 E F G; 1: H and detail anywhere; 5:
# D), shared traces with two grid ranges (E grids 0..7, F grids 6..9), two
# regions (G) next to one, T N equal with N different (A 120 x 64, B 40 x 192),
# N equal with T different (A, C), both shrinking (D -> C), an HBM-history
# world (H) smaller than D, and a batch that holds no whole grids (B: first id 7).
STATIONS = {s.name: s for s in (
    Station("A", "w120", 120, 64, 0, 0, 1, 2, 41),
    Station("B", "w40", 40, 192, 7, 0, 1, 2, 43),
    Station("C", "w40", 40, 64, 64, 0, 1, 2, 47),
    Station("C2", "w40", 40, 64, 128, 0, 1, 2, 49),
    Station("D", "w2d", 60, 256, 0, 0, 1, 5, 53),
    Station("E", "w30", 30, 128, 0, 16, 1, 2, 59),
    Station("F", "w30", 30, 64, 96, 16, 1, 2, 59),
    Station("G", "wr2", 30, 96, 32, 0, 2, 2, 61),
    Station("H", "wh", 50, 96, 16, 0, 1, 1, 67),
)}
RESULT_GETTERS = ("results", "totals", "grid_stats", "grid_stat", "pareto", "capture", "paired", "boot")
GETTERS = RESULT_GETTERS + ("timeline", "trajectory", "detail", "actions", "features", "samples")
# the object a getter reads first (paired / boot: then the snapshot; features: then the actions)
OBJECT = dict({g: "res" for g in RESULT_GETTERS}, timeline="traj", trajectory="traj", detail="detail",
              actions="actions", features="features", samples="samples")
# (ending call, getter) pairs of the table. set_scenarios frees the trajectory
# and detail allocations, so no in-bounds ESTATE probe of them exists after it.
PAIRS = ([("set_world", g) for g in GETTERS] +
         [("set_scenarios", g) for g in GETTERS if OBJECT[g] not in ("traj", "detail")] +
         [("rollout", g) for g in ("trajectory", "timeline", "detail")] +
         [("policy_rollout", g) for g in ("samples", "actions", "features", "trajectory", "timeline")] +
         [("policy_grad", g) for g in ("trajectory", "timeline")] + [("mlp_backward", "samples")])


@functools.lru_cache(maxsize=None)
def build(name):
    """(WorldSpec, ScenarioSet, [load 0, load 1], [None, TraceGen of load 1]) of a station."""
    import pyoracle as po
    from ccka import abi, configs
    from ccka.world import (ScenarioSet, WorldSpec, carbon_intensity, catalog_small, deployment, price_tiles,
                            reference_pools)
    s = STATIONS[name]
    if s.world == "w2d":  # two HPA deployments: the lane-skewed schedule (tests/test_gpu_ctx_reuse.py step 4)
        spec = configs.config2_world(n_steps=s.T)
        spec.deploys = [deployment(abi.SCALER_HPA, cap_sel=abi.CAP_SPOT),
                        deployment(abi.SCALER_HPA, cap_sel=abi.CAP_OD, req_cpu=400, target=60)]
        sc = ScenarioSet(s.N, s.first_id)
    elif s.world == "wr2":  # two regions, the second half of the batch in region 1
        cat = catalog_small()
        spec = WorldSpec(catalog=cat, ci=carbon_intensity(2, configs.SEED), price=price_tiles(cat, 2, 3, configs.SEED),
                         pools=reference_pools(), deploys=[deployment(abi.SCALER_HPA)], n_steps=s.T, max_nodes=8)
        sc = configs.hpa_scenarios(s.N, s.first_id, 2, None)
        sc.region = (np.arange(s.N) >= s.N // 2).astype(np.uint8)
    elif s.world == "wh":  # a 900 s down window: the general kernel over the HBM history
        spec = configs.config2_world(n_steps=s.T)
        spec.deploys = [deployment(abi.SCALER_HPA, down_stab=900)]
        sc = configs.hpa_scenarios(s.N, s.first_id)
    elif s.traces:
        spec = configs.config2_world(n_steps=s.T)
        sc = configs.config4_scenarios(s.first_id // s.traces, s.N // s.traces, s.traces)
    else:
        spec = configs.config2_world(n_steps=s.T)
        sc = configs.hpa_scenarios(s.N, s.first_id)
    assert (spec.n_steps, sc.n, sc.first_id, sc.n_traces, spec.ci.shape[0]) == (s.T, s.N, s.first_id, s.traces, s.regions)
    cols, first = (s.traces, 0) if s.traces else (s.N, s.first_id)
    gens = [configs.trace_gen(s.seed), configs.trace_gen(s.seed + 1)]
    loads = [po.gen_load(g, s.T, len(spec.deploys), cols, first_id=first) for g in gens]
    for a in loads:
        a.setflags(write=False)
    return spec, sc, loads, [None, gens[1]]


class Ctx:
    """The context as include/ccka.h describes it."""

    def __init__(self):
        self.world = None          # station whose world is set
        self.sc = None             # station whose scenario set stands
        self.T = self.N = 0        # the shape a getter's count is formed from (N: the last accepted set's)
        self.first_id = self.traces = 0
        self.load = None           # load variant on the device
        self.weights = None        # "cfg" (configs.mlp_weights) or "exact" (mlp_ref.exact_case)
        self.states = None         # "set": MLP_ROWS exact-case rows; "loop": a loop's last features
        self.forward = False       # the MLP actions are the forward of the states
        self.detail_on = self.fused_off = self.feat_on = False
        self.timed = False
        self.engine = 0
        self.snap = None           # (run, station) of the snapshot
        self.obj = dict.fromkeys(("res", "traj", "detail", "actions", "features", "samples"))
        self.ended_by = dict.fromkeys(self.obj)
        # elements each object was last written with (kept when it ends; 0 once its allocation is freed)
        self.written = dict(res=0, traj=0, detail=0, actions=0, features=0, samples=0, coef=0)

    # ---- helpers ----
    def _end(self, call, *names):
        for n in names:
            if self.obj[n] is not None:
                self.ended_by[n] = call
            self.obj[n] = None

    def _write(self, name, run, count):
        self.obj[name] = run
        self.ended_by[name] = None
        self.written[name] = count

    def count(self, getter):
        """Elements the getter copies under the current shape."""
        T, N = self.T, self.N
        return {"traj": T * N, "detail": N, "actions": T * N, "features": (T + 1) * N * 64, "samples": T * N,
                "res": N}[OBJECT[getter]]

    def in_bounds(self, getter):
        """The probe rule: the getter's copy fits what its object was last written with."""
        n, o = self.count(getter), OBJECT[getter]
        ok = 1 <= n <= self.written[o]
        if getter == "samples":
            ok = ok and self.N <= self.written["coef"]
        if getter == "features":  # read with the actions
            ok = ok and self.T * self.N <= self.written["actions"]
        return ok

    @property
    def can_run(self):
        return self.world is not None and self.sc is not None and self.load is not None

    # ---- inputs ----
    def set_world(self, name, valid=True):
        if not valid:
            return EINVAL, None  # fails validation: nothing changes
        s = STATIONS[name]
        self.world, self.T = s.world, s.T
        self.sc = self.load = None
        self._end("set_world", *self.obj)
        self.timed = False
        return OK, None

    def set_scenarios(self, name, valid=True):
        if self.world is None:
            return ESTATE, None
        self.sc = self.load = None  # a failing call ends the earlier set and its load too
        if not valid:
            return EINVAL, None
        s = STATIONS[name]
        assert s.world == self.world, "a sequence sets only scenario sets drawn for the world"
        self.sc, self.N, self.first_id, self.traces = name, s.N, s.first_id, s.traces
        self._end("set_scenarios", *self.obj)
        self.timed = False
        self.written.update(res=s.N, traj=0, detail=0)  # fresh result columns; trajectory and detail freed
        return OK, None

    def set_load(self, variant):
        if self.sc is None:
            return ESTATE, None
        self.load = variant
        return OK, None

    def set_weights(self, which):
        self.weights = which
        return OK, None

    def switch(self, name, on):
        setattr(self, name, bool(on))
        return OK, None

    # ---- runs ----
    def _ran(self, call, kind, traj, engine):
        s = STATIONS[self.sc]
        run = (self.sc, kind, self.load)
        self._write("res", run, s.N)
        if traj:
            self._write("traj", run, s.T * s.N)
        else:
            self._end(call, "traj")
        if self.detail_on:
            self._write("detail", run, s.N)
        else:
            self._end(call, "detail")
        self.timed = True
        self.engine = engine
        return run

    def rollout(self, traj):
        if not self.can_run:
            return ESTATE, None
        s = STATIONS[self.sc]
        self._ran("rollout", "roll", traj, 1 if self.detail_on else s.roll_engine)
        return OK, None

    def _loop(self, call, kind, traj, record, feat):
        if not self.can_run or self.weights is None:
            return ESTATE, None
        assert self.weights == "cfg", "a sequence runs the loops under configs.mlp_weights only"
        s = STATIONS[self.sc]
        run = self._ran(call, kind, traj, 3 if self.fused_off else loop_engine(self.sc))
        if record:
            self._write("actions", run, s.T * s.N)
        else:
            self._end(call, "actions")
        if feat:
            self._write("features", run, (s.T + 1) * s.N * 64)
        else:
            self._end(call, "features")
        self.states, self.forward = "loop", False
        return OK, run

    def policy_rollout(self, traj, record):
        st, run = self._loop("policy_rollout", "loop", traj, record, self.feat_on)
        if st == OK:
            self._end("policy_rollout", "samples")
        return st, None

    def policy_grad(self):
        st, run = self._loop("policy_grad", "grad", False, True, True)
        if st == OK:
            s = STATIONS[self.sc]
            self._write("samples", run, s.T * s.N)
            self.written["coef"] = s.N
        return st, run  # the gradient is the run's payload too

    def mlp_backward(self, rows=MLP_ROWS):
        if self.weights is None:
            return ESTATE, None
        assert self.weights == "exact", "a sequence runs the backward on mlp_ref.exact_case only"
        self._end("mlp_backward", "samples")
        self.written.update(samples=rows, coef=rows)  # its rows went through the samples' buffers
        return OK, rows

    def mlp_set_states(self):
        self.states, self.forward = "set", False
        return OK, None

    def mlp_forward(self):
        if self.weights is None or self.states is None:
            return ESTATE, None
        self.timed = True
        self.forward = True
        return OK, None

    def mlp_actions(self):
        """Drawn only after a forward of set states (the call has no state rule of its own)."""
        assert self.states == "set" and self.forward
        return OK, self.weights

    # ---- getters ----
    def kernel_ms(self):
        return (OK if self.timed else ESTATE), None

    def last_engine(self):
        return OK, self.engine

    def get_status(self, getter):
        """The status a getter would return now, without the capture's side effect."""
        snap = self.snap
        st, _ = self.get(getter)
        self.snap = snap
        return st

    def get(self, getter, base=None):
        """Status and payload key of a getter; `base` is the baseline grid of paired / boot (None: the same id)."""
        o = OBJECT[getter]
        if self.obj["res"] is None and getter in RESULT_GETTERS + ("timeline", "detail"):
            return ESTATE, None
        if self.obj[o] is None or (getter == "features" and self.obj["actions"] is None):
            return ESTATE, None
        run = self.obj[o]
        s = STATIONS[run[0]]
        if getter in ("paired", "boot") and self.snap is None:
            return ESTATE, None
        if getter in ("grid_stats", "grid_stat", "pareto", "timeline") and not s.grids_ok:
            return EINVAL, None
        if getter in ("capture", "paired", "boot") and not s.paired_ok:
            return EINVAL, None
        if getter == "capture":
            self.snap = (run, run[0])
            return OK, run
        if getter in ("paired", "boot"):
            snap_run, snap_st = self.snap
            b = STATIONS[snap_st]
            lo, hi = b.first_id // GS, (b.first_id + b.N) // GS
            cur_lo, cur_hi = s.first_id // GS, (s.first_id + s.N) // GS
            if s.traces != b.traces:
                return EINVAL, None
            if base is None and not (lo <= cur_lo and cur_hi <= hi):
                return EINVAL, None
            if base is not None and not lo <= base < hi:
                return EINVAL, None
            return OK, (run, snap_run, base)
        return OK, run


@functools.lru_cache(maxsize=None)
def loop_engine(name):
    """The closed loop of a station, from loop_check's restated rule."""
    import loop_check
    spec, sc, _, _ = build(name)
    return loop_check.loop_engine(spec, sc)


# ---------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------
_RARE = ("trajectory", "timeline", "detail", "samples", "paired", "boot", "capture", "features", "pareto", "actions",
         "grid_stat", "grid_stats", "totals", "results")


def _probe_args(rng, m, getter):
    """A baseline for paired / boot: the same id, a grid inside the snapshot, or one outside."""
    if getter not in ("paired", "boot") or m.snap is None:
        return ()
    b = STATIONS[m.snap[1]]
    lo, hi = b.first_id // GS, (b.first_id + b.N) // GS
    return (None,) if rng.random() < 0.4 else (int(rng.integers(lo, hi)),) if rng.random() < 0.8 else (hi,)


def sequence(seed):
    """40-60 calls as (method, args...) tuples, drawn with np.random.default_rng(seed).
    Every episode is [a move] [switches] a run, each followed by probes; after a
    call that ends something, the getters it ended are probed first."""
    rng = np.random.default_rng(seed)
    m, calls = Ctx(), []
    names = list(STATIONS)

    def emit(meth, *args):
        calls.append((meth,) + args)
        return getattr(m, meth)(*args)

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    def readable():
        return [g for g in GETTERS if m.get_status(g) == OK]

    def probes(k, before=()):
        """The getters a call just ended (ESTATE, under the in-bounds rule) first, then k others."""
        ended = [g for g in before if m.get_status(g) == ESTATE and m.in_bounds(g)]
        fresh = [g for g in readable() if g not in before]
        rng.shuffle(ended)
        rng.shuffle(fresh)
        ended.sort(key=_RARE.index)                 # the getters few states reach come first
        for g in ended[:int(rng.integers(3, 6))] + fresh[:int(rng.integers(1, 4))]:
            emit("get", g, *_probe_args(rng, m, g))
        for _ in range(k):
            pool = [g for g in GETTERS if m.get_status(g) != ESTATE or m.in_bounds(g)]
            res = m.obj["res"]
            if res is not None and STATIONS[res[0]].paired_ok and rng.random() < 0.6:  # the sweep stations' own calls
                pool = ["capture"] if m.snap is None else ["capture", "paired", "paired", "boot", "boot"]
            if not pool:
                return
            g = pick(pool)
            emit("get", g, *_probe_args(rng, m, g))
            if rng.random() < 0.1:
                emit("kernel_ms")

    def rich_run():
        """A run that leaves much to read, so that the next ending call ends it."""
        if not m.detail_on and rng.random() < 0.4:
            emit("switch", "detail_on", True)
        r = rng.random()
        if r < 0.35:
            emit("rollout", True)
        else:
            if m.weights != "cfg":
                emit("set_weights", "cfg")
            if r < 0.75:
                emit("policy_grad")
            else:
                if not m.feat_on:
                    emit("switch", "feat_on", True)
                emit("policy_rollout", True, True)
        emit("last_engine")

    def move():
        cur = m.sc or next((n for n in names if STATIONS[n].world == m.world), None)
        same_world = [n for n in names if STATIONS[n].world == m.world and n != cur]
        if m.can_run and rng.random() < 0.6:
            rich_run()
        r = rng.random()
        before = readable()
        sweep = m.sc in ("E", "F")
        if r < 0.05:                                   # a world that fails validation: nothing changes
            emit("set_world", pick(names), False)
            probes(2)
            return
        if r < 0.10:                                   # a scenario set that fails: the set and its load end
            emit("set_scenarios", cur, False)
            probes(2)
            emit("rollout", False)                      # ESTATE: the library checks the set before it launches
            emit("set_load", 0)
            emit("set_scenarios", cur)
        elif r < (0.45 if sweep else 0.22) and same_world:  # another set of the same world
            emit("set_scenarios", pick(same_world))
        elif r < (0.6 if sweep else 0.32) and m.sc is not None:  # the same set again (equal N)
            emit("set_scenarios", m.sc)
        else:
            other = [n for n in names if STATIONS[n].world != m.world]
            if m.sc in ("A", "B") and rng.random() < 0.75:  # the equal-count pair
                tgt = "B" if m.sc == "A" else "A"
            else:
                if rng.random() < 0.3:                 # no longer horizon: what the world ends stays in bounds
                    other = [n for n in other if STATIONS[n].T <= m.T] or other
                tgt = pick(other + [n for n in other if n in ("E", "F", "D", "A", "B")])
            emit("set_world", tgt)
            if rng.random() < 0.6:                     # the broken order: no scenario set yet
                probes(int(rng.integers(0, 2)), before)
                emit("set_load", 0)                     # ESTATE, and nothing is launched from here
            emit("set_scenarios", tgt)
        if rng.random() < 0.45:                        # the other broken order: a set without a load
            probes(int(rng.integers(0, 2)), before)
            emit("rollout", bool(rng.integers(2)))      # ESTATE before anything is launched
        else:
            probes(0, before)
        emit("set_load", int(rng.integers(2)))

    def run():
        r = rng.random()
        before = readable()
        s = STATIONS[m.sc]
        if m.obj["samples"] and s.T * s.N <= 4865 and rng.random() < 0.35:
            r = 0.8                                     # the backward that ends the samples
        if r < 0.36:
            if m.detail_on and rng.random() < (0.8 if m.sc == "D" else 0.4):
                emit("switch", "detail_on", False)  # the station's own engine; what held the detail ends
            emit("rollout", bool(rng.random() < (0.35 if m.obj["traj"] else 0.7)))
        elif r < 0.60:
            if m.weights != "cfg" and rng.random() < 0.9:
                emit("set_weights", "cfg")
            if m.weights in (None, "cfg"):
                emit("policy_rollout", bool(rng.random() < (0.3 if m.obj["traj"] else 0.6)),
                     bool(rng.random() < (0.4 if m.obj["actions"] else 0.7)))
        elif r < 0.74:
            if m.weights != "cfg":
                emit("set_weights", "cfg")
            emit("policy_grad")
        elif r < 0.84:
            if m.weights != "exact" and (m.weights is not None or rng.random() < 0.7):
                emit("set_weights", "exact")
            # as many rows as the samples hold where an exact case has them: the probe after it stays in bounds
            emit("mlp_backward", 4865 if m.obj["samples"] and s.T * s.N <= 4865 else MLP_ROWS)
        elif r < 0.92:
            if rng.random() < 0.8:
                if m.weights != "exact":
                    emit("set_weights", "exact")
                emit("mlp_set_states")
            emit("mlp_forward")
            if m.states == "set" and m.forward and m.weights == "exact":
                emit("mlp_actions")
            emit("kernel_ms")
        else:
            emit("set_load", int(rng.integers(2)))      # a new load: the results stay the last run's
        emit("last_engine")
        if rng.random() < 0.5:
            probe_all("results")
        probes(int(rng.integers(0, 3)), before)

    def switches():
        r = rng.random()
        if r < 0.25:
            emit("switch", "detail_on", not m.detail_on)
        elif r < 0.40:
            emit("switch", "fused_off", not m.fused_off)
        elif r < 0.55:
            emit("switch", "feat_on", not m.feat_on)

    def probe_all(*getters):
        for g in getters:
            if m.get_status(g) != ESTATE or m.in_bounds(g):
                emit("get", g, *_probe_args(rng, m, g))

    def goto(name):
        if m.world != STATIONS[name].world:
            emit("set_world", name)
            if rng.random() < 0.3:
                emit("set_load", 0)                     # the broken order: ESTATE without a scenario set
        emit("set_scenarios", name)
        if rng.random() < 0.3:
            emit("rollout", False)                      # the other broken order: ESTATE without a load
        emit("set_load", int(rng.integers(2)))

    def weights(which):
        if m.weights != which:
            emit("set_weights", which)

    def switch(name, on):
        if getattr(m, name) != on:
            emit("switch", name, on)

    # Scripted episodes: what the random episodes reach too rarely for the floors
    # of tests/test_ctx_model.py. Every sequence opens with two of them.
    def ended_by_a_rollout():
        goto(pick(["D", "A", "D", "G", "D", "H"]))
        switch("detail_on", True)
        emit("rollout", True)
        emit("last_engine")
        probe_all("trajectory", "timeline", "detail", "pareto", "grid_stat", "grid_stats")
        switch("detail_on", False)
        emit("rollout", False)
        emit("last_engine")
        probe_all("trajectory", "timeline", "detail", "results", "totals")

    def ended_by_a_loop():
        goto(pick(["A", "C", "E", "G", "H", "D"]))
        weights("cfg")
        emit("policy_grad")
        emit("rollout", True)                           # the records and samples stay the loop's
        probe_all("samples", "actions", "features", "trajectory")
        switch("feat_on", False)
        emit("policy_rollout", False, False)
        emit("last_engine")
        probe_all("samples", "actions", "features", "trajectory", "timeline", "totals")

    def ended_by_grad_and_backward():
        goto(pick(["C", "C2", "E", "F", "G", "H"]))     # T N <= 4865: the backward's rows cover the samples
        weights("cfg")
        emit("rollout", True)
        emit("policy_grad")
        emit("last_engine")
        probe_all("trajectory", "timeline", "samples", "grid_stats")
        weights("exact")
        emit("mlp_backward", 4865)
        probe_all("samples", "actions", "features")

    def sweep_pair():
        first, second = ("E", "F") if rng.random() < 0.5 else ("F", "E")
        goto(first)
        emit("rollout", bool(rng.integers(2)))
        emit("get", "capture")
        emit("get", "paired")
        emit("get", "boot", *_probe_args(rng, m, "boot"))
        probe_all("pareto", "grid_stat")
        emit("set_scenarios", second)
        probe_all("capture", "paired", "boot", "pareto", "results", "totals")
        emit("set_load", int(rng.integers(2)))
        emit("rollout", False)
        emit("get", "paired")                           # the same ids: not all inside the snapshot
        b = STATIONS[first]
        emit("get", "paired", int(rng.integers(b.first_id // GS, (b.first_id + b.N) // GS)))
        emit("get", "boot", int(rng.integers(b.first_id // GS, (b.first_id + b.N) // GS)))
        emit("get", "capture")                          # the snapshot is this batch now
        emit("get", "paired")
        emit("set_world", pick(["A", "G", "H"]))        # alone: the snapshot stays, nothing to pair it with
        probe_all("paired", "boot", "capture", "results")
        emit("set_load", 0)

    def equal_count_pair():
        switch("detail_on", False)
        for name in ("A", "B", "A", "D") if rng.random() < 0.5 else ("B", "A", "B", "D"):  # D: the skewed schedule
            goto(name)
            emit("rollout", True)
            probe_all("trajectory", "timeline", "results")
        emit("last_engine")

    def world_alone():
        goto(pick(["A", "D", "H"]))
        weights("cfg")
        switch("detail_on", True)
        emit("policy_grad")
        emit("rollout", True)
        emit("set_world", pick([n for n in names if STATIONS[n].T <= m.T and STATIONS[n].world != m.world]))
        probe_all("trajectory", "timeline", "detail", "samples", "actions", "features", "results")
        emit("set_load", 0)
        emit("kernel_ms")
        switch("detail_on", False)

    def set_again():
        goto("B")
        weights("cfg")
        switch("detail_on", True)
        emit("policy_grad")
        probe_all("detail", "samples")
        emit("set_scenarios", "C")                      # fewer scenarios
        probe_all("actions", "samples", "features", "totals")
        emit("set_load", int(rng.integers(2)))
        emit("policy_grad")
        probe_all("detail", "grid_stats")
        emit("set_scenarios", "C2")                     # as many
        probe_all("actions", "samples", "features", "grid_stats")
        emit("set_load", int(rng.integers(2)))
        switch("detail_on", False)

    scripted = (ended_by_a_rollout, ended_by_a_loop, ended_by_grad_and_backward, sweep_pair, equal_count_pair,
                world_alone, set_again)
    if rng.random() < 0.75:
        emit("set_weights", "cfg")
    if rng.random() < 0.3:                              # before any world: every launch is ESTATE
        emit("set_scenarios", "A")
        emit("rollout", False)
        emit("kernel_ms")
    scripted[seed % 7]()
    scripted[(seed // 7 + seed % 7 + 1) % 7]()
    if not m.can_run:
        goto(m.sc or next(n for n in names if STATIONS[n].world == m.world))
    target = int(rng.integers(52, 61))
    while len(calls) < target:
        if rng.random() < 0.65:
            move()
        switches()
        run()
    return calls[:60]


def replay(calls):
    """[(call, status, payload key, facts)] of a sequence on a fresh model; facts:
    for a getter the object's ending call and the in-bounds rule at that moment,
    for a run the engine."""
    m, out = Ctx(), []
    for c in calls:
        facts = {}
        if c[0] == "get":
            facts = dict(ended_by=m.ended_by[OBJECT[c[1]]], in_bounds=m.in_bounds(c[1]))
        st, key = getattr(m, c[0])(*c[1:])
        if c[0] in ("rollout", "policy_rollout", "policy_grad") and st == OK:
            facts = dict(engine=m.engine)
        out.append((c, st, key, facts))
    return out
