"""Device time of the fleet timeline (docs/SEMANTICS.md 7) on config 2's
trajectory (1e5 scenarios x 1440 steps, 2.3 GB of records), in the layout the
single-deployment engine writes ([N][T]) and for the same world forced onto the
lockstep general engine ([T][N]): the sums alone for one whole-batch grid per
step and for grids of 1000 per hour, and a NODES p95 on top of the first. HIP
events around back-to-back launches (ccka_debug_timeline_ms: a warm-up, then
the median of 5), two alternating rounds. Beside them, in the same process:
the streaming floor of the records over the measured copy ceiling, and the wall
time of ccka_get_trajectory_native for the same records, the only way to such
numbers without the timeline. The sums must take less time than that readback
(exit status 1 otherwise).

    python tools/timeline_time.py [--scenarios 100000] [--steps 1440] [--reps 10] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd"))
from ccka import abi, configs  # noqa: E402
from ccka.engine import Engine  # noqa: E402
from ccka.world import TRAJ_DTYPE  # noqa: E402

from sweep_stat_time import copy_gbs  # noqa: E402


def kernel_ms(eng, spec, reps):
    fn = eng.lib.ccka_debug_timeline_ms
    fn.argtypes = [C.c_void_p, C.POINTER(abi.TimelineSpec), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    s, q = C.c_double(), C.c_double()
    eng._chk(fn(eng.ctx, C.byref(spec), reps, C.byref(s), C.byref(q)), "ccka_debug_timeline_ms")
    return s.value, q.value


def readback_ms(eng, buf):
    """Wall time of ccka_get_trajectory_native into touched host memory, the faster of two."""
    best = None
    for _ in range(2):
        t = time.perf_counter()
        eng._chk(eng.lib.ccka_get_trajectory_native(eng.ctx, buf.ctypes.data_as(C.POINTER(abi.TrajRec)), buf.size,
                                                    None), "ccka_get_trajectory_native")
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def _layout(eng):
    lay = C.c_int32()
    eng._chk(eng.lib.ccka_trajectory_layout(eng.ctx, C.byref(lay)), "ccka_trajectory_layout")
    return lay.value


def measure(eng, n, reps, floor_ms, buf):
    shapes = {"whole_batch_per_step": abi.timeline_spec(n, 1),
              "grids_of_1000_per_hour": abi.timeline_spec(1000 if n % 1000 == 0 else n, 60),
              "whole_batch_per_step_nodes_p95": abi.timeline_spec(n, 1, "nodes", 950000)}
    rounds = []
    for _ in range(2):  # alternate the shapes, twice: the spread between rounds is the noise
        rounds.append({k: kernel_ms(eng, sp, reps if sp.q_field == 0 else max(1, reps // 5))
                       for k, sp in shapes.items()})
    out = {"layout": "NT" if _layout(eng) == abi.TRAJ_NT else "TN", "engine": eng.last_engine()[0]}
    for k in shapes:
        s = min(r[k][0] for r in rounds)
        out[k] = {"sum_ms": s, "sum_over_floor": s / floor_ms, "rounds_sum_ms": [r[k][0] for r in rounds]}
        if shapes[k].q_field:
            q = min(r[k][1] for r in rounds)
            out[k].update(select_ms=q, select_over_floor=q / floor_ms, rounds_select_ms=[r[k][1] for r in rounds])
    out["get_trajectory_native_wall_ms"] = readback_ms(eng, buf)
    out["readback_over_slowest_sums"] = out["get_trajectory_native_wall_ms"] / max(
        out[k]["sum_ms"] for k in shapes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    eng = Engine(0)
    name, cus = eng.device_info()
    eng.set_world(configs.config2_world(n_steps=a.steps))
    eng.set_scenarios(configs.hpa_scenarios(a.scenarios))
    eng.gen_load(configs.trace_gen())
    nbytes = a.scenarios * a.steps * TRAJ_DTYPE.itemsize
    gbs = copy_gbs(eng)
    floor_ms = nbytes / (gbs * 1e9) * 1e3
    buf = np.empty(a.scenarios * a.steps, TRAJ_DTYPE)
    buf.view(np.uint8)[:] = 0  # touched: the readback pays no page faults
    out = {"device": name.strip() or "gfx950", "cus": cus, "scenarios": a.scenarios, "steps": a.steps,
           "launches_per_sample": a.reps, "samples": "median of 5 per call, the faster of two alternating rounds",
           "record_bytes": nbytes, "copy_ceiling_gbs_read_plus_write": gbs, "streaming_floor_ms": floor_ms}
    for key, mode in (("single_deployment_engine", 0), ("lockstep_general_engine", 2)):
        eng.set_engine(mode)
        try:
            eng.rollout(trajectory=True)
        finally:
            eng.set_engine(0)
        out[key] = measure(eng, a.scenarios, a.reps, floor_ms, buf)
    out = json.loads(json.dumps(out), parse_float=lambda v: float(f"{float(v):.5g}"))
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()
    slow = [k for k in ("single_deployment_engine", "lockstep_general_engine") if out[k]["readback_over_slowest_sums"] <= 1]
    if slow:
        sys.exit(f"the timeline's sums took longer than the trajectory readback on: {slow}")


if __name__ == "__main__":
    main()
