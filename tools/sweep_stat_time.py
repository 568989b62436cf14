"""Device time of the sweep statistics at the config-4 shape (4096 grids x 1024
shared traces): grid_stats_kernel alone, the selection kernel for all four
objectives at p95, and for the mixed statistic (cost and gCO2 SUM, SLO p95,
energy tail from p90), each from HIP events around back-to-back launches
(ccka_debug_grid_stat_ms), beside the streaming floor of the result columns
over the measured copy ceiling. The statistic does not depend on the horizon,
so a short one is rolled out.

    python tools/sweep_stat_time.py [--grids 4096] [--traces 1024] [--steps 60] [--reps 50] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd"))
from ccka import abi, configs  # noqa: E402
from ccka.engine import Engine  # noqa: E402

ROW_BYTES = 8 + 4 + 8 + 8  # cost int64, SLO int32, gCO2 and energy binary64


def kernel_ms(eng, grid_size, stat, reps):
    fn = eng.lib.ccka_debug_grid_stat_ms
    fn.argtypes = [C.c_void_p, C.c_int64, C.POINTER(abi.SweepStat), C.c_int32, C.POINTER(C.c_double),
                   C.POINTER(C.c_double)]
    s, q = C.c_double(), C.c_double()
    eng._chk(fn(eng.ctx, grid_size, C.byref(stat), reps, C.byref(s), C.byref(q)), "ccka_debug_grid_stat_ms")
    return s.value, q.value


def copy_gbs(eng, nbytes=1 << 31, reps=5):
    fn = eng.lib.ccka_debug_copy_gbs
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
    g = C.c_double()
    eng._chk(fn(eng.ctx, nbytes, reps, C.byref(g)), "ccka_debug_copy_gbs")
    return g.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=configs.CONFIG4_GRIDS)
    ap.add_argument("--traces", type=int, default=configs.CONFIG4_TRACES)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    eng = Engine(0)
    name, cus = eng.device_info()
    eng.set_world(configs.config2_world(n_steps=a.steps))
    eng.set_scenarios(configs.config4_scenarios(0, a.grids, a.traces))
    eng.gen_load(configs.config4_trace_gen())
    eng.rollout()
    p95 = abi.sweep_stat(*[("quantile", 950000)] * 4)
    mixed = abi.sweep_stat(slo=("quantile", 950000), energy=("tail", 900000))
    # alternate the two statistics, twice: the spread between rounds is the noise
    rounds = []
    for _ in range(2):
        s1, q1 = kernel_ms(eng, a.traces, p95, a.reps)
        s2, q2 = kernel_ms(eng, a.traces, mixed, a.reps)
        rounds.append({"grid_stats_ms": [s1, s2], "select_p95_ms": q1, "select_mixed_ms": q2})
    sums = sorted(v for r in rounds for v in r["grid_stats_ms"])
    sum_ms = 0.5 * (sums[1] + sums[2])
    p95_ms = min(r["select_p95_ms"] for r in rounds)
    mixed_ms = min(r["select_mixed_ms"] for r in rounds)
    gbs = copy_gbs(eng)
    nbytes = a.grids * a.traces * ROW_BYTES
    floor_ms = nbytes / (gbs * 1e9) * 1e3
    out = {
        "device": name.strip() or "gfx950", "cus": cus, "grids": a.grids, "traces": a.traces, "steps": a.steps,
        "launches_per_sample": a.reps, "samples": "median of 5 per call, two alternating rounds",
        "grid_stats_kernel_ms": sum_ms,
        "select_all_quantile_p95_ms": p95_ms,
        "select_mixed_ms": mixed_ms,
        "select_p95_over_grid_stats": p95_ms / sum_ms,
        "select_mixed_over_grid_stats": mixed_ms / sum_ms,
        "result_column_bytes": nbytes,
        "copy_ceiling_gbs_read_plus_write": gbs,
        "streaming_floor_ms": floor_ms,
        "grid_stats_over_floor": sum_ms / floor_ms,
        "select_p95_over_floor": p95_ms / floor_ms,
        "select_mixed_over_floor": mixed_ms / floor_ms,
        "rounds": rounds,
    }
    # the same scenario count as grids of twice the size: past the LDS staging
    # limit (1024), every pass re-reads the columns
    g2, t2 = a.grids // 2, a.traces * 2
    eng.set_scenarios(configs.config4_scenarios(0, g2, t2))
    eng.gen_load(configs.config4_trace_gen())
    eng.rollout()
    s3, q3 = kernel_ms(eng, t2, p95, a.reps)
    out["double_grid_size"] = {"grids": g2, "traces": t2, "grid_stats_kernel_ms": s3,
                               "select_all_quantile_p95_ms": q3}
    out = json.loads(json.dumps(out), parse_float=lambda v: float(f"{float(v):.5g}"))
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
