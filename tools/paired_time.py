"""Device time of the paired comparison at the config-4 shape (4096 grids x 1024
shared traces): paired_capture_kernel, and paired_kernel with every objective
SUM (the streaming pass alone) and with p95 on all four objectives, against one
baseline grid and in SAME mode, each from HIP events around back-to-back
launches (ccka_debug_paired_ms). In the same process: the p95 selection of the
sweep statistics on the same columns (ccka_debug_grid_stat_ms), the streaming
floor of the bytes the comparison reads over the measured copy ceiling, and the
wall time of Engine.results() for the batch, the route without this feature.
Only the result columns matter, so a short horizon is rolled out.

Exits 1 unless the device time with p95 on all four objectives (the slower of
the two baseline modes) is below that readback's wall time.

    python tools/paired_time.py [--grids 4096] [--traces 1024] [--steps 60] [--reps 50] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ccka import abi, configs  # noqa: E402
from ccka.engine import Engine  # noqa: E402
from sweep_stat_time import ROW_BYTES, copy_gbs, kernel_ms  # noqa: E402

SNAP_BYTES = 32  # four int64 per scenario


def paired_ms(eng, grid_size, base_grid, stat, reps):
    fn = eng.lib.ccka_debug_paired_ms
    fn.argtypes = [C.c_void_p, C.POINTER(abi.PairedSpec), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    spec = abi.paired_spec(grid_size, base_grid, stat)
    cap, par = C.c_double(), C.c_double()
    eng._chk(fn(eng.ctx, C.byref(spec), reps, C.byref(cap), C.byref(par)), "ccka_debug_paired_ms")
    return cap.value, par.value


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
    eng.paired_capture(a.traces)
    p95 = abi.sweep_stat(*[("quantile", 950000)] * 4)
    # the variants in turn, twice: the spread between the rounds is the noise
    rounds = []
    for _ in range(2):
        c1, s_fix = paired_ms(eng, a.traces, 0, None, a.reps)
        c2, q_fix = paired_ms(eng, a.traces, 0, p95, a.reps)
        c3, q_same = paired_ms(eng, a.traces, abi.PAIRED_SAME, p95, a.reps)
        _, sel = kernel_ms(eng, a.traces, p95, a.reps)
        rounds.append({"capture_ms": [c1, c2, c3], "paired_all_sum_ms": s_fix, "paired_p95_fixed_ms": q_fix,
                       "paired_p95_same_ms": q_same, "grid_select_p95_ms": sel})
    best = lambda k: min(r[k] for r in rounds)  # noqa: E731
    caps = sorted(v for r in rounds for v in r["capture_ms"])
    capture_ms = 0.5 * (caps[2] + caps[3])
    fixed_ms, same_ms = best("paired_p95_fixed_ms"), best("paired_p95_same_ms")
    select_ms = best("grid_select_p95_ms")
    # the readback without the feature: every result column of the batch to the host, wall time
    eng.results()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = eng.results()
        walls.append((time.perf_counter() - t0) * 1e3)
    readback_ms = sorted(walls)[1]
    readback_bytes = sum(v.nbytes for v in res.values())
    gbs = copy_gbs(eng)
    n = a.grids * a.traces
    bytes_fixed = n * ROW_BYTES + a.traces * SNAP_BYTES   # one baseline grid, re-read from L2
    bytes_same = n * (ROW_BYTES + SNAP_BYTES)
    floor = lambda b: b / (gbs * 1e9) * 1e3  # noqa: E731
    device_ms = max(fixed_ms, same_ms)
    out = {
        "device": name.strip() or "gfx950", "cus": cus, "grids": a.grids, "traces": a.traces, "steps": a.steps,
        "launches_per_sample": a.reps, "samples": "median of 5 per call, two alternating rounds",
        "capture_kernel_ms": capture_ms,
        "paired_all_sum_ms": best("paired_all_sum_ms"),
        "paired_p95_fixed_baseline_ms": fixed_ms,
        "paired_p95_same_ms": same_ms,
        "grid_select_p95_ms": select_ms,
        "paired_p95_fixed_over_grid_select": fixed_ms / select_ms,
        "paired_p95_same_over_grid_select": same_ms / select_ms,
        "copy_ceiling_gbs_read_plus_write": gbs,
        "bytes_read_fixed_baseline": bytes_fixed,
        "bytes_read_same": bytes_same,
        "streaming_floor_fixed_ms": floor(bytes_fixed),
        "streaming_floor_same_ms": floor(bytes_same),
        "capture_bytes_read_plus_written": n * (ROW_BYTES + SNAP_BYTES),
        "capture_streaming_floor_ms": floor(n * (ROW_BYTES + SNAP_BYTES)),
        "results_readback_wall_ms": readback_ms,
        "results_readback_wall_ms_samples": walls,
        "results_readback_bytes": readback_bytes,
        "paired_p95_device_ms_slower_mode": device_ms,
        "device_below_readback": device_ms < readback_ms,
        "rounds": rounds,
    }
    out = json.loads(json.dumps(out), parse_float=lambda v: float(f"{float(v):.5g}"))
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()
    return 0 if device_ms < readback_ms else 1


if __name__ == "__main__":
    sys.exit(main())
