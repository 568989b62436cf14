"""Device time of the paired bootstrap (docs/SEMANTICS.md 9), B = 1000 replicates,
p2.5 / p97.5: boot_delta_kernel, boot_sums_kernel and boot_select_kernel, each
alone, from HIP events around back-to-back launches (ccka_debug_boot_ms: median
of 5 samples after a warm-up; two alternating rounds here, their agreement
reported), at

    4096 grids x 1024 pairs   against one baseline grid and in SAME mode
    2 grids x 100,000 pairs   (the deltas gathered from the L2-resident array)

Beside them, in the same process: paired_kernel on the same columns
(ccka_debug_paired_ms), the wall time of Engine.results() for the batch (the
route without the feature, before any host resampling), and a VALU-issue
estimate: Philox calls times the instruction counts of the sums kernel's inner
loop as tools/boot_isa.py read them from the gfx950 ISA
(profiles/boot/isa_counts.json; left out when that file is for another tile
width or other sources than this tree's). The estimate assumes --valu-cycles cycles per wave
instruction, four issue slots for a 32-bit multiply and --ghz; it is a figure to
hold the measurement against, not a measurement.

The grid-tile width K and the staging limit are chosen by the A/B this tool
runs on the 4096 x 1024 shape: the sums kernel for every (K, staged / gathered)
instantiation; the table is written out whole, losers included.

Exits 1 unless the device time of the 4096 x 1024 case (the three kernels, the
slower baseline mode) is below the readback's wall time.

    python tools/boot_time.py [--grids 4096] [--traces 1024] [--replicates 1000] [--reps 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ccka import abi, configs  # noqa: E402
from ccka.engine import Engine  # noqa: E402
from paired_time import paired_ms  # noqa: E402

ISA_COUNTS = os.path.join(ROOT, "profiles", "boot", "isa_counts.json")


def isa_counts(tile):
    """(the counts tools/boot_isa.py read from the ISA, None) while they describe
    this tree's sums kernel at this tile width, else (None, why not)."""
    from boot_isa import source_hashes
    if not os.path.exists(ISA_COUNTS):
        return None, "no profiles/boot/isa_counts.json (run tools/boot_isa.py)"
    with open(ISA_COUNTS) as f:
        c = json.load(f)
    if c["tile"] != tile:
        return None, f"isa_counts.json is for tile {c['tile']}, the build's is {tile}"
    if c["sources_sha256"] != source_hashes():
        return None, "isa_counts.json is stale: the kernel's sources changed (run tools/boot_isa.py)"
    return c, None


def roll(eng, grids, traces, steps):
    eng.set_world(configs.config2_world(n_steps=steps))
    eng.set_scenarios(configs.config4_scenarios(0, grids, traces))
    eng.gen_load(configs.config4_trace_gen())
    eng.rollout()
    eng.paired_capture(traces)


def boot_ms(eng, traces, base_grid, B, reps, tile=0, stage=-1):
    spec = abi.boot_spec(traces, base_grid, B, 0x123456789ABCDEF, 25000, 975000)
    d, s, q = eng.debug_boot_ms(spec, reps, tile, stage)
    return {"delta_ms": d, "sums_ms": s, "select_ms": q, "total_ms": d + s + q}


def two_rounds(fns):
    """Every variant in turn, twice; per variant the minimum and the rounds' relative spread."""
    rounds = [[f() for f in fns] for _ in range(2)]
    out = []
    for a, b in zip(*rounds):
        best = {k: min(a[k], b[k]) for k in a}
        best["round_spread"] = abs(a["total_ms"] - b["total_ms"]) / max(min(a["total_ms"], b["total_ms"]), 1e-9)
        out.append(best)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=configs.CONFIG4_GRIDS)
    ap.add_argument("--traces", type=int, default=configs.CONFIG4_TRACES)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--long-grids", type=int, default=2)
    ap.add_argument("--long-traces", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--valu-cycles", type=float, default=4.0)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.replicates

    eng = Engine(0)
    name, cus = eng.device_info()
    stage, tile = eng.debug_boot_limits()
    roll(eng, a.grids, a.traces, a.steps)
    fixed, same = two_rounds([lambda: boot_ms(eng, a.traces, 0, B, a.reps),
                              lambda: boot_ms(eng, a.traces, abi.PAIRED_SAME, B, a.reps)])
    _, pk_fixed = paired_ms(eng, a.traces, 0, None, 20)
    _, pk_same = paired_ms(eng, a.traces, abi.PAIRED_SAME, None, 20)
    # the A/B of the tile width and of staging: the sums kernel alone, one baseline grid
    variants = []
    for k in (1, 2, 4, 8):
        lim = stage if k * stage <= 4096 else 4096 // k   # a staged workgroup holds 128 KiB at the most
        if lim >= a.traces:
            variants.append((k, lim))         # staged: the tile's records fit the workgroup's LDS
        variants.append((k, 0))               # gathered from the delta array
    ab = two_rounds([(lambda k=k, s=s: boot_ms(eng, a.traces, 0, B, a.reps, k, s)) for k, s in variants])
    ab_table = [{"tile": k, "staged": s > 0, "sums_ms": r["sums_ms"], "round_spread": r["round_spread"]}
                for (k, s), r in zip(variants, ab)]
    # the readback without the feature: every result column of the batch to the host, wall time
    eng.results()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = eng.results()
        walls.append((time.perf_counter() - t0) * 1e3)
    readback_ms = sorted(walls)[1]
    readback_bytes = sum(v.nbytes for v in res.values())
    del res

    # the VALU-issue estimate of the sums kernel at the shipped tile
    isa, why = isa_counts(tile)
    calls = B * ((a.traces + 3) // 4) * ((a.grids + tile - 1) // tile)
    if isa:
        slots = 4 * isa["mul32"] + isa["add64"] + isa["other_valu"]
        valu_ms = calls / 64 * slots * a.valu_cycles / (cus * 4 * a.ghz * 1e9) * 1e3
        estimate = {"mul32": isa["mul32"], "add64": isa["add64"], "other_valu": isa["other_valu"],
                    "lds_read_b128": isa["lds_read_b128"], "issue_slots_per_call": slots,
                    "counts_from": "profiles/boot/isa_counts.json", "sources_sha256": isa["sources_sha256"],
                    "cycles_per_wave_instruction": a.valu_cycles, "ghz": a.ghz, "sums_kernel_ms": valu_ms}
    else:
        estimate = {"omitted": why}

    roll(eng, a.long_grids, a.long_traces, a.steps)
    (long_fixed,) = two_rounds([lambda: boot_ms(eng, a.long_traces, 0, B, a.reps)])
    _, pk_long = paired_ms(eng, a.long_traces, 0, None, 20)

    device_ms = max(fixed["total_ms"], same["total_ms"])
    out = {
        "device": name.strip() or "gfx950", "cus": cus, "replicates": B, "lo_ppm": 25000, "hi_ppm": 975000,
        "tile_width": tile, "staging_limit": stage, "launches_per_sample": a.reps,
        "samples": "median of 5 per call after a warm-up, two alternating rounds, the minimum of the two",
        "config4": {"grids": a.grids, "pairs": a.traces, "fixed_baseline": fixed, "same": same,
                    "paired_kernel_fixed_ms": pk_fixed, "paired_kernel_same_ms": pk_same,
                    "gathers": a.grids * a.traces * B, "philox_calls": calls},
        "long": {"grids": a.long_grids, "pairs": a.long_traces, "fixed_baseline": long_fixed,
                 "paired_kernel_fixed_ms": pk_long},
        "sums_kernel_ab_config4_fixed_baseline": ab_table,
        "valu_estimate": estimate,
        "results_readback_wall_ms": readback_ms,
        "results_readback_wall_ms_samples": walls,
        "results_readback_bytes": readback_bytes,
        "bootstrap_device_ms_slower_mode": device_ms,
        "device_below_readback": device_ms < readback_ms,
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
