"""Instruction counts of boot_sums_kernel's inner loop (one trip = one Philox
call, four draws, K grids), read from the gfx950 ISA: compiles csrc/boot.hip to
assembly with the Makefile's flags (no GPU needed), finds the staged
instantiation of the build's tile width kBootTile, takes its depth-2 loop and
counts 32-bit multiplies, 64-bit adds, other VALU instructions and LDS reads.
Writes profiles/boot/isa_counts.json with the SHA-256 of the sources the
kernel is built from; tools/boot_time.py uses the counts for its VALU-issue
estimate only while those hashes still match.

    python tools/boot_isa.py [--out profiles/boot/isa_counts.json]
"""
import argparse
import collections
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd", "csrc")
SOURCES = ("boot.hip", "dev_common.h", "kparams.h", "paired_dev.h", "select_dev.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]


def source_hashes():
    out = {}
    for f in SOURCES:
        with open(os.path.join(CSRC, f), "rb") as fh:
            out[f] = hashlib.sha256(fh.read()).hexdigest()
    return out


def build_tile():
    with open(os.path.join(CSRC, "kparams.h")) as fh:
        return int(re.search(r"constexpr int kBootTile = (\d+);", fh.read()).group(1))


def inner_loop(asm, tile):
    """The instructions of the depth-2 loop of boot_sums_kernel<tile, true>."""
    name = f"_ZN4ccka16boot_sums_kernelILi{tile}ELb1EEEvNS_10BootParamsE"
    body = re.split(rf"^{name}:.*$", asm, maxsplit=1, flags=re.M)[1].split("s_endpgm", 1)[0].splitlines()
    start = next(i for i, ln in enumerate(body) if "Inner Loop Header: Depth=2" in ln)
    ops = []
    for ln in body[start:]:
        ln = ln.strip()
        if not ln or ln.startswith((";", ".")):
            continue
        ops.append(ln.split()[0])
        if ops[-1].startswith("s_cbranch"):
            return ops
    raise RuntimeError("no loop end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boot", "isa_counts.json"))
    a = ap.parse_args()
    tile = build_tile()
    asm = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", "-", "boot.hip"], cwd=CSRC, check=True,
                         capture_output=True, text=True).stdout
    ops = collections.Counter(inner_loop(asm, tile))
    valu = {k: v for k, v in ops.items() if k.startswith("v_")}
    mul32 = sum(v for k, v in valu.items() if k.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")))
    add64 = sum(v for k, v in valu.items() if k.startswith("v_lshl_add_u64"))
    out = {"kernel": f"boot_sums_kernel<{tile}, staged>", "tile": tile, "loop": "depth 2: one Philox call, four draws",
           "mul32": mul32, "add64": add64, "other_valu": sum(valu.values()) - mul32 - add64,
           "lds_read_b128": ops.get("ds_read_b128", 0), "instructions": dict(sorted(ops.items())),
           "flags": " ".join(FLAGS), "sources_sha256": source_hashes()}
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
