"""Compare the device code of two builds kernel by kernel.
Each directory holds one assembly file per unit, made with that unit's Makefile flags plus
`--cuda-device-only -S` (hipcc $(HIPFLAGS) [$(MLPFLAGS)] --cuda-device-only -S -o DIR/unit.s unit.hip).
A kernel is its code (.type .. .Lfunc_end), its .amdhsa_kernel block and its metadata entry; .file / .ident /
.loc lines, the per-file numbering of local labels, runs of blanks and the file a kernel sits in are ignored. Prints
"identical" or the number of differing lines with the register, scratch and spill figures of both sides;
exits 1 if a kernel differs, or exists on one side only, whose symbol contains none of the --allow strings.
usage: python tools/kernel_diff.py parent_asm/ head_asm/ [--allow SUBSTRING ...] [--show]"""
import argparse
import difflib
import glob
import os
import re
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
          ".sgpr_spill_count")
SKIP = re.compile(r"\s*\.(file|ident|loc)\b")
LABEL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_|\b)")  # .LBB3_12 -> .LBB_12, BB3_12 -> BB_12, .Lfunc_end3 -> .Lfunc_end


def kernels(directory):
    """{symbol: (lines, {field: value})} over every *.s of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text, meta, cur, entry = {}, [], None, None
        for raw in open(path):
            line = LABEL.sub(r"\1\2", raw.rstrip())
            if SKIP.match(line):
                continue
            m = re.match(r"\s*\.type\s+(\S+),@function", line) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = m.group(1)
            if cur is not None:
                text.setdefault(cur, []).append(" ".join(line.split()))  # (comment columns follow the label widths)
                if line.startswith(".Lfunc_end:"):
                    cur = None
            if re.match(r"  - \.", line):  # a kernel's metadata entry begins
                entry = []
                meta.append(entry)
            elif line.startswith("amdhsa.") or line == "...":
                entry = None
            if entry is not None:
                entry.append(line)
        for entry in meta:
            name = next((ln.split()[-1] for ln in entry if ln.lstrip("- ").startswith(".name:")), None)
            if name in text:
                fig = {f: ln.split()[-1] for ln in entry for f in FIELDS if ln.lstrip("- ").startswith(f + ":")}
                out[name] = (text[name] + entry, fig)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--allow", action="append", default=[], help="substring of a kernel symbol that may differ")
    ap.add_argument("--show", action="store_true", help="print the differing lines")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.head)
    bad = 0
    for sym in sorted(set(old) | set(new)):
        allowed = any(s in sym for s in a.allow)
        if sym not in old or sym not in new:
            print(f"{sym}: only in {'head' if sym in new else 'parent'}")
            bad += not allowed
            continue
        if old[sym][0] == new[sym][0]:
            print(f"{sym}: identical")
            continue
        d = [ln for ln in difflib.unified_diff(old[sym][0], new[sym][0], n=0, lineterm="")
             if ln[0] in "+-" and ln[:3] not in ("+++", "---")]
        figs = " ".join(f"{f[1:]} {old[sym][1].get(f)}->{new[sym][1].get(f)}" for f in FIELDS)
        print(f"{sym}: {len(d)} differing lines{' (allowed)' if allowed else ''}; {figs}")
        if a.show:
            print("\n".join("    " + ln for ln in d))
        bad += not allowed
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
