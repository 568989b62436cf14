"""tools/kernel_diff.py on two hand-written three-kernel builds: one kernel
moved to another file (so its local labels are renumbered), one changed, one
identical."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_diff.py")


def _kernel(sym, index, body, kernarg=16):
    return f"""\t.file\t"unit{index}.hip"
\t.globl\t{sym}
\t.type\t{sym},@function
{sym}:
\t.loc\t1 {index + 7} 0
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB{index}_1:{' ' * (30 - len(str(index)))}; =>This Inner Loop Header: Depth=1
{body}
\ts_cbranch_scc1 .LBB{index}_1
; %bb.2:                                ;   in Loop: Header=BB{index}_1 Depth=1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_kernarg_size {kernarg}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{sym}, .Lfunc_end{index}-{sym}
"""


def _meta(sym, vgpr, spill=0):
    return f"""  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .name:           {sym}
    .private_segment_fixed_size: {4 * spill}
    .sgpr_count:     12
    .sgpr_spill_count: 0
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: {spill}
"""


def _unit(path, kernels):
    # kernels: (symbol, body, vgprs, spills); the index in the file numbers the labels
    text = "".join(_kernel(s, i, b) for i, (s, b, _, _) in enumerate(kernels))
    meta = "".join(_meta(s, v, sp) for s, _, v, sp in kernels)
    path.write_text(text + '\t.ident\t"clang"\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n' + meta +
                    "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


def _run(*args):
    return subprocess.run([sys.executable, TOOL, *map(str, args)], capture_output=True, text=True)


def test_moved_changed_identical(tmp_path):
    old, new = tmp_path / "parent", tmp_path / "head"
    old.mkdir()
    new.mkdir()
    same = ("k_same", "\tv_add_u32 v0, v0, v1", 4, 0)
    moved = ("k_moved", "\tv_mul_lo_u32 v0, v0, v1", 6, 0)
    _unit(old / "a.s", [same, moved])
    _unit(old / "b.s", [("k_changed", "\tv_sub_u32 v0, v0, v1\n\tv_mov_b32 v2, 0", 8, 1)])
    _unit(new / "a.s", [same])
    _unit(new / "b.s", [moved, ("k_changed", "\tv_sub_u32 v0, v1, v0", 7, 0)])  # k_moved: .LBB1_ -> .LBB0_, k_changed: 0 -> 1
    r = _run(old, new)
    lines = dict(ln.split(": ", 1) for ln in r.stdout.strip().splitlines())
    assert r.returncode == 1, r.stdout + r.stderr
    assert lines["k_same"] == "identical" and lines["k_moved"] == "identical"
    ch = lines["k_changed"]
    # two old code lines against one new one, and three metadata figures that changed (two lines each)
    assert ch.startswith("9 differing lines;"), ch
    for want in ("vgpr_count 8->7", "agpr_count 0->0", "sgpr_count 12->12", "private_segment_fixed_size 4->0",
                 "vgpr_spill_count 1->0", "sgpr_spill_count 0->0"):
        assert want in ch, ch
    ok = _run(old, new, "--allow", "k_changed")
    assert ok.returncode == 0 and "(allowed)" in ok.stdout
    assert _run(old, new, "--allow", "k_same").returncode == 1
    assert _run(old, old).returncode == 0
