"""Build-time variants of one kernel unit as separate libccka.so copies under
csrc/build/variants/<name>/, linked with the main build's other objects. Profiling aid only.
NAME=-DX builds rollout_d1.hip (the single-deployment engine) with extra flags, e.g.
-DCCKA_ABLATE_BUILD=1 (kparams.h; tools/ablate.py). NAME=r@other.hip replaces rollout.hip (the general
kernel's one- and two-deployment instantiations of rollout_kernel.h; NAME=r@rollout.hip:-DGK_STAMPS builds
rollout.hip itself with the phase stamps), NAME=p@other.hip pg.hip, NAME=m@other.hip mlp.hip
(NAME=m@mlp.hip:-DX builds mlp.hip itself with extra flags), NAME=a@other.cpp abi_mlp.cpp (the weight
packing; mutation checks of tests/test_gpu_mlp.py and tests/test_gpu_pg.py), NAME=s@-DX rollout_sk.hip (the general
kernel's lane-skewed schedule; -DCCKA_SK_ONE instantiates <2, 8> only, -DCCKA_SK_LF2=1 instantiates its kernels
with the lane-local provisioning branch, which the main build's abi_rollout.o then switches on), NAME=x@DIR every
abi_*.cpp of DIR, a directory laid out like csrc/ with ../../include/ccka.h beside it (an earlier commit's files, or a
mutated copy: the checks of tests/test_gpu_ctx_state.py; the units share ctx.h, so all of them are rebuilt). Set
VARIANTS_NO_MAKE=1 to link against the objects already built.
usage: python tools/build_variants.py name=-DCCKA_ABLATE_BUILD=1 [name2="-DA -DB" ...]"""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
         "-Wall", "-Wno-unused-function"]
if not os.environ.get("VARIANTS_NO_MAKE"):
    subprocess.run(["make", "-s", "-C", CSRC], check=True)
procs = []
abi_sets = []
for arg in sys.argv[1:]:
    name, _, defs = arg.partition("=")
    if defs.startswith("x@"):  # the C ABI's units from another directory
        out = os.path.join(CSRC, "build", "variants", name)
        os.makedirs(out, exist_ok=True)
        units = sorted(glob.glob(os.path.join(defs[2:], "abi_*.cpp")))
        assert units, defs
        objs = [os.path.join(out, os.path.basename(u)[:-4] + ".o") for u in units]
        abi_sets.append((name, out, objs, [subprocess.Popen(["/opt/rocm/bin/hipcc", *FLAGS, "-c", "-o", o, u])
                                           for u, o in zip(units, objs)]))
        continue
    src, base, extra = "rollout_d1.hip", "rollout_d1.o", []
    if defs.startswith("r@"):  # the general kernel's source (built with the MLP flags, as the Makefile does)
        defs, base, extra = defs[1:], "rollout.o", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    elif defs.startswith("p@"):  # the policy-gradient kernels' source
        defs, base, extra = defs[1:], "pg.o", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    elif defs.startswith("s@"):  # the lane-skewed general kernel's unit
        defs, src, base, extra = defs[2:], "rollout_sk.hip", "rollout_sk.o", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    elif defs.startswith("m@"):  # the MLP kernels' source
        defs, base, extra = defs[1:], "mlp.o", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    elif defs.startswith("a@"):  # the MLP's host side (weight fragment packing), e.g. a mutated copy elsewhere
        defs, base, extra = defs[1:], "abi_mlp.o", ["-I", CSRC]
    if defs.startswith("@"):  # NAME=@other.hip[:flags]: another source file in csrc/ (e.g. a committed version)
        src, _, defs = defs[1:].partition(":")
    out = os.path.join(CSRC, "build", "variants", name)
    os.makedirs(out, exist_ok=True)
    obj = os.path.join(out, base)
    procs.append((name, out, obj, subprocess.Popen(["/opt/rocm/bin/hipcc", *FLAGS, *extra, *defs.split(), "-c", "-o",
                                                    obj, os.path.join(CSRC, src)])))
for name, out, objs, ps in abi_sets:
    assert all(p.wait() == 0 for p in ps), name
    mine = {os.path.basename(o) for o in objs}
    others = [f for f in sorted(glob.glob(os.path.join(CSRC, "build", "*.o"))) if os.path.basename(f) not in mine]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                    os.path.join(out, "libccka.so"), *objs, *others, "-L/opt/rocm/lib", "-lrccl",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    print("built", name)
for name, out, obj, p in procs:
    assert p.wait() == 0, name
    # the main build's other objects (the Makefile's UNITS and ABI_UNITS, as built)
    others = [f for f in sorted(glob.glob(os.path.join(CSRC, "build", "*.o")))
              if os.path.basename(f) != os.path.basename(obj)]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                    os.path.join(out, "libccka.so"), obj, *others, "-L/opt/rocm/lib", "-lrccl",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    print("built", name)
