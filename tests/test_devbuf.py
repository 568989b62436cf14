"""DevBuf (csrc/devbuf.h), the owner type of libccka.so's device buffers, on
the CPU: csrc/devbuf_test.cpp instantiates it over a counting, failable malloc
allocator and is built by `make -C csrc devbuf-test` with the host compiler
under AddressSanitizer + UndefinedBehaviorSanitizer (leak detection on). The
program asserts the reserve / resize policies, n == 0, the size_t overflow
refusal, failure and recovery, a group's all-or-none failure, release twice,
both moves, and that every allocation was freed; any sanitizer report aborts it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cost-and-carbon-aware-kubernetes-autoscaler_amd", "csrc")
PROGRAM = os.path.join(CSRC, "build", "devbuf_test")


def test_devbuf_under_sanitizers():
    subprocess.run(["make", "-s", "-C", CSRC, "devbuf-test"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr \
        and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "devbuf ok" in r.stdout
