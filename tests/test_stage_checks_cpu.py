"""The arithmetic behind the argument tests of the per-receiver stages' process() (csrc/ddc_stage_checks.h), without a
GPU and outside Python: tests/stage_checks_test.cpp is a program of its own, built with a host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_checks_under_asan_and_ubsan(tmp_path):
    """Byte ranges that are disjoint, touch, share one byte, are identical or nested, in both argument orders; the
    bytes nrx rows of n items span at a stride, for item sizes 2, 4, 8; strict and "or NULL" pointer alignment; the
    squelch's completed blocks against a counting loop for B in {1, 2, 48, 4095, 4096}, starts around multiples of B up
    to beyond 2^63."""
    exe = str(tmp_path / "stage_checks_test")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "stage_checks_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
