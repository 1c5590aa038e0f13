"""The wideband blanker's integer arithmetic (csrc/ddc_wblank_gate.h, what k_wblank_* and ddc_wblank.cpp both use), without
a GPU and outside Python: tests/wblank_gate_test.cpp is a program of its own, built with a host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wblank_gate_under_asan_and_ubsan(tmp_path):
    """Vectors written out in the program: the codes -2^23 and 2^23 - 1, p = 2^47 and a block sum of 2^59, mean thr16 at
    2^63 with the comparison's strictness, every (num, r) of the scaling against a 64-bit restatement, toward zero on
    both sides, the re-pack of negative values byte by byte and back, the carried lengths for D = 0, 1, 255 and all
    between, the block grid at stream positions beyond 2^32 and at the top of uint64."""
    exe = str(tmp_path / "wblank_gate_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "wblank_gate_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
