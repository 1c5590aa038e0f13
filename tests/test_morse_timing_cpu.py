"""The Morse decoder's element timing and capacity arithmetic (csrc/ddc_morse_timing.h, what k_morse and ddc_morse.cpp both
use), without a GPU and outside Python: tests/morse_timing_test.cpp is a program of its own, built with a host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_morse_timing_under_asan_and_ubsan(tmp_path):
    """Vectors written out in the program: the tracker's negative step with its arithmetic shift, the bounds of a pair,
    both clamps, FIXED; the element count at 15, 16 and 255 (and beyond) with LONG; marks of 2^24 - 1, 2^24 and more
    samples; sample counts across and beyond 2^32 and 2^63; an emission and a rising edge on the same sample, and the
    sample before; WORD at 79, 80 and 81 samples of 16 a dot; the least distance of two emissions reached by marks of
    one sample, and the bound against every window of such a series."""
    exe = str(tmp_path / "morse_timing_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "morse_timing_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
