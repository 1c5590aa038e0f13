"""The MFSK decoder's symbol clock and capacity arithmetic (csrc/ddc_mfsk_bits.h, what k_mfsk and ddc_mfsk.cpp both use),
without a GPU and outside Python: tests/mfsk_bits_test.cpp is a program of its own, built with a host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mfsk_bits_under_asan_and_ubsan(tmp_path):
    """The jump to the next wrap against the clock sample by sample, with and without a borrowed wrap pending, for random
    acc and inc and for inc = 1 and 2^29 (the jump of 2^32 samples included); a clock corrected at random, always early
    and always late against a phase kept in 64 signed bits: the same strobes, the late correction's borrow one sample
    long, no two strobes nearer than the least distance, no window of n samples over the bound; the modem test's
    bounds; the slot arithmetic of what a receiver carries."""
    exe = str(tmp_path / "mfsk_bits_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "mfsk_bits_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
