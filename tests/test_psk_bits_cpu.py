"""The PSK decoder's symbol clock, framing and capacity arithmetic (csrc/ddc_psk_bits.h, what k_psk and ddc_psk.cpp both
use), without a GPU and outside Python: tests/psk_bits_test.cpp is a program of its own, built with a host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psk_bits_under_asan_and_ubsan(tmp_path):
    """The jump to the next strobe against the clock sample by sample, for random acc and inc and for inc = 1 and 2^29 (the
    jump of 2^32 samples included); both corrections at acc = 0 and acc = inc - 1; the modem test's bounds; framing: idle
    zeros, "1 0 0", "a", NaN qualities, 16, 17 and 40 ones (LONG), nb's saturation, restart; the least distance of two
    strobes reached by a clock that is advanced every time, and both bounds against every window of such a series."""
    exe = str(tmp_path / "psk_bits_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "psk_bits_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
