"""The SITOR decoder's bit clock, framing and capacity arithmetic (csrc/ddc_sitor_bits.h, what k_sitor and ddc_sitor.cpp both
use), without a GPU and outside Python: tests/sitor_bits_test.cpp is a program of its own, built with a host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sitor_bits_under_asan_and_ubsan(tmp_path):
    """The jump to the next strobe against the clock sample by sample, for random acc and inc and for inc = 1 and 2^29 (the
    jump of 2^32 samples included); both corrections at the edges of their ranges; the modem test's bounds and the weight
    of all 128 codes; rules a - c: phasing at each of the 7 bit phases for every lock, the all-valid wrong phases that
    rule b reframes, unlock after `unlock` bad characters, relock needing 7 lock fresh bits, lock = 0, NaN qualities,
    restart; both bounds against every window of a series whose decision alternates at every sample of a first half.
    The program reports how near the bound that series comes: its least strobe distance at inc = step = 2^29 is 6
    samples against D = 4 (two samples of a first half at twice the speed, four of a second half)."""
    exe = str(tmp_path / "sitor_bits_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "sitor_bits_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
    m = re.search(r"least strobe distance (\d+) against the bound (\d+)", p.stdout)
    print(p.stdout.strip())
    assert m and int(m.group(2)) == 4 and 4 <= int(m.group(1)) <= 6
