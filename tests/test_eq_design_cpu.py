"""The equaliser's host arithmetic (csrc/ddc_eq_design.h: the stability test and the section designs), without a GPU and
outside Python: tests/eq_design_test.cpp is a program of its own, built with a host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eq_design_under_asan_and_ubsan(tmp_path):
    """The stability triangle |a2| < 1, |a1| < 1 + a2 on, one ulp inside and one ulp outside its edges and at its corners;
    NaN and the infinities in each of the five places; the designs' argument tests (a refusal leaves *out alone); every
    kind at both audio rates over corners from 1e-12 of the rate to 1e-12 below its half, Q from 1e-6 to 1e12 and gains
    from -400 to 20000 dB: what comes out passes the stability test, and over the ordinary range (corner 0.002 .. 0.49 of
    the rate, Q 0.1 .. 30, +-60 dB) a section always comes out."""
    exe = str(tmp_path / "eq_design_test")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "eq_design_test.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
