"""The radiofax decoder's pixel clock, line structure and capacity arithmetic (csrc/ddc_fax_bits.h, what k_fax and ddc_fax.cpp
both use), without a GPU and outside Python: tests/fax_bits_test.cpp is a program of its own, built with a host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process."""
import os
import subprocess

import numpy as np
import pytest

import fax_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fax_bits") / "fax_bits_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "libperseus-sdr_amd", "csrc"), "-o", path,
                    os.path.join(ROOT, "tests", "fax_bits_test.cpp")], check=True)
    return path


def test_fax_bits_under_asan_and_ubsan(exe):
    """The strobes' closed form and the pixel's slot against the clock sample by sample for every class of inc (1, small,
    odd, powers of two, 2^31 - 1 and 2^31) and acc; every window's strobes against fax_most_pixels, which acc = 2^32 - 1
    reaches; the product's halves against 128-bit arithmetic up to 2^40 samples; the lines of pixel streams that begin at
    every column against fax_most_lines at widths 16, 64, 100 and 8192; the modem test's bounds (overlapping ranges in
    either order); the line rule on hand-made tone lines: classes, runs, need, the broken run, the hysteresis band and the
    level carried over a line's end, the run's saturation."""
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:") and "runtime error:" not in p.stderr, (p.stdout[-500:], p.stderr[-1500:])
    print(p.stdout.strip())


@pytest.mark.parametrize("width", [16, 100, 8192])
def test_the_line_rule_against_the_python_rule(exe, tmp_path, width):
    """Random pixel streams of three kinds (uniform bytes, bytes around the three levels 64, 128 and 192, tone lines of 0 ..
    15 periods with noise) through fax_pixel in the program and through fax_ref.lines_from_pixels: the same records and
    the same state behind the last pixel, which lies inside a line."""
    g = np.random.default_rng(900 + width)
    count = 40 * width + width // 3
    col = np.arange(count) % width
    per = g.integers(0, 16, size=count // width + 1)[np.arange(count) // width]
    tones = np.where((col * per * 2 // width) % 2 == 0, 230, 20) + g.integers(-45, 46, size=count)
    for k, px in enumerate((g.integers(0, 256, size=count), g.choice([63, 64, 127, 128, 191, 192, 0, 255], size=count), np.clip(tones, 0, 255))):
        px = px.astype(np.uint8)
        path = str(tmp_path / f"px{k}.bin")
        px.tofile(path)
        modem = (None, 1 << 30, width, 3, 600.0, 127.5, 7, 9, 10, 14, 2)
        p = subprocess.run([exe] + [str(v) for v in (width, 7, 9, 10, 14, 2)] + [path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "runtime error:" not in p.stderr, p.stderr[-1500:]
        rows = p.stdout.strip().split("\n")
        want, l = R.lines_from_pixels(px, 5 + 3 * np.arange(count), modem)
        got = np.array([tuple(int(v) for v in r.split()) for r in rows[:-1]], dtype=R.LINE)
        assert len(got) == 40 and got.tobytes() == want.tobytes(), (k, got[:3], want[:3])
        state = [int(v) for v in rows[-1].split()[1:]]
        assert state == [l[n] for n in ("col", "crossings", "white", "level", "run", "cls", "active", "lines", "pixels", "images")], (k, state, l)
        if k == 2 and width >= 100:                                   # (16 pixels hold no 10 periods)
            assert (want["flags"] & R.START).any() and (want["flags"] & R.STOP).any() and l["images"] >= 1
