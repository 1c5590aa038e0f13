"""The radiofax decoder's definition on the CPU: the float32 model against the double reference on the GPU tests' own
inputs (TOL_FAX and the condition it rests on), fax_encode -> reference -> fax_image at the compressed and the real mode,
and the capacity bounds against brute force.  Nothing here runs k_fax."""
import numpy as np
import pytest

import fax_ref as R


@pytest.mark.parametrize("nrx", [9, 1024])
def test_model_against_double_and_the_seam(pkg, nrx):
    """case(W, 9) for every window and case(W, 1024) for the big ones, every receiver and sample: the worst |f_model -
    f_ref| per window is at most the figure in MODEL_WORST and more than a third of it (the larger set decides), TOL_FAX is
    7 x the largest.  The same runs show the condition the tolerance rests on: the reference's |f| <= F_MOST = 0.9
    everywhere, so no value sits on the arctangent's seam.  On the nine, FaxRef's float32 arithmetic gives model_disc's
    bits, its pixels lie inside pixel_bounds of the reference's g, and the reference has seen images begin and end."""
    for W in (R.WINDOWS if nrx == 9 else R.BIG_WINDOWS):
        bank, sel, z = R.case(W, nrx)
        pix, lines, disc, g, where, st = R.run_cuts(R.FaxRef(bank, sel, W), z)
        most = float(np.abs(disc).max())
        model = R.model_disc(bank, sel, W, z)
        worst = float(np.abs(model.astype(np.float64) - disc).max())
        print(f"W {W} nrx {nrx}: |f| <= {most:.3f}, model {worst:.3e} (MODEL_WORST {R.MODEL_WORST[W]:.3e})")
        assert most <= R.F_MOST
        assert worst <= R.MODEL_WORST[W]
        if nrx == 1024 or W not in R.BIG_WINDOWS:
            assert worst > R.MODEL_WORST[W] / 3.0
        assert (st["images"] >= 1).sum() >= nrx - nrx // 8 and all(len(l) >= 13 for l in lines)
        if nrx == 9:
            m = R.run_cuts(R.FaxRef(bank, sel, W, np.float32), z)
            assert m[2].tobytes() == model.tobytes()
            for j in range(nrx):
                lo, hi = R.pixel_bounds(g[j], bank[sel[j][0]][4])
                assert ((m[0][j] >= lo) & (m[0][j] <= hi)).all() and np.array_equal(m[4][j], where[j]), j
    assert R.TOL_FAX == 7 * max(R.MODEL_WORST.values())


def test_cuts_and_control_on_the_reference():
    """the reference against itself: every cut list gives one batch's records, pixels and status, disc to the last bit"""
    W = 16
    bank, sel, z = R.case(W, 5)
    one = R.run_cuts(R.FaxRef(bank, sel, W), z)
    for cuts in R.cut_lists(z.shape[1], 256, *R.events(bank, sel[:1], W, z[:1])):
        got = R.run_cuts(R.FaxRef(bank, sel, W), z, cuts)
        for j in range(5):
            assert got[0][j].tobytes() == one[0][j].tobytes() and got[1][j].tobytes() == one[1][j].tobytes(), (cuts, j)
        assert np.abs(got[2] - one[2]).max() < 1e-12
        assert all(np.array_equal(got[5][k], one[5][k]) for k in R.INT_STATUS)


@pytest.mark.parametrize("real", [False, True])
def test_the_picture_comes_back(pkg, real):
    """fax_encode of eight grey bars (48 lines at the compressed mode: width 64, 3 samples per pixel; 40 lines at 120 lines a
    minute, IOC 576, 9765.625 Hz with fax_modem's defaults), 11 black pixels ahead, noise 20 dB below the carrier, 20
    seeds -> the reference -> fax_image.  On every seed one image is found, start and stop, with its phasing lines; its
    column lies within 2 of where the sender's lines begin (fax_ref.e2e_error); all rows or one less.  The worst error of
    a pixel more than box + 2 columns from a bar's edge is at most E2E_WORST, the measured figure (17 and 22 grey levels),
    more than half of it, and below 32, less than one bar step (36); the GPU test asserts twice the figure."""
    worst = 0.0
    for seed in range(20):
        modem, rate, z, img, lead = R.e2e_case(pkg, seed, real=real, rows=40 if real else 48)
        out = R.run_cuts(R.FaxRef([modem], [(0, R.ON)], len(modem[0])), z[None, :])
        assert out[5]["images"][0] == 1 and out[5]["active"][0] == 0, seed
        err, col, rows = R.e2e_error(pkg, out[1][0], out[0][0], modem, img, lead)
        worst = max(worst, err)
    print(f"real {real}: worst error {worst:.1f} grey levels (E2E_WORST {R.E2E_WORST[real]})")
    assert R.E2E_WORST[real] / 2.0 < worst <= R.E2E_WORST[real] < 32.0
    assert R.E2E_BOUND == 2.0 * R.E2E_WORST[False]


def test_fax_modem_and_encode(pkg):
    """fax_modem's figures at the real modes: IOC 576 and 288 at 120 and 60 lines a minute -- width round(pi IOC), inc
    2^32 width lpm / 60 / rate, box the samples per pixel, black and white on 0 and 255, the tone ranges around 300 / 675
    and 450 Hz apart in either order, taps of sum 1; fax_encode's series has modulus 1 and the deviation asked for."""
    rate = 9765.625
    for ioc, lpm, width, start in ((576, 120, 1810, 150), (288, 120, 905, 337.5), (576, 60, 1810, 300), (288, 60, 905, 675)):
        h, inc, w, box, scale, bias, s_lo, s_hi, p_lo, p_hi, need = pkg.fax_modem(rate, 64, lpm=lpm, ioc=ioc)
        assert w == width and abs(inc - 2.0 ** 32 * width * lpm / 60.0 / rate) <= 0.5 and box == min(16, round(rate * 60.0 / lpm / width))
        fd = 2.0 * 400.0 / rate
        assert abs(scale * -fd + bias) < 1e-3 and abs(scale * fd + bias - 255.0) < 1e-3
        stop = 450.0 * 60.0 / lpm
        assert s_lo <= start <= s_hi and p_lo <= stop <= p_hi and (s_hi < p_lo or p_hi < s_lo)
        assert h.dtype == np.float32 and h.shape == (64,) and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
    modem = pkg.fax_modem(rate, 32, lpm=R.E2E_LPM, width=64, start_hz=4 * R.E2E_LPM / 60, stop_hz=7 * R.E2E_LPM / 60, need=2)
    z = pkg.fax_encode(R.grey_bars(3, 64), modem, rate, start_lines=1, phasing_lines=1, stop_lines=1)
    assert z.dtype == np.complex64 and abs(np.abs(z) - 1.0).max() < 1e-6
    f = np.angle(z[1:] * np.conj(z[:-1])) / np.pi
    assert abs(np.abs(f).max() - 2.0 * 400.0 / rate) < 1e-4
    with pytest.raises(pkg.PddcError):
        pkg.fax_modem(3000.0, 64)                                          # 0.83 samples per pixel


def test_capacity_bounds_against_brute_force():
    """max_pixels and max_lines in Python's integers against the clock walked sample by sample from the worst acc, for incs
    of every class and n = 0 .. 300, and against every acc of a coarse grid: the bound is met and never passed."""
    for inc in (1, 3, 65537, (1 << 24) + 1, 1431655765, 1592092837, (1 << 31) - 1, 1 << 31):
        bank = [(None, inc, 16)]
        for n in list(range(0, 300)) + [4096, 32768]:
            bound = R.max_pixels(bank, n)
            most = 0
            for acc in (0, 1, (1 << 31), (1 << 32) - inc, (1 << 32) - 1):
                a, k = acc % (1 << 32), 0
                if n < 300:
                    for _ in range(n):
                        k += (a + inc) >> 32
                        a = (a + inc) & 0xFFFFFFFF
                else:
                    k = (a + n * inc) >> 32
                most = max(most, k)
            assert most == bound, (inc, n, most, bound)
            assert R.max_lines(bank, n) == (-(-bound // 16) if bound else 0)
            for col in (0, 7, 15):                                         # lines ended by `bound` pixels from column col
                assert (col + bound) // 16 <= R.max_lines(bank, n)
            assert bound == 0 or (15 + bound) // 16 == R.max_lines(bank, n)
