"""The carrier stage without a GPU: the reference's own properties (tests/carrier_ref.py), the precondition the GPU
tests' inputs have to meet, the measurement that sets the GPU tolerances, the Python helpers, and the argument checks and
symbols of the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import carrier_ref as CR
from conftest import ROOT

K0, N0 = 1024, 3000
NAMES = ("pddc_carrier_create", "pddc_carrier_destroy", "pddc_carrier_reset", "pddc_carrier_set_rx", "pddc_carrier_process",
         "pddc_carrier_read", "pddc_carrier_tile_outputs", "pddc_carrier_group")


@pytest.fixture(scope="module")
def carriers():
    return CR.am_carriers(K0, N0)


def test_no_slip_precondition(carriers):
    """The GPU tests' input and receivers (tests/test_gpu_carrier.py: am_carriers(1024, 3000), modes and loop bandwidths
    10 / 30 / 60 Hz interleaved): the double reference's |e| stays below E_MAX = 0.75 at every sample of every receiver,
    so no last-bit difference can flip the detector at its wrap.  No receiver is left out."""
    z, _ = carriers
    rx = CR.interleaved_rx(K0)
    assert {r[0] for r in rx} == set(CR.MODES) and len({r[1] for r in rx}) == 3
    ref = CR.CarrierRef(rx, CR.hilbert(3), **CR.PARAMS)
    ref.process(z)
    on = np.array([r[0] != CR.OFF for r in rx])
    worst = np.abs(ref.e).max(axis=1)
    for i, bw in enumerate(CR.BANDWIDTHS):
        rows = on & ((np.arange(K0) // 4) % 3 == i)
        print(f"{bw:g} Hz: largest |e| {worst[rows].max():.3f}, largest final q {ref.q[rows].max():.4f}")
    assert np.all(worst < CR.E_MAX), np.flatnonzero(worst >= CR.E_MAX)
    assert np.all(worst[on] > 0) and not ref.e[~on].any()


def test_float32_model_against_double(carriers):
    """The measurement that sets TOL_CARRIER: the float32 model against the double reference, K = 1024, n = 3000, a 30 Hz
    loop, L = 127, every receiver once in every mode; per mode the worst receiver's max |u - ref| / max |ref|.  OFF is
    exact.  TOL = 7 x the worst case per mode; a re-measurement may not exceed the written worst cases by more than
    0.5 %.  The status behind the batch is within the same tolerance (carrier_ref.py's docstring has the figures)."""
    z, _ = carriers
    kp, ki = CR.loop_gains(30.0)
    rx = [(m, kp, ki) for m in CR.MODES for _ in range(K0)]
    zz = np.concatenate([z] * len(CR.MODES), axis=0)
    h = CR.hilbert(127)
    rd = CR.CarrierRef(rx, h, **CR.PARAMS)
    rf = CR.CarrierRef(rx, h, f32=True, **CR.PARAMS)
    ud, uf = rd.process(zz), rf.process(zz)
    assert uf.dtype == np.complex64 and ud.dtype == np.complex128
    assert np.abs(rd.e).max() < CR.E_MAX
    e = CR.err_rows(uf, ud)
    for i, m in enumerate(CR.MODES):
        s = slice(i * K0, (i + 1) * K0)
        worst, tol = float(e[s].max()), CR.TOL_CARRIER[m]
        dth = np.abs(CR.theta_diff(rf.theta[s], rd.theta[s])).max()
        dv = np.abs(rf.v[s].astype(np.float64) - rd.v[s]).max()
        dq = np.abs(rf.q[s].astype(np.float64) - rd.q[s]).max()
        print(f"{CR.MODE_NAMES[m]}: worst {worst:.3e} (written {CR.MODEL_WORST_CARRIER[m]:.3e}, TOL {tol:.3e}); theta {dth} units, "
              f"v {dv:.3e} of {np.abs(rd.v[s]).max():.3e}, q {dq:.3e} of {rd.q[s].max():.3e}")
        assert worst <= 1.005 * CR.MODEL_WORST_CARRIER[m]
        assert tol == 7 * CR.MODEL_WORST_CARRIER[m]
        # the status as a phase (carrier_ref.py): the model's own error leaves the device six sevenths of the tolerance
        assert dth <= tol / (2.0 * np.pi) * 2.0 ** 32 / 7 and dv <= tol / np.pi / 7 and dq <= tol / np.pi / 7
    off = slice(0, K0)
    assert np.array_equal(CR.bits(uf[off]), CR.bits(zz[off])) and np.array_equal(ud[off], zz[off].astype(np.complex128))
    assert not rd.theta[off].any() and not rd.q[off].any()


def test_float32_model_on_the_gpu_receivers(carriers):
    """The float32 model on the receivers of tests/test_gpu_carrier.py (modes and 10 / 30 / 60 Hz loops interleaved, L = 3):
    it is inside TOL_CARRIER at every bandwidth -- the narrow loops come closest, carrier_ref.py says why and has the
    figures -- and its status is inside the phase equivalents."""
    z, _ = carriers
    rx = CR.interleaved_rx(K0)
    rd = CR.CarrierRef(rx, CR.hilbert(3), **CR.PARAMS)
    rf = CR.CarrierRef(rx, CR.hilbert(3), f32=True, **CR.PARAMS)
    e = CR.err_rows(rf.process(z), rd.process(z))
    mode, band = np.array([r[0] for r in rx]), (np.arange(K0) // 4) % 3
    for m in (CR.DSB, CR.USB, CR.LSB):
        tol = CR.TOL_CARRIER[m]
        for i, bw in enumerate(CR.BANDWIDTHS):
            s = (mode == m) & (band == i)
            dth = np.abs(CR.theta_diff(rf.theta[s], rd.theta[s])).max()
            dv, dq = np.abs(rf.v[s] - rd.v[s]).max(), np.abs(rf.q[s] - rd.q[s]).max()
            print(f"{CR.MODE_NAMES[m]} {bw:g} Hz: err {e[s].max():.3e} ({e[s].max() / tol:.2f} of TOL), theta {dth} units, v {dv:.2e}, q {dq:.2e}")
            assert e[s].max() <= tol
            assert dth <= tol / (2.0 * np.pi) * 2.0 ** 32 / 2 and dv <= tol / np.pi / 7 and dq <= tol / np.pi / 7


def test_lock_and_frequency(carriers):
    """What the loop is for, on the double reference: after 1500 outputs at 30 Hz every one of the 1024 receivers is
    locked and freq rate / 2 is within 1 Hz of the carrier's offset (the worst measured here is 0.22 Hz, the loop's own
    noise and the rest of its transient; another draw gave 0.62 Hz)."""
    z, off = carriers
    kp, ki = CR.loop_gains(30.0)
    ref = CR.CarrierRef([(CR.DSB, kp, ki)] * K0, CR.hilbert(3), **CR.PARAMS)
    ref.process(z[:, :1500])
    st = ref.read()
    worst = np.abs(st["freq"].astype(np.float64) * CR.RATE / 2.0 - off).max()
    print(f"after 1500 outputs: largest q {st['err'].max():.4f}, worst frequency error {worst:.3f} Hz")
    assert st["locked"].all() and st["err"].max() < CR.PARAMS["lock_thr"] / 2
    assert worst < 1.0
    # an empty channel (noise alone) does not lock
    rng = np.random.default_rng(3)
    noise = (0.003 * (rng.standard_normal((4, 1500)) + 1j * rng.standard_normal((4, 1500)))).astype(np.complex64)
    idle = CR.CarrierRef([(CR.DSB, kp, ki)] * 4, CR.hilbert(3), **CR.PARAMS)
    idle.process(noise)
    assert not idle.read()["locked"].any()


def test_sideband_selection():
    """A carrier with a tone only in the upper sideband comes out of USB with the tone and out of LSB with it suppressed
    by more than 80 dB after the filter's transient; the lower-sideband tone gives the mirror image (L = 127).  The loop
    is all but at rest here (kp 1e-6, ki 0, the carrier at phase 0): for the detector a single-sideband tone is phase
    modulation, a running loop follows it by about kp e per output and that wobble, not the filter, then bounds the
    suppression (33 dB at 30 Hz) -- an AM signal, whose sidebands are symmetric, gives the detector nothing to follow."""
    n, f = 4000, 1000.0 / CR.RATE
    m = np.arange(n)
    for sgn in (1, -1):
        z = (0.3 + 0.1 * np.exp(sgn * 2j * np.pi * f * m)).astype(np.complex64)
        ref = CR.CarrierRef([(CR.USB, 1e-6, 0.0), (CR.LSB, 1e-6, 0.0)], CR.hilbert(127), **CR.PARAMS)
        u = ref.process(np.stack([z, z]))
        usb, lsb = (float(np.std(u[i].real[500:])) for i in (0, 1))
        kept, gone = (usb, lsb) if sgn > 0 else (lsb, usb)
        print(f"tone {'above' if sgn > 0 else 'below'}: kept {kept:.4f} rms, suppressed {gone:.3e} rms, {20 * np.log10(kept / gone):.1f} dB")
        assert abs(kept - 0.2 / np.sqrt(2.0)) < 1e-3 and gone < 1e-4 * kept


def test_sideband_selection_with_a_running_loop():
    """The same tones through a 30 Hz loop, which is what a listener gets: the other sideband is still more than 30 dB
    down.  The bound is the loop's wobble worked out, not measured: the detector sees the tone as a phase of amplitude
    (0.1 / 0.3) / pi half-turns, the proportional path integrates kp times that over the tone, kp e / (2 pi f)
    half-turns at f = 1000 / 9765.625 cycles per output, that is 0.0045 half-turns or 0.014 rad; a carrier of 0.3 wobbling
    by 0.014 rad puts 0.3 x 0.014 = 0.0042 of amplitude, 0.0030 rms, into the rejected output, 33.5 dB below the 0.1414 rms
    that is kept.  3.5 dB are left for the small-angle steps of that sum."""
    n, f = 4000, 1000.0 / CR.RATE
    m = np.arange(n)
    kp, ki = CR.loop_gains(30.0)
    for sgn in (1, -1):
        z = ((0.3 + 0.1 * np.exp(sgn * 2j * np.pi * f * m)) * np.exp(0.2j)).astype(np.complex64)
        ref = CR.CarrierRef([(CR.USB, kp, ki), (CR.LSB, kp, ki)], CR.hilbert(127), **CR.PARAMS)
        u = ref.process(np.stack([z, z]))
        assert np.abs(ref.e).max() < CR.E_MAX
        usb, lsb = (float(np.std(u[i].real[2500:])) for i in (0, 1))
        kept, gone = (usb, lsb) if sgn > 0 else (lsb, usb)
        print(f"30 Hz loop, tone {'above' if sgn > 0 else 'below'}: kept {kept:.4f} rms, suppressed {gone:.3e} rms, {20 * np.log10(kept / gone):.1f} dB")
        assert abs(kept - 0.2 / np.sqrt(2.0)) < 2e-3 and 20 * np.log10(kept / gone) > 30.0


def test_reference_streaming_equals_one_shot(carriers):
    """the reference cut into batches (0, 1, 2, L - 1, L included) equals the reference in one batch, u and status"""
    z = carriers[0][:24, :900]
    rx = CR.interleaved_rx(24)
    for L in (3, 31):
        h = CR.hilbert(L)
        for f32 in (False, True):
            one = CR.CarrierRef(rx, h, f32=f32, **CR.PARAMS)
            want = one.process(z)
            cuts = [0, 1, 2, L - 1, L, 0, 255, 257]
            cuts.append(900 - sum(cuts))
            r = CR.CarrierRef(rx, h, f32=f32, **CR.PARAMS)
            got = CR.run_cuts(r, z, cuts)
            assert got.dtype == want.dtype and np.array_equal(got, want), (L, f32)
            a, b = r.read(), one.read()
            for name in CR.STATUS.names:
                assert np.array_equal(a[name], b[name]), name


def test_reference_set_rx(carriers):
    """kp / ki alone keep theta, v, q and the history: the loop goes on without a gap.  Another mode clears them: from
    there on the receiver is one that was created then.  Bad calls raise and change nothing."""
    z = carriers[0][:8, :1200]
    rx = CR.interleaved_rx(8)
    h = CR.hilbert(31)
    cut = 700
    r = CR.CarrierRef(rx, h, **CR.PARAMS)
    first = r.process(z[:, :cut])
    kept = (r.theta.copy(), r.v.copy(), r.q.copy(), r.hist.copy())
    for bad in ((8, CR.DSB, 0.1, 0.01), (-1, CR.DSB, 0.1, 0.01), (1, 4, 0.1, 0.01), (1, CR.DSB, 0.0, 0.01), (1, CR.DSB, 0.6, 0.01),
                (1, CR.DSB, 0.1, -0.01), (1, CR.DSB, 0.1, 0.3), (1, CR.DSB, np.nan, 0.01)):
        with pytest.raises(ValueError):
            r.set_rx(*bad)
    kp60, ki60 = CR.loop_gains(60.0)
    r.set_rx(2, rx[2][0], kp60, ki60)                  # the gains alone (USB)
    r.set_rx(5, CR.LSB, rx[5][1], rx[5][2])            # DSB -> LSB
    assert r.theta[2] == kept[0][2] != 0 and r.v[2] == kept[1][2] and r.q[2] == kept[2][2] and np.array_equal(r.hist[2], kept[3][2])
    assert r.theta[5] == 0 and r.v[5] == 0 and r.q[5] == 0 and not r.hist[5].any()
    second = r.process(z[:, cut:])
    plain = CR.CarrierRef(rx, h, **CR.PARAMS).process(z)
    for j in (0, 1, 3, 4, 6, 7):
        assert np.array_equal(np.concatenate([first[j], second[j]]), plain[j])
    assert np.array_equal(first[2], plain[2, :cut]) and not np.array_equal(second[2], plain[2, cut:])
    # no gap: the first output behind the change is rotated by the theta and filtered over the history the old gains left
    assert second[2, 0] == plain[2, cut] and second[2, 1] != plain[2, cut + 1]
    alone = CR.CarrierRef([(CR.LSB, rx[5][1], rx[5][2])], h, **CR.PARAMS).process(z[5:6, cut:])
    assert np.array_equal(second[5], alone[0])


def test_helpers(pkg):
    for bw, rate, zeta in ((30.0, 9765.625, 0.7071), (10.0, 39062.5, 1.0), (60.0, 9765.625, 0.5)):
        wn = 2.0 * np.pi * bw / rate
        kp, ki = pkg.carrier_loop(bw, rate, zeta)
        assert kp == pytest.approx(2.0 * zeta * wn, rel=1e-12) and ki == pytest.approx(wn * wn, rel=1e-12)
        assert pkg.carrier_loop(bw, rate) == pytest.approx(CR.loop_gains(bw, rate), rel=1e-12)
    for L in (3, 31, 127, 255):
        h = pkg.carrier_hilbert(L)
        D = (L - 1) // 2
        assert h.dtype == np.float32 and h.shape == (L,)
        assert np.array_equal(h, -h[::-1]) and not h[D % 2::2].any() and h[D] == 0       # antisymmetric, even offsets zero
        k = np.arange(L) - D
        ideal = np.where(k % 2 != 0, 2.0 / (np.pi * np.where(k == 0, 1, k)), 0.0) * np.kaiser(L, 8.0)
        assert np.array_equal(h, ideal.astype(np.float32)) and np.array_equal(h, CR.hilbert(L))
        assert h[D + 1] > 0 and h[D - 1] < 0
    assert not np.array_equal(pkg.carrier_hilbert(31, beta=4.0), pkg.carrier_hilbert(31))
    for bad in (2, 4, 1, 0, -3):
        with pytest.raises(ValueError):
            pkg.carrier_hilbert(bad)
    assert pkg.carrier_status_dtype() == CR.STATUS and CR.STATUS.itemsize == 16
    assert (pkg.PDDC_CARRIER_OFF, pkg.PDDC_CARRIER_DSB, pkg.PDDC_CARRIER_USB, pkg.PDDC_CARRIER_LSB) == CR.MODES
    TT, G = pkg.carrier_tile_outputs(), pkg.carrier_group()
    assert TT >= 1 and 1 <= G <= 64


def test_symbols_declared_and_exported(pkg):
    L = pkg.ddc_lib()
    src = open(os.path.join(ROOT, "include", "perseus_ddc.h")).read()
    for name in NAMES:
        assert f"{name}(" in src and hasattr(L, name), name
    for word in ("PDDC_CARRIER_OFF", "PDDC_CARRIER_DSB", "PDDC_CARRIER_USB", "PDDC_CARRIER_LSB", "pddc_carrier_params",
                 "pddc_carrier_rx", "pddc_carrier_status", "cannot overflow"):
        assert word in src, word


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    kp, ki = pkg.carrier_loop(30.0, CR.RATE)

    def create(rx=((1, kp, ki), (2, 0.5, 0.25), (0, 1e-6, 0.0), (3, kp, ki)), nrx=None, params=(0.25, 1.0 / 64, 0.05), taps=None,
               ntaps=None, null_rx=False, null_params=False, null_taps=False):
        arr = (pkg.CarrierRx * max(len(rx), 1))(*[pkg.CarrierRx(*r) for r in rx])
        par = pkg.CarrierParams(*params)
        h = np.ascontiguousarray(pkg.carrier_hilbert(31) if taps is None else taps, dtype=np.float32)
        c = C.c_void_p()
        rc = L.pddc_carrier_create(C.byref(c), 0, len(rx) if nrx is None else nrx, None if null_params else C.byref(par),
                                   None if null_rx else arr, None if null_taps else h.ctypes.data_as(C.POINTER(C.c_float)),
                                   h.size if ntaps is None else ntaps)
        if rc == 0:
            L.pddc_carrier_destroy(c)
        return rc

    nan, inf = float("nan"), float("inf")
    spoilt = pkg.carrier_hilbert(31).copy()
    spoilt[7] = nan
    blown = pkg.carrier_hilbert(31).copy()
    blown[30] = inf
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(1, kp, ki)] * 1025), dict(null_rx=True), dict(null_params=True), dict(null_taps=True),
           dict(taps=np.zeros(30, np.float32)), dict(taps=np.zeros(256, np.float32)), dict(taps=np.zeros(257, np.float32)),
           dict(taps=np.zeros(1, np.float32)), dict(ntaps=0), dict(ntaps=-31), dict(ntaps=2), dict(taps=spoilt), dict(taps=blown),
           dict(params=(0.0, 0.1, 0.05)), dict(params=(0.5, 0.1, 0.05)), dict(params=(-0.1, 0.1, 0.05)), dict(params=(nan, 0.1, 0.05)),
           dict(params=(0.25, 0.0, 0.05)), dict(params=(0.25, 1.5, 0.05)), dict(params=(0.25, nan, 0.05)),
           dict(params=(0.25, 0.1, 0.0)), dict(params=(0.25, 0.1, -1.0)), dict(params=(0.25, 0.1, inf)), dict(params=(0.25, 0.1, nan)),
           dict(rx=[(4, kp, ki)]), dict(rx=[(-1, kp, ki)]), dict(rx=[(1, kp, ki), (1, 0.0, ki)]), dict(rx=[(1, 0.6, ki)]),
           dict(rx=[(1, -0.1, ki)]), dict(rx=[(1, nan, ki)]), dict(rx=[(1, inf, ki)]), dict(rx=[(0, 0.0, 0.0)]),
           dict(rx=[(1, kp, -0.01)]), dict(rx=[(1, kp, 0.26)]), dict(rx=[(1, kp, nan)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.CarrierRx * 1)(pkg.CarrierRx(1, kp, ki))
    par = pkg.CarrierParams(0.25, 1.0 / 64, 0.05)
    h = pkg.carrier_hilbert(3)
    assert L.pddc_carrier_create(None, 0, 1, C.byref(par), arr, h.ctypes.data_as(C.POINTER(C.c_float)), 3) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(rx=[(3, 0.5, 0.25)] * 1024, taps=pkg.carrier_hilbert(255), params=(0.49999, 1.0, 3.0e38)) == pkg.PDDC_ENODEV
        assert create(rx=[(0, 1e-30, 0.0)], taps=pkg.carrier_hilbert(3)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Carrier([(pkg.PDDC_CARRIER_USB, kp, ki)], pkg.carrier_hilbert(127))
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(rx=[(7, kp, ki)], hilbert=pkg.carrier_hilbert(31)), dict(rx=[(1, kp, ki)], hilbert=np.zeros(32, np.float32)),
               dict(rx=[(1, 0.75, ki)], hilbert=pkg.carrier_hilbert(31)), dict(rx=[(1, kp, ki)], hilbert=pkg.carrier_hilbert(31), vmax=0.5),
               dict(rx=[], hilbert=pkg.carrier_hilbert(31)), dict(rx=[(1, kp, ki)] * 1025, hilbert=pkg.carrier_hilbert(31))):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Carrier(**kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    assert L.pddc_carrier_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_carrier_set_rx(None, 0, 1, kp, ki) == pkg.PDDC_EINVAL
    assert L.pddc_carrier_read(None, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_carrier_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_carrier_destroy(None) == 0
