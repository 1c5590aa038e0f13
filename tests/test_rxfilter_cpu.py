"""The receiver filter without a GPU: its reference (tests/rxfilter_ref.py) against the cut, on an impulse, across a filter
change and on tones through rxfilter_bank's filters; the float32 model that sets the GPU tolerance; the argument checks."""
import ctypes as C

import numpy as np
import pytest

import rxfilter_ref as RR


def test_reference_is_cut_invariant():
    """The double reference and the float32 model give bit-equal values when the series is cut at 0, 1, 2, 30, 0, 31, 255,
    256, 125 (T = 64: batches of 0, 1 and fewer than T - 1 inputs, the record spanning three batches)."""
    assert sum(RR.CUTS) == 700
    z = RR.parity_inputs(9)[:5]
    bank = RR.parity_bank(4, 64)
    sel = RR.select(5, 4)
    for fn in (RR.rxfilter_ref, RR.rxfilter_model32):
        one = fn(z, bank, sel)
        assert one.shape == (5, 700) and np.all(np.isfinite(one.view(np.float64)))
        assert np.array_equal(one.view(np.float64), fn(z, bank, sel, RR.CUTS).view(np.float64))


def test_an_impulse_gives_the_receivers_own_filter():
    bank = RR.parity_bank(3, 17)
    sel = [2, 0, 1, 2]
    z = np.zeros((4, 40), np.complex64)
    z[:, 5] = 1.0 - 2.0j
    out = RR.rxfilter_ref(z, bank, sel)
    for j, f in enumerate(sel):
        want = np.zeros(40, np.complex128)
        want[5:5 + 17] = bank[f].astype(np.float64) * (1.0 - 2.0j)
        assert np.array_equal(out[j], want), j
    assert np.array_equal(RR.rxfilter_model32(z, bank, sel).view(np.float64), out.view(np.float64))


def test_a_filter_change_keeps_the_inputs():
    """set_rx at m0: outputs before m0 are the old filter's, outputs from m0 on the new filter's over the same inputs, those
    before m0 included -- each equal to a run with that filter alone."""
    z = RR.parity_inputs(9)[:3]
    bank = RR.parity_bank(4, 64)
    m0 = 333

    def change(i, r):
        if i == 1:
            r.set_rx(1, 3)

    for f32 in (False, True):
        got = RR.run_cuts(RR.RxFilterRef(bank, [0, 1, 2], f32=f32), z, [m0, 700 - m0], before=change)
        old = RR.run_cuts(RR.RxFilterRef(bank, [0, 1, 2], f32=f32), z)
        new = RR.run_cuts(RR.RxFilterRef(bank, [0, 3, 2], f32=f32), z)
        assert np.array_equal(got[:, :m0], old[:, :m0])
        assert np.array_equal(got[:, m0:], new[:, m0:])
        assert not np.array_equal(old[1], new[1]) and np.array_equal(old[[0, 2]], new[[0, 2]])


def test_rxfilter_bank_passes_and_stops_a_tone(pkg):
    """A 0.2 cycles/sample tone through T = 129 filters with fc = 0.3 and fc = 0.1 of rxfilter_bank: the wide one passes it
    within 1e-4 dB, out of the narrow one it comes more than 100 dB down (the reference gives +4e-6 dB and -111.8 dB).
    The helper is the restated formula bit for bit, its rows sum to 1, and a half width outside (0, rate / 2) is refused."""
    bank = pkg.rxfilter_bank(48000.0, [0.3 * 48000.0, 0.1 * 48000.0], 129)
    assert bank.dtype == np.float32 and bank.shape == (2, 129)
    assert np.array_equal(bank, RR.kaiser_bank(1.0, [0.3, 0.1], 129))
    assert np.max(np.abs(bank.astype(np.float64).sum(axis=1) - 1.0)) < 1e-6
    assert np.array_equal(bank, bank[:, ::-1])                         # symmetric: the common delay (T - 1) / 2
    i = np.arange(2000)
    z = np.tile(np.exp(2j * np.pi * 0.2 * i).astype(np.complex64), (2, 1))
    out = RR.rxfilter_ref(z, bank, [0, 1])[:, 128:]
    level = 20 * np.log10(np.sqrt(np.mean(np.abs(out) ** 2, axis=1)))
    print(f"0.2 cycles/sample: fc 0.3 {level[0]:+.2e} dB, fc 0.1 {level[1]:.1f} dB")
    assert abs(level[0]) <= 1e-4 and level[1] < -100.0
    for bad in ([0.0], [-1.0], [24000.0], [1000.0, 30000.0], []):
        with pytest.raises(pkg.PddcError):
            pkg.rxfilter_bank(48000.0, bad, 129)
    with pytest.raises(pkg.PddcError):
        pkg.rxfilter_bank(48000.0, [1000.0], 0)


def test_float32_model_against_double():
    """The measurement that sets TOL_RXFILTER: the float32 model against the double reference on the GPU parity test's very
    inputs (|re|, |im| <= 1), every (B, T) of SHAPES, receiver j on filter (7 j + 3) mod B.  TOL = 7 x the worst case; the
    recorded constants are what this measures (to the digits written)."""
    worst = {}
    for nrx in (9, 1024):
        z = RR.parity_inputs(nrx)
        assert z.shape == (nrx, 300 if nrx == 1024 else 700)
        assert max(float(np.max(np.abs(z.real))), float(np.max(np.abs(z.imag)))) <= 1.0
        for B, T in RR.SHAPES:
            bank, sel = RR.parity_bank(B, T), RR.select(nrx, B)
            e = float(np.max(np.abs(RR.rxfilter_model32(z, bank, sel) - RR.rxfilter_ref(z, bank, sel))))
            worst[(B, T)] = max(worst.get((B, T), 0.0), e)
    for k, v in worst.items():
        print(f"(B, T) = {k}: worst |model32 - ref| {v:.3e} (written {RR.MODEL_WORST[k]:.3e})")
        assert abs(v - RR.MODEL_WORST[k]) <= 0.0005 * RR.MODEL_WORST[k] + 1e-12, k
    assert RR.MODEL_WORST_RXFILTER == max(RR.MODEL_WORST.values())
    assert RR.TOL_RXFILTER == 7 * RR.MODEL_WORST_RXFILTER


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    good = dict(nrx=4, B=3, T=64)

    def create(bank="ok", sel="ok", null_out=False, **kw):
        a = dict(good, **kw)
        n = a["B"] * a["T"] if a["B"] > 0 and a["T"] > 0 else 1
        g = np.full(min(n, 1 << 20), 0.01, np.float32)
        if callable(bank):
            bank(g)
        s = np.array([j % max(a["B"], 1) for j in range(max(a["nrx"], 1))], np.int32)
        if callable(sel):
            sel(s)
        h = C.c_void_p()
        rc = L.pddc_rxfilter_create(None if null_out else C.byref(h), 0, a["nrx"],
                                    None if bank is None else g.ctypes.data_as(C.POINTER(C.c_float)), a["B"], a["T"],
                                    None if sel is None else s.ctypes.data_as(C.POINTER(C.c_int)))
        if rc == 0:
            L.pddc_rxfilter_destroy(h)
        return rc

    def poke(i, v):
        def f(g):
            g[i] = v
        return f

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(nrx=1025), dict(B=0), dict(B=-3), dict(B=65), dict(T=0), dict(T=-1), dict(T=257),
           dict(bank=None), dict(sel=None), dict(bank=poke(0, nan)), dict(bank=poke(191, inf)), dict(bank=poke(17, -inf)),
           dict(sel=poke(0, -1)), dict(sel=poke(3, 3)), dict(sel=poke(2, 1 << 20)), dict(null_out=True)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(nrx=1024, B=64, T=256) == pkg.PDDC_ENODEV
        assert create(nrx=1, B=1, T=1) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.RxFilter(RR.parity_bank(3, 64), [0, 1, 2, 0])
        assert e.value.code == pkg.PDDC_ENODEV
    with pytest.raises(pkg.PddcError) as e:
        pkg.RxFilter(RR.parity_bank(3, 64), [0, 1, 3])
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError):
        pkg.RxFilter(np.zeros(64, np.float32), [0])
    assert L.pddc_rxfilter_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_rxfilter_set_rx(None, 0, 0) == pkg.PDDC_EINVAL
    assert L.pddc_rxfilter_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_rxfilter_destroy(None) == 0


def test_tile_outputs(pkg):
    assert pkg.rxfilter_tile_outputs() > 0
