"""The equaliser without a GPU: the reference (tests/eq_ref.py) against scipy's sosfilt, its own properties, the section
designs through eq_response, the argument checks of the C ABI, and the preconditions the GPU tests' inputs have to meet."""
import ctypes as C

import numpy as np
import pytest

import eq_ref as ER

F32, F64 = np.float32, np.float64
SQ = 1.0 / np.sqrt(2.0)
HALF_POWER_DB = -10.0 * np.log10(2.0)             # -3.0103


def same(a, b):
    return np.array_equal(ER.bits(a), ER.bits(b))


def db(h):
    return 20.0 * np.log10(np.abs(h))


def test_the_reference_is_sosfilt():
    """White noise of sigma 0.1, 6000 samples, through the eight design sets (the 20 Hz notch, the hum notches, the CW peak
    filter twice and a voice chain, at 9765.625 Hz and 48 kHz): the reference's outputs before the rounding against
    scipy.signal.sosfilt with a0 = 1 -- at most 1e-12 of the output's peak apart (measured: the same bits on all eight),
    and the float32 output is that double rounded once."""
    sosfilt = pytest.importorskip("scipy.signal").sosfilt
    rng = np.random.default_rng(1)
    for name, (rate, cascade) in ER.design_sets().items():
        x = (0.1 * rng.standard_normal(6000)).astype(F32)[None, :]
        r = ER.EqRef([cascade], 8, keep_double=True)
        out = r.process(x)
        sos = np.array([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in cascade])
        y = sosfilt(sos, x[0].astype(F64))
        e = float(np.abs(y - r.double[0]).max() / np.abs(y).max())
        print(f"{name}: {e:.1e} of the peak from sosfilt, bits equal: {same(y, r.double[0])}")
        assert e <= 1e-12
        assert same(out[0], r.double[0].astype(F32))


@pytest.mark.parametrize("S", ER.SECTIONS)
def test_reference_streaming_equals_one_batch(S):
    K, n = 2 * (S + 1) + 3, 700
    x, rx = ER.gpu_series()[:K, :n], ER.interleaved_rx(K, S)
    out, st, _ = ER.eq_ref(x, rx, S)
    cuts = [0, 1, 2, 0, max(S - 1, 0), S, 97, 1, 0]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    out2, st2, _ = ER.eq_ref(x, rx, S, cuts=cuts)
    assert same(out, out2) and same(st, st2)
    # ... and the bits do not depend on the object's S
    out8, st8, _ = ER.eq_ref(x, rx, 8)
    assert same(out, out8) and same(st, st8[:, :S]) and not ER.bits(st8[:, S:]).any()


def test_reference_zeros_stay_plus_zero():
    x = np.zeros((len(ER.pool()), 300), F32)
    p = ER.pool()
    out, st, _ = ER.eq_ref(x, [[p[j], p[(j + 1) % len(p)]] for j in range(len(p))], 2)
    # (the outputs' bits; a state can be -0, as b2 v - a2 y is with a negative b2 or a positive a2 and an earlier -0)
    assert not ER.bits(out).any() and not st.any()


def test_reference_off_passes_the_words_and_set_rx_keeps_the_states():
    K, n = 3, 600
    x = ER.gpu_series()[40:40 + K, :n].copy()
    x[1, 100] = -0.0
    x[1, 101:103].view(np.uint32)[:] = (0x7FC12345, 0x00000001)                 # a NaN with a payload, a denormal
    p = ER.pool()
    r = ER.EqRef([[p[0], p[1], p[2]], [], [p[3]]], 4)
    a = r.process(x[:, :200])
    assert same(a[1], x[1, :200]) and not ER.bits(r.state[1]).any()
    held = r.state.copy()
    r.set_rx(0, [p[0]])                           # 3 -> 1: section 0 keeps its state
    r.process(x[:, 200:200])
    assert same(r.state, held)                    # a batch of 0 moves nothing
    b = r.process(x[:, 200:400])
    alone = ER.EqRef([[p[0]]], 1)
    alone.state[0, 0] = held[0, 0]
    assert same(b[0], alone.process(x[:1, 200:400])[0]) and not ER.bits(r.state[0, 1:]).any()
    r.set_rx(0, [p[0], p[1], p[2]])               # 1 -> 3: the regrown sections start from rest
    r.set_rx(2, [p[3]], ER.RESTART)
    c = r.process(x[:, 400:])
    grown = ER.EqRef([[p[0], p[1], p[2]]], 4)
    grown.state[0, 0] = alone.state[0, 0]
    assert same(c[0], grown.process(x[:1, 400:])[0])
    fresh = ER.EqRef([[p[3]]], 1)
    assert same(c[2], fresh.process(x[2:3, 400:])[0])
    for bad in ((K, [p[0]], 0), (-1, [p[0]], 0), (0, [p[0]] * 5, 0), (0, [p[0]], 2), (0, [(1.0, 0.0, 0.0, 2.0, 0.5)], 0),
                (0, [(1.0, 0.0, 0.0, 0.0, 1.0)], 0), (0, [(np.nan, 0.0, 0.0, 0.0, 0.0)], 0)):
        with pytest.raises(ValueError):
            r.set_rx(*bad)


def test_design_responses(pkg):
    """The library's designs (pddc_eq_design) through eq_response; the cookbook's responses are analytic, so the figures
    hold to 1e-9 in amplitude: a notch's |H(f0)| = 0, a peak's |H(f0)| = 10^(gain_db / 20), low- and high-pass at
    Q = 1/sqrt(2) -3.0103 dB at f0 and unity at DC / Nyquist, the one-pole sections -3.0103 dB at their corner, a shelf
    gain_db at its far end and 0 dB at its near end, a band-pass 0 dB at f0.  And the library's sections are the
    reference's own (two independent writings of the formulas) to 1e-13."""
    tol = 1e-9
    for rate in ER.RATES:
        ny = rate / 2.0

        def H(kind, f, q=SQ, g=0.0, at=()):
            s = pkg.eq_section(kind, rate, f, q, g)
            want = ER.design(kind, rate, f, q, g)
            assert np.allclose(tuple(s), want, rtol=1e-13, atol=1e-15), (kind, f, tuple(s), want)
            return np.abs(pkg.eq_response([s], rate, np.array(at, F64)))

        for f0, q in ((1000.0, 10.0), (50.0, 5.0), (0.3 * rate, 2.0)):
            assert H(pkg.PDDC_EQ_NOTCH, f0, q, at=[f0])[0] <= tol
            assert np.all(np.abs(H(pkg.PDDC_EQ_NOTCH, f0, q, at=[0.0, ny]) - 1.0) <= tol)
            assert abs(H(pkg.PDDC_EQ_BANDPASS, f0, q, at=[f0])[0] - 1.0) <= tol
            for g in (18.0, -12.0, 3.0):
                assert abs(H(pkg.PDDC_EQ_PEAK, f0, q, g, at=[f0])[0] - 10.0 ** (g / 20.0)) <= tol * 10.0 ** (max(g, 0.0) / 20.0)
                assert np.all(np.abs(H(pkg.PDDC_EQ_PEAK, f0, q, g, at=[0.0, ny]) - 1.0) <= tol)
        for f0 in (300.0, 2700.0, 0.2 * rate):
            lp, hp = H(pkg.PDDC_EQ_LOWPASS, f0, at=[0.0, f0, ny]), H(pkg.PDDC_EQ_HIGHPASS, f0, at=[0.0, f0, ny])
            assert abs(lp[0] - 1.0) <= tol and abs(lp[1] - SQ) <= tol and lp[2] <= tol
            assert hp[0] <= tol and abs(hp[1] - SQ) <= tol and abs(hp[2] - 1.0) <= tol
            assert abs(db(lp[1]) - HALF_POWER_DB) <= 1e-8
            l1, h1 = H(pkg.PDDC_EQ_LOWPASS1, f0, at=[0.0, f0, ny]), H(pkg.PDDC_EQ_HIGHPASS1, f0, at=[0.0, f0, ny])
            assert abs(l1[0] - 1.0) <= tol and abs(l1[1] - SQ) <= tol and l1[2] <= tol
            assert h1[0] <= tol and abs(h1[1] - SQ) <= tol and abs(h1[2] - 1.0) <= tol
            for g in (6.0, -6.0, 12.0):
                a = 10.0 ** (g / 20.0)
                ls, hs = H(pkg.PDDC_EQ_LOWSHELF, f0, SQ, g, at=[0.0, ny]), H(pkg.PDDC_EQ_HIGHSHELF, f0, SQ, g, at=[0.0, ny])
                assert abs(ls[0] - a) <= tol * max(a, 1.0) and abs(ls[1] - 1.0) <= tol
                assert abs(hs[1] - a) <= tol * max(a, 1.0) and abs(hs[0] - 1.0) <= tol
        tau = 75e-6 if rate > 20000 else 750e-6
        de = pkg.eq_deemphasis(rate, tau)
        fc = 1.0 / (2.0 * np.pi * tau)
        assert de.b2 == 0.0 and de.a2 == 0.0 and abs(np.abs(pkg.eq_response([de], rate, [fc]))[0] - SQ) <= tol
    # a cascade's response is the product, and ER.response is eq_response
    rate, cas = ER.design_sets()["voice@48000"]
    f = np.linspace(0.0, 24000.0, 101)
    assert np.allclose(pkg.eq_response(cas, rate, f), ER.response(cas, rate, f), rtol=1e-12, atol=1e-13)
    assert np.allclose(pkg.eq_response(cas, rate, f), np.prod([pkg.eq_response([c], rate, f) for c in cas], axis=0), rtol=1e-12, atol=1e-13)


def test_designed_sections_are_stable(pkg):
    """every kind over a grid of corner, Q and gain: the library gives a section, and it passes the stability test"""
    made = 0
    for rate in ER.RATES:
        for kind in ER.KINDS:
            for f in (5.0, 20.0, 50.0, 300.0, 700.0, 2700.0, 0.45 * rate, 0.499 * rate):
                for q in (0.1, 0.5, SQ, 2.0, 30.0, 100.0):
                    for g in (-40.0, -6.0, 0.0, 6.0, 18.0, 40.0):
                        assert ER.section_ok(tuple(pkg.eq_section(kind, rate, f, q, g))), (rate, kind, f, q, g)
                        made += 1
    assert made == 2 * 9 * 8 * 6 * 6
    nan, inf = float("nan"), float("inf")
    for bad in ((9, 48000.0, 1000.0, 1.0, 0.0), (-1, 48000.0, 1000.0, 1.0, 0.0), (0, 48000.0, 0.0, 1.0, 0.0), (0, 48000.0, 24000.0, 1.0, 0.0),
                (0, 48000.0, -5.0, 1.0, 0.0), (0, 48000.0, 1000.0, 0.0, 0.0), (0, 48000.0, 1000.0, -1.0, 0.0), (0, nan, 1000.0, 1.0, 0.0),
                (0, 48000.0, nan, 1.0, 0.0), (0, 48000.0, 1000.0, nan, 0.0), (4, 48000.0, 1000.0, 1.0, nan), (4, 48000.0, 1000.0, 1.0, inf),
                (0, inf, 1000.0, 1.0, 0.0), (0, 48000.0, 1000.0, inf, 0.0)):
        with pytest.raises(pkg.PddcError) as e:
            pkg.eq_section(*bad)
        assert e.value.code == pkg.PDDC_EINVAL, bad
    for tau in (0.0, -1.0, nan, 1e-9):            # (1e-9: a corner above half the rate)
        with pytest.raises(pkg.PddcError):
            pkg.eq_deemphasis(48000.0, tau)
    assert pkg.ddc_lib().pddc_eq_design(0, 48000.0, 1000.0, 1.0, 0.0, None) == pkg.PDDC_EINVAL


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    good = (0.5, 0.1, 0.2, -0.3, 0.4)

    def create(rx=((good,), (), (good, good)), nrx=None, S=2, null_nsec=False, null_sec=False, null_params=False, nsec=None):
        K = len(rx)
        ns = (C.c_int * max(K, 1))(*([len(r) for r in rx] if nsec is None else nsec))
        sec = (pkg.EqSection * max(K * max(S, 1), 1))()
        for j, r in enumerate(rx):
            for s, c in enumerate(r[:max(S, 0)]):
                sec[j * S + s] = pkg.EqSection(*c)
        par = pkg.EqParams(S)
        h = C.c_void_p()
        rc = L.pddc_eq_create(C.byref(h), 0, K if nrx is None else nrx, None if null_params else C.byref(par),
                              None if null_nsec else ns, None if null_sec else sec)
        if rc == 0:
            L.pddc_eq_destroy(h)
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(good,)] * 1025), dict(null_nsec=True), dict(null_sec=True), dict(null_params=True),
           dict(S=3), dict(S=0), dict(S=-1), dict(S=16), dict(S=5),
           dict(rx=((good, good, good),), S=2), dict(rx=((good,),), nsec=[-1]), dict(rx=((good,),), S=1, nsec=[2]),
           dict(rx=(((1.0, 0.0, 0.0, 2.0, 0.5),),)), dict(rx=(((1.0, 0.0, 0.0, 0.0, 1.0),),)), dict(rx=(((1.0, 0.0, 0.0, -1.5, 0.5),),)),
           dict(rx=(((1.0, 0.0, 0.0, 0.0, -1.0),),)), dict(rx=((good, (1.0, 0.0, 0.0, 2.0, 0.5)),))]
    for k in range(5):
        for v in (nan, inf, -inf):
            c = list(good)
            c[k] = v
            bad.append(dict(rx=((good,), (tuple(c),))))
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    # the message names the section
    assert create(rx=((good,), (good, (1.0, 0.0, 0.0, 2.0, 0.5)))) == pkg.PDDC_EINVAL
    assert b"receiver 1, section 1" in L.pddc_last_error()
    par = pkg.EqParams(2)
    ns, sec = (C.c_int * 1)(1), (pkg.EqSection * 2)(pkg.EqSection(*good))
    assert L.pddc_eq_create(None, 0, 1, C.byref(par), ns, sec) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        # sections behind nsec are not read: garbage there is fine
        assert create(rx=((good, (nan, nan, nan, 9.0, 9.0)),), nsec=[1]) == pkg.PDDC_ENODEV
        for S in ER.SECTIONS:
            assert create(rx=[(good,) * S] * 1024, S=S) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Eq([[good]], 1)
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(rx=[[good]], sections=3), dict(rx=[[good, good]], sections=1), dict(rx=[], sections=1),
               dict(rx=[[(1.0, 0.0, 0.0, 2.0, 0.5)]], sections=1), dict(rx=[[good]], sections=1 << 40)):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Eq(**kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    st = (C.c_double * 4)()
    assert L.pddc_eq_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_eq_set_rx(None, 0, 1, sec, 0) == pkg.PDDC_EINVAL
    assert L.pddc_eq_read_state(None, st, None) == pkg.PDDC_EINVAL
    assert L.pddc_eq_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_eq_destroy(None) == 0
    assert pkg.eq_tile_outputs() >= 1 and pkg.eq_tile_outputs() == L.pddc_eq_tile_outputs()
    assert (pkg.PDDC_EQ_RESTART, pkg.PDDC_EQ_MAX_SECTIONS) == (ER.RESTART, max(ER.SECTIONS))
    assert (pkg.PDDC_EQ_LOWPASS, pkg.PDDC_EQ_HIGHPASS, pkg.PDDC_EQ_BANDPASS, pkg.PDDC_EQ_NOTCH, pkg.PDDC_EQ_PEAK, pkg.PDDC_EQ_LOWSHELF,
            pkg.PDDC_EQ_HIGHSHELF, pkg.PDDC_EQ_LOWPASS1, pkg.PDDC_EQ_HIGHPASS1) == ER.KINDS
    assert C.sizeof(pkg.EqSection) == 40 and C.sizeof(pkg.EqParams) == 4


def test_gpu_inputs_meet_their_preconditions():
    """Preconditions of tests/test_gpu_eq.py, on the reference alone.  At S = 8 and K = 1024 every place among a wave's 8
    receivers sees every section count 0 .. 8 and every design of the pool; at K = 37 and S = 1, 2, 4 every count occurs,
    at S = 1, 2 in every place.  The pool holds every kind.  Over the first 37 rows at every S: the outputs are finite,
    the zero row stays +0 with zero states, the silent row's output decays, the denormal row's inputs and outputs are
    float32 denormals, rows with sections differ from their input and rows without have its words."""
    x = ER.gpu_series()
    assert x.shape == (ER.K0, ER.N0) and np.isfinite(x).all()
    assert not x[ER.ZERO_ROW].any() and x[ER.SILENT_ROW, :ER.SILENT_FROM].any() and not x[ER.SILENT_ROW, ER.SILENT_FROM:].any()
    tiny = np.finfo(F32).tiny
    d = x[ER.DENORMAL_ROW]
    assert np.count_nonzero((d != 0) & (np.abs(d) < tiny)) >= ER.N0 // 2
    rx = ER.interleaved_rx(ER.K0, 8)
    pool = ER.pool()
    assert ER.GROUP * 9 <= ER.K0 and len(pool) >= 9
    seen = {(j % ER.GROUP, len(r)) for j, r in enumerate(rx)}
    assert seen >= {(p, n) for p in range(ER.GROUP) for n in range(9)}
    firsts = {(j % ER.GROUP, pool.index(r[0])) for j, r in enumerate(rx) if r}
    assert firsts == {(p, k) for p in range(ER.GROUP) for k in range(len(pool))}
    for S in ER.SECTIONS:
        few = ER.interleaved_rx(ER.FEW, S)
        assert {len(r) for r in few} == set(range(S + 1)) and all(len(r) <= S for r in few)
        if S <= 2:
            assert {(j % ER.GROUP, len(r)) for j, r in enumerate(few)} >= {(p, n) for p in range(ER.GROUP) for n in range(S + 1)}
        out, st, _ = ER.eq_ref(x[:ER.FEW], few, S)
        print(f"S {S}: max |out| {np.abs(out).max():.3g}, max |state| {np.abs(st).max():.3g}")
        assert np.isfinite(out).all() and np.isfinite(st).all()
        assert not ER.bits(out[ER.ZERO_ROW]).any() and not st[ER.ZERO_ROW].any()
        assert np.abs(out[ER.SILENT_ROW, -100:]).max() < 1e-3 * np.abs(out[ER.SILENT_ROW, :ER.SILENT_FROM]).max()
        o = out[ER.DENORMAL_ROW]
        assert np.count_nonzero((o != 0) & (np.abs(o) < tiny)) >= ER.N0 // 2
        for j, r in enumerate(few):
            assert same(out[j], x[j]) == (not r or j == ER.ZERO_ROW), j
            assert st[j, :len(r)].any() or j in (ER.ZERO_ROW, ER.SILENT_ROW) or not r    # (a silent row's states can decay to 0)
            assert not ER.bits(st[j, len(r):]).any()
