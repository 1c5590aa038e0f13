"""The noise blanker without a GPU: the host arithmetic and the argument checks of the C ABI, the reference's own
properties (tests/blanker_ref.py), and the preconditions the GPU tests' inputs have to meet."""
import ctypes as C

import numpy as np
import pytest

import blanker_ref as BR

F32 = np.float32


def test_host_arithmetic_and_constants(pkg):
    assert pkg.blanker_status_dtype() == BR.STATUS and BR.STATUS.itemsize == 12
    assert pkg.blanker_tile_outputs() >= 1
    assert pkg.PDDC_NB_ON == BR.ON == 0x1
    assert C.sizeof(pkg.BlankerParams) == 20 and C.sizeof(pkg.BlankerRx) == 8


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()

    def create(rx=((16.0, 1), (8.0, 0), (1e-30, 1)), nrx=None, params=(48, 3, 5, 0.25, 2.0), null_rx=False, null_params=False):
        arr = (pkg.BlankerRx * max(len(rx), 1))(*[pkg.BlankerRx(*r) for r in rx])
        par = pkg.BlankerParams(*params)
        b = C.c_void_p()
        rc = L.pddc_blanker_create(C.byref(b), 0, len(rx) if nrx is None else nrx, None if null_params else C.byref(par),
                                   None if null_rx else arr)
        if rc == 0:
            L.pddc_blanker_destroy(b)
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(16.0, 1)] * 1025), dict(null_rx=True), dict(null_params=True),
           dict(params=(0, 3, 5, 0.25, 2.0)), dict(params=(4097, 3, 5, 0.25, 2.0)), dict(params=(-48, 3, 5, 0.25, 2.0)),
           dict(params=(48, -1, 5, 0.25, 2.0)), dict(params=(48, 129, 5, 0.25, 2.0)),
           dict(params=(48, 3, -1, 0.25, 2.0)), dict(params=(48, 3, 129, 0.25, 2.0)),
           dict(params=(48, 3, 5, 0.0, 2.0)), dict(params=(48, 3, 5, -0.25, 2.0)), dict(params=(48, 3, 5, 1.0000001, 2.0)),
           dict(params=(48, 3, 5, nan, 2.0)), dict(params=(48, 3, 5, inf, 2.0)),
           dict(params=(48, 3, 5, 0.25, 0.9999999)), dict(params=(48, 3, 5, 0.25, nan)), dict(params=(48, 3, 5, 0.25, inf)),
           dict(params=(48, 3, 5, 0.25, -2.0)),
           dict(rx=[(16.0, 2)]), dict(rx=[(16.0, 1), (16.0, 0x80000001)]),
           dict(rx=[(0.0, 1)]), dict(rx=[(-16.0, 1)]), dict(rx=[(nan, 0)]), dict(rx=[(inf, 1)]), dict(rx=[(16.0, 1), (-inf, 0)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.BlankerRx * 1)(pkg.BlankerRx(16.0, 1))
    par = pkg.BlankerParams(48, 3, 5, 0.25, 2.0)
    assert L.pddc_blanker_create(None, 0, 1, C.byref(par), arr) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        # every limit from the inside
        assert create() == pkg.PDDC_ENODEV
        assert create(rx=[(3.0e38, 1)] * 1024, params=(4096, 128, 128, 1.0, 3.0e38)) == pkg.PDDC_ENODEV
        assert create(rx=[(1e-38, 0)], params=(1, 0, 0, 1e-30, 1.0)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Blanker([(16.0, pkg.PDDC_NB_ON)], 48, 3, 5)
        assert e.value.code == pkg.PDDC_ENODEV
    with pytest.raises(pkg.PddcError) as e:
        pkg.Blanker([(16.0, 4)], 48, 3, 5)
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        pkg.Blanker([(16.0, 1)], 1 << 40, 3, 5)
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        pkg.Blanker([(16.0, 1)], 48, 3, 5, beta=2.0)
    assert e.value.code == pkg.PDDC_EINVAL
    assert L.pddc_blanker_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_blanker_set_rx(None, 0, 16.0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_blanker_read(None, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_blanker_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_blanker_delay(None) == pkg.PDDC_EINVAL
    assert L.pddc_blanker_destroy(None) == 0


def same_status(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in BR.STATUS.names)


@pytest.fixture(scope="module")
def small():
    K, n = 12, 3200
    return BR.impulse_series(K, n, 3), BR.interleaved_rx(K)


@pytest.mark.parametrize("par", [(48, 3, 5), (1, 1, 0), (256, 0, 0), (64, 0, 7), (1000, 128, 128)])
def test_reference_streaming_equals_one_shot(small, par):
    """cuts of 0, 1, D - 1, D, 2 D and B - 1 samples -- batches shorter than D and than B included --, and one sample
    at a time over a stretch; the status too"""
    z, rx = small
    B, W, R = par
    D, n = W + R, z.shape[1]
    out, status, _ = BR.blanker_ref(z, rx, **BR.params(*par))
    assert status["triggers"].sum() > 0
    cuts = [0, 1, max(D - 1, 0), D, 2 * D, B - 1, 0] + [1] * 40
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    r = BR.BlankerRef(rx, **BR.params(*par))
    assert np.array_equal(BR.bits(BR.run_cuts(r, z, cuts)), BR.bits(out))
    assert same_status(r.read(), status)


def brute_force_gate(t, z, W, R):
    """the definition word for word, one receiver: t bool [n], z complex64 [n] -> (out [n], blanked)"""
    n, D = t.size, W + R
    invR1 = F32(1.0) / F32(R + 1)
    out = np.zeros(n, np.complex64)
    blanked = 0
    trig = np.flatnonzero(t)
    for i in range(n):
        c = i - D
        near = [abs(c - u) for u in trig if abs(c - u) <= D]
        re, im = (z.real[c], z.imag[c]) if c >= 0 else (F32(0), F32(0))
        if near:
            blanked += 1
            dist = min(near)
            if dist <= W:
                re, im = F32(0), F32(0)
            else:
                g = F32(dist - W) * invR1
                re, im = F32(re * g), F32(im * g)
        out.real[i], out.imag[i] = re, im
    return out, blanked


@pytest.mark.parametrize("par", [(48, 3, 5), (1, 1, 0), (32, 0, 0), (64, 0, 7), (100, 128, 128), (16, 4, 0)])
def test_reference_gate_against_the_definition_word_for_word(par):
    """The reference's vectorised gate (running maxima / minima of trigger positions) against a loop over every output
    and every trigger; `blanked` equals the count of outputs with g != 1; OFF rows are the input delayed by D bit for
    bit, -0 and all; the first D outputs are +0."""
    K, n = 6, 700
    z = BR.impulse_series(K, n, 5)
    z[:, 7] = -0.0
    rx = BR.interleaved_rx(K)
    B, W, R = par
    D = W + R
    out, status, r = BR.blanker_ref(z, rx, **BR.params(*par))
    assert np.array_equal(status["triggers"], r.t.sum(axis=1))
    for j in range(K):
        want, blanked = brute_force_gate(r.t[j], z[j], W, R)
        assert np.array_equal(BR.bits(out[j]), BR.bits(want)), j
        assert status["blanked"][j] == blanked == int((r.dist[j] <= D).sum())
        assert np.array_equal(BR.bits(out[j, :D]), np.zeros(2 * D, np.int32))
        if not rx[j][1]:
            assert not r.t[j].any() and blanked == 0
            delayed = np.concatenate([np.zeros(D, np.complex64), z[j, :n - D]])
            assert np.array_equal(BR.bits(out[j]), BR.bits(delayed))
    assert status["triggers"].sum() > 0


def test_reference_output_power_is_bounded_by_the_limit():
    """From the definition, not from a measurement: a sample of an ON receiver whose power exceeds ref thr (ref > 0)
    triggers and is zeroed, so every output with g != 0 whose source sample saw ref > 0 has p = (re re) + (im im), formed
    as the definition forms it, at or below that sample's ref thr: with g = 1 it is the source's p, with 0 < g < 1 both
    parts shrink and float32 products and sums are monotonic."""
    K, n = 48, 2000
    z, rx = BR.impulse_series(K, n, 9), BR.interleaved_rx(K)
    for par in ((48, 3, 5), (1, 1, 0), (64, 0, 7), (200, 128, 128)):
        W, D = par[1], par[1] + par[2]
        out, status, r = BR.blanker_ref(z, rx, **BR.params(*par))
        p = (out.real * out.real) + (out.imag * out.imag)
        assert p.dtype == F32
        lim = np.zeros((K, n), F32)
        lim[:, D:] = (r.refs * r.thr[:, None])[:, :n - D]
        seen = np.zeros((K, n), bool)
        seen[:, D:] = (r.refs > 0)[:, :n - D]
        on = np.array([f[1] for f in rx], bool)[:, None]
        check = on & seen & (r.dist > W)
        assert check.sum() > K * n // 8
        assert np.all(p[check] <= lim[check]), par
        # and the input was not: the blanker had something to do
        pin = (z.real * z.real) + (z.imag * z.imag)
        assert (pin[:, :n - D][check[:, D:]] > lim[:, D:][check[:, D:]]).sum() == 0
        assert (pin[:, :n - D] > lim[:, D:])[(on & seen)[:, D:]].sum() == r.t[:, :n - D].sum() > 0


def test_reference_set_rx():
    """OFF -> ON takes effect at the next sample: the triggers from there on are those of a receiver that was ON all
    along (it was metered while OFF), none before; ON -> OFF stops them at once but what was triggered stays gated; a
    bad call is refused and changes nothing."""
    K, n, cut = 6, 900, 400
    par = (48, 3, 5)
    z = BR.impulse_series(K, n, 13)
    z[:, cut] = 40.0 + 0j                                          # a burst on the first sample after the change
    z[:, cut - 2] = 40.0 + 0j                                      # and one just before it
    on_all, _, ra = BR.blanker_ref(z, [(16.0, BR.ON)] * K, **BR.params(*par))
    assert ra.t[:, cut].all() and ra.t[:, cut - 2].all()
    r = BR.BlankerRef([(16.0, 0)] * K, **BR.params(*par))
    first = r.process(z[:, :cut])
    assert not r.t.any()
    for j in range(K):
        r.set_rx(j, 16.0, BR.ON)
    for bad in ((K, 16.0, 1), (-1, 16.0, 1), (0, 0.0, 1), (0, -1.0, 1), (0, np.inf, 1), (0, np.nan, 0), (0, 16.0, 2)):
        with pytest.raises(ValueError):
            r.set_rx(*bad)
    second = r.process(z[:, cut:])
    assert np.array_equal(r.t, ra.t[:, cut:]) and r.t[:, 0].all()
    assert np.array_equal(r.read()["ref"].view(np.uint32), ra.read()["ref"].view(np.uint32))
    D = 8
    delayed = np.concatenate([np.zeros((K, D), np.complex64), z[:, :n - D]], axis=1)
    got = np.concatenate([first, second], axis=1)
    assert np.array_equal(BR.bits(got[:, :cut]), BR.bits(delayed[:, :cut]))       # the burst at cut - 2 passes ...
    assert not got[:, cut + D - par[1]:cut + D + par[1] + 1].any()                 # ... the one at cut is gated
    # ON -> OFF: the trigger taken at cut - 2 goes on gating the outputs after the change
    r = BR.BlankerRef([(16.0, BR.ON)] * K, **BR.params(*par))
    first = r.process(z[:, :cut])
    for j in range(K):
        r.set_rx(j, 16.0, 0)
    second = r.process(z[:, cut:])
    assert not r.t.any()
    got = np.concatenate([first, second], axis=1)
    assert not got[:, cut - 2 + D - 3:cut - 2 + D + 4].any() and np.array_equal(BR.bits(got[:, :cut]), BR.bits(on_all[:, :cut]))
    assert np.array_equal(BR.bits(got[:, cut + 2 * D:]), BR.bits(delayed[:, cut + 2 * D:]))


def test_gpu_inputs_exercise_the_gate(pkg):
    """Preconditions of tests/test_gpu_blanker.py, on the reference alone, over impulse_series(1024, 3000, 21) and
    interleaved_rx: no parameter set triggers before its first block ends or on an OFF receiver; the last (B = 4096)
    triggers nothing; every other one has at least 10 triggers per ON receiver on average.  For the two sets of the cut
    test, among the ON receivers: two triggers more than 1 and less than 2 D apart (overlapping windows); a trigger
    closer than D to a tile seam and one closer than D to a batch cut, on either side of each; a trigger before a cut
    whose window reaches across it, so that the outputs after the cut have their centres in the batch before and the
    carried history and bits are read; a trigger in the stream's last D samples; for (48, 3, 5) outputs with every
    ramp step 1 .. R."""
    K, n, TT = BR.GPU_K, BR.GPU_N, pkg.blanker_tile_outputs()
    z, rx = BR.impulse_series(K, n, BR.GPU_SEED), BR.interleaved_rx(K)
    on = np.array([r[1] for r in rx], bool)
    assert 0 < on.sum() < K and len({r[0] for r in rx}) >= 4 and all(8 <= r[0] <= 64 for r in rx)
    assert {tuple(on[g:g + 4]) for g in range(0, K, 4)} >= {(True, True, False, True), (True, False, True, True), (False, True, True, False)}
    for par in BR.param_sets(TT):
        B, W, R = par
        D = W + R
        out, status, r = BR.blanker_ref(z, rx, **BR.params(*par))
        t = r.t
        print(f"B {B} W {W} R {R}: {status['triggers'][on].mean():.1f} triggers, {status['blanked'][on].mean():.1f} blanked "
              f"outputs per ON receiver")
        assert not t[:, :min(B, n)].any() and not t[~on].any()
        if B > n:
            assert not t.any() and not status["blanked"].any() and not status["ref"].any()
            assert np.array_equal(BR.bits(out[:, D:]), BR.bits(z[:, :n - D])) and not out[:, :D].any()
            continue
        assert status["triggers"][on].mean() >= 10
        if par not in BR.CUT_SETS:
            continue
        js, us = np.nonzero(t)
        gaps = np.diff(us)[np.diff(js) == 0]
        assert ((gaps > 1) & (gaps < 2 * D)).any()
        assert ((us % TT < D) & (us >= TT)).any() and (TT - us % TT <= D).any()
        bounds = np.cumsum(BR.gpu_cuts(TT, D, n))[:-1]
        after = [b for b in bounds if ((us >= b) & (us < b + D)).any()]
        before = [b for b in bounds if ((us >= b - D) & (us < b)).any()]
        assert after and before
        # ... and the first output after such a cut is gated by it: its centre b - D lies in the batch before
        assert any((r.dist[:, b] <= D)[on].any() for b in before)
        assert (us >= n - D).any()
        if par == (48, 3, 5):
            d = r.dist[on]
            assert set(np.unique(d[(d > W) & (d <= D)] - W).tolist()) == set(range(1, R + 1))
