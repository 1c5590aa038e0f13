"""The squelch without a GPU: the host arithmetic and the argument checks of the C ABI, the reference's own properties
(tests/squelch_ref.py), and the preconditions the GPU tests' inputs have to meet."""
import ctypes as C

import numpy as np
import pytest

import squelch_ref as SR

F32 = np.float32


def test_blocks_is_host_arithmetic(pkg):
    L = pkg.ddc_lib()
    befores = [0, 1, 47, 48, 999, 4095, 4096, (1 << 40) - 1, 1 << 40, (1 << 40) + 12345]
    for B in (1, 2, 48, 256, 1000, 4095, 4096):
        ns = sorted({0, 1, B - 1, B, B + 1, 3 * B + 5, 3000, 1 << 20} - {-1})
        for before in befores:
            for n in ns:
                assert pkg.squelch_blocks(B, before, n) == (before + n) // B - before // B, (B, before, n)
    for B in (0, -1, 4097, 1 << 20, -(1 << 31)):
        assert pkg.squelch_blocks(B, 0, 1 << 20) == 0 and L.pddc_squelch_blocks(B, 5, 100000) == 0
    assert pkg.squelch_tile_outputs() >= 1
    assert (pkg.PDDC_SQL_GATE, pkg.PDDC_SQL_RELATIVE) == (SR.GATE, SR.RELATIVE)
    assert pkg.squelch_status_dtype() == SR.STATUS and SR.STATUS.itemsize == 20


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()

    def create(rx=((0.5, 0.25, 0), (2.0, 2.0, 3), (0.0, 0.0, 1)), nrx=None, params=(48, 2, 3, 37, 1.0), null_rx=False,
               null_params=False):
        arr = (pkg.SquelchRx * max(len(rx), 1))(*[pkg.SquelchRx(*r) for r in rx])
        par = pkg.SquelchParams(*params)
        s = C.c_void_p()
        rc = L.pddc_squelch_create(C.byref(s), 0, len(rx) if nrx is None else nrx, None if null_params else C.byref(par),
                                   None if null_rx else arr)
        if rc == 0:
            L.pddc_squelch_destroy(s)
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(1.0, 0.5, 0)] * 1025), dict(null_rx=True), dict(null_params=True),
           dict(params=(0, 2, 3, 37, 1.0)), dict(params=(4097, 2, 3, 37, 1.0)), dict(params=(-48, 2, 3, 37, 1.0)),
           dict(params=(48, 0, 3, 37, 1.0)), dict(params=(48, 65536, 3, 37, 1.0)),
           dict(params=(48, 2, 0, 37, 1.0)), dict(params=(48, 2, 65536, 37, 1.0)),
           dict(params=(48, 2, 3, 0, 1.0)), dict(params=(48, 2, 3, 65537, 1.0)),
           dict(params=(48, 2, 3, 37, 0.999)), dict(params=(48, 2, 3, 37, nan)), dict(params=(48, 2, 3, 37, inf)),
           dict(params=(48, 2, 3, 37, -2.0)),
           dict(rx=[(0.5, 0.25, 4)]), dict(rx=[(0.5, 0.25, 0), (0.5, 0.25, 0x80000000)]),
           dict(rx=[(0.25, 0.5, 0)]), dict(rx=[(0.5, -0.25, 0)]), dict(rx=[(-1.0, -2.0, 0)]),
           dict(rx=[(nan, 0.25, 0)]), dict(rx=[(0.5, nan, 0)]), dict(rx=[(inf, 0.25, 0)]), dict(rx=[(inf, inf, 0)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.SquelchRx * 1)(pkg.SquelchRx(0.5, 0.25, 0))
    par = pkg.SquelchParams(48, 2, 3, 37, 1.0)
    assert L.pddc_squelch_create(None, 0, 1, C.byref(par), arr) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(rx=[(3.0e38, 0.0, 3)] * 1024, params=(4096, 65535, 65535, 65536, 3.0e38)) == pkg.PDDC_ENODEV
        assert create(params=(1, 1, 1, 1, 1.0)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Squelch([(0.5, 0.25, pkg.PDDC_SQL_GATE)], 48, 2, 3, 37)
        assert e.value.code == pkg.PDDC_ENODEV
    with pytest.raises(pkg.PddcError) as e:
        pkg.Squelch([(0.5, 0.25, 8)], 48, 2, 3, 37)
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        pkg.Squelch([(0.5, 0.25, 0)], 1 << 40, 2, 3, 37)
    assert e.value.code == pkg.PDDC_EINVAL
    n = C.c_size_t()
    assert L.pddc_squelch_process(None, None, None, 8, 8, 8, None, 8, None, None, 0, C.byref(n), None) == pkg.PDDC_EINVAL
    assert L.pddc_squelch_set_rx(None, 0, 0.5, 0.25, 0) == pkg.PDDC_EINVAL
    assert L.pddc_squelch_next_blocks(None, 8, C.byref(n)) == pkg.PDDC_EINVAL
    assert L.pddc_squelch_read(None, None, 0, None) == pkg.PDDC_EINVAL
    assert L.pddc_squelch_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_squelch_destroy(None) == 0


def same(a, b):
    return all(np.array_equal(SR.bits(x), SR.bits(y)) for x, y in zip(a, b))


def test_reference_streaming_equals_one_shot():
    """arbitrary cuts, batches of 0 and of fewer than B samples included; the status too"""
    K, n = 24, 1500
    z, a, rx = SR.keyed_series(K, n, 3), SR.audio_series(K, n, 4), SR.interleaved_rx(K)
    for B, attack, hang, R in ((1, 1, 1, 1), (48, 2, 3, 37), (256, 1, 2, 4096), (1000, 1, 1, 300)):
        par = SR.params(B, attack, hang, R)
        out, lv, st, status, _ = SR.squelch_ref(z, a, rx, **par)
        assert lv.shape == st.shape == (K, n // B)
        cuts = [0, 1, 2, 0, 47, 48, 255, 257, 1, 0]
        cuts.append(n - sum(cuts))
        r = SR.SquelchRef(rx, **par)
        assert same(SR.run_cuts(r, z, a, cuts), (out, lv, st))
        got = r.read()
        for name in SR.STATUS.names:
            assert np.array_equal(got[name].view(np.uint32), status[name].view(np.uint32)), name


def test_reference_gate_properties():
    """A fully open ungated receiver returns a's bits; a closed gated one returns +0; a receiver opens after exactly
    `attack` qualifying blocks and closes after exactly `hang`; a level between close_thr and open_thr toggles nothing;
    the floor is frozen while open."""
    B, attack, hang, R = 8, 3, 4, 5
    amp = lambda v, blocks: np.full(blocks * B, np.sqrt(v), F32)
    # levels: low, 2 high (not enough), low, then high from block 4 on; between the thresholds from block 12; low from 16
    env = np.concatenate([amp(0.01, 1), amp(1.0, 2), amp(0.01, 1), amp(1.0, 8), amp(0.3, 4), amp(0.01, 8)])
    n = env.size
    z = (env + 0j).astype(np.complex64)[None, :].repeat(3, axis=0)
    a = SR.audio_series(3, n, 9)
    a[:, 5] = -0.0
    rx = [(0.5, 0.1, 0), (0.5, 0.1, SR.GATE), (30.0, 5.0, SR.GATE | SR.RELATIVE)]
    out, lv, st, status, ref = SR.squelch_ref(z, a, rx, **SR.params(B, attack, hang, R, up=1.0))
    assert np.array_equal(SR.bits(out[0]), SR.bits(a[0]))                      # ungated: a's bits, -0 included
    # blocks 4, 5, 6 qualify: open after the decision of block 6 = 4 + attack - 1
    first_open = 4 + attack - 1
    # blocks 16, 17, 18, 19 are below close: closed after the decision of block 16 + hang - 1; 12 .. 15 toggle nothing
    last_open = 16 + hang - 2
    want = np.zeros(n // B, np.uint8)
    want[first_open:last_open + 1] = 1
    for j in range(3):
        assert np.array_equal(st[j], want), (j, st[j])
    assert status["opens"].tolist() == [1, 1, 1] and status["open"].tolist() == [0, 0, 0]
    s0 = (first_open + 1) * B                                                  # the first sample under the open decision
    for j in (1, 2):
        assert np.array_equal(SR.bits(out[j, :s0]), np.zeros(s0, np.int32))    # +0, not -0, whatever a is
        ramp = (np.arange(1, R, dtype=F32) * (F32(1) / F32(R))) * a[j, s0:s0 + R - 1]
        assert np.array_equal(SR.bits(out[j, s0:s0 + R - 1]), SR.bits(ramp.astype(F32)))
        s1 = (last_open + 2) * B                                               # the first sample under the close decision
        assert np.array_equal(SR.bits(out[j, s0 + R - 1:s1]), SR.bits(a[j, s0 + R - 1:s1]))   # fully open: a's bits
        assert np.array_equal(SR.bits(out[j, s1 + R - 1:]), np.zeros(n - s1 - R + 1, np.int32))
    # the floor: the smallest level while closed, frozen while open (up = 1)
    r = SR.SquelchRef(rx, **SR.params(B, attack, hang, R, up=1.0))
    floors = []
    for k in range(n // B):
        r.process(z[:, k * B:(k + 1) * B], a[:, k * B:(k + 1) * B])
        floors.append(r.read()["floor"].copy())
    floors = np.array(floors)
    assert np.all(floors[first_open:last_open + 1] == floors[first_open])
    assert np.all(floors[0] == lv[:, 0]) and np.all(np.diff(floors, axis=0) <= 0)
    # with up > 1 the floor rises while closed and only then
    r = SR.SquelchRef(rx[:1], **SR.params(B, attack, hang, R, up=1.5))
    zz = (np.concatenate([amp(0.01, 1), amp(0.04, 3)]) + 0j).astype(np.complex64)[None, :]
    _, lv2, _ = r.process(zz, np.zeros(zz.shape, F32))
    assert r.read()["floor"][0] == F32(lv2[0, 0] * F32(1.5) * F32(1.5) * F32(1.5)) < lv2[0, 3]


def test_reference_set_rx_and_clear_peak():
    K, n = 8, 600
    z, a, rx = SR.keyed_series(K, n, 5), SR.audio_series(K, n, 6), SR.interleaved_rx(K)
    par = SR.params(16, 1, 2, 20)
    plain = SR.squelch_ref(z, a, rx, **par)
    r = SR.SquelchRef(rx, **par)
    first = r.process(z[:, :300], a[:, :300])
    st = r.read(clear_peak=True)
    assert np.array_equal(st["peak"], np.max(first[1], axis=1))
    r.set_rx(1, 1e30, 0.0, 0)                                  # receiver 1: ungated from the next sample on
    for bad in ((K, 0.5, 0.25, 0), (-1, 0.5, 0.25, 0), (0, 0.25, 0.5, 0), (0, np.inf, 0.25, 0), (0, 0.5, np.nan, 0), (0, 0.5, 0.25, 4)):
        with pytest.raises(ValueError):
            r.set_rx(*bad)
    second = r.process(z[:, 300:], a[:, 300:])
    assert np.array_equal(r.read()["peak"], np.max(second[1], axis=1))
    out = np.concatenate([first[0], second[0]], axis=1)
    for j in range(K):
        if j != 1:
            assert np.array_equal(SR.bits(out[j]), SR.bits(plain[0][j]))
    c = int(r.c[1])
    assert c == r.R and np.array_equal(SR.bits(out[1, 300 + 20:]), SR.bits(a[1, 300 + 20:]))


@pytest.fixture(scope="module")
def gpu_inputs():
    return SR.keyed_series(1024, 3000, 11), SR.audio_series(1024, 3000, 12), SR.interleaved_rx(1024)


def test_gpu_inputs_exercise_the_gate(gpu_inputs):
    """Preconditions of tests/test_gpu_squelch.py, on the reference alone: over keyed_series(1024, 3000) every parameter
    set that completes a block sees at least 100 open and 100 close events in total (the last, B = 4096, completes none
    and must leave everything as created), and at least one receiver's ramp is reversed before completing (0 < c < R at
    a decision change)."""
    z, a, rx = gpu_inputs
    assert {r[2] for r in rx} == set(SR.FLAG_SETS)
    reversals = 0
    for B, attack, hang, R in SR.param_sets(256):
        out, lv, st, status, ref = SR.squelch_ref(z, a, rx, **SR.params(B, attack, hang, R))
        print(f"B {B} attack {attack} hang {hang} R {R}: {ref.open_events} open, {ref.close_events} close events, "
              f"{ref.reversals} reversed ramps")
        if B > 3000:
            assert lv.shape == (1024, 0) and ref.open_events == 0
            assert not status["open"].any() and not status["level"].any() and np.isinf(status["floor"]).all()
            gated = np.array([r[2] & SR.GATE for r in rx], bool)
            assert not out[gated].any() and np.array_equal(SR.bits(out[~gated]), SR.bits(a[~gated]))
            continue
        assert ref.open_events >= 100 and ref.close_events >= 100, (B, ref.open_events, ref.close_events)
        reversals += ref.reversals
    assert reversals >= 1
