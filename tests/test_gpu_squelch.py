"""Squelch (pddc_squelch_*, k_squelch) on the GPU against the numpy float32 reference (tests/squelch_ref.py) fed the very
float32 arrays uploaded.  Every comparison is by int32 / uint8 views and exact equality: there are no tolerances.  The
inputs' preconditions (enough open and close events, a reversed ramp) are asserted in tests/test_squelch_cpu.py."""
import ctypes as C
import types

import numpy as np
import pytest

import demod_ref as DR
import squelch_ref as SR
import tuner_ref as TR

pytestmark = pytest.mark.gpu
K0, N0 = 1024, 3000


def make(pkg, rx, par):
    B, attack, hang, R = par
    return pkg.Squelch(rx, B, attack, hang, R, up=SR.UP)


def run(pkg, z, a, rx, par, cuts=None, before=None):
    """all of z, a (torch [K, n]) through a fresh Squelch in the given batches -> numpy (out, levels, states, status);
    before(i, s) is called ahead of batch i"""
    import torch
    s = make(pkg, rx, par)
    outs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, s)
        due = s.next_blocks(b)
        o = s.process(z[:, off:off + b], a[:, off:off + b])
        assert o[0].shape == (len(rx), b) and o[1].shape == o[2].shape == (len(rx), due)
        outs.append(o)
        off += b
    assert off == z.shape[1]
    status = s.read()
    s.close()
    return tuple(torch.cat([o[i] for o in outs], dim=1).cpu().numpy() for i in range(3)) + (status,)


def same(got, want, what=""):
    for name, g, w in zip(("out", "levels", "states"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(SR.bits(g), SR.bits(w)), (what, name)
    if len(got) > 3 and len(want) > 3:
        for name in SR.STATUS.names:
            assert np.array_equal(got[3][name].view(np.uint32), want[3][name].view(np.uint32)), (what, "status", name)


@pytest.fixture(scope="module")
def series(dev):
    import torch
    z, a, rx = SR.keyed_series(K0, N0, 11), SR.audio_series(K0, N0, 12), SR.interleaved_rx(K0)
    return types.SimpleNamespace(z=z, a=a, rx=rx, zd=torch.from_numpy(z).to(dev), ad=torch.from_numpy(a).to(dev))


def test_bits_against_the_reference(pkg, dev, series):
    """K = 1024, n = 3000, thresholds and flag sets interleaved receiver by receiver; the six parameter sets (B, attack,
    hang, R), the last of which completes no block: out, levels, states and read() after the batch equal squelch_ref's."""
    TT = pkg.squelch_tile_outputs()
    for par in SR.param_sets(TT):
        got = run(pkg, series.zd, series.ad, series.rx, par)
        want = SR.squelch_ref(series.z, series.a, series.rx, **SR.params(*par))
        assert got[1].shape == (K0, N0 // par[0])
        same(got, want[:4], par)
        if par[0] > N0:
            assert got[1].shape[1] == 0 and not got[3]["open"].any() and np.isinf(got[3]["floor"]).all()


@pytest.mark.parametrize("par", [(48, 2, 3, 37), (1000, 1, 1, 300)])
def test_bits_against_the_cut_and_the_company(pkg, dev, series, par):
    """One batch against batches of 0, 1, 2, B - 1, TT - 1, TT, TT + 1, 3 TT + 5 and the rest, for K = 1024, 7 and 1;
    the receiver order reversed; a receiver alone against itself among the 1024; read(clear_peak=True) between two
    batches against the streaming reference."""
    TT, B = pkg.squelch_tile_outputs(), par[0]
    cuts = [0, 1, 2, B - 1, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(N0 - sum(cuts))
    assert cuts[-1] > 0
    z, a, rx = series.zd, series.ad, series.rx
    one = run(pkg, z, a, rx, par)
    same(run(pkg, z, a, rx, par, cuts), one, "cut")
    rev = run(pkg, z.flip(0).contiguous(), a.flip(0).contiguous(), rx[::-1], par, cuts[::-1])
    same(rev, tuple(x[::-1] for x in one), "reversed")
    few = run(pkg, z[500:507].contiguous(), a[500:507].contiguous(), rx[500:507], par, cuts)
    same(few, tuple(x[500:507] for x in one), "K 7")
    for j in (0, 1, 2, 3, 6, 1023):
        alone = run(pkg, z[j:j + 1].contiguous(), a[j:j + 1].contiguous(), rx[j:j + 1], par, cuts)
        same(alone, tuple(x[j:j + 1] for x in one), f"alone {j}")
    # read(clear_peak=True) between two batches
    rows = slice(500, 507)
    ref = SR.SquelchRef(rx[rows], **SR.params(*par))
    s = make(pkg, rx[rows], par)
    zz, aa = z[rows].contiguous(), a[rows].contiguous()
    for lo, hi in ((0, 1700), (1700, N0)):
        s.process(zz[:, lo:hi], aa[:, lo:hi])
        ref.process(series.z[rows, lo:hi], series.a[rows, lo:hi])
        got, want = s.read(clear_peak=True), ref.read(clear_peak=True)
        again = s.read()
        for name in SR.STATUS.names:
            assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), (name, lo)
        assert not again["peak"].any() and np.array_equal(again["level"], got["level"])
    s.close()


def test_strides_and_in_place(pkg, dev, series):
    """z as the view Tuner.process returns (stride = capacity > n); a and out with capacity > n, levels and states with
    blk_stride > blocks, the padding keeps its fill value; out is a gives the bits of out of place."""
    import torch
    M, hop, T, Rd, K, S = 1024, 512, 64, 4, 13, 1200
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((S, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, Rd), Rd)
    cap = t.next_outputs(S) + 37
    zv = t.process(rows, out=torch.empty((K, cap), dtype=torch.complex64, device=dev))
    n = zv.shape[1]
    assert zv.stride(0) == cap > n > 256
    par = (48, 1, 2, 37)
    power = float((zv.abs() ** 2).mean())
    rx = [(power * (0.8 + 0.05 * (j % 5)), power * 0.7, SR.FLAG_SETS[j % 4] & SR.GATE) for j in range(K)]
    abuf = torch.full((K, n + 5), 3.0, dtype=torch.float32, device=dev)
    abuf[:, :n] = torch.from_numpy(SR.audio_series(K, n, 8)).to(dev)
    av = abuf[:, :n]
    want = SR.squelch_ref(zv.cpu().numpy(), av.cpu().numpy(), rx, **SR.params(*par))
    assert 0 < want[2].mean() < 1
    blocks = n // par[0]
    s = make(pkg, rx, par)
    obuf = torch.full((K, n + 11), 7.0, dtype=torch.float32, device=dev)
    lbuf = torch.full((K, blocks + 3), 5.0, dtype=torch.float32, device=dev)
    sbuf = torch.full((K, blocks + 3), 9, dtype=torch.uint8, device=dev)
    out, lv, st = s.process(zv, av, out=obuf, levels=lbuf, states=sbuf)
    status = s.read()
    assert out.data_ptr() == obuf.data_ptr() and lv.data_ptr() == lbuf.data_ptr() and st.data_ptr() == sbuf.data_ptr()
    same((out.cpu().numpy(), lv.cpu().numpy(), st.cpu().numpy(), status), want[:4], "strided")
    assert bool((obuf[:, n:] == 7.0).all()) and bool((lbuf[:, blocks:] == 5.0).all()) and bool((sbuf[:, blocks:] == 9).all())
    assert bool((abuf[:, n:] == 3.0).all())
    s.reset()
    out2, lv2, st2 = s.process(zv, av, out=av)                 # in place
    assert out2.data_ptr() == abuf.data_ptr()
    same((out2.cpu().numpy(), lv2.cpu().numpy(), st2.cpu().numpy(), s.read()), want[:4], "in place")
    assert bool((abuf[:, n:] == 3.0).all())
    s.close()
    t.close()


def test_set_rx_between_batches(pkg, dev, series):
    """Threshold and flag changes on some receivers against the streaming reference, bit for bit; the receivers that were
    not touched have the bits of a run without the changes; a bad call is refused and changes nothing."""
    K, par = 12, (48, 2, 3, 37)
    cuts = [700, 1, 999, 1300]
    rows = slice(100, 100 + K)
    rx = series.rx[rows]
    z, a = series.zd[rows].contiguous(), series.ad[rows].contiguous()
    changes = {1: [(2, 1.5, 0.01, SR.GATE), (3, 40.0, 2.0, SR.GATE | SR.RELATIVE)],      # thresholds; flags too
               2: [(2, 0.02, 0.02, 0), (7, rx[7][0], rx[7][1], rx[7][2] ^ SR.GATE)],    # gate off; the gate alone
               3: [(0, 3.0e38, 0.0, SR.GATE), (7, rx[7][0], rx[7][1], rx[7][2])]}        # never opens again; back
    bad = ((1, 0.5, 0.25, 4), (1, 0.25, 0.5, 0), (1, float("nan"), 0.25, 0), (1, float("inf"), 0.25, 0),
           (1, 0.5, -0.25, 0), (K, 0.5, 0.25, 0), (-1, 0.5, 0.25, 0))

    def before(i, s):
        for c in changes.get(i, ()):
            s.set_rx(*c)
        for b in bad:
            with pytest.raises(pkg.PddcError) as e:
                s.set_rx(*b)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, z, a, rx, par, cuts, before)
    clean = run(pkg, z, a, rx, par, cuts)
    touched = {c[0] for cs in changes.values() for c in cs}
    for j in range(K):
        if j not in touched:
            same(tuple(x[j:j + 1] for x in got), tuple(x[j:j + 1] for x in clean), f"untouched {j}")
    ref = SR.SquelchRef(rx, **SR.params(*par))
    outs, off = [], 0
    for i, b in enumerate(cuts):
        for c in changes.get(i, ()):
            ref.set_rx(*c)
        outs.append(ref.process(series.z[rows, off:off + b], series.a[rows, off:off + b]))
        off += b
    want = tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3)) + (ref.read(),)
    same(got, want, "set_rx")
    assert any(not np.array_equal(got[0][j], clean[0][j]) for j in touched)


def test_a_refused_process_changes_nothing(pkg, dev, series):
    """process calls refused for capacity (each stride), for a misaligned or missing pointer and for an overlap of out
    with z, between the batches: the next correct call's bits are those of an object that never saw them.  reset starts
    the series again."""
    import torch
    K, par = 9, (48, 2, 3, 37)
    cuts = [700, 300, 2000]
    rows = slice(300, 300 + K)
    rx = series.rx[rows]
    z, a = series.zd[rows].contiguous(), series.ad[rows].contiguous()
    clean = run(pkg, z, a, rx, par, cuts)
    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, s):
        b = cuts[i]
        due = s.next_blocks(b)
        assert due >= 5
        f32 = lambda cols: torch.empty((K, cols), dtype=torch.float32, device=dev)
        u8 = lambda cols: torch.empty((K, cols), dtype=torch.uint8, device=dev)
        for kw in (dict(out=f32(b - 1)), dict(levels=f32(due - 1)), dict(states=u8(due - 1)),
                   dict(levels=f32(due - 1), states=u8(due - 1))):
            with pytest.raises(pkg.PddcError) as e:
                s.process(z[:, :b], a[:, :b], **kw)
            assert e.value.code == ECAP, kw
        o, lv, st = f32(b), f32(due), u8(due)
        zz = torch.empty((K, b + 1), dtype=torch.complex64, device=dev)   # out over z's bytes: a partial overlap
        stream = torch.cuda.current_stream().cuda_stream
        cnt = C.c_size_t(77)

        def call(zp=z.data_ptr(), ap=a.data_ptr(), n=b, zs=N0, as_=N0, op=o.data_ptr(), os_=b, lp=lv.data_ptr(),
                 sp=st.data_ptr(), bs=due):
            return L.pddc_squelch_process(s._h, zp, ap, n, zs, as_, op, os_, lp, sp, bs, C.byref(cnt), stream)

        assert call(zs=b - 1) == ECAP and call(as_=b - 1) == ECAP and call(os_=b - 1) == ECAP and call(bs=due - 1) == ECAP
        assert call(bs=due - 1, lp=None) == ECAP and call(bs=due - 1, sp=None) == ECAP
        assert call(zp=z.data_ptr() + 4) == EINVAL and call(ap=a.data_ptr() + 2) == EINVAL
        assert call(op=o.data_ptr() + 1) == EINVAL and call(lp=lv.data_ptr() + 2) == EINVAL
        assert call(zp=None) == EINVAL and call(ap=None) == EINVAL and call(op=None) == EINVAL
        assert call(zp=zz.data_ptr(), zs=b + 1, op=zz.data_ptr() + 8 * b, os_=b) == EINVAL       # out inside z
        assert call(op=a.data_ptr() + 4, os_=N0) == EINVAL                                       # out over a, shifted
        assert call(op=a.data_ptr(), os_=N0 - 1) == EINVAL                                       # out is a, another stride
        assert cnt.value == 77
        assert call(zp=None, ap=None, n=0, zs=0, as_=0, op=None, os_=0, lp=None, sp=None, bs=0) == pkg.PDDC_OK
        assert cnt.value == 0

    got = run(pkg, z, a, rx, par, cuts, disturb)
    same(got, clean, "refused")
    s = make(pkg, rx, par)                                      # reset starts the series again
    first = tuple(t.clone() for t in s.process(z, a))
    st1 = s.read()
    s.reset()
    fresh = s.read()
    assert not fresh["level"].any() and not fresh["opens"].any() and np.isinf(fresh["floor"]).all()
    second = s.process(z, a)
    for x, y, w in zip(first, second, clean):
        assert np.array_equal(SR.bits(x.cpu().numpy()), SR.bits(y.cpu().numpy()))
        assert np.array_equal(SR.bits(x.cpu().numpy()), SR.bits(w))
    st2 = s.read()
    for name in SR.STATUS.names:
        assert np.array_equal(st1[name].view(np.uint32), st2[name].view(np.uint32))
    s.close()


def test_end_to_end(pkg, O, dev):
    """2^19 samples with a carrier in channel 300 keyed on for the middle third (and a little noise), packed by the
    package's pack24, through Channelizer (1024, hop 512) -> Tuner (T = 64, R = 4) -> Demod AM -> Squelch (B = 8, attack
    2, hang 2, GATE | RELATIVE) on one stream: out, levels and states equal squelch_ref on the downloaded z and a; the
    open interval starts and ends within attack + 2 and hang + 2 blocks of the keyed interval, the tuner's delay taken
    off; a second receiver on an empty channel never opens and its out is all +0."""
    import torch
    c = DR.CHAIN
    ns, amp, noise = 1 << 19, 0.45, 0.003
    on, off = ns // 3, 2 * ns // 3
    i = np.arange(ns, dtype=np.int64)
    ph = 2.0 * np.pi * ((DR.CARRIER_WORD * i) & DR.MASK).astype(np.float64) / 2.0 ** 32
    rng = np.random.default_rng(77)
    x = amp * ((i >= on) & (i < off)) * np.exp(1j * ph) + noise * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns))
    sig = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    packed = pkg.pack24_f32(torch.from_numpy(sig).to(dev))
    assert np.array_equal(packed.cpu().numpy(), O.pack24_f32(sig))
    words = [DR.CARRIER_WORD, (700 << 22) + 999]
    B, attack, hang, R = 8, 2, 2, 16
    w, h = pkg.tuner_prototype(c["nchan"], c["proto_taps"]), pkg.tuner_lowpass(c["ntaps"], c["decim"])
    ch = pkg.Channelizer(c["nchan"], w, c["hop"])
    t = pkg.Tuner(ch, words, h, c["decim"])
    d = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)] * 2)
    rx = [(100.0, 30.0, pkg.PDDC_SQL_GATE | pkg.PDDC_SQL_RELATIVE)] * 2
    s = pkg.Squelch(rx, B, attack, hang, R, up=SR.UP)
    z = t.process(ch.process(packed.clone()))
    a = d.process(z)
    out, lv, st = s.process(z, a)
    status = s.read()
    zn, an = z.cpu().numpy(), a.cpu().numpy()
    assert zn.shape == an.shape == (2, 239) and lv.shape == (2, 239 // B)
    want = SR.squelch_ref(zn, an, rx, **SR.params(B, attack, hang, R))
    same((out.cpu().numpy(), lv.cpu().numpy(), st.cpu().numpy(), status), want[:4], "chain")
    # output m is centred on sample m hop decim + ((T - 1) / 2) hop + (prototype length - 1) / 2
    per = c["hop"] * c["decim"]
    delay = (c["ntaps"] - 1) / 2.0 * c["hop"] + (c["nchan"] * c["proto_taps"] - 1) / 2.0
    kon, koff = (on - delay) / per / B, (off - delay) / per / B
    opened = np.flatnonzero(want[2][0])
    assert opened.size and np.all(np.diff(opened) == 1), want[2][0]
    print(f"keyed blocks {kon:.2f} .. {koff:.2f}, open after blocks {opened[0]} .. {opened[-1]}")
    assert abs(opened[0] - kon) <= attack + 2 and abs(opened[-1] + 1 - koff) <= hang + 2
    assert want[3]["opens"].tolist() == [1, 0] and not want[2][1].any()
    assert np.array_equal(SR.bits(out[1].cpu().numpy()), np.zeros(239, np.int32))
    assert np.count_nonzero(out[0].cpu().numpy()) > (koff - kon - hang - attack) * B
    for obj in (s, d, t, ch):
        obj.close()
