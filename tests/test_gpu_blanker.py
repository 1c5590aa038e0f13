"""Blanker (pddc_blanker_*, k_blanker) on the GPU against the numpy float32 reference (tests/blanker_ref.py) fed the very
complex64 arrays uploaded.  Every comparison is by int32 / uint32 views and exact equality: there are no tolerances
(the end-to-end test's RxFilter and Demod stages keep their own).  The inputs' preconditions (overlapping windows,
triggers next to tile seams and batch cuts, in the last D samples, every ramp step) are asserted in
tests/test_blanker_cpu.py."""
import types

import numpy as np
import pytest

import blanker_ref as BR
import demod_ref as DR
import rxfilter_ref as RR
import tuner_ref as TR

pytestmark = pytest.mark.gpu
K0, N0 = BR.GPU_K, BR.GPU_N


def make(pkg, rx, par):
    B, W, R = par
    return pkg.Blanker(rx, B, W, R, beta=BR.BETA, cap=BR.CAP)


def run(pkg, z, rx, par, cuts=None, before=None):
    """all of z (torch [K, n]) through a fresh Blanker in the given batches -> numpy (out, status); before(i, b) is called
    ahead of batch i"""
    import torch
    b = make(pkg, rx, par)
    assert b.delay == par[1] + par[2]
    outs, off = [], 0
    for i, c in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, b)
        o = b.process(z[:, off:off + c])
        assert o.shape == (len(rx), c) and o.dtype == torch.complex64
        outs.append(o)
        off += c
    assert off == z.shape[1]
    status = b.read()
    b.close()
    return torch.cat(outs, dim=1).cpu().numpy(), status


def same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype == np.complex64, (what, got[0].shape, want[0].shape)
    assert np.array_equal(BR.bits(got[0]), BR.bits(want[0])), (what, "out")
    for name in BR.STATUS.names:
        assert np.array_equal(got[1][name].view(np.uint32), want[1][name].view(np.uint32)), (what, "status", name)


@pytest.fixture(scope="module")
def series(dev):
    import torch
    z, rx = BR.impulse_series(K0, N0, BR.GPU_SEED), BR.interleaved_rx(K0)
    return types.SimpleNamespace(z=z, rx=rx, zd=torch.from_numpy(z).to(dev), refs={})


def reference(series, par):
    """blanker_ref over the whole series, computed once per parameter set and left unchanged"""
    if par not in series.refs:
        series.refs[par] = BR.blanker_ref(series.z, series.rx, **BR.params(*par))[:2]
    return series.refs[par]


def test_bits_against_the_reference(pkg, dev, series):
    """K = 1024, n = 3000, ON and OFF receivers and six thresholds interleaved; the seven parameter sets (B, W, R), the last
    of which completes no block: out and read() after the batch equal blanker_ref's."""
    TT = pkg.blanker_tile_outputs()
    for par in BR.param_sets(TT):
        got = run(pkg, series.zd, series.rx, par)
        want = reference(series, par)
        print(par, "triggers", int(want[1]["triggers"].sum()), "blanked", int(want[1]["blanked"].sum()))
        same(got, want, par)
        if par[0] > N0:
            assert not got[1]["triggers"].any() and not got[1]["blanked"].any() and not got[1]["ref"].any()
        else:
            assert got[1]["triggers"].sum() > 10 * K0 // 2


@pytest.mark.parametrize("par", BR.CUT_SETS)
def test_bits_against_the_cut_and_the_company(pkg, dev, series, par):
    """One batch against batches of 0, 1, 2, D - 1, D, 2 D + 1, TT - 1, TT, TT + 1, 3 TT + 5 and the rest, for K = 1024,
    7, 5 and 1; the receiver order reversed; a receiver alone against itself among the 1024."""
    TT, D = pkg.blanker_tile_outputs(), par[1] + par[2]
    cuts = BR.gpu_cuts(TT, D, N0)
    z, rx = series.zd, series.rx
    one = reference(series, par)
    same(run(pkg, z, rx, par), one, "one batch")
    same(run(pkg, z, rx, par, cuts), one, "cut")
    rev = run(pkg, z.flip(0).contiguous(), rx[::-1], par, cuts[::-1])
    same(rev, tuple(x[::-1] for x in one), "reversed")
    for lo, k in ((500, 7), (771, 5)):
        few = run(pkg, z[lo:lo + k].contiguous(), rx[lo:lo + k], par, cuts)
        same(few, tuple(x[lo:lo + k] for x in one), f"K {k}")
    for j in (0, 1, 2, 3, 6, 1023):
        alone = run(pkg, z[j:j + 1].contiguous(), rx[j:j + 1], par, cuts)
        same(alone, tuple(x[j:j + 1] for x in one), f"alone {j}")


def test_strides(pkg, dev):
    """z as the view Tuner.process returns (stride = capacity > n), out with capacity > n: the slack beyond n keeps its
    canary pattern on both sides, and the bits are blanker_ref's on a host copy of the view."""
    import torch
    M, hop, T, Rd, K, S = 1024, 512, 64, 4, 13, 1200
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((S, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, Rd), Rd)
    cap = t.next_outputs(S) + 37
    zbuf = torch.full((K, cap), 3.0 - 4.0j, dtype=torch.complex64, device=dev)
    zv = t.process(rows, out=zbuf)
    n = zv.shape[1]
    assert zv.stride(0) == cap > n > 256
    par = (32, 2, 3)
    # Gaussian rows: p exceeds 3 times its mean in about 5 % of the samples
    rx = [(3.0 + 0.5 * (j % 3), BR.ON if j % 4 != 1 else 0) for j in range(K)]
    want = BR.blanker_ref(zv.cpu().numpy(), rx, **BR.params(*par))[:2]
    on = np.array([r[1] for r in rx], bool)
    assert want[1]["triggers"][on].min() >= 1 and not want[1]["triggers"][~on].any()
    b = make(pkg, rx, par)
    canary = 7.0 + 9.0j
    obuf = torch.full((K, n + 11), canary, dtype=torch.complex64, device=dev)
    out = b.process(zv, out=obuf)
    status = b.read()
    assert out.data_ptr() == obuf.data_ptr() and out.stride(0) == n + 11
    same((out.cpu().numpy(), status), want, "strided")
    assert bool((obuf[:, n:] == canary).all()) and bool((zbuf[:, n:] == 3.0 - 4.0j).all())
    b.close()
    t.close()


def test_set_rx_between_batches(pkg, dev, series):
    """Threshold changes and ON <-> OFF on some receivers against the streaming reference, bit for bit; the receivers
    that were not touched have the bits of a run without the changes; a bad call is refused and changes nothing."""
    K, par = 12, (48, 3, 5)
    cuts = [700, 1, 999, 1300]
    rows = slice(99, 99 + K)
    rx = series.rx[rows]
    z = series.zd[rows].contiguous()
    assert rx[0][1] and rx[1][1] and not rx[2][1] and rx[7][1]
    changes = {1: [(2, 16.0, BR.ON), (3, 1000.0, BR.ON)],             # OFF -> ON; a threshold out of the bursts' reach
               2: [(0, rx[0][0], 0), (7, 4.0, BR.ON)],                 # ON -> OFF; a threshold the noise itself exceeds
               3: [(0, 8.0, BR.ON), (2, 16.0, 0), (7, rx[7][0], rx[7][1])]}    # and back
    bad = ((1, 16.0, 2), (1, 0.0, 1), (1, -8.0, 1), (1, float("nan"), 1), (1, float("inf"), 0), (K, 16.0, 1), (-1, 16.0, 1))

    def before(i, b):
        for c in changes.get(i, ()):
            b.set_rx(*c)
        for c in bad:
            with pytest.raises(pkg.PddcError) as e:
                b.set_rx(*c)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, z, rx, par, cuts, before)
    clean = run(pkg, z, rx, par, cuts)
    touched = {c[0] for cs in changes.values() for c in cs}
    for j in range(K):
        if j not in touched:
            same(tuple(x[j:j + 1] for x in got), tuple(x[j:j + 1] for x in clean), f"untouched {j}")
    ref = BR.BlankerRef(rx, **BR.params(*par))
    outs, off = [], 0
    for i, c in enumerate(cuts):
        for ch in changes.get(i, ()):
            ref.set_rx(*ch)
        outs.append(ref.process(series.z[rows, off:off + c]))
        off += c
    same(got, (np.concatenate(outs, axis=1), ref.read()), "set_rx")
    assert all(not np.array_equal(got[0][j], clean[0][j]) for j in touched)


def test_a_refused_process_changes_nothing(pkg, dev, series):
    """process calls refused for an overlap of out with z (out == z included), a misaligned pointer, a stride below n and
    NULL, between the batches: the next good batch and read() equal an object that never saw them.  reset starts every
    series again; n = 0 and n < D on a fresh object both work."""
    import torch
    K, par = 9, (1000, 128, 128)
    D = par[1] + par[2]
    cuts = [700, 300, 2000]
    rows = slice(300, 300 + K)
    rx = series.rx[rows]
    z = series.zd[rows].contiguous()
    want = tuple(x[rows] for x in reference(series, par))
    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, b):
        c = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            b.process(z[:, :c], out=torch.empty((K, c - 1), dtype=torch.complex64, device=dev))
        assert e.value.code == ECAP
        with pytest.raises(pkg.PddcError) as e:
            b.process(z[:, :c], out=z[:, :c])
        assert e.value.code == EINVAL
        o = torch.empty((K, c), dtype=torch.complex64, device=dev)
        zz = torch.empty((K, c + 1), dtype=torch.complex64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(zp=z.data_ptr(), n=c, zs=N0, op=o.data_ptr(), os_=c):
            return L.pddc_blanker_process(b._h, zp, n, zs, op, os_, stream)

        assert call(zs=c - 1) == ECAP and call(os_=c - 1) == ECAP
        assert call(zp=z.data_ptr() + 4) == EINVAL and call(op=o.data_ptr() + 4) == EINVAL
        assert call(zp=None) == EINVAL and call(op=None) == EINVAL
        assert call(op=z.data_ptr(), os_=N0) == EINVAL                                          # out == z
        assert call(op=z.data_ptr() + 8, os_=N0) == EINVAL                                      # out over z, shifted
        assert call(zp=zz.data_ptr(), zs=c + 1, op=zz.data_ptr() + 8 * c, os_=c) == EINVAL      # out inside z's rows
        assert call(op=z.data_ptr() + 8 * (N0 * (K - 1) + c - 1), os_=c) == EINVAL              # one shared value
        assert call(zp=None, n=0, zs=0, op=None, os_=0) == pkg.PDDC_OK

    same(run(pkg, z, rx, par, cuts, disturb), want, "refused")
    b = make(pkg, rx, par)
    assert b.process(z[:, :0]).shape == (K, 0)                       # n = 0 and n < D on a fresh object
    st = b.read()
    assert not st["ref"].any() and not st["triggers"].any() and not st["blanked"].any()
    head = [b.process(z[:, :D - 1]), b.process(z[:, D - 1:D + 2])]
    assert not torch.view_as_real(head[0]).any()
    rest = b.process(z[:, D + 2:])
    first = torch.cat(head + [rest], dim=1).cpu().numpy()
    st1 = b.read()
    same((first, st1), want, "short batches")
    b.reset()                                                        # reset starts every series again
    fresh = b.read()
    assert not fresh["ref"].any() and not fresh["triggers"].any() and not fresh["blanked"].any()
    same((b.process(z).cpu().numpy(), b.read()), want, "after reset")
    b.close()


def test_end_to_end(pkg, O, dev):
    """2^18 samples of noise, packed by the package's pack24, through Channelizer (1024, hop 512) -> Tuner (T = 64, R = 1,
    two receivers on one word) -> Blanker (B = 32, W = 2, R = 4; receiver 0 ON, receiver 1 OFF) -> RxFilter (65 taps) ->
    Demod (AM) on one stream.  Bursts of 40 times the rms are added to the tuner's output on the device.  The blanker's
    rows equal blanker_ref's on a host copy of the tuner's own output with the bursts; RxFilter reads the blanker's output
    view (row stride > n) and Demod RxFilter's without a copy, each within its own tolerance of its reference on the
    device's own input; the audio's peak on the blanked receiver is below a quarter of the other's (three adjacent bursts of 40 rms add up
    in the filter; the noise's own peak is a few rms)."""
    import torch
    M, hop, Tt, ns, Tf = 1024, 512, 64, 1 << 18, 65
    word = 300 << 22
    gen = torch.Generator(device="cpu").manual_seed(31)
    sig = (0.05 * torch.randn((ns, 2), generator=gen, dtype=torch.float32)).to(dev)
    packed = pkg.pack24_f32(sig)
    bank = pkg.rxfilter_bank(1.0, [0.2], Tf)
    ch = pkg.Channelizer(M, pkg.tuner_prototype(M, 4), hop)
    tu = pkg.Tuner(ch, [word, word], pkg.tuner_lowpass(Tt, 1), 1)
    par = (32, 2, 4)
    rx = [(16.0, BR.ON), (16.0, 0)]
    bl = make(pkg, rx, par)
    rf = pkg.RxFilter(bank, [0, 0])
    de = pkg.Demod([(DR.AM, 0, 0), (DR.AM, 0, 0)])
    z = tu.process(ch.process(packed.clone()))
    n = z.shape[1]
    assert n > 400
    rms = float(z.abs().pow(2).mean().sqrt())
    at = [100, 101, 102, 230, 300, 301, n - 3]
    z[:, at] += 40.0 * rms
    obuf = torch.zeros((2, n + 9), dtype=torch.complex64, device=dev)
    y = bl.process(z, out=obuf)
    assert y.data_ptr() == obuf.data_ptr() and y.stride(0) == n + 9
    f = rf.process(y)
    a = de.process(f)
    status = bl.read()
    torch.cuda.synchronize()
    zh = z.cpu().numpy()
    want = BR.blanker_ref(zh, rx, **BR.params(*par))[:2]
    same((y.cpu().numpy(), status), want, "chain")
    assert status["triggers"][0] >= len(at) and status["triggers"][1] == 0
    yh = y.cpu().numpy()
    assert float(np.max(np.abs(yh))) <= 1.0
    fref = RR.rxfilter_ref(yh, bank, [0, 0])
    assert float(np.max(np.abs(f.cpu().numpy().astype(np.complex128) - fref))) <= RR.TOL_RXFILTER
    am = np.abs(f.cpu().numpy().astype(np.complex128))
    ah = a.cpu().numpy().astype(np.float64)
    assert a.shape == (2, n) and float(np.max(np.abs(ah - am))) <= DR.TOL_DEMOD[DR.AM]
    print(f"end to end: {n} values, rms {rms:.3e}, audio peak blanked {ah[0].max():.3e}, not blanked {ah[1].max():.3e}")
    assert ah[0].max() < 0.25 * ah[1].max()
    for o in (de, rf, bl, tu, ch):
        o.close()
