"""Carrier (pddc_carrier_*, k_carrier) on the GPU: against the double reference (tests/carrier_ref.py) within the
tolerances measured on the CPU (TOL_CARRIER: 7 x the float32 model's error), and against itself, bit for bit, over batch
cuts, K, the receivers' order and company, strides and in place.  The input is the one whose precondition (the
reference's |e| < 0.75 everywhere) tests/test_carrier_cpu.py asserts; it is asserted again wherever a reference is made."""
import ctypes as C
import types

import numpy as np
import pytest

import carrier_ref as CR

pytestmark = pytest.mark.gpu
K0, N0 = 1024, 3000


def make(pkg, rx, L):
    return pkg.Carrier(rx, CR.hilbert(L), **CR.PARAMS)


def run(pkg, z, rx, L, cuts=None, before=None):
    """all of z (torch [K, n]) through a fresh Carrier in the given batches -> (u numpy complex64 [K, n], status);
    before(i, c) is called ahead of batch i"""
    import torch
    c = make(pkg, rx, L)
    outs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, c)
        o = c.process(z[:, off:off + b])
        assert o.shape == (len(rx), b) and o.dtype == torch.complex64
        outs.append(o)
        off += b
    assert off == z.shape[1]
    status = c.read()
    c.close()
    return torch.cat(outs, dim=1).cpu().numpy(), status


def same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype == np.complex64, (what, got[0].shape, want[0].shape)
    assert np.array_equal(CR.bits(got[0]), CR.bits(want[0])), (what, "u")
    for name in CR.STATUS.names:
        assert np.array_equal(got[1][name].view(np.uint32), want[1][name].view(np.uint32)), (what, "status", name)


def close_to(got, ref_u, ref, modes, z, what=""):
    """u (unless ref_u is None) and the status against the double reference `ref` (after its batches), per mode within
    TOL_CARRIER"""
    u, st = got
    want = ref.read()
    for m in CR.MODES:
        rows = np.flatnonzero(np.asarray(modes) == m)
        if not rows.size:
            continue
        tol = CR.TOL_CARRIER[m]
        if ref_u is not None:
            if m == CR.OFF:
                assert np.array_equal(CR.bits(u[rows]), CR.bits(z[rows])), (what, "OFF")
            e = float(CR.err_rows(u[rows], ref_u[rows]).max())
            print(f"{what} {CR.MODE_NAMES[m]}: err {e:.3e} (TOL {tol:.3e})")
            assert e <= tol, (what, m, e)
        dth = int(np.abs(CR.theta_diff(st["theta"][rows], want["theta"][rows])).max())
        turn = tol / np.pi                          # the tolerance as a phase in half-turns (carrier_ref.py)
        dv = float(np.abs(st["freq"][rows].astype(np.float64) - ref.v[rows]).max())
        dq = float(np.abs(st["err"][rows].astype(np.float64) - ref.q[rows]).max())
        print(f"{what} {CR.MODE_NAMES[m]}: theta {dth} units (of {tol / (2 * np.pi) * 2.0 ** 32:.0f}), freq {dv:.3e}, err {dq:.3e} (of {turn:.3e})")
        assert dth <= tol / (2.0 * np.pi) * 2.0 ** 32, (what, m, dth)
        assert dv <= turn and dq <= turn, (what, m, dv, dq)
        sure = np.abs(ref.q[rows] - float(ref.lock_thr)) > turn
        assert np.array_equal(st["locked"][rows][sure], want["locked"][rows][sure]), (what, m)


@pytest.fixture(scope="module")
def series(dev):
    import torch
    z, off = CR.am_carriers(K0, N0)
    return types.SimpleNamespace(z=z, off=off, rx=CR.interleaved_rx(K0), zd=torch.from_numpy(z).to(dev))


@pytest.mark.parametrize("L", [3, 31, 255])
def test_parity_with_the_double_reference(pkg, dev, series, L):
    """K = 1024, n = 3000, modes and loop bandwidths (10 / 30 / 60 Hz) interleaved receiver by receiver: u within the
    measured tolerance of its mode, read()'s theta, freq and err within the phase equivalent of the tolerance, locked
    where the reference's q is not within the tolerance of lock_thr; OFF receivers equal z by uint32 views.  After 3000
    outputs every receiver with a loop is locked and its freq is within 1 Hz of the carrier's offset."""
    ref = CR.CarrierRef(series.rx, CR.hilbert(L), **CR.PARAMS)
    want = ref.process(series.z)
    assert np.abs(ref.e).max() < CR.E_MAX
    modes = [r[0] for r in series.rx]
    got = run(pkg, series.zd, series.rx, L)
    close_to(got, want, ref, modes, series.z, f"L {L}")
    on = np.array(modes) != CR.OFF
    st = got[1]
    assert st["locked"][on].all() and np.abs(st["freq"][on].astype(np.float64) * CR.RATE / 2.0 - series.off[on]).max() < 1.0
    assert not st["theta"][~on].any() and not st["freq"][~on].any() and not st["err"][~on].any() and st["locked"][~on].all()


@pytest.mark.parametrize("L", [31, 255])
def test_bits_against_the_cut_and_the_company(pkg, dev, series, L):
    """One batch against batches of 0, 1, 2, L - 1, L, TT - 1, TT, TT + 1, 3 TT + 5 and the rest, for K = group - 1, group,
    group + 1, 7, 1 and 1024; the receiver order reversed; a receiver alone against itself among the 1024; in place
    against out of place; strides larger than n, the padding keeps its fill.  u and the status by uint32 views."""
    import torch
    TT, G = pkg.carrier_tile_outputs(), pkg.carrier_group()
    cuts = [0, 1, 2, L - 1, L, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(N0 - sum(cuts))
    assert cuts[-1] > 0
    z, rx = series.zd, series.rx
    one = run(pkg, z, rx, L)
    pick = lambda r, rows: (r[0][rows], r[1][rows])
    same(run(pkg, z, rx, L, cuts), one, "cut")
    same(run(pkg, z.flip(0).contiguous(), rx[::-1], L, cuts[::-1]), pick(one, slice(None, None, -1)), "reversed")
    for K in (G - 1, G, G + 1, 7):
        rows = slice(500, 500 + K)
        same(run(pkg, z[rows].contiguous(), rx[rows], L, cuts), pick(one, rows), f"K {K}")
    for j in (0, 1, G - 1, G, 1023):
        same(run(pkg, z[j:j + 1].contiguous(), rx[j:j + 1], L, cuts), pick(one, slice(j, j + 1)), f"alone {j}")
    # in place, and strides larger than n
    K = 2 * G + 3
    rows = slice(200, 200 + K)
    zbuf = torch.full((K, N0 + 37), 3.0 + 0j, dtype=torch.complex64, device=dev)
    zbuf[:, :N0] = z[rows]
    obuf = torch.full((K, N0 + 11), 7.0 + 0j, dtype=torch.complex64, device=dev)
    c = make(pkg, rx[rows], L)
    off = 0
    for b in cuts:
        o = c.process(zbuf[:, off:off + b], out=obuf[:, off:])
        assert o.data_ptr() == obuf[:, off:].data_ptr() or b == 0
        off += b
    same((obuf[:, :N0].cpu().numpy(), c.read()), pick(one, rows), "strided")
    assert bool((obuf[:, N0:] == 7.0).all()) and bool((zbuf[:, N0:] == 3.0).all())
    assert np.array_equal(CR.bits(zbuf[:, :N0].cpu().numpy()), CR.bits(series.z[rows]))
    c.reset()
    off = 0
    for b in cuts:
        v = zbuf[:, off:off + b]
        o = c.process(v, out=v)
        assert o.data_ptr() == v.data_ptr()
        off += b
    same((zbuf[:, :N0].cpu().numpy(), c.read()), pick(one, rows), "in place")
    assert bool((zbuf[:, N0:] == 3.0).all())
    c.close()


def test_set_rx_between_batches(pkg, dev, series):
    """Gains and modes changed on some receivers between the batches, against the streaming double reference (whose |e|
    stays below 0.75 through every restart).  kp / ki alone leave no gap: the first output behind the change has the
    bits of the run without it.  Another mode starts fresh: from there on the receiver has the bits of one created
    then.  The receivers that were not touched have the bits of a run without the changes; a bad call is refused and
    changes nothing."""
    K, L = 12, 31
    cuts = [700, 1, 999, 1300]
    rows = slice(100, 100 + K)
    rx = series.rx[rows]
    assert [r[0] for r in rx] == [CR.OFF, CR.DSB, CR.USB, CR.LSB] * 3
    z, zn = series.zd[rows].contiguous(), series.z[rows]
    g10, g30, g60 = (CR.loop_gains(b) for b in CR.BANDWIDTHS)
    changes = {1: [(1, CR.LSB) + g30, (2, CR.USB) + g60, (7, CR.OFF) + g60, (10, CR.DSB) + g10],
               2: [(8, CR.USB) + g30],
               3: [(7, CR.LSB) + g60, (2, CR.USB) + g30, (4, CR.DSB) + g60, (1, CR.DSB) + g30]}
    nan = float("nan")
    bad = ((1, 4) + g30, (1, -1) + g30, (1, CR.DSB, 0.0, 0.01), (1, CR.DSB, 0.6, 0.01), (1, CR.DSB, nan, 0.01),
           (1, CR.DSB, 0.1, -0.01), (1, CR.DSB, 0.1, 0.26), (1, CR.DSB, 0.1, nan), (K, CR.DSB) + g30, (-1, CR.DSB) + g30)

    def before(i, c):
        for ch in changes.get(i, ()):
            c.set_rx(*ch)
        for b in bad:
            with pytest.raises(pkg.PddcError) as e:
                c.set_rx(*b)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, z, rx, L, cuts, before)
    clean = run(pkg, z, rx, L, cuts)
    touched = {ch[0] for cs in changes.values() for ch in cs}
    for j in range(K):
        if j not in touched:
            same((got[0][j:j + 1], got[1][j:j + 1]), (clean[0][j:j + 1], clean[1][j:j + 1]), f"untouched {j}")
    # the gains alone: receiver 2 ahead of batch 1 (output 700) and of batch 3 (output 1700)
    assert np.array_equal(CR.bits(got[0][2, :701]), CR.bits(clean[0][2, :701]))
    assert not np.array_equal(CR.bits(got[0][2, 701:760]), CR.bits(clean[0][2, 701:760]))
    # another mode: receiver 10 is a DSB receiver created at output 700, receiver 8 a USB one created at 701
    for j, at, r in ((10, 700, (CR.DSB,) + g10), (8, 701, (CR.USB,) + g30)):
        alone = run(pkg, z[j:j + 1, at:].contiguous(), [r], L)
        same((got[0][j:j + 1, at:], got[1][j:j + 1]), alone, f"fresh {j}")
    # against the streaming reference, batch by batch with the tolerance of the receiver's mode in that batch
    ref = CR.CarrierRef(rx, CR.hilbert(L), **CR.PARAMS)
    wants, tols, off = [], [], 0
    for i, b in enumerate(cuts):
        for ch in changes.get(i, ()):
            ref.set_rx(*ch)
        wants.append(ref.process(zn[:, off:off + b]))
        assert np.abs(ref.e).max() < CR.E_MAX, i
        tols.append(np.array([CR.TOL_CARRIER[int(m)] for m in ref.mode]))
        off += b
    scale = np.max(np.abs(np.concatenate(wants, axis=1)), axis=1)
    off = 0
    for i, b in enumerate(cuts):
        e = np.max(np.abs(got[0][:, off:off + b].astype(np.complex128) - wants[i]), axis=1) / scale
        print(f"batch {i}: err / TOL {np.round(e / np.maximum(tols[i], 1e-30), 3)}")
        assert np.all(e <= tols[i]), (i, e, tols[i])
        off += b
    close_to(got, None, ref, ref.mode, None, "set_rx")


def test_a_refused_process_changes_nothing(pkg, dev, series):
    """process calls refused for capacity (each stride), for a misaligned or missing pointer and for an overlap of u with
    z that is not in place, between the batches: the next correct call's bits are those of an object that never saw
    them.  reset starts the series again and read() then gives the create values."""
    import torch
    K, L = 9, 31
    cuts = [700, 300, 2000]
    rows = slice(300, 300 + K)
    rx = series.rx[rows]
    z = series.zd[rows].contiguous()
    clean = run(pkg, z, rx, L, cuts)
    lib = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, c):
        b = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            c.process(z[:, :b], out=torch.empty((K, b - 1), dtype=torch.complex64, device=dev))
        assert e.value.code == ECAP
        with pytest.raises(pkg.PddcError) as e:
            c.process(z[:, :b], out=torch.empty((K, b), dtype=torch.float32, device=dev))
        assert e.value.code == -1
        o = torch.empty((K, b), dtype=torch.complex64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(zp=z.data_ptr(), n=b, zs=N0, up=o.data_ptr(), us=b):
            return lib.pddc_carrier_process(c._h, zp, n, zs, up, us, stream)

        assert call(zs=b - 1) == ECAP and call(us=b - 1) == ECAP
        assert call(zp=z.data_ptr() + 4) == EINVAL and call(up=o.data_ptr() + 4) == EINVAL
        assert call(zp=None) == EINVAL and call(up=None) == EINVAL
        assert call(up=z.data_ptr() + 8, us=N0) == EINVAL                   # u over z, shifted
        assert call(up=z.data_ptr(), us=N0 - 1) == EINVAL                   # u is z, another stride
        assert call(zp=None, n=0, zs=0, up=None, us=0) == pkg.PDDC_OK

    same(run(pkg, z, rx, L, cuts, disturb), clean, "refused")
    c = make(pkg, rx, L)
    fresh = c.read()
    assert not fresh["theta"].any() and not fresh["freq"].any() and not fresh["err"].any() and fresh["locked"].all()
    first = c.process(z).cpu().numpy()
    st1 = c.read()
    c.reset()
    again = c.read()
    for name in CR.STATUS.names:
        assert np.array_equal(again[name], fresh[name]), name
    second = c.process(z).cpu().numpy()
    same((second, c.read()), (first, st1), "reset")
    same((first, st1), clean, "one batch")
    c.close()


def test_the_chain(pkg, dev, series):
    """Carrier followed by Demod in PDDC_DEMOD_SSB with word 0 and no flags gives exactly u.re, by uint32 views (DSB, and
    the other modes beside it); once locked, a DSB receiver's u.re is its carrier's envelope and u.im is small against it."""
    K, L = 40, 31
    rows = slice(600, 600 + K)
    rx = series.rx[rows]
    z = series.zd[rows].contiguous()
    c = make(pkg, rx, L)
    d = pkg.Demod([(pkg.PDDC_DEMOD_SSB, 0, 0)] * K)
    u = c.process(z)
    a = d.process(u)
    un, an = u.cpu().numpy(), a.cpu().numpy()
    assert an.dtype == np.float32 and np.array_equal(CR.bits(an), CR.bits(np.ascontiguousarray(un.real)))
    dsb = [j for j in range(K) if rx[j][0] == CR.DSB]
    assert len(dsb) == K // 4
    # the envelope is in u.re and u.im holds what is left of the carrier's phase: small against it once locked
    tail = un[dsb, 1500:]
    assert np.all(np.abs(tail.imag).max(axis=1) < 0.2 * np.abs(tail.real).max(axis=1))
    assert np.all(tail.real.min(axis=1) > 0)
    c.close()
    d.close()


def test_silence(pkg, dev, series):
    """atan2f(0, 0) = 0 on the device: receivers fed zeros (silence, or a receiver behind a blanker) in every mode give
    u = +0 and keep theta, v and q at 0, by uint32 views against the float32 model; and a stage that has seen only zeros
    is a stage just created: the series that follows has the bits of a fresh object's."""
    import torch
    L, n0 = 31, 300
    rx = series.rx[:8]
    zero = np.zeros((8, n0), np.complex64)
    model = CR.CarrierRef(rx, CR.hilbert(L), f32=True, **CR.PARAMS)
    want = model.process(zero)
    assert not CR.bits(want).any() and not model.theta.any() and not model.v.any() and not model.q.any()
    c = make(pkg, rx, L)
    u = c.process(torch.from_numpy(zero).to(dev)).cpu().numpy()
    st = c.read()
    assert u.shape == (8, n0) and not CR.bits(u).any()
    for name in ("theta", "freq", "err"):
        assert not st[name].view(np.uint32).any(), name
    z = series.zd[:8].contiguous()
    after = c.process(z).cpu().numpy()
    same((after, c.read()), run(pkg, z, rx, L), "after silence")
    c.close()
