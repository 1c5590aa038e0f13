"""Denoise (pddc_denoise_*, k_denoise) on the GPU: against the double reference (tests/denoise_ref.py) within TOL_DENOISE
-- 8 x the error of the independent float32 model on these very inputs, re-measured by tests/test_denoise_cpu.py -- and
bit for bit against itself under every cut, order and company.  n = 3000 everywhere; rows are noise plus keyed tones at
levels spread over 70 dB with modes and (beta, gmin, alpha) interleaved row by row, one row of zeros and one that goes
silent after 1000 samples."""
import functools
import types

import numpy as np
import pytest

import denoise_ref as R
import tuner_ref as TR

pytestmark = pytest.mark.gpu

N = R.N_GPU
SIZES = [pytest.param(nfft, hop, K, id=f"{nfft}-{hop}-{K}") for nfft, hop, K in R.SIZES]
BIT_SIZES = [pytest.param(256, 128, 1024, id="256-128-1024"), pytest.param(1024, 256, 37, id="1024-256-37")]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("out", "noise")):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, (what, name, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, np.argwhere(bits(g) != bits(w))[:4].tolist())


def within(got, ref, what=""):
    for g, r, name in zip(got, ref, ("out", "noise")):
        e = R.metric(g, r)
        print(f"denoise {what} {name}: {e:.3g} (tolerance {R.TOL_DENOISE:.3g})")
        assert np.all(np.isfinite(g)) and e <= R.TOL_DENOISE, (what, name, e)


@functools.lru_cache(maxsize=None)
def inputs(K):
    return R.rows(K), R.receivers(K)


@functools.lru_cache(maxsize=None)
def reference(nfft, hop, K, with_changes=False):
    x, rx = inputs(K)
    return R.oneshot(x, nfft, hop, R.window(nfft, hop), rx, R.changes(K) if with_changes else ())


def run(pkg, xd, rx, nfft, hop, sizes=None, events=(), before=None):
    """xd (torch [K, n]) through a fresh Denoise in the given batches, the set_rx calls of `events` (position, j, ...) in
    front of the batch that begins at their position -> numpy (out, noise)"""
    import torch
    s = pkg.Denoise(rx, nfft, hop, window=R.window(nfft, hop))
    n = xd.shape[1]
    sizes = [n] if sizes is None else sizes
    assert sum(sizes) == n
    pending = sorted(events, key=lambda e: e[0])
    outs, at = [], 0
    for i, b in enumerate(sizes):
        while pending and pending[0][0] == at:
            s.set_rx(*pending.pop(0)[1:])
        if before:
            before(i, s)
        outs.append(s.process(xd[:, at:at + b]).clone())
        at += b
    assert not pending, "a set_rx falls between batches"
    got = torch.cat(outs, dim=1).cpu().numpy(), s.read_noise()
    s.close()
    return got


@pytest.fixture(scope="module")
def dev_rows(dev):
    import torch
    return {K: torch.from_numpy(inputs(K)[0]).to(dev) for K in (1024, 37)}


@pytest.mark.parametrize("nfft,hop,K", SIZES)
def test_against_the_reference(pkg, dev, dev_rows, nfft, hop, K):
    x, rx = inputs(K)
    got = run(pkg, dev_rows[K], rx, nfft, hop)
    ref = reference(nfft, hop, K)
    within(got, ref, f"{nfft}/{hop} K={K}")
    assert not np.any(got[0][R.ZERO_ROW]) and not np.any(got[1][R.ZERO_ROW])
    assert not np.any(got[0][:, :nfft]) and pkg.denoise_delay(nfft) == nfft
    assert np.any(got[0][R.SILENT_ROW]) and not np.any(got[0][R.SILENT_ROW, 1000 + 2 * nfft:])


@pytest.mark.parametrize("nfft,hop,K", BIT_SIZES)
def test_bits_against_the_cut_and_the_company(pkg, dev, dev_rows, nfft, hop, K):
    """One batch against batches of 0, 1, 2, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, tile_frames hop -+ 1,
    3 nfft + 5 and the rest (in as many runs as n = 3000 needs: denoise_ref.cut_runs); the receivers in reversed order;
    7 rows and 1 row alone against the same rows among the many."""
    x, rx = inputs(K)
    xd = dev_rows[K]
    whole = run(pkg, xd, rx, nfft, hop)
    assert np.any(whole[0]) and np.all(np.isfinite(whole[0]))
    for sizes in R.cut_runs(nfft, hop, pkg.denoise_tile_frames()):
        same(run(pkg, xd, rx, nfft, hop, sizes), whole, f"cut {sizes}")
    back = run(pkg, xd.flip(0).contiguous(), rx[::-1], nfft, hop)
    same((back[0][::-1], back[1][::-1]), whole, "reversed")
    for lo, cnt in ((K // 2 - 2, 7), (3, 1), (K - 1, 1), (R.ZERO_ROW, 1)):
        sl = slice(lo, lo + cnt)
        few = run(pkg, xd[sl].contiguous(), rx[sl], nfft, hop, [1000, 2000])
        same(few, (whole[0][sl], whole[1][sl]), f"rows {lo} .. {lo + cnt - 1} alone")


@pytest.mark.parametrize("nfft,hop,K", BIT_SIZES)
def test_set_rx_between_batches(pkg, dev, dev_rows, nfft, hop, K):
    """Mode, parameters, HOLD and RESTART between batches: against the streaming reference, and bit-identical under a
    second, different cut with the calls at the same sample positions; a bad call is refused and changes nothing."""
    x, rx = inputs(K)
    xd = dev_rows[K]
    ev = R.changes(K)
    cuts = list(R.CHANGE_POSITIONS)
    sizes = list(np.diff([0] + cuts + [N]))
    nan, inf = float("nan"), float("inf")
    bad = ((1, 2, 2.0, 0.1, 0.98, 0), (1, 1, 0.0, 0.1, 0.98, 0), (1, 1, nan, 0.1, 0.98, 0), (1, 1, inf, 0.1, 0.98, 0),
           (1, 1, 2.0, -0.1, 0.98, 0), (1, 1, 2.0, 1.5, 0.98, 0), (1, 1, 2.0, nan, 0.98, 0), (1, 1, 2.0, 0.1, 1.0, 0),
           (1, 1, 2.0, 0.1, -0.5, 0), (1, 1, 2.0, 0.1, nan, 0), (1, 1, 2.0, 0.1, 0.98, 4), (K, 1, 2.0, 0.1, 0.98, 0),
           (-1, 1, 2.0, 0.1, 0.98, 0))

    def before(i, s):
        for b in bad:
            with pytest.raises(pkg.PddcError) as e:
                s.set_rx(*b)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, xd, rx, nfft, hop, sizes, ev, before=before)
    ref, Nref = R.stream_with_changes(K, x, nfft, hop, R.window(nfft, hop), rx, ev, cuts)
    assert np.array_equal(ref, reference(nfft, hop, K, True)[0])
    within(got, (ref, Nref), f"set_rx {nfft}/{hop}")
    plain = reference(nfft, hop, K)[0]
    assert R.metric(got[0], plain) > 100 * R.TOL_DENOISE          # the calls did something
    cuts2 = sorted(set(cuts) | {1, 699, 1101, 1500 + hop, 1500 + hop + 1, 2999})
    same(run(pkg, xd, rx, nfft, hop, list(np.diff([0] + cuts2 + [N])), ev), got, "second cut")


def test_strides_and_the_demod_view(pkg, dev):
    """The input is the view Demod.process returns behind a small Tuner, in a buffer of capacity > n (row stride > n); out
    with capacity > n; both paddings keep their fill; the bits are those of the contiguous copy."""
    import torch
    M, hop, T, Rd, K, S = 1024, 512, 64, 4, 13, 6200
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((S, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, Rd), Rd)
    z = t.process(rows)
    n = z.shape[1]
    d = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, pkg.PDDC_DEMOD_DCBLOCK)] * K)
    abuf = torch.full((K, n + 5), 3.0, dtype=torch.float32, device=dev)
    av = d.process(z, out=abuf)
    assert av.data_ptr() == abuf.data_ptr() and av.stride(0) == n + 5 > n > 1400
    rx = R.receivers(K)
    xin = av.cpu().numpy()
    for nfft, dh in ((256, 64), (512, 256)):
        ref = R.oneshot(xin, nfft, dh, R.window(nfft, dh), rx)
        s = pkg.Denoise(rx, nfft, dh, window=R.window(nfft, dh))
        obuf = torch.full((K, n + 11), 7.0, dtype=torch.float32, device=dev)
        out = s.process(av, out=obuf)
        assert out.data_ptr() == obuf.data_ptr() and out.shape == (K, n)
        got = out.cpu().numpy(), s.read_noise()
        within(got, ref, f"strided {nfft}/{dh}")
        assert bool((obuf[:, n:] == 7.0).all()) and bool((abuf[:, n:] == 3.0).all())
        assert np.array_equal(bits(av.cpu().numpy()), bits(xin))
        s.close()
        same(run(pkg, torch.from_numpy(xin).to(dev), rx, nfft, dh, [n // 3, n - n // 3]), got, "contiguous")
    d.close()
    t.close()


def test_a_refused_process_changes_nothing(pkg, dev, dev_rows):
    """process calls refused for capacity (each stride), for a misaligned or missing pointer and for any overlap of out
    with x (in place included), between the batches: the next correct call's bits are those of an object that never saw
    them.  reset starts the series again with the first run's bits; read_noise is zeros before the first frame."""
    import torch
    nfft, hop, K = 256, 64, 9
    sizes = [700, 300, 2000]
    rows = slice(300, 300 + K)
    x, rx = inputs(1024)
    rx = rx[rows]
    xd = dev_rows[1024][rows].contiguous()
    clean = run(pkg, xd, rx, nfft, hop, sizes)
    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, s):
        b = sizes[i]
        with pytest.raises(pkg.PddcError) as e:
            s.process(xd[:, :b], out=torch.empty((K, b - 1), dtype=torch.float32, device=dev))
        assert e.value.code == ECAP
        o = torch.empty((K, b), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(xp=xd.data_ptr(), n=b, xs=N, op=o.data_ptr(), os_=b):
            return L.pddc_denoise_process(s._h, xp, n, xs, op, os_, stream)

        assert call(xs=b - 1) == ECAP and call(os_=b - 1) == ECAP
        assert call(xp=xd.data_ptr() + 2) == EINVAL and call(op=o.data_ptr() + 1) == EINVAL
        assert call(xp=None) == EINVAL and call(op=None) == EINVAL
        assert call(op=xd.data_ptr(), os_=N) == EINVAL                                           # in place is not offered
        assert call(op=xd.data_ptr() + 4, os_=N) == EINVAL                                       # out over x, shifted
        assert call(op=xd.data_ptr() + 4 * (N * (K - 1) + b - 1), os_=b) == EINVAL               # out's first value is x's last
        assert call(xp=None, n=0, xs=0, op=None, os_=0) == pkg.PDDC_OK
        assert L.pddc_denoise_read_noise(s._h, None, stream) == EINVAL

    same(run(pkg, xd, rx, nfft, hop, sizes, before=disturb), clean, "refused")
    s = pkg.Denoise(rx, nfft, hop, window=R.window(nfft, hop))
    assert not bits(s.read_noise()).any()
    s.process(xd[:, :hop - 1])
    assert not bits(s.read_noise()).any()                       # no frame yet
    s.reset()
    first = s.process(xd).clone()
    n1 = s.read_noise()
    s.reset()
    assert not bits(s.read_noise()).any()
    second = s.process(xd)
    same((first.cpu().numpy(), n1), clean, "first")
    same((second.cpu().numpy(), s.read_noise()), clean, "after reset")
    s.close()
