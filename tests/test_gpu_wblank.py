"""GPU tests of the wideband blanker (pddc_wblank_*, k_wblank_*): every output byte, the trigger and blanked counters and
the reference are those of tests/wblank_ref.py -- exact equality, no tolerances -- whatever the cut into batches and
the samples a workgroup walks."""
import ctypes as C
import functools

import numpy as np
import pytest

import wblank_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small():
    return R.small_stream()[0]


@functools.lru_cache(maxsize=None)
def small_ref(params, thr16=256, on=True):
    return R.wblank_fast(small(), *params, ((0, thr16, on),))


@functools.lru_cache(maxsize=None)
def cut_case(params):
    packed, cuts, edges = R.cut_stream(params)
    return packed, cuts, R.wblank_fast(packed, *params)


def up(packed, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(packed)).to(dev)


def run(pkg, dev, wb, packed, cuts=None, sets=None):
    """the stream through wb in batches of `cuts` samples (one batch without them), sets = {batch index: (thr, on)}
    applied in front of that batch -> the output bytes on the host"""
    import torch
    d = up(packed, dev)
    n = packed.size // 6
    out = torch.empty(6 * n, dtype=torch.uint8, device=dev)
    at = 0
    for k, c in enumerate(cuts if cuts is not None else [n]):
        if sets and k in sets:
            wb.set(*sets[k])
        got = wb.process(d[6 * at:6 * (at + c)], out=out[6 * at:6 * (at + c)])
        assert got.numel() == 6 * c
        at += c
    assert at == n
    return out.cpu().numpy()


def check(wb, got, ref, n):
    st = wb.read()
    assert np.array_equal(got, ref["out"]), np.flatnonzero(got != ref["out"])[:8] // 6
    assert (int(st["triggers"]), int(st["blanked"]), int(st["mean"]), int(st["samples"])) == \
           (ref["triggers"], ref["blanked"], ref["mean"], n)


@pytest.mark.parametrize("params", R.PARAM_SETS[:4])
@pytest.mark.parametrize("thr", R.THRS)
def test_parameter_sets_and_thresholds(pkg, dev, params, thr):
    assert pkg.wblank_tile_samples() == 2048
    wb = pkg.WBlank(*params, thr=thr)
    assert wb.delay == R.delay_of(params[2], params[3])
    ref = small_ref(params, int(thr * 16))
    if thr == 1.0 and params[1] >= 4 and params[0] <= 256:
        assert ref["triggers"] > R.N_SMALL // 4             # neighbourhoods overlap everywhere
    check(wb, run(pkg, dev, wb, small()), ref, R.N_SMALL)
    wb.close()


@pytest.mark.parametrize("params", R.PARAM_SETS[:4])
def test_off_is_the_input_delayed(pkg, dev, params):
    wb = pkg.WBlank(*params, thr=16.0, on=False)
    got = run(pkg, dev, wb, small())
    D = wb.delay
    assert not got[:6 * D].any() and np.array_equal(got[6 * D:], small()[:small().size - 6 * D])
    check(wb, got, small_ref(params, 256, False), R.N_SMALL)
    wb.close()


def test_a_block_longer_than_the_stream_is_the_input_delayed(pkg, dev):
    B, H, W, r = R.PARAM_SETS[4]
    short = small()[:6 * R.N_SHORT]
    assert B > R.N_SHORT
    wb = pkg.WBlank(B, H, W, r, thr=1.0)
    got = run(pkg, dev, wb, short, cuts=[1000, 88, R.N_SHORT - 1088])
    D = wb.delay
    assert not got[:6 * D].any() and np.array_equal(got[6 * D:], short[:short.size - 6 * D])
    check(wb, got, R.wblank_fast(short, B, H, W, r, ((0, 16, True),)), R.N_SHORT)
    wb.close()


@pytest.mark.parametrize("params", R.PARAM_SETS[:4])
@pytest.mark.parametrize("run_tiles", [0, 1, 2, 3])
def test_cuts_and_runs(pkg, dev, tune, params, run_tiles):
    """one batch against the cut list, with impulses on both sides of every cut; wblank_run automatic and forced to one,
    two and three tiles; and the rounds of a batch cut as small as a batch"""
    tile = pkg.wblank_tile_samples()
    tune("wblank_run", run_tiles * tile)
    assert pkg.wblank_run_samples() == max(run_tiles, 1) * tile
    packed, cuts, ref = cut_case(params)
    assert cuts == R.cut_list(R.N_SMALL, R.delay_of(params[2], params[3]), params[0], tile)
    wb = pkg.WBlank(*params)
    check(wb, run(pkg, dev, wb, packed), ref, R.N_SMALL)
    wb.reset()
    check(wb, run(pkg, dev, wb, packed, cuts), ref, R.N_SMALL)
    if run_tiles == 2:
        tune("wblank_chunk", 3 * tile + 8)
        wb.reset()
        check(wb, run(pkg, dev, wb, packed), ref, R.N_SMALL)
    wb.close()


@pytest.mark.parametrize("run_tiles", [0, 2])
def test_a_delay_longer_than_a_block(pkg, dev, tune, run_tiles):
    """D = 255 > B = 64 with triggers at samples 70 and 200: the outputs n < D are made from no input and are not counted
    as blanked, in one batch, with the first D outputs spread over several batches, and under the cut list"""
    params = R.PARAM_DEEP
    D = R.delay_of(params[2], params[3])
    tune("wblank_run", run_tiles * pkg.wblank_tile_samples())
    ref = small_ref(params)
    assert D > params[0] and ref["t"][70] and ref["t"][200]
    wb = pkg.WBlank(*params)
    check(wb, run(pkg, dev, wb, small()), ref, R.N_SMALL)
    wb.reset()
    first = [8, 56, 64, 72, 56, 248, 8]                      # edges at 8, 64, 128, 200, 256 (the first output with an input
    assert sum(first[:5]) == 256 and sum(first[:4]) == 200   # is 255), 504, 512
    check(wb, run(pkg, dev, wb, small(), first + [R.N_SMALL - sum(first)]), ref, R.N_SMALL)
    packed, cuts, cref = cut_case(params)
    wb.reset()
    check(wb, run(pkg, dev, wb, packed, cuts), cref, R.N_SMALL)
    wb.close()


def test_set_between_batches(pkg, dev):
    """thresholds and ON / OFF changed between batches: triggers taken under the old threshold still gate samples of the
    next batch (an impulse on the last sample in front of each change)"""
    params = R.PARAM_SETS[2]
    edges = [10008, 20480, 30000]
    packed, _ = R.small_stream(extra=[e - 1 for e in edges])
    sched = ((0, 256, True), (edges[0], 16 * 4096, True), (edges[1], 64, False), (edges[2], 64, True))
    ref = R.wblank_fast(packed, *params, sched)
    D = R.delay_of(params[2], params[3])
    for e in edges[:2]:
        assert ref["t"][e - 1] and (ref["num"][e:e + D] >= 0).all()
    assert not ref["t"][edges[1]:edges[2]].any() and ref["t"][edges[2]:].any()      # the impulse in front of ON: OFF took it
    wb = pkg.WBlank(*params, thr=16.0)
    cuts = [edges[0], edges[1] - edges[0], edges[2] - edges[1], R.N_SMALL - edges[2]]
    got = run(pkg, dev, wb, packed, cuts, sets={1: (4096.0, True), 2: (4.0, False), 3: (4.0, True)})
    check(wb, got, ref, R.N_SMALL)
    with pytest.raises(pkg.PddcError) as e:
        wb.set(0.5, True)
    assert e.value.code == pkg.PDDC_EINVAL
    assert pkg.ddc_lib().pddc_wblank_set(wb._h, 64, 2) == pkg.PDDC_EINVAL
    wb.close()


def test_extremes(pkg, dev):
    B, H, W, r = R.PARAM_SETS[2]
    n = 16 * B
    wb = pkg.WBlank(B, H, W, r, thr=1.0)
    zeros = np.zeros(6 * n, dtype=np.uint8)
    got = run(pkg, dev, wb, zeros)
    assert not got.any()
    check(wb, got, R.wblank_fast(zeros, B, H, W, r, ((0, 16, True),)), n)
    full = R.full_scale_stream(n, B)
    for thr in (1.0, 4096.0):
        wb.reset()
        wb.set(thr, True)
        ref = R.wblank_fast(full, B, H, W, r, ((0, int(16 * thr), True),))
        assert ref["triggers"] == 0
        check(wb, run(pkg, dev, wb, full, cuts=[5 * B + 8, n - 5 * B - 8]), ref, n)
    # a trigger decision that hangs on 64-bit products: all but one sample a block at full scale, the limit just under
    # their power at thr16 = 16 (every one a trigger) and just over it at thr16 = 17 (none)
    near = R.near_full_scale_stream(n, B)
    for thr16 in (16, 17):
        wb.reset()
        wb.set(thr16 / 16.0, True)
        ref = R.wblank_fast(near, B, H, W, r, ((0, thr16, True),))
        assert ref["triggers"] == (0 if thr16 == 17 else (n - B) - (n - B) // B)
        check(wb, run(pkg, dev, wb, near, cuts=[3 * B + 8, n - 3 * B - 8]), ref, n)
    # a trigger on the last sample of a batch and of the stream
    packed = small()
    cut = 20480
    ext, _ = R.small_stream(extra=[cut - 1])
    ref = R.wblank_fast(ext, B, H, W, r)
    assert ref["t"][cut - 1] and ref["t"][R.N_SMALL - 1] and packed.size == ext.size
    wb.reset()
    wb.set(16.0, True)
    check(wb, run(pkg, dev, wb, ext, cuts=[cut, R.N_SMALL - cut]), ref, R.N_SMALL)
    wb.close()


def test_surroundings_and_a_busy_side_stream(pkg, dev):
    """out between poisoned guard bytes that stay untouched, the input unchanged, and the call on a side stream that is
    still busy when process() returns: nothing waits, nothing is synchronised"""
    import torch
    import stream_order as SO
    params = R.PARAM_SETS[2]
    packed = small()
    n = R.N_SMALL
    side = SO.side_streams(dev)[0]
    d = up(packed, dev)
    G = 4096
    buf = torch.full((6 * n + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
    wb = pkg.WBlank(*params)
    torch.cuda.synchronize()
    gate = SO.occupy(side, dev, 30.0)
    half = 6 * 24000
    wb.process(d[:half], out=buf[G:G + half], stream=side.cuda_stream)
    wb.process(d[half:], out=buf[G + half:G + 6 * n], stream=side.cuda_stream)
    busy = not gate.query()
    side.synchronize()
    st = wb.read(stream=side.cuda_stream)
    assert busy, "the side stream was idle before process() returned: nothing shown"
    got = buf.cpu().numpy()
    ref = small_ref(params)
    assert (got[:G] == 0xA5).all() and (got[G + 6 * n:] == 0xA5).all()
    assert np.array_equal(got[G:G + 6 * n], ref["out"])
    assert np.array_equal(d.cpu().numpy(), packed)
    assert (int(st["triggers"]), int(st["blanked"])) == (ref["triggers"], ref["blanked"])
    wb.close()


def test_refusals_leave_the_stream_alone(pkg, dev):
    import torch
    L = pkg.ddc_lib()
    params = R.PARAM_SETS[2]
    packed = small()
    n = R.N_SMALL
    ref = small_ref(params)
    d = up(packed, dev)
    out = torch.zeros(6 * n + 64, dtype=torch.uint8, device=dev)
    wb = pkg.WBlank(*params)
    st = torch.cuda.current_stream().cuda_stream
    cut = 24000
    wb.process(d[:6 * cut], out=out[:6 * cut])
    EINVAL = pkg.PDDC_EINVAL
    ip, op = d.data_ptr() + 6 * cut, out.data_ptr() + 6 * cut
    m = n - cut
    call = lambda i, k, o: L.pddc_wblank_process(wb._h, i, k, o, st)
    assert call(ip, m, ip) == EINVAL                                   # in place
    assert call(ip, m, ip + 6 * m - 16) == EINVAL                      # one shared chunk
    assert call(ip, m, ip - 6 * m + 16) == EINVAL
    assert call(ip + 2, m - 8, op) == EINVAL and call(ip, m - 8, op + 6) == EINVAL      # misaligned
    assert call(ip, m - 4, op) == EINVAL                               # not a multiple of 8
    assert call(None, m, op) == EINVAL and call(ip, m, None) == EINVAL
    assert b"wblank" in L.pddc_last_error()
    assert call(None, 0, None) == pkg.PDDC_OK
    assert L.pddc_wblank_process(None, ip, m, op, st) == EINVAL
    wb.process(d[6 * cut:], out=out[6 * cut:6 * n])
    check(wb, out[:6 * n].cpu().numpy(), ref, n)
    # reset: the bytes of a fresh object
    wb.reset()
    st0 = wb.read()
    assert (int(st0["triggers"]), int(st0["blanked"]), int(st0["mean"]), int(st0["samples"])) == (0, 0, 0, 0)
    check(wb, run(pkg, dev, wb, packed), ref, n)
    wb.close()


def test_a_larger_batch(pkg, dev):
    """2^22 samples in one batch and in three ragged ones, impulses on the cuts"""
    packed, _ = R.large_stream()
    params = R.PARAM_SETS[2]
    ref = R.wblank_fast(packed, *params)
    wb = pkg.WBlank(*params)
    check(wb, run(pkg, dev, wb, packed), ref, R.N_LARGE)
    wb.reset()
    check(wb, run(pkg, dev, wb, packed, R.large_cuts()), ref, R.N_LARGE)
    wb.close()


def test_chain_into_spectrum_and_channelizer(pkg, dev):
    """WBlank's output goes into Spectrum and Channelizer as it is; on the band scenario the median of Spectrum's sums
    behind WBlank is within 0.1 dB of that of the clean stream"""
    import torch
    clean, dirty = R.band_streams()
    n = clean.size // 6
    wb = pkg.WBlank(256, 8, 4, 3, thr=16.0)
    d_dirty, d_clean = up(dirty, dev), up(clean, dev)
    blanked = wb.process(d_dirty)
    assert np.array_equal(blanked.cpu().numpy(), R.wblank_fast(dirty, 256, 8, 4, 3)["out"])

    def median_db(t):
        sp = pkg.Spectrum(4096)
        nseg = sp.process(t)
        s, _, k = sp.read()
        sp.close()
        assert nseg == k == n // 4096
        return 10 * np.log10(np.median(s.cpu().numpy().astype(np.float64)))

    fc, fd, fb = median_db(d_clean), median_db(d_dirty), median_db(blanked)
    print(f"Spectrum median: clean {fc:.3f} dB, dirty {fd:.3f} dB, behind WBlank {fb:.3f} dB")
    assert abs(fb - fc) <= 0.1
    assert fd - fc >= 20.0
    ch = pkg.Channelizer(1024, pkg.channelizer_prototype(1024, 4))
    rows = ch.process(blanked)
    assert rows.shape[0] == pkg.channelizer_rows(1024, 1024, 4096, 0, n) and rows.shape[1] == 1024
    assert torch.isfinite(torch.view_as_real(rows)).all()
    ch.close()
    wb.close()
