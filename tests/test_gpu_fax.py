"""Fax (pddc_fax_*, k_fax) on the GPU against the numpy reference in double (tests/fax_ref.py).
disc, f of every sample: within fax_ref.TOL_FAX, 7 x the float32 model's worst case on the parity test's very inputs
(tests/test_fax_cpu.py), never taken from k_fax.  npix, counts and every record's start: exactly the reference's, they are
functions of inc and m alone.  Every pixel between the roundings of the reference's g -+ |scale| TOL_FAX.  Crossings,
white, flags, run and the integer status: exactly fax_ref.lines_from_pixels of the device's own pixels.  Against itself every
output has the same bytes however the series is cut: no tolerance, no exclusions."""
import types

import numpy as np
import pytest

import fax_ref as R
import stream_order as S
import tuner_ref as TR

pytestmark = pytest.mark.gpu

FILL_I, FILL_P, FILL_F = 0x5A5A5A5A, 0xC3, -5.0


def gather(pkg, out):
    """the device's (pix, npix, lines, counts) -> (one pixel array, one LINE array per receiver)"""
    pix, npix, lines, counts = (t.cpu().numpy() for t in out[:4])
    rec = lines.view(pkg.fax_line_dtype())[..., 0]
    assert (npix >= 0).all() and (npix <= pix.shape[1]).all() and (counts >= 0).all() and (counts <= rec.shape[1]).all()
    return [pix[j, :npix[j]].copy() for j in range(pix.shape[0])], [rec[j, :counts[j]].copy() for j in range(rec.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Fax in the given batches -> (pixels per receiver,
    LINE records per receiver, disc float32 [nrx, n], status); before(i, f) is called ahead of batch i; pad > 0: pix, lines
    and disc are views of filled tensors whose rows lie further apart than the batch needs, and what lies behind a row's
    pixels, records and samples must keep the fill"""
    import torch
    f = pkg.Fax(bank, sel, W)
    nrx = z.shape[0]
    px, ln, ds, off = [[] for _ in range(nrx)], [[] for _ in range(nrx)], [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        pcap, lcap = f.max_pixels(b), f.max_lines(b)
        assert pcap == R.max_pixels(bank, b) and lcap == R.max_lines(bank, b)
        kw = {}
        if pad:
            kw = dict(pix=torch.full((nrx, pcap + pad), FILL_P, dtype=torch.uint8, device=z.device),
                      lines=torch.full((nrx, lcap + pad, 4), FILL_I, dtype=torch.int32, device=z.device),
                      disc=torch.full((nrx, b + pad), FILL_F, dtype=torch.float32, device=z.device))
        out = f.process(z[:, off:off + b], want_disc=True, **kw)
        assert out[1].shape == (nrx,) and out[3].shape == (nrx,) and out[0].dtype == torch.uint8
        if pad:
            p, k, l, c, d = (t.cpu().numpy() for t in out)
            for j in range(nrx):
                assert (p[j, k[j]:] == FILL_P).all() and (l[j, c[j]:] == FILL_I).all() and (d[j, b:] == FILL_F).all(), (i, j)
        pj, lj = gather(pkg, out)
        for j in range(nrx):
            px[j].append(pj[j])
            ln[j].append(lj[j])
        ds.append(out[4].cpu().numpy()[:, :b])
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in px], [np.concatenate(q) for q in ln], np.concatenate(ds, axis=1), st


def same_bits(a, b, rows=None):
    """two results of run() by their bytes (on `rows` of disc: an OFF receiver's row is not written)"""
    da, db = (a[2], b[2]) if rows is None else (a[2][rows], b[2][rows])
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and da.tobytes() == db.tobytes()
            and a[3].tobytes() == b[3].tobytes())


def against_reference(got, ref, bank, sel, what, rows=None, carried=None):
    """the module header's comparisons for every receiver in `rows` (all of them unless given); `carried`: per receiver
    the line state in front of the device's pixels, for lines_from_pixels (fresh unless given)"""
    px, ln, disc, st = got
    rpix, rlines, rdisc, rg, rwhere, rst = ref
    rows = range(len(px)) if rows is None else rows
    worst, edge = 0.0, 0
    for j in rows:
        modem = bank[sel[j][0]]
        assert px[j].shape == rpix[j].shape and ln[j].shape == rlines[j].shape, (what, j, px[j].shape, rpix[j].shape, ln[j].shape, rlines[j].shape)
        assert np.array_equal(ln[j]["start"], rlines[j]["start"]), (what, j)
        worst = max(worst, float(np.abs(disc[j].astype(np.float64) - rdisc[j]).max()))
        lo, hi = R.pixel_bounds(rg[j], modem[4])
        p = px[j].astype(np.int64)
        bad = np.flatnonzero((p < lo) | (p > hi))
        assert bad.size == 0, (what, j, bad[:4], p[bad[:4]], rg[j][bad[:4]])
        edge += int((p != rpix[j]).sum())
        own, state = R.lines_from_pixels(px[j], rwhere[j], modem, None if carried is None else carried[j])
        for k in ("crossings", "white", "flags", "run"):
            assert np.array_equal(ln[j][k], own[k]), (what, j, k, ln[j], own)
        for k in ("acc", "col", "lines", "pixels"):
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        if carried is None:
            assert st["images"][j] == state["images"] and st["active"][j] == state["active"], (what, j)
        assert abs(float(st["f_last"][j]) - float(rst["f_last"][j])) <= R.TOL_FAX, (what, j)
    print(f"{what}: |disc - ref| {worst:.2e} (TOL_FAX {R.TOL_FAX:.2e}), {edge} pixels on the other side of a rounding edge, {len(rows)} receivers")
    assert worst <= R.TOL_FAX, (what, worst)


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = R.case(W, key[1])
        _REFS[key] = R.run_cuts(R.FaxRef(bank, sel, W), z)
    return tuple(x[:nrx] for x in _REFS[key])


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """fax_ref.case(W, nrx) for W = 1, 2, 16, 255, 256 (1024 receivers: 16, 255, 256), one batch of 4096 samples: start
    tone, phasing, grey wedges and bars and stop tone over and over at widths 64 and 100, 2.5 .. 4 samples per pixel
    and inc = 2^31, boxcars of 1, 3 and 16, noise 20 dB down, every fifth receiver REVERSE on a mirrored signal.  Every
    receiver is compared; every one has ended 13 lines or more and the device has seen images begin and end."""
    import torch
    for W in (R.BIG_WINDOWS if nrx == 1024 else R.WINDOWS):
        bank, sel, z = R.case(W, nrx)
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, parity_ref(W, nrx), bank, sel, f"nrx {nrx} W {W}")
        assert all(len(got[1][j]) >= 13 for j in range(nrx)) and got[3]["images"].sum() >= nrx
        assert all(got[3]["lines"][j] == len(got[1][j]) and got[3]["pixels"][j] == len(got[0][j]) for j in range(nrx))


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of fax_ref.cut_lists (batches of 0 and 1, cuts on and beside the
    kernel's tile seams, forty batches of one sample, cuts just before, on and behind a strobe and a line's last pixel):
    pixels, records, disc and status have the same bytes.  A receiver's bytes are the same alone, among the nine and as
    receiver 1000 of 1024, and with input, pix, lines and disc rows further apart than the batch needs (odd pixel
    capacities, so the rows begin at every alignment), the padding untouched."""
    import torch
    bank, sel, z = R.case(W, 9)
    n, TT = z.shape[1], pkg.fax_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    against_reference(one, parity_ref(W, 9), bank, sel, f"W {W}")
    lists = R.cut_lists(n, TT, *R.events(bank, sel[:1], W, z[:1]))
    for cuts in lists:
        assert same_bits(run(pkg, zd, bank, sel, W, cuts), one), cuts
    for j in (2, 8):
        alone = run(pkg, zd[j:j + 1], bank, [sel[j]], W, lists[1])
        assert all(alone[k][0].tobytes() == one[k][j].tobytes() for k in range(4)), j
    big, bsel, bz = R.case(W, 1024)
    bz = bz.copy()
    bz[1000] = z[2]
    bsel = list(bsel)
    bsel[1000] = sel[2]
    crowd = run(pkg, torch.from_numpy(bz).to(dev), big, bsel, W, lists[0])
    assert all(crowd[k][1000].tobytes() == one[k][2].tobytes() for k in range(4))
    wide = torch.zeros((9, n + 13), dtype=torch.complex64, device=dev)
    wide[:, :n] = zd
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    assert same_bits(run(pkg, view, bank, sel, W, lists[0], pad=7), one)
    assert same_bits(run(pkg, view, bank, sel, W, pad=3), one)


def test_tile_seams(pkg, dev):
    """5 receivers (a ragged last group), W = 16, series of 255, 256, 257, 511 and 513 samples against the reference, the
    longest cut in two at TT - 1 and at TT with the same bytes; and one receiver whose inc puts a strobe on the last
    sample of a tile (inc = 2^24: samples 255 and 511) and on the first sample of one (inc = ceil(2^32 / 257): sample
    256)."""
    import torch
    TT, W = pkg.fax_tile_outputs(), 16
    assert TT == 256
    bank, sel, z = R.case(W, 5)
    for n in (TT - 1, TT, TT + 1, 2 * TT - 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(z[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel, W)
        against_reference(one, R.run_cuts(R.FaxRef(bank, sel, W), z[:, :n]), bank, sel, f"{n} samples")
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert same_bits(run(pkg, zd, bank, sel, W, [cut, n - cut]), one), cut
    x = z[:1, :2 * TT + 1]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for inc, at in ((1 << 24, [255, 511]), (-(-(1 << 32) // 257), [256])):
        bank1 = [bank[0][:1] + (inc,) + bank[0][2:]]
        got = run(pkg, xd, bank1, [(0, R.ON)], W, pad=2)
        ref = R.run_cuts(R.FaxRef(bank1, [(0, R.ON)], W), x)
        assert list(ref[4][0]) == at and len(got[0][0]) == len(at)
        against_reference(got, ref, bank1, [(0, R.ON)], f"inc {inc}")
        assert same_bits(run(pkg, xd, bank1, [(0, R.ON)], W, [TT - 1, 1, 1, TT]), got)


# ---- receiver control --------------------------------------------------------------------------------------------------

def control_case():
    """8 receivers of the parity series on modem 0 (width 64, 2.5 samples per pixel: a line is 160 samples), W = 16, a bank
    of two modems (the second modem 2 of bank16: another inc, boxcar and width 64), three batches of 1500, 1000 and
    the remaining samples: both cuts lie inside a line.  Receiver 0 runs undisturbed; 1 is OFF throughout and its input
    row is NaN; 2 is OFF in the first batch and ON from the second; 3 is restarted in front of the second batch; 4 goes
    to the other modem in front of the third batch and 5 is switched OFF there; 6 is on the second modem from the start; 7
    becomes REVERSE in front of the second batch and plain again in front of the third."""
    full = R.bank16(16)
    bank = [full[0], full[2]]
    sel = [(0, R.ON), (0, 0), (0, 0), (0, R.ON), (0, R.ON), (0, R.ON), (1, R.ON), (0, R.ON)]
    z = np.stack([R.parity_row(j, bank[sel[j][0]], 71000 + j) for j in range(8)])
    z[1] = complex(np.nan, np.nan)

    def changes(at_b, at_c):
        def before(i, f):
            if i == at_b:
                f.set_rx(2, 0, R.ON)
                f.set_rx(3, 0, R.ON | R.RESTART)
                f.set_rx(7, 0, R.ON | R.REVERSE)
            if i == at_c:
                f.set_rx(4, 1, R.ON)
                f.set_rx(5, 0, 0)
                f.set_rx(7, 0, R.ON)
        return before
    return bank, sel, z, changes


def test_receiver_control(pkg, dev):
    """control_case against the reference given the same changes: disc, counts, starts and pixels of every ON receiver as
    in the parity test, records and integer status exactly the reference's (its pixels are the device's wherever no g
    lies on a rounding edge, and the test says how many did).  The OFF receiver's NaN row is never read.  read() between
    set_rx and the next batch shows what the next batch will find (RESTART: active, acc, col and f_last 0; another modem:
    active and col 0, acc and f_last kept) and the counters as they were.  Another cut with the same change points: the
    same bytes.  reset() gives the outputs of a fresh object."""
    import torch
    bank, sel, z, changes = control_case()
    W, n = 16, z.shape[1]
    cuts = [1500, 1000, n - 2500]
    ref = R.run_cuts(R.FaxRef(bank, sel, W), z, cuts, before=changes(1, 2))
    zd = torch.from_numpy(z).to(dev)
    on = [0, 2, 3, 4, 5, 6, 7]
    seen = {}

    def watched(i, f):
        before_change = f.read() if i in (1, 2) else None
        changes(1, 2)(i, f)
        if i in (1, 2):
            seen[i] = (before_change, f.read())
    got = run(pkg, zd, bank, sel, W, cuts, before=watched)
    px, ln, disc, st = got
    worst = 0.0
    for j in on:
        assert px[j].shape == ref[0][j].shape and np.array_equal(ln[j]["start"], ref[1][j]["start"]), j
        lo, hi = R.pixel_bounds(ref[3][j], bank[0][4])
        assert ((px[j] >= lo) & (px[j] <= hi)).all(), j
        if np.array_equal(px[j], ref[0][j]):
            assert ln[j].tobytes() == ref[1][j].tobytes(), j
            assert all(st[k][j] == ref[5][k][j] for k in R.INT_STATUS), j
        live = disc[j][np.abs(ref[2][j]) > 0] if j in (2, 5) else disc[j]
        want = ref[2][j][np.abs(ref[2][j]) > 0] if j in (2, 5) else ref[2][j]
        worst = max(worst, float(np.abs(live.astype(np.float64) - want).max()))
    same = sum(np.array_equal(px[j], ref[0][j]) for j in on)
    print(f"control: |disc - ref| {worst:.2e}, {same} of {len(on)} receivers with the reference's very pixels")
    assert worst <= R.TOL_FAX and same >= 4
    assert px[1].size == 0 and ln[1].size == 0 and not st[1:2].view(np.uint8).any()
    counters = ("lines", "pixels", "images")
    was, now = seen[1]
    assert was["acc"][3] != 0 and was["col"][3] != 0 and was["lines"][3] > 5 and was["f_last"][3] != 0
    assert now["active"][3] == 0 and now["acc"][3] == 0 and now["col"][3] == 0 and now["f_last"][3] == 0
    assert all(now[k][3] == was[k][3] for k in counters)
    assert now[[0, 4, 5, 6, 7]].tobytes() == was[[0, 4, 5, 6, 7]].tobytes()
    was, now = seen[2]
    assert was["col"][4] != 0 and now["col"][4] == 0 and now["active"][4] == 0 and now["acc"][4] == was["acc"][4] != 0
    assert now["f_last"][4] == was["f_last"][4] and all(now[k][4] == was[k][4] for k in counters)
    assert ln[2].size and ln[2]["start"].min() >= cuts[0] and st["pixels"][2] == len(px[2]) < len(px[0])
    fresh = run(pkg, zd[2:3, cuts[0]:], bank, [(0, R.ON)], W)
    assert fresh[0][0].tobytes() == px[2].tobytes() and np.array_equal(fresh[1][0]["start"] + np.uint64(cuts[0]), ln[2]["start"])
    a, b, c = cuts
    other = run(pkg, zd, bank, sel, W, [1, a - 1, 0, 63, b - 63, 30, c - 30], before=changes(3, 5))
    assert same_bits(other, got, rows=[0, 3, 4, 6, 7])
    f = pkg.Fax(bank, sel, W)
    fresh_read = f.read()
    assert not fresh_read.view(np.uint8).any()
    first = gather(pkg, f.process(zd[:, :700]))
    f.reset()
    assert f.read().tobytes() == fresh_read.tobytes()
    again = gather(pkg, f.process(zd[:, :700]))
    assert all(x.tobytes() == y.tobytes() for k in range(2) for x, y in zip(first[k], again[k]))
    f.close()


def test_a_refused_call_queues_nothing(pkg, dev):
    """Between the batches of a run: a pix_stride and a line_stride below their bounds, a z_stride and a disc_stride below
    n (PDDC_ECAPACITY), through Python and through the C ABI; misaligned and NULL pointers, a disc and a pix inside z's
    rows (PDDC_EINVAL); a bad set_rx.  Nothing is written (the outputs keep their fill), and the next good batch gives the
    bytes of an undisturbed run.  n = 0 sets npix and counts to 0.  create refuses overlapping tone ranges, a width of
    15, a boxcar of 17, inc = 0 and inc above 2^31, and need = 0."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = R.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 1500, n - 1800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        pcap, lcap = f.max_pixels(b), f.max_lines(b)
        assert pcap == ((b * (1 << 31) - 1) >> 32) + 1 and lcap == (pcap - 1) // 64 + 1
        pix = torch.full((nrx, pcap), FILL_P, dtype=torch.uint8, device=dev)
        lines = torch.full((nrx, lcap, 4), FILL_I, dtype=torch.int32, device=dev)
        npix = torch.full((nrx,), FILL_I, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), FILL_I, dtype=torch.int32, device=dev)
        disc = torch.full((nrx, b), FILL_F, dtype=torch.float32, device=dev)
        for kw in (dict(pix=pix[:, :pcap - 1]), dict(lines=lines[:, :lcap - 1]), dict(disc=disc[:, :b - 1])):
            with pytest.raises(pkg.PddcError) as e:
                f.process(zd[:, :b], **dict(dict(pix=pix, npix=npix, lines=lines, counts=counts), **kw))
            assert e.value.code == pkg.PDDC_ECAPACITY, kw.keys()
        for rx, modem, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, 16, 1), (0, 0, 8), (0, 0, 0x100)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, modem, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        st = torch.cuda.current_stream().cuda_stream
        q = dict(z=zd.data_ptr(), p=pix.data_ptr(), k=npix.data_ptr(), l=lines.data_ptr(), c=counts.data_ptr(), d=disc.data_ptr())

        def call(**kw):
            a = dict(q, n=b, zs=n, ps=pcap, ls=lcap, ds=b)
            a.update(kw)
            return lib.pddc_fax_process(f._h, a["z"], a["n"], a["zs"], a["p"], a["ps"], a["k"], a["l"], a["ls"], a["c"], a["d"], a["ds"], st)
        assert call(z=q["z"] + 4) == call(l=q["l"] + 4) == call(k=q["k"] + 2) == call(c=q["c"] + 2) == call(d=q["d"] + 2) == pkg.PDDC_EINVAL
        assert call(z=None) == call(p=None) == call(k=None) == call(l=None) == call(c=None) == pkg.PDDC_EINVAL
        assert call(zs=b - 1) == call(ps=pcap - 1) == call(ls=lcap - 1) == call(ds=b - 1) == pkg.PDDC_ECAPACITY
        assert call(d=q["z"] + 8 * b, ds=2 * n) == pkg.PDDC_EINVAL                                # disc inside z's rows
        assert call(p=q["z"] + 8 * b, ps=8 * n) == pkg.PDDC_EINVAL                                # pix inside z's rows
        torch.cuda.synchronize()
        assert (pix == FILL_P).all() and (lines == FILL_I).all() and (npix == FILL_I).all() and (counts == FILL_I).all() and (disc == FILL_F).all()
        f.process(zd[:, :0], npix=npix, counts=counts)
        torch.cuda.synchronize()
        assert not npix.any() and not counts.any()

    got = run(pkg, zd, bank, sel, W, cuts, before=disturb)
    assert same_bits(got, clean)
    good = bank[0]
    for k, v in ((6, 10), (7, 12), (2, 15), (2, 8193), (3, 0), (3, 17), (1, 0), (1, (1 << 31) + 1), (10, 0), (10, 256), (4, np.inf)):
        bad = good[:k] + (v,) + good[k + 1:]
        with pytest.raises(pkg.PddcError) as e:
            pkg.Fax([bad], [(0, R.ON)], W)
        assert e.value.code == pkg.PDDC_EINVAL, (k, v)
    pkg.Fax([good[:6] + (10, 14, 7, 9, 2)], [(0, R.ON)], W).close()        # the start tone above the stop tone: IOC 288's order


# ---- end to end --------------------------------------------------------------------------------------------------------

def test_a_picture_comes_back(pkg, dev):
    """fax_encode of a 64 x 48 picture of eight grey bars at test_fax_cpu.py's compressed mode (width 64, fax_ref.E2E), 11
    black pixels ahead so that the receiver's lines are not the sender's, noise 20 dB down, in batches of 977 samples:
    fax_image of the device's records and pixels finds one image, its column within 2 of the sender's, 47 or 48 rows, and
    every pixel more than box + 2 columns from a bar's edge within the CPU test's bound, fax_ref.E2E_BOUND."""
    import torch
    modem, rate, z, img, lead = R.e2e_case(pkg, seed=3)
    n = z.shape[0]
    cuts = [977] * (n // 977) + ([n % 977] if n % 977 else [])
    px, ln, _, st = run(pkg, torch.from_numpy(z.reshape(1, -1).copy()).to(dev), [modem], [(0, R.ON)], R.E2E_W, cuts)
    err, col, rows = R.e2e_error(pkg, ln[0], px[0], modem, img, lead)
    print(f"end to end: column {col} (sent {lead}), {rows} rows, worst error {err:.2f} grey levels (bound {R.E2E_BOUND})")
    assert st["images"][0] == 1 and st["active"][0] == 0
    assert err <= R.E2E_BOUND


def test_in_place_behind_the_tuner(pkg, dev):
    """The Tuner's output tensor, a view whose row stride is its capacity, is read in place: the bytes of the same series
    copied to a contiguous tensor."""
    import torch
    M, hop, T, Rd, K, rows_n = 1024, 512, 64, 4, 13, 1200
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((rows_n, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, Rd), Rd)
    cap = t.next_outputs(rows_n) + 37
    zv = t.process(rows, out=torch.empty((K, cap), dtype=torch.complex64, device=dev))
    n = zv.shape[1]
    assert zv.stride(0) == cap > n > 256
    bank, sel = R.bank16(16), R.sel16(K)
    want = run(pkg, zv.contiguous(), bank, sel, 16)
    got = run(pkg, zv, bank, sel, 16, [n // 3, n - n // 3])
    assert same_bits(got, want) and sum(len(p) for p in got[0]) > K * n // 5
    t.close()


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed, the download
    on the null stream does not wait, and everything, read() included, has the bytes of the same batches on the null
    stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.fax_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    bank, sel = R.bank16(W), R.sel16(K)
    x = np.stack([R.parity_row(j, bank[sel[j][0]], 72000 + j, n=total) for j in range(K)])
    scr = x.copy()
    scr[:, keep:] = x[:, keep:][:, ::-1]
    S.side_streams(dev, 1)

    def alloc(obj):
        bufs = [[S.Buf((K, obj.max_pixels(b)), torch.uint8, dev), S.Buf((K,), torch.int32, dev), S.Buf((K, obj.max_lines(b), 4), torch.int32, dev),
                 S.Buf((K,), torch.int32, dev), S.Buf((K, b), torch.float32, dev)] for b in warm + main]
        torch.cuda.synchronize()
        return bufs

    def batches(obj, src, st, sizes, bufs, off, sync_each):
        views = []
        for b, bf in zip(sizes, bufs):
            views.append(obj.process(src[:, off:off + b], pix=bf[0].t, npix=bf[1].t, lines=bf[2].t, counts=bf[3].t, disc=bf[4].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    real = torch.from_numpy(x).to(dev)
    obj = pkg.Fax(bank, sel, W)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > K * total // 5 and sum(int(c[3].sum()) for c in clean) > K

    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Fax(bank, sel, W)
    bufs = alloc(obj)
    side = S.side_streams(dev)[0]
    st = side.cuda_stream
    vw, off = batches(obj, live, st, warm, bufs[:2], 0, False)
    side.synchronize()
    gate = S.occupy(side, dev, 100.0)
    with torch.cuda.stream(side):
        live.copy_(real, non_blocking=True)
    vm, _ = batches(obj, live, st, main, bufs[2:], off, False)
    closed1 = not gate.query()
    intact = all(b.untouched() for bl in bufs[2:] for b in bl)
    closed2 = not gate.query()
    side.synchronize()
    reads = obj.read(stream=st)
    got = [[S.host(t) for t in v] for v in vw + vm]
    obj.close()
    assert closed1, "the host did not run ahead of the side stream: process() stalled it"
    assert intact, "an output was written while the side stream was still busy: a launch or copy on another stream"
    assert closed2, "the download on the null stream waited for the side stream"
    for i, (g, w) in enumerate(zip(got, clean)):
        npix, counts = w[1], w[3]
        assert S.same_bits(g[1], w[1]) and S.same_bits(g[3], w[3]) and S.same_bits(g[4], w[4]), i
        for j in range(K):                                            # what was written (the rest is canary)
            assert S.same_bits(g[0][j, :npix[j]], w[0][j, :npix[j]]) and (g[0][j, npix[j]:] == S.CANARY).all(), (i, j)
            assert S.same_bits(g[2][j, :counts[j]], w[2][j, :counts[j]]), (i, j)
            assert (g[2][j, counts[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
    assert reads.tobytes() == clean_read.tobytes()
