"""Fax's rows of the non-finite table (include/perseus_ddc.h, "fax", "Non-finite samples"), with the helpers of
tests/nonfinite.py as they are: a NaN or an infinity stays in its row, the row does what the header says, RESTART gives the
row back, and nothing outside rows, counts and strides is read or written."""
import numpy as np
import pytest

import fax_ref as R
import nonfinite as NF

pytestmark = pytest.mark.gpu

W, K, BOX = 16, 35, 3
NF_SEEDS = {0: 73000, 16: 73016, 31: 73031, 34: 73034}


def nonfinite_case(TT):
    """35 receivers (2 x 16 + 3) on bank16's modem 1 (width 100, 2.5 samples per pixel, a boxcar of 3), W = 16.  -> (bank,
    sel, z, the poisoned rows, the columns: nonfinite.placements' -- 0, W - 1, the tile seam's TT - 1 and TT, 2 TT + 3,
    n - 1 -- and a strobe, a line's last pixel and the sample behind each, of row 0's clean reference)"""
    bank, sel = [R.bank16(W)[1]], [(0, R.ON)] * K
    assert bank[0][3] == BOX
    rows = NF.poisoned_rows(K)
    z = np.stack([R.parity_row(j, bank[0], NF_SEEDS.get(j, 74000 + j)) for j in range(K)])
    strobe, end = R.events(bank, sel[:1], W, z[:1])
    cols = sorted(set(NF.placements(TT, W, z.shape[1])) | {strobe, strobe + 1, end, end + 1})
    return bank, sel, z, rows, cols


def run(pkg, dev, z, bank, sel, cuts, before=None, spare=2):
    """z [K, n] through a fresh Fax in batches.  The input lies in a tensor with `spare` more rows and 5 more columns, all
    nonfinite.never_read; pix, lines and disc are views of never_read tensors with spare rows and columns, npix and counts
    have spare entries: what lies outside the rows, the counts and the strides must come back as it went.  -> (pixels,
    LINE records, disc [K, n], status)"""
    import torch
    Kz, n = z.shape
    host = NF.never_read((Kz + spare, n + 5), np.complex64)
    host[:Kz, :n] = z
    zd = torch.from_numpy(host).to(dev)
    f = pkg.Fax(bank, sel, W)
    px, ln, ds, off = [[] for _ in range(Kz)], [[] for _ in range(Kz)], [], 0
    for i, b in enumerate(cuts):
        if before:
            before(i, f)
        pcap, lcap = f.max_pixels(b), f.max_lines(b)
        fills = [NF.never_read((Kz + spare, pcap + 3), np.uint8), NF.never_read((Kz + spare,), np.int32),
                 NF.never_read((Kz + spare, lcap + 2, 4), np.int32), NF.never_read((Kz + spare,), np.int32),
                 NF.never_read((Kz + spare, b + 3), np.float32)]
        t = [torch.from_numpy(x.copy()).to(dev) for x in fills]
        f.process(zd[:Kz, off:off + b], pix=t[0][:Kz], npix=t[1][:Kz], lines=t[2][:Kz], counts=t[3][:Kz], disc=t[4][:Kz])
        got = [x.cpu().numpy() for x in t]
        npix, counts = got[1][:Kz], got[3][:Kz]
        if b == 0:
            assert not npix.any() and not counts.any()
            got[4][:Kz, :0] = 0
        else:
            assert (npix >= 0).all() and (npix <= pcap).all() and (counts >= 0).all() and (counts <= lcap).all()
        for g, fill in zip(got, fills):                                   # the spare rows and entries
            assert g[Kz:].tobytes() == fill[Kz:].tobytes(), i
        for j in range(Kz):
            k, c = (int(npix[j]), int(counts[j])) if b else (0, 0)
            assert got[0][j, k:].tobytes() == fills[0][j, k:].tobytes() and got[2][j, c:].tobytes() == fills[2][j, c:].tobytes(), (i, j)
            assert got[4][j, b:].tobytes() == fills[4][j, b:].tobytes(), (i, j)
            px[j].append(got[0][j, :k].copy())
            ln[j].append(got[2][j, :c].copy().view(pkg.fax_line_dtype())[..., 0])
        ds.append(got[4][:Kz, :b].copy())
        off += b
    assert off == n and zd.cpu().numpy().tobytes() == host.tobytes()
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in px], [np.concatenate(q) for q in ln], np.concatenate(ds, axis=1), st


@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """nonfinite_case with a NaN or an infinity in rows 0, 16, 31 and 34 at its columns (tile seams, a strobe, a line's end),
    the batches of nonfinite.cuts_for.  The other receivers' pixels, records, disc and status are those of the clean run
    bit for bit.  A poisoned row does what the header says: npix, counts, every start, acc and col are the clean run's (the
    clock never sees the data); disc is NaN exactly where the double reference of the poisoned series is (from the sample
    through W more wherever the taps are not zero) and within TOL_FAX of it elsewhere; a pixel whose boxcar holds such a
    value reads 0, every other pixel lies inside the reference's bounds; W + box samples behind the last poisoned sample
    disc and the pixels are the clean run's again, bit for bit.  RESTART gives the row back: the clean series behind it
    reads as on a fresh object, the counters aside.  One batch gives the same bytes."""
    TT = pkg.fax_tile_outputs()
    bank, sel, z, rows, cols = nonfinite_case(TT)
    n = z.shape[1]
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, dev, z, bank, sel, cuts)
    got = run(pkg, dev, zp, bank, sel, cuts)
    others = [j for j in range(K) if j not in rows]
    NF.clean_rows_identical(got[2], clean[2], others, "disc")
    for j in others:
        assert got[0][j].tobytes() == clean[0][j].tobytes() and got[1][j].tobytes() == clean[1][j].tobytes(), j
        assert got[3][j].tobytes() == clean[3][j].tobytes(), j
    ref = R.run_cuts(R.FaxRef(bank, [sel[j] for j in rows], W), zp[rows])
    touched = np.zeros(n, bool)                                            # samples whose f the header lets be NaN
    for c in cols:
        touched[c:c + W + 1] = True
    for k, j in enumerate(rows):
        assert got[0][j].shape == clean[0][j].shape and np.array_equal(got[1][j]["start"], clean[1][j]["start"]), j
        assert got[3]["acc"][j] == clean[3]["acc"][j] and got[3]["col"][j] == clean[3]["col"][j] and got[3]["pixels"][j] == clean[3]["pixels"][j]
        rn, gn = np.isnan(ref[2][k]), np.isnan(got[2][j])
        assert np.array_equal(rn, gn) and rn.any() and not (rn & ~touched).any(), j
        assert np.abs(got[2][j][~gn].astype(np.float64) - ref[2][k][~rn]).max() <= R.TOL_FAX, j
        where = ref[4][k]
        under = np.array([rn[max(m - BOX + 1, 0):m + 1].any() for m in where])
        assert under.any() and not got[0][j][under].any(), j
        lo, hi = R.pixel_bounds(ref[3][k][~under], bank[0][4])
        p = got[0][j][~under].astype(np.int64)
        assert ((p >= lo) & (p <= hi)).all(), j
        gone = np.ones(n, bool)                                            # samples W + box behind every poisoned one
        for c in cols:
            gone[c:c + W + BOX] = False
        assert got[2][j][gone].tobytes() == clean[2][j][gone].tobytes(), j
        assert got[0][j][gone[where]].tobytes() == clean[0][j][gone[where]].tobytes(), j
        own, state = R.lines_from_pixels(got[0][j], where, bank[0])
        for key in ("crossings", "white", "flags", "run"):
            assert np.array_equal(got[1][j][key], own[key]), (j, key)
    two = np.concatenate([zp, z], axis=1)

    def restart(i, f):
        if i == len(cuts):
            for j in rows:
                f.set_rx(j, 0, R.ON | R.RESTART)
    both = run(pkg, dev, two, bank, sel, cuts + [n], before=restart)
    for j in rows:
        assert both[2][j, n:].tobytes() == clean[2][j].tobytes(), j
        assert both[0][j][len(got[0][j]):].tobytes() == clean[0][j].tobytes(), j
        back = both[1][j][len(got[1][j]):]
        assert np.array_equal(back["start"], clean[1][j]["start"] + np.uint64(n)), j
        for key in ("crossings", "white", "flags", "run"):
            assert np.array_equal(back[key], clean[1][j][key]), (j, key)
        assert both[3]["lines"][j] == got[3]["lines"][j] + clean[3]["lines"][j]
        assert both[3]["acc"][j] == clean[3]["acc"][j] and both[3]["col"][j] == clean[3]["col"][j] and both[3]["active"][j] == clean[3]["active"][j]
    one = run(pkg, dev, zp, bank, sel, [n])
    for j in range(K):
        assert one[0][j].tobytes() == got[0][j].tobytes() and one[1][j].tobytes() == got[1][j].tobytes(), j
    NF.same_or_both_nan(one[2], got[2], "disc, one batch")
    assert one[3].tobytes() == got[3].tobytes() or np.isnan(got[3]["f_last"]).any()
