"""Mfsk's rows of the non-finite table (include/perseus_ddc.h, "mfsk", "Non-finite samples"), with the helpers of
tests/nonfinite.py as they are: a NaN or an infinity stays in its row, the row is the reference's again W + 2 q samples on,
RESTART gives the row back, and nothing outside rows, counts and strides is read or written."""
import numpy as np
import pytest

import mfsk_ref as R
import nonfinite as NF

pytestmark = pytest.mark.gpu

W, K, SPS, M = 16, 35, 16, 8
# the poisoned rows' seeds, chosen on the double reference so that its margin holds on the poisoned series too (asserted)
NF_SEEDS = {0: 73000, 16: 73016, 31: 73031, 34: 73034}


def nonfinite_case(TT):
    """35 receivers (2 x 16 + 3) on one modem: M = 8 tones a baud apart at 16 samples per symbol, W = 16, q = 4, step =
    inc / 4; each hears 70 seeded random tones, noise 20 dB below.  -> (bank, sel, z, the poisoned rows, the columns:
    nonfinite.placements' -- 0, W - 1, the tile seam's TT - 1 and TT, 2 TT + 3, n - 1)"""
    f = R.tone_freqs(M, SPS)
    h, inc, q, _ = R.modem(f, W, SPS)
    bank, sel = [(h, inc, q, inc // 4)], [(0, R.ON)] * K
    n = 73 * SPS
    z = np.stack([R.encode(np.random.default_rng(NF_SEEDS.get(j, 74000 + j) + 5).integers(0, M, 70), f, SPS, n, lead=SPS - q + (j % 8 - 4) / 2.0,
                           snr_db=R.PARITY_SNR, seed=NF_SEEDS.get(j, 74000 + j)) for j in range(K)])
    return bank, sel, z, NF.poisoned_rows(K), NF.placements(TT, W, n)


def run(pkg, dev, z, bank, sel, cuts, before=None, spare=2):
    """z [K, n] through a fresh Mfsk in batches.  The input lies in a tensor with `spare` more rows and 5 more columns, all
    nonfinite.never_read; syms and best are views of never_read tensors with spare rows and columns, counts has spare
    entries: what lies outside the rows, the counts and the strides must come back as it went.  -> (SYM records, best
    [K, n], status)"""
    import torch
    Kz, n = z.shape
    host = NF.never_read((Kz + spare, n + 5), np.complex64)
    host[:Kz, :n] = z
    zd = torch.from_numpy(host).to(dev)
    f = pkg.Mfsk(bank, sel, W)
    sy, bs, off = [[] for _ in range(Kz)], [], 0
    for i, b in enumerate(cuts):
        if before:
            before(i, f)
        cap = f.max_syms(b)
        fills = [NF.never_read((Kz + spare, cap + 2, 4), np.int32), NF.never_read((Kz + spare,), np.int32),
                 NF.never_read((Kz + spare, b + 3), np.float32)]
        t = [torch.from_numpy(x.copy()).to(dev) for x in fills]
        f.process(zd[:Kz, off:off + b], syms=t[0][:Kz], counts=t[1][:Kz], best=t[2][:Kz])
        got = [x.cpu().numpy() for x in t]
        counts = got[1][:Kz]
        if b == 0:
            assert not counts.any()
        else:
            assert (counts >= 0).all() and (counts <= cap).all()
        for g, fill in zip(got, fills):                                   # the spare rows and entries
            assert g[Kz:].tobytes() == fill[Kz:].tobytes(), i
        for j in range(Kz):
            c = int(counts[j])
            assert got[0][j, c:].tobytes() == fills[0][j, c:].tobytes() and got[2][j, b:].tobytes() == fills[2][j, b:].tobytes(), (i, j)
            sy[j].append(got[0][j, :c].copy().view(pkg.mfsk_sym_dtype())[..., 0])
        bs.append(got[2][:Kz, :b].copy())
        off += b
    assert off == n and zd.cpu().numpy().tobytes() == host.tobytes()
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in sy], np.concatenate(bs, axis=1), st


@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """nonfinite_case with a NaN or an infinity in rows 0, 16, 31 and 34 at its columns, the batches of nonfinite.cuts_for.
    The other receivers' records, best and status are those of the clean run bit for bit.  A poisoned row does what the
    header says: best is the clean run's, bit for bit, at every sample whose window holds no poisoned one; its strobes
    fall where the double reference of the poisoned series puts them (that reference's margin holds at every strobe that
    reads no poisoned sample), and every record whose strobe lies W + 2 q samples or more behind the last poisoned sample
    (or before the first) has the reference's tone and runner-up and its quality within TOL_MFSK; the counter and the
    clock end as the reference's.  RESTART gives the row back: the clean series behind it reads as on a fresh object, the
    starts and the counter aside.  One batch gives the same bytes where no NaN stands."""
    TT = pkg.mfsk_tile_outputs()
    bank, sel, z, rows, cols = nonfinite_case(TT)
    n, q = z.shape[1], bank[0][2]
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, dev, z, bank, sel, cuts)
    got = run(pkg, dev, zp, bank, sel, cuts)
    others = [j for j in range(K) if j not in rows]
    NF.clean_rows_identical(got[1], clean[1], others, "best")
    for j in others:
        assert got[0][j].tobytes() == clean[0][j].tobytes() and got[2][j].tobytes() == clean[2][j].tobytes(), j
    r = R.MfskRef(bank, [sel[j] for j in rows], W)
    r.trace = []
    ref = R.run_cuts(r, zp[rows])
    untouched = np.ones(n, bool)                                           # samples whose window holds no poisoned one
    for c in cols:
        untouched[c:c + W] = False
    for k, j in enumerate(rows):
        assert got[1][j][untouched].tobytes() == clean[1][j][untouched].tobytes(), j
        assert np.isfinite(got[1][j][untouched]).all() and not np.isfinite(zp[j]).all()
        assert np.array_equal(got[0][j]["start"], ref[0][k]["start"]), j
        m = ref[0][k]["start"].astype(np.int64) + q                        # the strobes' samples
        far = np.ones(m.size, bool)
        for c in cols:
            far &= (m < c) | (m >= c + W + 2 * q)
        assert far.sum() > m.size // 2 and np.isfinite(ref[0][k]["quality"][far]).all()
        # the reference's margin over those strobes; the others compare zeros and infinities, which every arithmetic agrees on
        margin = min(min(t[2], t[3]) for t in r.trace if t[0] == k and far[np.searchsorted(m, t[1])])
        assert margin >= R.MARGIN, (j, margin)
        for key in ("tone", "second"):
            assert np.array_equal(got[0][j][key][far], ref[0][k][key][far]), (j, key)
        assert np.abs(got[0][j]["quality"][far].astype(np.float64) - ref[0][k]["quality"][far]).max() <= R.TOL_MFSK, j
        for key in ("symbols", "acc", "skip"):
            assert got[2][key][j] == ref[3][key][k], (j, key)
    two = np.concatenate([zp, z], axis=1)

    def restart(i, f):
        if i == len(cuts):
            for j in rows:
                f.set_rx(j, 0, R.ON | R.RESTART)
    both = run(pkg, dev, two, bank, sel, cuts + [n], before=restart)
    for j in rows:
        assert both[1][j, n:].tobytes() == clean[1][j].tobytes(), j
        back = both[0][j][len(got[0][j]):]
        assert np.array_equal(back["start"], clean[0][j]["start"] + np.uint64(n)), j
        for key in ("tone", "second", "flags", "quality"):
            assert back[key].tobytes() == clean[0][j][key].tobytes(), (j, key)
        assert both[2]["symbols"][j] == got[2]["symbols"][j] + clean[2]["symbols"][j]
        for key in ("acc", "skip", "tone_last", "q_last"):
            assert both[2][key][j:j + 1].tobytes() == clean[2][key][j:j + 1].tobytes(), (j, key)
    one = run(pkg, dev, zp, bank, sel, [n])
    for j in range(K):
        assert np.array_equal(one[0][j]["start"], got[0][j]["start"]) and one[0][j]["tone"].tobytes() == got[0][j]["tone"].tobytes(), j
        NF.same_or_both_nan(one[0][j]["quality"], got[0][j]["quality"], "quality, one batch")
    NF.same_or_both_nan(one[1], got[1], "best, one batch")
