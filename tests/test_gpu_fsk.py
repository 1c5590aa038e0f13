"""Fsk (pddc_fsk_*, k_fsk) on the GPU against the numpy reference in double (tests/fsk_ref.py).
d: within fsk_ref.TOL_FSK, 7 x the float32 model's worst case on the parity test's very inputs (tests/test_fsk_cpu.py),
never taken from k_fsk.  Characters, counts and status: exactly the reference's (start, code, flags and the counters as
integers; quality and d_last, floats of d's making, within TOL_FSK) for every receiver whose reference margin holds --
the least |d| over its samples with s > 0 (the first behind zero history left out) is at least fsk_ref.MARGIN =
100 TOL_FSK.  quality and d_last are not compared by their bits: the double reference has other bits, and the float32
model's fmaf (two roundings, through double) is not the device's in every last case.  Only the 1024-receiver case may
leave receivers out, at most 10 % of them; everywhere else the margin is asserted for every receiver compared.
Against itself every output has the same bits however the series is cut: no tolerance, no exclusions."""
import numpy as np
import pytest

import fsk_ref as F
import nonfinite as NF
import stream_order as S

pytestmark = pytest.mark.gpu


def records(pkg, chars, counts):
    """the device's chars [nrx, cap, 4] int32 and counts -> one CHAR array per receiver"""
    c = chars.cpu().numpy().view(pkg.fsk_char_dtype())[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Fsk in the given batches -> (one CHAR array per
    receiver, d float32 [nrx, n] numpy, status); before(i, f) is called ahead of batch i; pad > 0: chars and d are views
    of tensors whose rows lie further apart than the batch needs"""
    import torch
    f = pkg.Fsk(bank, sel, W)
    nrx = z.shape[0]
    parts, ds, off = [[] for _ in range(nrx)], [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        cap = f.max_chars(b)
        assert cap == F.max_chars(bank, b)
        kw = {}
        if pad:
            kw = dict(chars=torch.zeros((nrx, cap + pad, 4), dtype=torch.int32, device=z.device),
                      d=torch.zeros((nrx, b + pad), dtype=torch.float32, device=z.device))
        chars, counts, d = f.process(z[:, off:off + b], want_d=True, **kw)
        assert d.shape == (nrx, b) and d.dtype == torch.float32 and counts.shape == (nrx,)
        for j, c in enumerate(records(pkg, chars, counts)):
            parts[j].append(c)
        ds.append(d.cpu().numpy())
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(p) for p in parts], np.concatenate(ds, axis=1), st


def same_bits(a, b):
    """two results of run() by their bytes"""
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def against_reference(got, ref, rows, what):
    """d of every receiver within TOL_FSK; characters and status of the receivers `rows` as the module's header says"""
    chars, d, st = got
    rchars, rd, margin, rst = ref
    e = float(np.abs(d.astype(np.float64) - rd).max()) if rd.size else 0.0
    print(f"{what}: |d - ref| {e:.2e} (TOL_FSK {F.TOL_FSK:.2e}), {len(rows)} of {len(chars)} receivers compared exactly")
    assert e <= F.TOL_FSK, (what, e)
    for j in rows:
        assert margin[j] >= F.MARGIN, (what, j, margin[j])
        for k in ("start", "code", "flags"):
            assert np.array_equal(chars[j][k], rchars[j][k]), (what, j, k, chars[j][k], rchars[j][k])
        assert np.abs(chars[j]["quality"].astype(np.float64) - rchars[j]["quality"]).max(initial=0.0) <= F.TOL_FSK, (what, j)
        for k in ("chars", "framing", "false_starts", "state"):
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        assert abs(float(st["d_last"][j]) - float(rst["d_last"][j])) <= F.TOL_FSK, (what, j)


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = F.case(W, key[1])
        _REFS[key] = F.run_cuts(F.FskRef(bank, sel, W), z)
    chars, d, margin, st = _REFS[key]
    return chars[:nrx], d[:nrx], margin[:nrx], st[:nrx]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """fsk_ref.case(W, nrx) for W = 1, 2, 16, 255, 256 (1024 receivers: all but 2, whose series has nine rows), one
    batch: one tap with REVERSE receivers that read a break; inc = 2^30 with nbits = 8 at 4 samples per bit; one modem
    at 16 samples per bit; banks of 16 modems with taps in the whole window, four of them with inc = 1.  Every receiver of the small sets is compared
    exactly; of the 1024 those whose margin holds, at least 90 %."""
    import torch
    for W in (F.BIG_WINDOWS if nrx == 1024 else F.WINDOWS):
        bank, sel, z = F.case(W, nrx)
        ref = parity_ref(W, nrx)
        rows = [j for j in range(nrx) if ref[2][j] >= F.MARGIN]
        assert len(rows) == nrx if nrx < 1024 else len(rows) >= nrx - nrx // 10, (W, len(rows))
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, ref, rows, f"nrx {nrx} W {W}")
        for j in rows:
            want = F.case_codes(W, j)
            if want is not None:
                assert list(got[0][j]["code"]) == want, (W, j)


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of fsk_ref.cut_lists (batches of 0 and 1, cuts on and beside the
    kernel's tile seams, forty batches of one sample): characters, d and status have the same bytes.  A receiver's bytes
    are the same alone and among the nine, and with input, chars and d rows further apart than the batch needs."""
    import torch
    bank, sel, z = F.case(W, 9)
    n, TT = z.shape[1], pkg.fsk_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    against_reference(one, parity_ref(W, 9), range(9), f"W {W}")
    for cuts in F.cut_lists(n, TT):
        assert same_bits(run(pkg, zd, bank, sel, W, cuts), one), cuts
    for j in (2, 8):
        alone = run(pkg, zd[j:j + 1], bank, [sel[j]], W, F.cut_lists(n, TT)[1])
        assert alone[0][0].tobytes() == one[0][j].tobytes() and alone[1][0].tobytes() == one[1][j].tobytes(), j
        assert alone[2][0].tobytes() == one[2][j].tobytes(), j
    wide = torch.zeros((9, n + 13), dtype=torch.complex64, device=dev)
    wide[:, :n] = zd
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    assert same_bits(run(pkg, view, bank, sel, W, F.cut_lists(n, TT)[0], pad=7), one)
    assert same_bits(run(pkg, view, bank, sel, W), one)


def test_tile_seams(pkg, dev):
    """5 receivers (a ragged last group), series of TT - 1, TT, TT + 1 and 2 TT + 1 samples: against the reference, and
    the longest cut in two at TT - 1 and at TT with the same bytes."""
    import torch
    TT, W = pkg.fsk_tile_outputs(), 16
    bank, sel, z = F.case(W, 5)
    ref = F.FskRef(bank, sel, W)
    for n in (TT - 1, TT, TT + 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(z[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel, W)
        ref.reset()
        against_reference(one, F.run_cuts(ref, z[:, :n]), range(5), f"{n} samples")
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert same_bits(run(pkg, zd, bank, sel, W, [cut, n - cut]), one), cut


def test_reverse(pkg, dev):
    """fsk_ref.reverse_inputs, the parity series with its tones exchanged, read by five REVERSE receivers: every one
    compared exactly with the reference, every one reads its text; without REVERSE none does, and d is the negative."""
    import torch
    W, nrx = 16, 5
    bank = [F.tailed_modem(W, 0)]
    z = F.reverse_inputs(nrx)
    sel = [(0, F.ON | F.REVERSE)] * nrx
    ref = F.run_cuts(F.FskRef(bank, sel, W), z)
    got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
    against_reference(got, ref, range(nrx), "reverse")                # asserts every receiver's margin
    for j in range(nrx):
        assert list(got[0][j]["code"]) == F.parity_text(j) and not got[0][j]["flags"].any()
    plain = run(pkg, torch.from_numpy(z).to(dev), bank, [(0, F.ON)] * nrx, W)
    assert all(list(plain[0][j]["code"]) != F.parity_text(j) for j in range(nrx))
    assert np.array_equal(plain[1], -got[1])                         # pm and ps exchanged: d changes its sign alone


# ---- receiver control --------------------------------------------------------------------------------------------------

CONTROL_CUTS = [460, 400, 404]


def control_case():
    """6 receivers of the parity series, W = 16, a bank of two modems (the second with nbits = 6), three batches of 460,
    400 and 404 samples, cut inside characters (they begin at 39 + 120 k).  Receiver 0 runs undisturbed; 1 is OFF throughout and its input row is NaN; 2 is OFF in the
    first batch and ON from the second; 3 is restarted in front of the second batch, inside a character; 4 goes to the
    other modem in front of the third batch, inside a character, and 5 is switched OFF there."""
    bank = [F.tailed_modem(16, 0), F.tailed_modem(16, 0, nbits=6)]
    sel = [(0, F.ON), (0, 0), (0, 0), (0, F.ON), (0, F.ON), (0, F.ON)]
    z = F.parity_inputs(6).copy()
    z[1] = complex(np.nan, np.nan)

    def changes(at_b, at_c):
        def before(i, f):
            if i == at_b:
                f.set_rx(2, 0, F.ON)
                f.set_rx(3, 0, F.ON | F.RESTART)
            if i == at_c:
                f.set_rx(4, 1, F.ON)
                f.set_rx(5, 0, 0)
        return before
    return bank, sel, z, changes


def test_receiver_control(pkg, dev):
    """control_case against the reference given the same changes, every receiver exactly.  The OFF receiver's NaN row is
    never read: count 0, d row +0 by its bits, status zero.  The receiver switched ON reads as a fresh object fed the
    samples from there on (starts count the object's samples).  RESTART and the modem change each lose the character
    they fall into, the counters stay.  Another cut with the same change points: the same bytes."""
    import torch
    bank, sel, z, changes = control_case()
    W, (a, b, c) = 16, CONTROL_CUTS
    ref = F.run_cuts(F.FskRef(bank, sel, W), z, CONTROL_CUTS, before=changes(1, 2))
    zd = torch.from_numpy(z).to(dev)
    got = run(pkg, zd, bank, sel, W, CONTROL_CUTS, before=changes(1, 2))
    against_reference(got, ref, range(6), "control")
    chars, d, st = got
    assert chars[1].size == 0 and not d[1].view(np.uint32).any() and st[1].tobytes() == bytes(F.STATUS.itemsize)
    assert not d[2, :a].view(np.uint32).any() and not d[5, a + b:].view(np.uint32).any()
    assert chars[2].size and chars[2]["start"].min() >= a and chars[5].size and chars[5]["start"].max() < a + b
    late = run(pkg, zd[2:3, a:].contiguous(), bank, [(0, F.ON)], W)
    assert np.array_equal(late[0][0]["start"] + np.uint64(a), chars[2]["start"]) and late[1].tobytes() == d[2:3, a:].tobytes()
    assert all(late[0][0][k].tobytes() == chars[2][k].tobytes() for k in ("code", "flags", "quality"))
    full = F.parity_text(0)
    assert list(chars[0]["code"]) == full
    assert len(chars[3]) == len(F.parity_text(3)) - 1 and len(chars[4]) < len(F.parity_text(4))
    assert st["chars"][3] == len(chars[3]) and st["chars"][5] == len(chars[5])
    other = run(pkg, zd, bank, sel, W, [1, a - 1, 0, 255, b - 255, 30, c - 30], before=changes(3, 5))
    assert same_bits(other, got)


def test_break_and_false_start(pkg, dev):
    """Noiseless lines, W = 16.  Receiver 0: one character, then space for good -- the character, one framing-error
    character with code 0, then nothing (no further edge while the line stays space), state IDLE.  Receiver 1: a space
    of 8 samples, half a bit, in a mark line -- an edge, mark under the START strobe: false_starts = 1, no character.  Receiver 2: a
    character whose stop element is cut short by a break of 12 bits, then mark, then a good character: three
    characters, the middle one a framing error."""
    import torch
    W, n = 16, 800
    bank = [F.tailed_modem(W, 0)]
    lines = [np.r_[F.keying([21], tail=0.0), np.ones(n, bool)][:n],
             np.r_[np.zeros(100, bool), np.ones(8, bool), np.zeros(n, bool)][:n],
             np.r_[F.keying([10], stop=1.0, tail=0.0), np.ones(12 * 16, bool), np.zeros(40, bool), F.keying([7], lead=0.0),
                   np.zeros(n, bool)][:n]]
    z = np.stack([F.two_tone(l, F.MARK, F.SPACE, None, 70 + j) for j, l in enumerate(lines)])
    sel = [(0, F.ON)] * 3
    ref = F.run_cuts(F.FskRef(bank, sel, W), z)
    got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W, [300, 500])
    against_reference(got, ref, range(3), "break")
    chars, d, st = got
    assert list(chars[0]["code"]) == [21, 0] and list(chars[0]["flags"]) == [0, F.FRAMING]
    assert (st["chars"][0], st["framing"][0], st["state"][0]) == (2, 1, F.IDLE)
    assert chars[1].size == 0 and (st["false_starts"][1], st["chars"][1], st["state"][1]) == (1, 0, F.IDLE)
    assert list(chars[2]["code"]) == [10, 0, 7] and list(chars[2]["flags"]) == [0, F.FRAMING, 0]


def test_a_refused_call_changes_nothing_and_reset(pkg, dev):
    """PDDC_ECAPACITY for a chars capacity below max_chars(n) and for a z or d stride below n, with nothing written
    (chars, counts and d keep their fill); PDDC_EINVAL for misaligned or NULL pointers, a d that overlaps z and a bad
    set_rx, between the batches: the next good batch gives the bytes of an undisturbed run.  n = 0 sets the counts to 0.
    After reset the outputs repeat those after create."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = F.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 500, n - 800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        cap = f.max_chars(b)
        assert cap == b // 104 + 1                                   # P = ceil(6.5 x 16) samples
        chars = torch.full((nrx, cap - 1, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        dd = torch.full((nrx, b), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], chars=chars, counts=counts, d=dd)
        assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], counts=counts, d=dd[:, :b - 1])
        assert e.value.code == pkg.PDDC_ECAPACITY
        torch.cuda.synchronize()
        assert (chars == 0x5A5A5A5A).all() and (counts == 0x5A5A5A5A).all() and (dd == 7.0).all()
        for rx, modem, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, 1, 1), (0, 0, 8)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, modem, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        ch = torch.zeros((nrx, cap, 4), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_fsk_process(f._h, *args, st)
        p = dict(z=zd.data_ptr(), c=ch.data_ptr(), k=counts.data_ptr(), d=dd.data_ptr())
        assert call(p["z"], b, b - 1, p["c"], cap, p["k"], p["d"], b) == pkg.PDDC_ECAPACITY
        assert call(p["z"], b, n, p["c"], cap - 1, p["k"], None, 0) == pkg.PDDC_ECAPACITY
        assert call(p["z"] + 4, b, n, p["c"], cap, p["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, p["c"] + 4, cap, p["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, p["c"], cap, p["k"] + 2, None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, p["c"], cap, p["k"], p["d"] + 2, b) == pkg.PDDC_EINVAL
        assert call(None, b, n, p["c"], cap, p["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, None, cap, p["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, p["c"], cap, None, None, 0) == pkg.PDDC_EINVAL
        assert call(p["z"], b, n, p["c"], cap, p["k"], p["z"] + 8 * b, 2 * n) == pkg.PDDC_EINVAL     # d inside z's rows
        torch.cuda.synchronize()
        assert (counts == 0x5A5A5A5A).all() and (dd == 7.0).all() and not ch.any()
        empty = f.process(zd[:, :0], counts=counts, want_d=True)
        torch.cuda.synchronize()
        assert not counts.any() and empty[2].shape == (nrx, 0)

    got = run(pkg, zd, bank, sel, W, cuts, before=disturb)
    assert same_bits(got, clean)
    f = pkg.Fsk(bank, sel, W)
    first = [f.process(zd[:, :300], want_d=True), f.process(zd[:, 300:], want_d=True)]
    f.reset()
    assert f.read().tobytes() == bytes(nrx * F.STATUS.itemsize)
    chars, counts, d = f.process(zd, want_d=True)
    again = records(pkg, chars, counts)
    parts = [records(pkg, c, k) for c, k, _ in first]
    for j in range(nrx):
        assert np.concatenate([parts[0][j], parts[1][j]]).tobytes() == again[j].tobytes() == clean[0][j].tobytes()
    assert torch.equal(torch.cat([first[0][2], first[1][2]], dim=1).view(torch.int32), d.view(torch.int32))
    assert f.read().tobytes() == clean[2].tobytes()
    f.close()


# ---- non-finite samples ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """35 receivers (2 x 16 + 3) of the parity series, W = 16, the batches of nonfinite.cuts_for around the tile seams; a
    NaN or an infinity in rows 0, 16, 31 and 34 at the columns of nonfinite.placements.  The other receivers' characters,
    d and status are those of the clean run bit for bit.  A poisoned row's d is +0 at the 16 samples whose window holds the
    value (against taps without a zero part the value makes M or S NaN, s NaN, and the definition then gives d = 0 and
    reads mark) and within TOL_FSK of the double reference of the poisoned series elsewhere: nothing is left behind once
    the value has left the window.  One batch gives the same bytes."""
    import torch
    W, K = 16, 35
    TT, n = pkg.fsk_tile_outputs(), F.PARITY_N
    bank = [F.tailed_modem(W, 0)]
    sel = [(0, F.ON)] * K
    z = F.parity_inputs(1024)[:K]
    rows, cols = NF.poisoned_rows(K), NF.placements(TT, W, n)
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W, cuts)
    got = run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W, cuts)
    others = [j for j in range(K) if j not in rows]
    NF.clean_rows_identical(got[1], clean[1], others, f"fsk d, {name}")
    for j in others:
        assert got[0][j].tobytes() == clean[0][j].tobytes() and got[2][j].tobytes() == clean[2][j].tobytes(), j
    model = F.run_cuts(F.FskRef(bank, [sel[j] for j in rows], W, f32=True), zp[rows])[1]
    ref = F.run_cuts(F.FskRef(bank, [sel[j] for j in rows], W), zp[rows])[1]
    d = np.ascontiguousarray(got[1][rows])
    hit = np.zeros(n, bool)
    for c in cols:
        hit[c:c + W] = True
    # the definition's own doing, model and reference alike: a power that is NaN makes s NaN, s > 0 false and d = +0
    assert not np.isnan(model).any() and not model[:, hit].any() and not ref[:, hit].any() and model[:, ~hit].all()
    assert not np.ascontiguousarray(d[:, hit]).view(np.uint32).any()
    assert np.abs(d.astype(np.float64) - ref).max() <= F.TOL_FSK
    assert same_bits(run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W), got)


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed (chars, counts
    and d still hold their canaries), the download on the null stream does not wait, and everything, read() included,
    has the bytes of the same batches on the null stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.fsk_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    bank = [F.tailed_modem(W, 0), F.tailed_modem(W, 1)]
    sel = [(j % 2, F.ON | (F.REVERSE if j % 5 == 0 else 0)) for j in range(K)]
    x = F.parity_inputs(1024)[:K, :total]
    scr = x.copy()
    scr[:, keep:] = x[:, keep:][:, ::-1]
    S.side_streams(dev, 1)

    def alloc(obj):
        bufs = [[S.Buf((K, obj.max_chars(b), 4), torch.int32, dev), S.Buf((K,), torch.int32, dev),
                 S.Buf((K, b), torch.float32, dev)] for b in warm + main]
        torch.cuda.synchronize()
        return bufs

    def batches(obj, src, st, sizes, bufs, off, sync_each):
        views = []
        for b, bf in zip(sizes, bufs):
            views.append(obj.process(src[:, off:off + b], chars=bf[0].t, counts=bf[1].t, d=bf[2].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    # the clean run
    real = torch.from_numpy(x).to(dev)
    obj = pkg.Fsk(bank, sel, W)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > K                    # characters were decoded in these batches

    # the busy run
    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Fsk(bank, sel, W)
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
        counts = w[1]
        assert S.same_bits(g[1], w[1]) and S.same_bits(g[2], w[2]), i
        for j in range(K):                                            # chars: the written records (the rest is canary)
            assert S.same_bits(g[0][j, :counts[j]], w[0][j, :counts[j]]), (i, j)
            assert (g[0][j, counts[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
    assert reads.tobytes() == clean_read.tobytes()
