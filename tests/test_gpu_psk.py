"""Psk (pddc_psk_*, k_psk) on the GPU against the numpy reference in double (tests/psk_ref.py).
sym, the (d, x) pair of every strobe: within psk_ref.TOL_PSK, 7 x the float32 model's worst case on the parity test's very
inputs (tests/test_psk_cpu.py), never taken from k_psk.  Characters (start, code, nbits, flags), counts, nsym and the
integer status (chars, symbols, acc, reg): exactly the reference's for every receiver whose reference margin holds -- the
least |d| of its strobes and the least |p[m] - p[e]| / (p[m] + p[e]) where the clock's comparator is consulted are at least
psk_ref.MARGIN = 4 TOL_PSK; quality, d_last and x_last within TOL_PSK.  Only the 1024-receiver case may leave receivers
out, at most 10 % of them; everywhere else the margin is asserted for every receiver compared.  Against itself every
output has the same bits however the series is cut: no tolerance, no exclusions."""
import numpy as np
import pytest

import nonfinite as NF
import psk_ref as P
import stream_order as S

pytestmark = pytest.mark.gpu


def records(pkg, chars, counts):
    """the device's chars [nrx, cap, 4] int32 and counts -> one CHAR array per receiver"""
    c = chars.cpu().numpy().view(pkg.psk_char_dtype())[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


def pairs(sym, nsym):
    """the device's sym [nrx, cap, 2] float32 and nsym -> one [nsym, 2] array per receiver"""
    s, k = sym.cpu().numpy(), nsym.cpu().numpy()
    assert (k >= 0).all() and (k <= s.shape[1]).all()
    return [s[j, :k[j]].copy() for j in range(s.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Psk in the given batches -> (one CHAR array
    per receiver, one float32 [nsym, 2] array per receiver, status); before(i, f) is called ahead of batch i; pad > 0: chars
    and sym are views of tensors whose rows lie further apart than the batch needs"""
    import torch
    f = pkg.Psk(bank, sel, W)
    nrx = z.shape[0]
    parts, sy, off = [[] for _ in range(nrx)], [[] for _ in range(nrx)], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert cap == P.max_chars(bank, b) and scap == P.max_syms(bank, b)
        kw = {}
        if pad:
            kw = dict(chars=torch.zeros((nrx, cap + pad, 4), dtype=torch.int32, device=z.device),
                      sym=torch.zeros((nrx, scap + pad, 2), dtype=torch.float32, device=z.device))
        chars, counts, sym, nsym = f.process(z[:, off:off + b], want_sym=True, **kw)
        assert counts.shape == (nrx,) and nsym.shape == (nrx,) and sym.dtype == torch.float32
        for j, (c, s) in enumerate(zip(records(pkg, chars, counts), pairs(sym, nsym))):
            parts[j].append(c)
            sy[j].append(s)
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in parts], [np.concatenate(s) for s in sy], st


def same_bits(a, b):
    """two results of run() by their bytes"""
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2].tobytes() == b[2].tobytes())


def against_reference(got, ref, rows, what, margin=True):
    """the (d, x) pairs of every receiver in `rows` within TOL_PSK, their characters and status as the module's header
    says; the receivers outside `rows` are those whose margin does not hold: their strobes may fall elsewhere"""
    chars, sym, st = got
    rchars, rsym, rmargin, rst, _ = ref
    worst = 0.0
    for j in rows:
        if margin:
            assert rmargin[j] >= P.MARGIN, (what, j, rmargin[j])
        assert sym[j].shape == rsym[j].shape, (what, j, sym[j].shape, rsym[j].shape)
        if rsym[j].size:
            worst = max(worst, float(np.abs(sym[j].astype(np.float64) - rsym[j]).max()))
        for k in ("start", "code", "nbits", "flags"):
            assert np.array_equal(chars[j][k], rchars[j][k]), (what, j, k, chars[j], rchars[j])
        if rchars[j].size:
            assert np.abs(chars[j]["quality"].astype(np.float64) - rchars[j]["quality"]).max() <= P.TOL_PSK, (what, j)
        for k in ("chars", "symbols", "acc", "reg"):
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        for k in ("d_last", "x_last"):
            assert abs(float(st[k][j]) - float(rst[k][j])) <= P.TOL_PSK, (what, j, k, st[k][j], rst[k][j])
    print(f"{what}: |(d, x) - ref| {worst:.2e} (TOL_PSK {P.TOL_PSK:.2e}), {len(rows)} of {len(chars)} receivers compared")
    assert worst <= P.TOL_PSK, (what, worst)


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = P.case(W, key[1])
        _REFS[key] = P.run_cuts(P.PskRef(bank, sel, W), z)
    chars, sym, margin, st, strobes = _REFS[key]
    return chars[:nrx], sym[:nrx], margin[:nrx], st[:nrx], strobes[:nrx]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """psk_ref.case(W, nrx) for W = 1, 2, 16, 255, 256 (1024 receivers: 16, 255, 256), one batch: inc = 2^29 with q = 1,
    step = inc / 16 and step = inc; 16 samples per symbol with step = inc / 4 and step = 0; banks of 16 modems with taps
    in the whole window, increments that are no power of two, q = 1 .. 4 and four steps.  Every receiver of the small sets
    is compared; of the 1024 those whose margin holds, at least 90 %.  The text is the receiver's own."""
    import torch
    for W in (P.BIG_WINDOWS if nrx == 1024 else P.WINDOWS):
        bank, sel, z = P.case(W, nrx)
        ref = parity_ref(W, nrx)
        rows = [j for j in range(nrx) if ref[2][j] >= P.MARGIN]
        assert len(rows) == nrx if nrx < 1024 else len(rows) >= nrx - nrx // 10, (W, len(rows))
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, ref, rows, f"nrx {nrx} W {W}")
        read = sum(pkg.psk_varicode(got[0][j]["code"]).endswith(P.PARITY_TEXTS[j % 9]) for j in rows)
        assert read >= len(rows) - len(rows) // 4, (W, read, len(rows))   # (a fixed clock at a bad phase reads nothing)


def test_the_slowest_modem(pkg, dev):
    """psk_ref.slow_case: q = 64 at inc = 2^24, 256 samples per symbol and 256 taps, 5 receivers: the early sample lies
    128 outputs back, the whole of what is kept in front of a tile.  One batch against the reference, and cut at every
    tile seam and 2 q behind one with the same bytes."""
    import torch
    bank, sel, z = P.slow_case()
    ref = P.run_cuts(P.PskRef(bank, sel, 256), z)
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, 256)
    against_reference(one, ref, range(5), "slow")
    assert (one[2]["symbols"] == P.SLOW_SYMS + 2).all()
    n, TT = z.shape[1], pkg.psk_tile_outputs()
    assert same_bits(run(pkg, zd, bank, sel, 256, [TT] * (n // TT) + [n % TT]), one)
    assert same_bits(run(pkg, zd, bank, sel, 256, [TT + 128, 1, 127, n - TT - 256]), one)


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of psk_ref.cut_lists (batches of 0 and 1, cuts on and beside the
    kernel's tile seams, at a strobe, at strobe - q and at strobe - 2 q, forty batches of one sample): characters, sym
    and status have the same bytes.  A receiver's bytes are the same alone and among the nine, and with input, chars and
    sym rows further apart than the batch needs."""
    import torch
    bank, sel, z = P.case(W, 9)
    n, TT = z.shape[1], pkg.psk_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    ref = parity_ref(W, 9)
    against_reference(one, ref, range(9), f"W {W}")
    lists = P.cut_lists(n, TT, strobe=ref[4][0][20], q=bank[sel[0][0]][2])
    assert len(lists) == 4
    for cuts in lists:
        assert same_bits(run(pkg, zd, bank, sel, W, cuts), one), cuts
    for j in (2, 8):
        alone = run(pkg, zd[j:j + 1], bank, [sel[j]], W, lists[1])
        assert alone[0][0].tobytes() == one[0][j].tobytes() and alone[1][0].tobytes() == one[1][j].tobytes(), j
        assert alone[2][0].tobytes() == one[2][j].tobytes(), j
    wide = torch.zeros((9, n + 13), dtype=torch.complex64, device=dev)
    wide[:, :n] = zd
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    assert same_bits(run(pkg, view, bank, sel, W, lists[0], pad=7), one)
    assert same_bits(run(pkg, view, bank, sel, W), one)


def test_tile_seams(pkg, dev):
    """5 receivers (a ragged last group), series of TT - 1, TT, TT + 1 and 2 TT + 1 samples: against the reference, and
    the longest cut in two at TT - 1 and at TT with the same bytes."""
    import torch
    TT, W = pkg.psk_tile_outputs(), 16
    bank, sel, z = P.case(W, 5)
    for n in (TT - 1, TT, TT + 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(z[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel, W)
        against_reference(one, P.run_cuts(P.PskRef(bank, sel, W), z[:, :n]), range(5), f"{n} samples")
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert same_bits(run(pkg, zd, bank, sel, W, [cut, n - cut]), one), cut


# ---- receiver control --------------------------------------------------------------------------------------------------

CONTROL_CUTS = [200, 200, P.PARITY_SYMS * 16 + 48 - 400]


def control_case():
    """7 receivers of the parity series at 16 samples per symbol, W = 16, a bank of two modems (the second with step =
    inc / 8 and q = 3), three batches of 200, 200 and the remaining samples: sample 200 lies in every receiver's first
    character, sample 400 in its last.  Receiver 0 runs undisturbed; 1 is OFF throughout and its input row is NaN; 2 is
    OFF in the first batch and ON from the second; 3 is restarted in front of the second batch; 4 goes to the other modem
    in front of the third batch and 5 is switched OFF there; 6 is on the second modem from the start."""
    h, inc, q, step = P.modem(16, 16)
    bank = [(h, inc, q, step), (h, inc, 3, inc // 8)]
    sel = [(0, P.ON), (0, 0), (0, 0), (0, P.ON), (0, P.ON), (0, P.ON), (1, P.ON)]
    z = P.parity_inputs(9, 16)[:7].copy()
    z[1] = complex(np.nan, np.nan)

    def changes(at_b, at_c):
        def before(i, f):
            if i == at_b:
                f.set_rx(2, 0, P.ON)
                f.set_rx(3, 0, P.ON | P.RESTART)
            if i == at_c:
                f.set_rx(4, 1, P.ON)
                f.set_rx(5, 0, 0)
        return before
    return bank, sel, z, changes


def test_receiver_control(pkg, dev):
    """control_case against the reference given the same changes, every receiver.  The OFF receiver's NaN row is never
    read: count 0, nsym 0, status that of a fresh receiver.  The receiver switched ON reads as a fresh object fed the
    samples from there on -- starts count the object's samples, so the fresh object is given the same number of samples
    first, switched OFF.  RESTART and the modem change lose the character they fall into, the counters stay.  Another cut
    with the same change points: the same bytes."""
    import torch
    bank, sel, z, changes = control_case()
    W, (a, b, c) = 16, CONTROL_CUTS
    assert a + b + c == z.shape[1]
    ref = P.run_cuts(P.PskRef(bank, sel, W), z, CONTROL_CUTS, before=changes(1, 2))
    zd = torch.from_numpy(z).to(dev)
    got = run(pkg, zd, bank, sel, W, CONTROL_CUTS, before=changes(1, 2))
    against_reference(got, ref, range(7), "control")
    chars, sym, st = got
    assert chars[1].size == 0 and sym[1].size == 0 and not st[1:2].view(np.uint8).any()
    assert chars[2].size and chars[2]["start"].min() >= a and sym[2].shape[0] == st["symbols"][2] < sym[0].shape[0]
    assert sym[5].shape[0] == st["symbols"][5] < sym[0].shape[0]
    late = run(pkg, zd[2:3], bank, [(0, 0)], W, [a, b + c], before=lambda i, f: f.set_rx(0, 0, P.ON) if i == 1 else None)
    assert late[0][0].tobytes() == chars[2].tobytes() and late[1][0].tobytes() == sym[2].tobytes()
    assert late[2].tobytes() == st[2:3].tobytes()
    # a fresh object fed the samples from the switch on differs in the starts alone, which count the object's samples
    fresh = run(pkg, zd[2:3, a:], bank, [(0, P.ON)], W)
    assert fresh[1][0].tobytes() == sym[2].tobytes() and np.array_equal(fresh[0][0]["start"] + np.uint64(a), chars[2]["start"])
    assert fresh[0][0]["code"].tobytes() == chars[2]["code"].tobytes()
    for j in (3, 4):
        assert st["chars"][j] == len(chars[j]) and st["symbols"][j] == sym[j].shape[0] >= sym[0].shape[0] - 1
    full = run(pkg, zd[3:5], bank, [(0, P.ON)] * 2, W)
    for j in (3, 4):                                                  # what an undisturbed receiver decodes is another thing
        assert chars[j]["code"].tobytes() != full[0][j - 3]["code"].tobytes()
        assert len(chars[j]) < len(full[0][j - 3]) or not np.array_equal(chars[j]["start"], full[0][j - 3]["start"])
    other = run(pkg, zd, bank, sel, W, [1, a - 1, 0, 63, b - 63, 30, c - 30], before=changes(3, 5))
    assert same_bits(other, got)


def test_a_refused_call_changes_nothing_and_reset(pkg, dev):
    """PDDC_ECAPACITY for a chars capacity below max_chars(n), a sym capacity below max_syms(n) and a z stride below n,
    with nothing written (chars, counts, sym and nsym keep their fill); PDDC_EINVAL for misaligned or NULL pointers, a
    sym that overlaps z and a bad set_rx, between the batches: the next good batch gives the bytes of an undisturbed run.
    n = 0 sets counts and nsym to 0.  After reset the outputs repeat those after create."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = P.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 500, n - 800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert scap == (b - 1) // 15 + 1 and cap == (scap - 1) // 3 + 1   # step = inc / 4 at inc = 2^28: D = 15
        chars = torch.full((nrx, cap - 1, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        nsym = torch.full((nrx,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        sym = torch.full((nrx, scap - 1, 2), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], chars=chars, counts=counts)
        assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], counts=counts, sym=sym, nsym=nsym)
        assert e.value.code == pkg.PDDC_ECAPACITY
        torch.cuda.synchronize()
        assert (chars == 0x5A5A5A5A).all() and (counts == 0x5A5A5A5A).all() and (sym == 7.0).all() and (nsym == 0x5A5A5A5A).all()
        for rx, modem, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, 2, 1), (0, 0, 2), (0, 0, 8)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, modem, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        ch = torch.zeros((nrx, cap, 4), dtype=torch.int32, device=dev)
        sy = torch.full((nrx, scap, 2), 7.0, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_psk_process(f._h, *args, st)
        q = dict(z=zd.data_ptr(), c=ch.data_ptr(), k=counts.data_ptr(), s=sy.data_ptr(), n=nsym.data_ptr())
        assert call(q["z"], b, b - 1, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap - 1, q["k"], None, 0, None) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap - 1, q["n"]) == pkg.PDDC_ECAPACITY
        assert call(q["z"] + 4, b, n, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"] + 4, cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"] + 2, None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"] + 4, scap, q["n"]) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap, q["n"] + 2) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap, None) == pkg.PDDC_EINVAL
        assert call(None, b, n, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, None, cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, None, None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["z"] + 8 * b, 2 * n, q["n"]) == pkg.PDDC_EINVAL     # sym inside z's rows
        torch.cuda.synchronize()
        assert (counts == 0x5A5A5A5A).all() and (nsym == 0x5A5A5A5A).all() and (sy == 7.0).all() and not ch.any()
        f.process(zd[:, :0], counts=counts, sym=sy, nsym=nsym)
        torch.cuda.synchronize()
        assert not counts.any() and not nsym.any() and (sy == 7.0).all()

    got = run(pkg, zd, bank, sel, W, cuts, before=disturb)
    assert same_bits(got, clean)
    f = pkg.Psk(bank, sel, W)
    fresh = f.read()
    assert not fresh.view(np.uint8).any()
    first = [f.process(zd[:, :300], want_sym=True), f.process(zd[:, 300:], want_sym=True)]
    first = [(records(pkg, r[0], r[1]), pairs(r[2], r[3])) for r in first]
    f.reset()
    assert f.read().tobytes() == fresh.tobytes()
    chars, counts, sym, nsym = f.process(zd, want_sym=True)
    again, sagain = records(pkg, chars, counts), pairs(sym, nsym)
    for j in range(nrx):
        assert np.concatenate([first[0][0][j], first[1][0][j]]).tobytes() == again[j].tobytes() == clean[0][j].tobytes()
        assert np.concatenate([first[0][1][j], first[1][1][j]]).tobytes() == sagain[j].tobytes() == clean[1][j].tobytes()
    assert f.read().tobytes() == clean[2].tobytes()
    f.close()


def test_capacity_on_the_device(pkg, dev):
    """W = 1, h = 1, inc = 2^29 and step = inc with psk_ref.advancing_input, which turns the phase at every strobe and
    falls off towards it, so that the clock is advanced every time: strobes lie D = 7 samples apart, the closest the
    definition lets them.  Batches of every length from 0 to 2 D + 1 and of 255, 256 and 257 samples that begin on a
    strobe hold exactly max_syms(n) strobes: the bound is reached, never exceeded, and the records lie inside the capacity
    the host asked for.  The (d, x) pairs and the status are the reference's."""
    import torch
    bank, sel, z, D, first = P.advancing_case()
    assert P.distance(bank) == D == 7
    sizes = list(range(0, 2 * D + 2)) + [255, 256, 257]
    ref = P.run_cuts(P.PskRef(bank, sel, 1), z)
    strobes = np.array(ref[4][0])
    assert (np.diff(strobes) == D).all() and strobes[0] == first
    cuts, at = [first], first                                         # every batch of `sizes` begins on a strobe
    for s in sizes:
        rest = -(-s // D) * D - s
        cuts += [s, rest] if rest else [s]
        at += s + rest
    n = z.shape[1]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    f = pkg.Psk(bank, sel, 1)
    zd = torch.from_numpy(z).to(dev)
    off, sy, k0 = 0, [], []
    for i, b in enumerate(cuts):
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert scap == P.max_syms(bank, b) == ((b - 1) // D + 1 if b else 0)
        sym = torch.full((1, max(scap, 1) + 2, 2), -5.0, dtype=torch.float32, device=dev)
        chars, counts, sym, nsym = f.process(zd[:, off:off + b], sym=sym)
        k = int(nsym.cpu().numpy()[0])
        if (off - first) % D == 0 and off >= first and b in sizes and i < len(cuts) - 1:
            assert k == scap, (off, b, k, scap)
            k0.append(b)
        assert k <= scap and int(counts.cpu().numpy()[0]) <= cap and (sym.cpu().numpy()[:, max(scap, 1):] == -5.0).all(), (off, b, k)
        sy.append(pairs(sym, nsym)[0])
        off += b
    assert len(k0) >= len(sizes)
    st = f.read()
    f.close()
    got = np.concatenate(sy)
    assert got.shape == ref[1][0].shape and np.abs(got - ref[1][0]).max() <= P.TOL_PSK
    assert st["symbols"][0] == len(strobes) == ref[3]["symbols"][0] and st["acc"][0] == ref[3]["acc"][0]


# ---- non-finite samples ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """35 receivers (2 x 16 + 3) of the parity series at 16 samples per symbol, W = 16, the batches of nonfinite.cuts_for
    around the tile seams; a NaN or an infinity in rows 0, 16, 31 and 34 at the columns of nonfinite.placements.  The other
    receivers' characters, sym and status are those of the clean run bit for bit.  A poisoned row's strobes are the double
    reference's of the poisoned series, and its (d, x) pairs are within TOL_PSK of that reference wherever the reference
    is finite -- which it is once the value has left the window, the 2 q outputs in front of the strobe and the
    differential pair: W - 1 + 2 q samples and one strobe more behind the column.  One batch gives the same bytes."""
    import torch
    W, K = 16, 35
    TT = pkg.psk_tile_outputs()
    h, inc, q, step = P.modem(W, 16)
    bank, sel = [(h, inc, q, step)], [(0, P.ON)] * K
    z = P.parity_inputs(1024, 16)[:K]
    n = z.shape[1]
    rows, cols = NF.poisoned_rows(K), NF.placements(TT, W, n)
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W, cuts)
    got = run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W, cuts)
    for j in range(K):
        if j not in rows:
            assert np.isfinite(clean[1][j]).all()
            assert got[0][j].tobytes() == clean[0][j].tobytes() and got[1][j].tobytes() == clean[1][j].tobytes(), j
            assert got[2][j].tobytes() == clean[2][j].tobytes(), j
    ref = P.run_cuts(P.PskRef(bank, [sel[j] for j in rows], W), zp[rows])
    span = W - 1 + 2 * q + 2 * 17                                     # the window, the early sample, and two strobes more
    for k, j in enumerate(rows):
        m = np.array(ref[4][k])
        assert got[1][j].shape == ref[1][k].shape, (j, got[1][j].shape, ref[1][k].shape)
        far = np.ones(m.size, bool)
        for c in cols:
            far &= (m < c) | (m > c + span)
        assert far.sum() > m.size // 2 and np.isfinite(ref[1][k][far]).all()
        assert np.abs(got[1][j][far].astype(np.float64) - ref[1][k][far]).max() <= P.TOL_PSK, j
        assert got[2]["symbols"][j] == ref[3]["symbols"][k] and got[2]["acc"][j] == ref[3]["acc"][k]
        assert np.isfinite(got[2]["d_last"][j]) and np.isfinite(got[2]["x_last"][j])
    assert same_bits(run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W), got)


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed (chars, counts,
    sym and nsym still hold their canaries), the download on the null stream does not wait, and everything, read()
    included, has the bytes of the same batches on the null stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.psk_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    h, inc, q, step = P.modem(W, 16)
    bank = [(h, inc, q, step), (h, inc, 2, inc // 16)]
    sel = [(j % 2, P.ON) for j in range(K)]
    x = P.parity_inputs(1024, 16)[:K, :total]
    assert x.shape[1] == total
    scr = x.copy()
    scr[:, keep:] = x[:, keep:][:, ::-1]
    S.side_streams(dev, 1)

    def alloc(obj):
        bufs = [[S.Buf((K, obj.max_chars(b), 4), torch.int32, dev), S.Buf((K,), torch.int32, dev),
                 S.Buf((K, obj.max_syms(b), 2), torch.float32, dev), S.Buf((K,), torch.int32, dev)] for b in warm + main]
        torch.cuda.synchronize()
        return bufs

    def batches(obj, src, st, sizes, bufs, off, sync_each):
        views = []
        for b, bf in zip(sizes, bufs):
            views.append(obj.process(src[:, off:off + b], chars=bf[0].t, counts=bf[1].t, sym=bf[2].t, nsym=bf[3].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    # the clean run
    real = torch.from_numpy(x).to(dev)
    obj = pkg.Psk(bank, sel, W)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > K // 2 and sum(int(c[3].sum()) for c in clean) > 40 * K

    # the busy run
    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Psk(bank, sel, W)
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
        counts, nsym = w[1], w[3]
        assert S.same_bits(g[1], w[1]) and S.same_bits(g[3], w[3]), i
        for j in range(K):                                            # the written records (the rest is canary)
            assert S.same_bits(g[0][j, :counts[j]], w[0][j, :counts[j]]), (i, j)
            assert (g[0][j, counts[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
            assert S.same_bits(g[2][j, :nsym[j]], w[2][j, :nsym[j]]), (i, j)
            assert (g[2][j, nsym[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
    assert reads.tobytes() == clean_read.tobytes()


# ---- one radio fact ----------------------------------------------------------------------------------------------------

def test_the_text_is_read_at_the_recorded_noise_level(pkg, dev):
    """tests/test_psk_cpu.py's radio case on the device: "CQ CQ DE TEST TEST pse k" at 16 and 40 samples per symbol, the
    clock 200 ppm off either way, eight starting phases, 20 seeds, noise psk_ref.NOISE_DB below the carrier: every one of
    the 640 receivers reads the text from the second word on, in batches of 977 samples."""
    import torch
    bank, sel, z = P.radio_case(P.NOISE_DB)
    n = z.shape[1]
    cuts = [977] * (n // 977) + ([n % 977] if n % 977 else [])
    chars, sym, st = run(pkg, torch.from_numpy(z).to(dev), bank, sel, P.RADIO_W, cuts)
    bad = [j for j in range(len(sel)) if P.RADIO_WANT not in pkg.psk_varicode(chars[j]["code"])]
    assert not bad, (bad, pkg.psk_varicode(chars[bad[0]]["code"]))
