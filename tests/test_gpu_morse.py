"""Morse (pddc_morse_*, k_morse) on the GPU against the numpy reference in double (tests/morse_ref.py).
p: within morse_ref.TOL_MORSE of the receiver's peak (the largest p of its row in the reference), 7 x the float32 model's
worst case on the parity test's very inputs (tests/test_morse_cpu.py), never taken from k_morse.  Characters, counts and
the integer status (chars, marks, two, nel, key): exactly the reference's for every receiver whose reference margin holds
-- the least distance, over the peak, of any p from the threshold it was compared with and of pk from ratio fl at a
block's end is at least morse_ref.MARGIN = 100 TOL_MORSE; pk and fl within TOL_MORSE of the peak.  Only the
1024-receiver case may leave receivers out, at most 10 % of them; everywhere else the margin is asserted for every
receiver compared.  Against itself every output has the same bits however the series is cut: no tolerance, no
exclusions."""
import numpy as np
import pytest

import morse_ref as M
import nonfinite as NF
import stream_order as S

pytestmark = pytest.mark.gpu


def records(pkg, chars, counts):
    """the device's chars [nrx, cap, 4] int32 and counts -> one CHAR array per receiver"""
    c = chars.cpu().numpy().view(pkg.morse_char_dtype())[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0, par=None):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Morse in the given batches -> (one CHAR array
    per receiver, p float32 [nrx, n] numpy, status); before(i, f) is called ahead of batch i; pad > 0: chars and p are
    views of tensors whose rows lie further apart than the batch needs"""
    import torch
    f = pkg.Morse(bank, sel, W, **(M.CASE_PARAMS if par is None else par))
    nrx = z.shape[0]
    parts, ps, off = [[] for _ in range(nrx)], [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        cap = f.max_chars(b)
        assert cap == M.max_chars(bank, b)
        kw = {}
        if pad:
            kw = dict(chars=torch.zeros((nrx, cap + pad, 4), dtype=torch.int32, device=z.device),
                      p=torch.zeros((nrx, b + pad), dtype=torch.float32, device=z.device))
        chars, counts, p = f.process(z[:, off:off + b], want_p=True, **kw)
        assert p.shape == (nrx, b) and p.dtype == torch.float32 and counts.shape == (nrx,)
        for j, c in enumerate(records(pkg, chars, counts)):
            parts[j].append(c)
        ps.append(p.cpu().numpy())
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in parts], np.concatenate(ps, axis=1), st


def same_bits(a, b):
    """two results of run() by their bytes"""
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def against_reference(got, ref, rows, what):
    """p of every receiver within TOL_MORSE of its peak; characters and status of the receivers `rows` as the module's
    header says"""
    chars, p, st = got
    rchars, rp, margin, rst, peak = ref
    scale = np.where(peak > 0, peak, 1.0)
    e = float((np.abs(p.astype(np.float64) - rp) / scale[:, None]).max()) if rp.size else 0.0
    print(f"{what}: |p - ref| / peak {e:.2e} (TOL_MORSE {M.TOL_MORSE:.2e}), {len(rows)} of {len(chars)} receivers compared exactly")
    assert e <= M.TOL_MORSE, (what, e)
    for j in rows:
        assert margin[j] >= M.MARGIN, (what, j, margin[j])
        assert chars[j].tobytes() == rchars[j].tobytes(), (what, j, chars[j], rchars[j])
        for k in ("chars", "marks", "two", "nel", "key"):
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        for k in ("pk", "fl"):
            assert abs(float(st[k][j]) - float(rst[k][j])) <= M.TOL_MORSE * scale[j], (what, j, k, st[k][j], rst[k][j])


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = M.case(W, key[1])
        _REFS[key] = M.run_cuts(M.MorseRef(bank, sel, W, **M.CASE_PARAMS), z)
    chars, p, margin, st, peak = _REFS[key]
    return chars[:nrx], p[:nrx], margin[:nrx], st[:nrx], peak[:nrx]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """morse_ref.case(W, nrx) for W = 1, 2, 16, 255, 256, one batch: one tap and two taps at
    4 samples per dot, with FIXED receivers and shift 0; one keyer at 16 samples per dot; banks of 16 keyers with taps in
    the whole window that start from 0.4, 1 and 2.5 times the true speed with shifts 0 .. 4.  Every receiver of the small
    sets is compared exactly; of the 1024 those whose margin holds, at least 90 %.  The text is the case's where it
    has one."""
    import torch
    for W in M.WINDOWS:
        bank, sel, z = M.case(W, nrx)
        ref = parity_ref(W, nrx)
        rows = [j for j in range(nrx) if ref[2][j] >= M.MARGIN]
        assert len(rows) == nrx if nrx < 1024 else len(rows) >= nrx - nrx // 10, (W, len(rows))
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, ref, rows, f"nrx {nrx} W {W}")
        for j in rows:
            want = M.case_text(W, j)
            if want is not None:
                assert pkg.morse_text(got[0][j]).endswith(want), (W, j, pkg.morse_text(got[0][j]), want)


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of morse_ref.cut_lists (batches of 0 and 1, cuts at 63, 64 and 65 and
    on and beside the kernel's tile seams, forty batches of one sample): characters, p and status have the same bytes.
    A receiver's bytes are the same alone and among the nine, and with input, chars and p rows further apart than the
    batch needs."""
    import torch
    bank, sel, z = M.case(W, 9)
    n, TT = z.shape[1], pkg.morse_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    against_reference(one, parity_ref(W, 9), range(9), f"W {W}")
    for cuts in M.cut_lists(n, TT):
        assert same_bits(run(pkg, zd, bank, sel, W, cuts), one), cuts
    for j in (2, 8):
        alone = run(pkg, zd[j:j + 1], bank, [sel[j]], W, M.cut_lists(n, TT)[1])
        assert alone[0][0].tobytes() == one[0][j].tobytes() and alone[1][0].tobytes() == one[1][j].tobytes(), j
        assert alone[2][0].tobytes() == one[2][j].tobytes(), j
    wide = torch.zeros((9, n + 13), dtype=torch.complex64, device=dev)
    wide[:, :n] = zd
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    assert same_bits(run(pkg, view, bank, sel, W, M.cut_lists(n, TT)[0], pad=7), one)
    assert same_bits(run(pkg, view, bank, sel, W), one)


def test_tile_seams(pkg, dev):
    """5 receivers (a ragged last group), series of TT - 1, TT, TT + 1 and 2 TT + 1 samples: against the reference, and
    the longest cut in two at TT - 1 and at TT with the same bytes."""
    import torch
    TT, W = pkg.morse_tile_outputs(), 16
    bank, sel, z = M.case(W, 5)
    ref = M.MorseRef(bank, sel, W, **M.CASE_PARAMS)
    for n in (TT - 1, TT, TT + 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(z[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel, W)
        ref.reset()
        against_reference(one, M.run_cuts(ref, z[:, :n]), range(5), f"{n} samples")
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert same_bits(run(pkg, zd, bank, sel, W, [cut, n - cut]), one), cut


# ---- receiver control --------------------------------------------------------------------------------------------------

CONTROL_CUTS = [460, 200, 640]


def control_case():
    """7 receivers of the parity series, W = 16, a bank of two keyers (the second starts from 2.5 times the true speed,
    shift 0), three batches of 460, 200 and 640 samples, cut where every receiver is still keying (a meter that starts
    afresh on noise alone puts its thresholds into the noise, where no margin holds).  Receiver 0 runs undisturbed; 1 is OFF
    throughout and its input row is NaN; 2 is OFF in the first batch and ON from the second; 3 is restarted in front of
    the second batch; 4 goes to the other keyer in front of the third batch and 5 is switched OFF there; 6 is FIXED on
    the second keyer from the start and keeps its two; 0 becomes FIXED in front of the third batch, which restarts
    nothing."""
    bank = [M.tailed_keyer(16, 0), M.tailed_keyer(16, 0, speed=2.5, shift=0)]
    sel = [(0, M.ON), (0, 0), (0, 0), (0, M.ON), (0, M.ON), (0, M.ON), (1, M.ON | M.FIXED)]
    z = M.parity_inputs(9)[:7].copy()
    z[1] = complex(np.nan, np.nan)

    def changes(at_b, at_c):
        def before(i, f):
            if i == at_b:
                f.set_rx(2, 0, M.ON)
                f.set_rx(3, 0, M.ON | M.RESTART)
            if i == at_c:
                f.set_rx(4, 1, M.ON)
                f.set_rx(5, 0, 0)
                f.set_rx(0, 0, M.ON | M.FIXED)
        return before
    return bank, sel, z, changes


def test_receiver_control(pkg, dev):
    """control_case against the reference given the same changes, every receiver exactly.  The OFF receiver's NaN row is
    never read: count 0, p row +0 by its bits, status that of a fresh receiver.  The receiver switched ON reads as a
    fresh object fed the samples from there on -- blocks and starts count the object's samples, so the fresh object is
    given the same number of samples first, switched OFF.  RESTART and the keyer change lose the character they fall
    into, the counters stay; FIXED keeps two.  Another cut with the same change points: the same bytes."""
    import torch
    bank, sel, z, changes = control_case()
    W, (a, b, c) = 16, CONTROL_CUTS
    ref = M.run_cuts(M.MorseRef(bank, sel, W, **M.CASE_PARAMS), z, CONTROL_CUTS, before=changes(1, 2))
    zd = torch.from_numpy(z).to(dev)
    got = run(pkg, zd, bank, sel, W, CONTROL_CUTS, before=changes(1, 2))
    against_reference(got, ref, range(7), "control")
    chars, p, st = got
    assert chars[1].size == 0 and not p[1].view(np.uint32).any()
    assert (st["chars"][1], st["marks"][1], st["two"][1], st["nel"][1], st["key"][1]) == (0, 0, bank[0][1], 0, 0)
    assert not p[2, :a].view(np.uint32).any() and not p[5, a + b:].view(np.uint32).any()
    assert chars[2].size and chars[2]["start"].min() >= a and chars[5].size and chars[5]["start"].max() < a + b
    late = run(pkg, zd[2:3], bank, [(0, 0)], W, [a, b + c], before=lambda i, f: f.set_rx(0, 0, M.ON) if i == 1 else None)
    assert late[0][0].tobytes() == chars[2].tobytes() and late[1].tobytes() == p[2:3].tobytes()
    assert late[2].tobytes() == st[2:3].tobytes()
    assert st["two"][6] == bank[1][1] and (chars[6]["two"] == bank[1][1]).all() and chars[6].size
    assert st["chars"][3] == len(chars[3]) and st["chars"][5] == len(chars[5]) and st["chars"][4] == len(chars[4])
    full = run(pkg, zd[3:5], bank, [(0, M.ON)] * 2, W)
    for j in (3, 4):                                                  # what an undisturbed receiver decodes is another thing
        assert chars[j].tobytes() != full[0][j - 3].tobytes() and (chars[j]["start"] < a).any()
    frozen = chars[0][chars[0]["start"] >= a + b]["two"]
    assert frozen.size and (frozen == st["two"][0]).all()
    other = run(pkg, zd, bank, sel, W, [1, a - 1, 0, 63, b - 63, 30, c - 30], before=changes(3, 5))
    assert same_bits(other, got)


def test_a_refused_call_changes_nothing_and_reset(pkg, dev):
    """PDDC_ECAPACITY for a chars capacity below max_chars(n) and for a z or p stride below n, with nothing written
    (chars, counts and p keep their fill); PDDC_EINVAL for misaligned or NULL pointers, a p that overlaps z and a bad
    set_rx, between the batches: the next good batch gives the bytes of an undisturbed run.  n = 0 sets the counts to 0.
    After reset the outputs repeat those after create."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = M.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 500, n - 800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        cap = f.max_chars(b)
        assert cap == (b - 1) // 9 + 1                                # two_min = 2048: 1 + 8 samples
        chars = torch.full((nrx, cap - 1, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        pp = torch.full((nrx, b), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], chars=chars, counts=counts, p=pp)
        assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], counts=counts, p=pp[:, :b - 1])
        assert e.value.code == pkg.PDDC_ECAPACITY
        torch.cuda.synchronize()
        assert (chars == 0x5A5A5A5A).all() and (counts == 0x5A5A5A5A).all() and (pp == 7.0).all()
        for rx, keyer, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, 1, 1), (0, 0, 8)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, keyer, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        ch = torch.zeros((nrx, cap, 4), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_morse_process(f._h, *args, st)
        q = dict(z=zd.data_ptr(), c=ch.data_ptr(), k=counts.data_ptr(), p=pp.data_ptr())
        assert call(q["z"], b, b - 1, q["c"], cap, q["k"], q["p"], b) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap - 1, q["k"], None, 0) == pkg.PDDC_ECAPACITY
        assert call(q["z"] + 4, b, n, q["c"], cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"] + 4, cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"] + 2, None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["p"] + 2, b) == pkg.PDDC_EINVAL
        assert call(None, b, n, q["c"], cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, None, cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, None, None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["z"] + 8 * b, 2 * n) == pkg.PDDC_EINVAL     # p inside z's rows
        torch.cuda.synchronize()
        assert (counts == 0x5A5A5A5A).all() and (pp == 7.0).all() and not ch.any()
        empty = f.process(zd[:, :0], counts=counts, want_p=True)
        torch.cuda.synchronize()
        assert not counts.any() and empty[2].shape == (nrx, 0)

    got = run(pkg, zd, bank, sel, W, cuts, before=disturb)
    assert same_bits(got, clean)
    f = pkg.Morse(bank, sel, W, **M.CASE_PARAMS)
    fresh = f.read()
    assert (fresh["two"] == bank[0][1]).all() and not any(fresh[k].any() for k in ("chars", "marks", "nel", "key", "pk", "fl"))
    first = [f.process(zd[:, :300], want_p=True), f.process(zd[:, 300:], want_p=True)]
    f.reset()
    assert f.read().tobytes() == fresh.tobytes()
    chars, counts, p = f.process(zd, want_p=True)
    again = records(pkg, chars, counts)
    parts = [records(pkg, c, k) for c, k, _ in first]
    for j in range(nrx):
        assert np.concatenate([parts[0][j], parts[1][j]]).tobytes() == again[j].tobytes() == clean[0][j].tobytes()
    assert torch.equal(torch.cat([first[0][2], first[1][2]], dim=1).view(torch.int32), p.view(torch.int32))
    assert f.read().tobytes() == clean[2].tobytes()
    f.close()


def test_capacity_on_the_device(pkg, dev):
    """W = 1, h = 1, FIXED: marks of one sample every D = 1 + gap samples on a clean line, the closest the definition
    lets characters follow each other, for two_min = 512 (D = 3) and 2049 (D = 10), side by side in one object whose
    bound is the smaller distance's.  Behind the first block, which primes the meter, every mark's sample is the
    emission sample of the mark before: batches of every length from 0 to 2 D + 1 and of 255, 256 and 257 samples that
    begin on one hold exactly max_chars(n) characters of the D = 3 receiver, one element each, D samples apart -- the
    bound is reached, never exceeded, and the records lie inside the capacity the host asked for."""
    import torch
    D = (3, 10)
    bank = [(np.ones(1, np.float32), 512, 512, 512, 0), (np.ones(1, np.float32), 2049, 2049, 2049, 0)]
    sel = [(0, M.ON | M.FIXED), (1, M.ON | M.FIXED)]
    assert M.distance(bank) == 3 and M.distance(bank[1:]) == 10
    sizes = list(range(0, 2 * D[0] + 2)) + [255, 256, 257]
    head = 90                                                         # a multiple of 3 and of 10 behind the first block
    n = head + sum(-(-s // 30) * 30 for s in sizes) + 30
    z = np.zeros((2, n), np.complex64)
    for j in range(2):
        z[j, ::D[j]] = 1.0
    ref = M.run_cuts(M.MorseRef(bank, sel, 1, **M.CASE_PARAMS), z)
    cuts = [head]
    for s in sizes:                                                   # each batch of s begins on a multiple of 30
        cuts += [s, -(-s // 30) * 30 - s] if s % 30 else [s]
    cuts.append(n - sum(cuts))
    f = pkg.Morse(bank, sel, 1, **M.CASE_PARAMS)
    zd = torch.from_numpy(z).to(dev)
    off, parts = 0, [[], []]
    for b in cuts:
        cap = f.max_chars(b)
        assert cap == M.max_chars(bank, b) == ((b - 1) // 3 + 1 if b else 0)
        chars = torch.full((2, max(cap, 1) + 2, 4), -1, dtype=torch.int32, device=dev)
        chars, counts = f.process(zd[:, off:off + b], chars=chars)
        k = counts.cpu().numpy()
        if off >= head and off % 30 == 0 and b in sizes and off + b < n - 30:
            assert k[0] == cap and k[1] == (b - 1) // 10 + 1 if b else k[0] == k[1] == 0, (off, b, k)
        assert (k <= cap).all() and (chars.cpu().numpy()[:, max(cap, 1):] == -1).all(), (off, b, k)
        for j, c in enumerate(records(pkg, chars, counts)):
            parts[j].append(c)
        off += b
    f.close()
    for j in range(2):
        c = np.concatenate(parts[j])
        assert c.tobytes() == ref[0][j].tobytes() and c.size > (n - 64) // D[j] - 3
        assert (np.diff(c["start"].astype(np.int64)) == D[j]).all() and (c["nel"] == 1).all() and (c["code"] == 2).all()


# ---- non-finite samples ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """35 receivers (2 x 16 + 3) of the parity series, W = 16, the batches of nonfinite.cuts_for around the tile seams; a
    NaN or an infinity in rows 0, 16, 31 and 34 at the columns of nonfinite.placements.  The other receivers' characters,
    p and status are those of the clean run bit for bit.  A poisoned row's p is +0 at the 16 samples whose window holds
    the value (no tap of the keyer is zero, so the power is NaN or infinite there, and the definition reads that as no
    signal) and within TOL_MORSE of the double reference of the poisoned series elsewhere: nothing is left behind once
    the value has left the window, and nothing that is not finite reaches the status.  One batch gives the same bytes."""
    import torch
    W, K = 16, 35
    TT, n = pkg.morse_tile_outputs(), M.PARITY_N
    bank = [M.tailed_keyer(W, 0)]
    sel = [(0, M.ON)] * K
    z = M.parity_inputs(1024)[:K]
    rows, cols = NF.poisoned_rows(K), NF.placements(TT, W, n)
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W, cuts)
    got = run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W, cuts)
    others = [j for j in range(K) if j not in rows]
    NF.clean_rows_identical(got[1], clean[1], others, f"morse p, {name}")
    for j in others:
        assert got[0][j].tobytes() == clean[0][j].tobytes() and got[2][j].tobytes() == clean[2][j].tobytes(), j
    ref = M.run_cuts(M.MorseRef(bank, [sel[j] for j in rows], W, **M.CASE_PARAMS), zp[rows])
    p = np.ascontiguousarray(got[1][rows])
    hit = np.zeros(n, bool)
    for c in cols:
        hit[c:c + W] = True
    assert not ref[1][:, hit].any() and np.isfinite(ref[1]).all()       # the definition's own doing
    assert not np.ascontiguousarray(p[:, hit]).view(np.uint32).any()
    assert np.isfinite(p).all() and np.isfinite(got[2]["pk"]).all() and np.isfinite(got[2]["fl"]).all()
    assert (np.abs(p.astype(np.float64) - ref[1]) / ref[4][:, None]).max() <= M.TOL_MORSE
    assert same_bits(run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W), got)


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed (chars, counts
    and p still hold their canaries), the download on the null stream does not wait, and everything, read() included,
    has the bytes of the same batches on the null stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.morse_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    bank = [M.tailed_keyer(W, 0), M.tailed_keyer(W, 1, speed=0.4)]
    sel = [(j % 2, M.ON | (M.FIXED if j % 5 == 0 else 0)) for j in range(K)]
    x = M.parity_inputs(1024)[:K, :total]
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
            views.append(obj.process(src[:, off:off + b], chars=bf[0].t, counts=bf[1].t, p=bf[2].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    # the clean run
    real = torch.from_numpy(x).to(dev)
    obj = pkg.Morse(bank, sel, W, **M.CASE_PARAMS)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > K                    # characters were decoded in these batches

    # the busy run
    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Morse(bank, sel, W, **M.CASE_PARAMS)
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
