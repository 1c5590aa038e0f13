"""Sitor (pddc_sitor_*, k_sitor) on the GPU against the numpy reference in double (tests/sitor_ref.py).
soft, d at every strobe: within sitor_ref.TOL_SITOR, 7 x the float32 model's worst case on the parity test's very inputs
(tests/test_sitor_cpu.py), never taken from k_sitor.  Records (start, code, flags), counts, nsoft and the integer status
(chars, symbols, errors, reframes, locked, acc, reg): exactly the reference's for every receiver whose reference margin
holds -- the least |d| over all its samples from the first full window on is at least sitor_ref.MARGIN = 4 TOL_SITOR;
quality and d_last within TOL_SITOR.  Only the 1024-receiver case may leave receivers out, at most a quarter of them;
everywhere else the margin is asserted for every receiver compared.  Against itself every output has the same bits however
the series is cut, receivers below the margin included: no tolerance, no exclusions."""
import numpy as np
import pytest

import nonfinite as NF
import sitor_ref as R
import stream_order as S

pytestmark = pytest.mark.gpu

FILL_I, FILL_F = 0x5A5A5A5A, -5.0


def records(pkg, chars, counts):
    """the device's chars [nrx, cap, 4] int32 and counts -> one CHAR array per receiver"""
    c = chars.cpu().numpy().view(pkg.sitor_char_dtype())[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


def softs(soft, nsoft):
    """the device's soft [nrx, cap] float32 and nsoft -> one array per receiver"""
    s, k = soft.cpu().numpy(), nsoft.cpu().numpy()
    assert (k >= 0).all() and (k <= s.shape[1]).all()
    return [s[j, :k[j]].copy() for j in range(s.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Sitor in the given batches -> (one CHAR array
    per receiver, one float32 array of soft values per receiver, status); before(i, f) is called ahead of batch i; pad > 0:
    chars and soft are views of filled tensors whose rows lie further apart than the batch needs, and what lies behind a
    row's records and soft values must keep the fill"""
    import torch
    f = pkg.Sitor(bank, sel, W)
    nrx = z.shape[0]
    parts, so, off = [[] for _ in range(nrx)], [[] for _ in range(nrx)], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert cap == R.max_chars(bank, b) and scap == R.max_syms(bank, b)
        kw = {}
        if pad:
            kw = dict(chars=torch.full((nrx, cap + pad, 4), FILL_I, dtype=torch.int32, device=z.device),
                      soft=torch.full((nrx, scap + pad), FILL_F, dtype=torch.float32, device=z.device))
        chars, counts, soft, nsoft = f.process(z[:, off:off + b], want_soft=True, **kw)
        assert counts.shape == (nrx,) and nsoft.shape == (nrx,) and soft.dtype == torch.float32
        if pad:
            ch, sf, k, ks = chars.cpu().numpy(), soft.cpu().numpy(), counts.cpu().numpy(), nsoft.cpu().numpy()
            for j in range(nrx):
                assert (ch[j, k[j]:] == FILL_I).all() and (sf[j, ks[j]:] == FILL_F).all(), (i, j)
        for j, (c, s) in enumerate(zip(records(pkg, chars, counts), softs(soft, nsoft))):
            parts[j].append(c)
            so[j].append(s)
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in parts], [np.concatenate(s) for s in so], st


def same_bits(a, b):
    """two results of run() by their bytes"""
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2].tobytes() == b[2].tobytes())


def against_reference(got, ref, rows, what, margin=True):
    """the soft values of every receiver in `rows` within TOL_SITOR, their records and status as the module's header says;
    the receivers outside `rows` are those whose margin does not hold: their strobes may fall elsewhere"""
    chars, soft, st = got
    rchars, rsoft, rmargin, rst = ref
    worst = 0.0
    for j in rows:
        if margin:
            assert rmargin[j] >= R.MARGIN, (what, j, rmargin[j])
        assert soft[j].shape == rsoft[j].shape, (what, j, soft[j].shape, rsoft[j].shape)
        if rsoft[j].size:
            worst = max(worst, float(np.abs(soft[j].astype(np.float64) - rsoft[j]).max()))
        for k in ("start", "code", "flags"):
            assert np.array_equal(chars[j][k], rchars[j][k]), (what, j, k, chars[j], rchars[j])
        if rchars[j].size:
            assert np.abs(chars[j]["quality"].astype(np.float64) - rchars[j]["quality"]).max() <= R.TOL_SITOR, (what, j)
        for k in R.INT_STATUS:
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        assert abs(float(st["d_last"][j]) - float(rst["d_last"][j])) <= R.TOL_SITOR, (what, j, st["d_last"][j], rst["d_last"][j])
    print(f"{what}: |soft - ref| {worst:.2e} (TOL_SITOR {R.TOL_SITOR:.2e}), {len(rows)} of {len(chars)} receivers compared")
    assert worst <= R.TOL_SITOR, (what, worst)


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = R.case(W, key[1])
        _REFS[key] = R.run_cuts(R.SitorRef(bank, sel, W), z)
    chars, soft, margin, st = _REFS[key]
    return chars[:nrx], soft[:nrx], margin[:nrx], st[:nrx]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """sitor_ref.case(W, nrx) for W = 1, 2, 16, 255, 256 (1024 receivers: 16, 255, 256), one batch: 30 character slots
    behind 4 phasing pairs at 8 and 16 samples per bit, noise 20 dB down; banks of 16 modems with taps in the whole
    window, increments that are no power of two, step 0, inc / 16, inc / 4 and inc, lock 0, 2, 3 and 4, every fifth
    receiver REVERSE on exchanged tones.  Every receiver of the small sets is compared; of the 1024 those whose margin
    holds, at least three quarters.  sitor_text reads the receiver's own text on at least three quarters of them."""
    import torch
    for W in (R.BIG_WINDOWS if nrx == 1024 else R.WINDOWS):
        bank, sel, z = R.case(W, nrx)
        ref = parity_ref(W, nrx)
        rows = [j for j in range(nrx) if ref[2][j] >= R.MARGIN]
        assert len(rows) == nrx if nrx < 1024 else len(rows) >= nrx - R.BELOW_CAP, (W, len(rows))
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, ref, rows, f"nrx {nrx} W {W}")
        assert all(got[2]["symbols"][j] == len(got[1][j]) > 200 for j in range(nrx))
        if W > 1:
            read = sum(R.reads(pkg.sitor_text(got[0][j]), R.case_text(W, j)) for j in rows)
            print(f"nrx {nrx} W {W}: {read} of {len(rows)} read their text")
            assert read >= len(rows) - len(rows) // 4, (W, read, len(rows))
        else:
            assert all(c.size == 0 for c in got[0]) and not got[2]["locked"].any()


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of sitor_ref.cut_lists (batches of 0 and 1, cuts on and beside the
    kernel's tile seams, forty batches of one sample, cuts just before, on and behind a strobe, a transition and a sample
    that is both): records, soft and status have the same bytes.  A receiver's bytes are the same alone and among the
    nine, and with input, chars and soft rows further apart than the batch needs, the padding untouched."""
    import torch
    bank, sel, z = R.case(W, 9)
    n, TT = z.shape[1], pkg.sitor_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    against_reference(one, parity_ref(W, 9), range(9), f"W {W}")
    # receiver 0's events, from the reference; a sample that is both is looked for among all nine
    strobe, trans, both = R.events(R.SitorRef(bank, sel[:1], W), z[:1])
    lists = R.cut_lists(n, TT, strobe, trans, both)
    for j in range(1, 9):
        if both is None:
            both = R.events(R.SitorRef(bank, sel[j:j + 1], W), z[j:j + 1])[2]
            lists = R.cut_lists(n, TT, strobe, trans, both)
    assert len(lists) == 6, "no sample of the nine rows is a strobe and a transition"
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
    assert same_bits(run(pkg, view, bank, sel, W, pad=3), one)


def test_tile_seams(pkg, dev):
    """5 receivers (a ragged last group), W = 16, series of 255, 256, 257, 511 and 513 samples against the reference, the
    longest cut in two at TT - 1 and at TT with the same bytes; and one receiver with hm = [1], hs = [0.5] whose inc puts a
    strobe on the last sample of a tile (inc = 2^24: samples 255 and 511) and on the first sample of one (inc = ceil(2^32
    / 257): sample 256), in one batch and cut around the seam."""
    import torch
    TT, W = pkg.sitor_tile_outputs(), 16
    assert TT == 256
    bank, sel, z = R.case(W, 5)
    for n in (TT - 1, TT, TT + 1, 2 * TT - 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(z[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel, W)
        against_reference(one, R.run_cuts(R.SitorRef(bank, sel, W), z[:, :n]), range(5), f"{n} samples")
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert same_bits(run(pkg, zd, bank, sel, W, [cut, n - cut]), one), cut
    one_tap = np.ones(1, np.complex64)
    x = R.parity_inputs(1)[:, :2 * TT + 1]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for inc, at in ((1 << 24, [255, 511]), (-(-(1 << 32) // 257), [256])):
        bank1 = [(one_tap, 0.5 * one_tap, inc, inc // 4, 3, 4)]
        got = run(pkg, xd, bank1, [(0, R.ON)], 1, pad=2)
        ref = R.SitorRef(bank1, [(0, R.ON)], 1)
        _, _, rsoft, _, where = ref.process(x, want_strobes=True)
        assert list(where[0]) == at and got[2]["symbols"][0] == len(at) and got[2]["acc"][0] == ref.read()["acc"][0], (inc, where)
        assert got[1][0].shape == rsoft[0].shape and np.abs(got[1][0] - rsoft[0]).max() <= R.TOL_SITOR
        assert same_bits(run(pkg, xd, bank1, [(0, R.ON)], 1, [TT - 1, 1, 1, TT]), got)


# ---- receiver control --------------------------------------------------------------------------------------------------

def control_case():
    """8 receivers of the parity series at 16 samples per bit, W = 16, a bank of two modems (the second with step = inc / 4
    and lock 2), three batches of 1500, 1000 and the remaining samples: both cuts lie inside a character of every
    receiver (a character is 112 samples).  Receiver 0 runs undisturbed; 1 is OFF throughout and its input row is NaN; 2 is
    OFF in the first batch and ON from the second; 3 is restarted in front of the second batch; 4 goes to the other modem
    in front of the third batch and 5 is switched OFF there; 6 is on the second modem from the start; 7 becomes REVERSE in
    front of the second batch and plain again in front of the third."""
    full = R.bank16(16)
    bank = [full[2], full[2][:3] + (full[2][2] // 4, 2, 4)]
    sel = [(0, R.ON), (0, 0), (0, 0), (0, R.ON), (0, R.ON), (0, R.ON), (1, R.ON), (0, R.ON)]
    z = np.stack([R.parity_row(j, 16, 3.0 / 32.0, 7000 + 100 * j) for j in range(8)])
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
    """control_case against the reference given the same changes, every receiver.  The OFF receiver's NaN row is never
    read: count 0, nsoft 0, status that of a fresh receiver.  The receiver switched ON reads as a fresh object fed the
    samples from there on, but for the starts, which count the object's samples.  RESTART and the modem change fall
    inside a character and lose it; read() between set_rx and the next batch shows the framing cleared as defined (RESTART:
    locked, acc and reg 0; another modem: locked and reg 0, acc kept) and the counters as they were.  Another cut with the
    same change points: the same bytes."""
    import torch
    bank, sel, z, changes = control_case()
    W, n = 16, z.shape[1]
    cuts = [1500, 1000, n - 2500]
    ref = R.run_cuts(R.SitorRef(bank, sel, W), z, cuts, before=changes(1, 2))
    assert (ref[2][[0, 2, 3, 4, 5, 6, 7]] >= R.MARGIN).all(), ref[2]
    zd = torch.from_numpy(z).to(dev)
    seen = {}

    def watched(i, f):
        before_change = f.read() if i in (1, 2) else None
        changes(1, 2)(i, f)
        if i in (1, 2):
            seen[i] = (before_change, f.read())
    got = run(pkg, zd, bank, sel, W, cuts, before=watched)
    against_reference(got, ref, [0, 2, 3, 4, 5, 6, 7], "control")
    chars, soft, st = got
    assert chars[1].size == 0 and soft[1].size == 0 and not st[1:2].view(np.uint8).any()
    counters = ("chars", "symbols", "errors", "reframes")
    was, now = seen[1]
    assert was["locked"][3] == 1 and was["acc"][3] != 0 and was["reg"][3] != 0 and was["chars"][3] > 5
    assert now["locked"][3] == 0 and now["acc"][3] == 0 and now["reg"][3] == 0 and all(now[k][3] == was[k][3] for k in counters)
    assert now[[0, 4, 5, 6, 7]].tobytes() == was[[0, 4, 5, 6, 7]].tobytes()
    was, now = seen[2]
    assert was["locked"][4] == 1 and now["locked"][4] == 0 and now["reg"][4] == 0 and now["acc"][4] == was["acc"][4] != 0
    assert all(now[k][4] == was[k][4] for k in counters)
    # the characters the changes fall into are lost: an undisturbed receiver has more of them
    full = run(pkg, zd[3:5], bank, [(0, R.ON)] * 2, W)
    for j in (3, 4):
        assert st["chars"][j] == len(chars[j]) < len(full[0][j - 3]) and st["symbols"][j] == len(soft[j])
    assert chars[2].size and chars[2]["start"].min() >= cuts[0] and len(soft[2]) == st["symbols"][2] < len(soft[0])
    assert len(soft[5]) == st["symbols"][5] < len(soft[0])
    assert st["errors"][7] > st["errors"][0]                           # a REVERSE stretch reads the complement: weight three
    fresh = run(pkg, zd[2:3, cuts[0]:], bank, [(0, R.ON)], W)
    assert fresh[1][0].tobytes() == soft[2].tobytes() and np.array_equal(fresh[0][0]["start"] + np.uint64(cuts[0]), chars[2]["start"])
    assert fresh[0][0]["code"].tobytes() == chars[2]["code"].tobytes()
    a, b, c = cuts
    other = run(pkg, zd, bank, sel, W, [1, a - 1, 0, 63, b - 63, 30, c - 30], before=changes(3, 5))
    assert same_bits(other, got)


def test_a_refused_call_changes_nothing_and_reset(pkg, dev):
    """The refusals, one by one, between the batches of a run: a misaligned pointer for each of z, chars, counts, soft and
    nsoft, a NULL z, chars, counts and (with soft) nsoft (PDDC_EINVAL); a z stride below n, a char_stride and a soft_stride
    below their bounds (PDDC_ECAPACITY), through the C ABI and through Python; a soft that overlaps z (PDDC_EINVAL); a bad
    set_rx.  Nothing is written (the outputs keep their fill), and the next good batch gives the bytes of an undisturbed
    run.  n = 0 sets counts and nsoft to 0.  After reset the outputs repeat those after create."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = R.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 1500, n - 1800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()
    D = R.distance(bank)
    assert D == (1 << 31) // R.parity_inc(8) == 4

    def disturb(i, f):
        b = cuts[i]
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert scap == (b - 1) // D + 1 and cap == (scap - 1) // 7 + 1
        chars = torch.full((nrx, cap - 1, 4), FILL_I, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), FILL_I, dtype=torch.int32, device=dev)
        nsoft = torch.full((nrx,), FILL_I, dtype=torch.int32, device=dev)
        soft = torch.full((nrx, scap - 1), FILL_F, dtype=torch.float32, device=dev)
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], chars=chars, counts=counts)
        assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], counts=counts, soft=soft, nsoft=nsoft)
        assert e.value.code == pkg.PDDC_ECAPACITY
        torch.cuda.synchronize()
        assert (chars == FILL_I).all() and (counts == FILL_I).all() and (soft == FILL_F).all() and (nsoft == FILL_I).all()
        for rx, modem, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, 16, 1), (0, 0, 8), (0, 0, 0x100)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, modem, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        ch = torch.zeros((nrx, cap, 4), dtype=torch.int32, device=dev)
        so = torch.full((nrx, scap), FILL_F, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_sitor_process(f._h, *args, st)
        q = dict(z=zd.data_ptr(), c=ch.data_ptr(), k=counts.data_ptr(), s=so.data_ptr(), n=nsoft.data_ptr())
        assert call(q["z"] + 4, b, n, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"] + 4, cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"] + 2, None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"] + 2, scap, q["n"]) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap, q["n"] + 2) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap, None) == pkg.PDDC_EINVAL
        assert call(None, b, n, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, None, cap, q["k"], None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["c"], cap, None, None, 0, None) == pkg.PDDC_EINVAL
        assert call(q["z"], b, b - 1, q["c"], cap, q["k"], None, 0, None) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap - 1, q["k"], None, 0, None) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["s"], scap - 1, q["n"]) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["c"], cap, q["k"], q["z"] + 8 * b, 2 * n, q["n"]) == pkg.PDDC_EINVAL      # soft inside z's rows
        assert call(q["z"], b, n, q["z"] + 8 * b, n // 2, q["k"], None, 0, None) == pkg.PDDC_EINVAL           # chars inside z's rows
        torch.cuda.synchronize()
        assert (counts == FILL_I).all() and (nsoft == FILL_I).all() and (so == FILL_F).all() and not ch.any()
        f.process(zd[:, :0], counts=counts, soft=so, nsoft=nsoft)
        torch.cuda.synchronize()
        assert not counts.any() and not nsoft.any() and (so == FILL_F).all()

    got = run(pkg, zd, bank, sel, W, cuts, before=disturb)
    assert same_bits(got, clean)
    f = pkg.Sitor(bank, sel, W)
    fresh = f.read()
    assert not fresh.view(np.uint8).any()
    first = [f.process(zd[:, :300], want_soft=True), f.process(zd[:, 300:], want_soft=True)]
    first = [(records(pkg, r[0], r[1]), softs(r[2], r[3])) for r in first]
    f.reset()
    assert f.read().tobytes() == fresh.tobytes()
    chars, counts, soft, nsoft = f.process(zd, want_soft=True)
    again, sagain = records(pkg, chars, counts), softs(soft, nsoft)
    for j in range(nrx):
        assert np.concatenate([first[0][0][j], first[1][0][j]]).tobytes() == again[j].tobytes() == clean[0][j].tobytes()
        assert np.concatenate([first[0][1][j], first[1][1][j]]).tobytes() == sagain[j].tobytes() == clean[1][j].tobytes()
    assert f.read().tobytes() == clean[2].tobytes()
    f.close()


def test_capacity_on_the_device(pkg, dev):
    """sitor_ref.advancing_case: the integer test's adversarial series at inc = step = 2^29 (D = 4), a decision that
    alternates at every sample of a bit's first half, keyed so that the strobes read phasing and text.  Batches of every
    length from 0 to 9 and of 255, 256 and 257 samples through the C ABI with char_stride and soft_stride exactly at the
    bounds: counts and nsoft are the reference's batch by batch, within the bounds, and the slot behind the last record
    and behind the last soft value, and the one behind the capacity, keep their fill.  soft and status are the
    reference's."""
    import torch
    bank, sel, z, _ = R.advancing_case()
    assert R.distance(bank) == 4
    n = z.shape[1]
    cuts = list(range(0, 10)) + [255, 256, 257]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    ref = R.SitorRef(bank, sel, 2)
    f = pkg.Sitor(bank, sel, 2)
    lib, st = pkg.ddc_lib(), torch.cuda.current_stream().cuda_stream
    zd = torch.from_numpy(z).to(dev)
    off, total, worst = 0, 0, 0.0
    for b in cuts:
        cap, scap = f.max_chars(b), f.max_syms(b)
        assert scap == ((b - 1) // 4 + 1 if b else 0) and cap == ((scap - 1) // 7 + 1 if b else 0)
        rc, rk, rs, _ = ref.process(z[:, off:off + b])
        chars = torch.full((1, cap + 1, 4), FILL_I, dtype=torch.int32, device=dev)
        soft = torch.full((1, scap + 1), FILL_F, dtype=torch.float32, device=dev)
        counts = torch.full((1,), FILL_I, dtype=torch.int32, device=dev)
        nsoft = torch.full((1,), FILL_I, dtype=torch.int32, device=dev)
        assert lib.pddc_sitor_process(f._h, zd.data_ptr() + 8 * off, b, n, chars.data_ptr(), cap, counts.data_ptr(), soft.data_ptr(),
                                      scap, nsoft.data_ptr(), st) == 0
        k, ks = int(counts.cpu()[0]), int(nsoft.cpu()[0])
        assert k == rk[0] <= cap and ks == len(rs[0]) <= scap, (off, b, k, rk[0], ks, len(rs[0]))
        ch, so = chars.cpu().numpy(), soft.cpu().numpy()
        assert (ch[0, k:] == FILL_I).all() and (so[0, ks:] == FILL_F).all(), (off, b)
        got = ch.view(pkg.sitor_char_dtype())[0, :k, 0]
        for name in ("start", "code", "flags"):
            assert np.array_equal(got[name], rc[0][name]), (off, b, name)
        if ks:
            worst = max(worst, float(np.abs(so[0, :ks] - rs[0]).max()))
        off, total = off + b, total + k
    assert worst <= R.TOL_SITOR and total > 20
    status, rst = f.read(), ref.read()
    f.close()
    assert all(status[k][0] == rst[k][0] for k in R.INT_STATUS) and status["locked"][0] == 1


# ---- non-finite samples ------------------------------------------------------------------------------------------------

NF_SEEDS = {0: 61000, 16: 61016, 31: 61031, 34: 61034}


def nonfinite_case(TT):
    """35 receivers (2 x 16 + 3) at 16 samples per bit, W = 16, bank16's modem 2 (step inc / 4, lock 2).  -> (bank, sel, z,
    the poisoned rows, the columns: nonfinite.placements' -- 0, W - 1, the tile seam's TT - 1 and TT, 2 TT + 3, n - 1 -- and
    a strobe, a transition and the sample behind each, of row 0's clean reference)"""
    W, K = 16, 35
    bank, sel = [R.bank16(W)[2]], [(0, R.ON)] * K
    rows = NF.poisoned_rows(K)
    z = np.stack([R.parity_row(j, 16, 3.0 / 32.0, NF_SEEDS.get(j, 60000 + j)) for j in range(K)])
    strobe, trans, _ = R.events(R.SitorRef(bank, sel[:1], W), z[:1])
    cols = sorted(set(NF.placements(TT, W, z.shape[1])) | {strobe, strobe + 1, trans, trans + 1})
    return bank, sel, z, rows, cols


@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_nonfinite_rows(pkg, dev, name):
    """nonfinite_case with a NaN or an infinity in rows 0, 16, 31 and 34 at its columns (tile seams, a strobe, a transition),
    the batches of nonfinite.cuts_for.  The other receivers' records, soft and status are those of the clean run bit for
    bit.  A poisoned row's records (start, code, flags), counts, nsoft and integer status are the double reference's of
    the poisoned series (a NaN power reads mark with d = +0 in any arithmetic; elsewhere the clean row's margin holds),
    its soft values within TOL_SITOR of it wherever both are finite.  Padded outputs keep their fill behind the records.
    RESTART gives the row back: the clean series behind it reads as on a fresh object, the counters aside.  One batch
    gives the same bytes."""
    import torch
    W = 16
    TT = pkg.sitor_tile_outputs()
    bank, sel, z, rows, cols = nonfinite_case(TT)
    K, n = z.shape
    cuts = NF.cuts_for(TT, n)
    zp = NF.plant(z, rows, cols, NF.POISON[name])
    clean = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W, cuts)
    two = np.concatenate([zp, z], axis=1)

    def restart(i, f):
        if i == len(cuts):
            for j in rows:
                f.set_rx(j, 0, R.ON | R.RESTART)
    both = run(pkg, torch.from_numpy(two).to(dev), bank, sel, W, cuts + [n], before=restart, pad=5)
    got = run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W, cuts, pad=5)
    for j in range(K):
        if j not in rows:
            assert np.isfinite(clean[1][j]).all()
            assert got[0][j].tobytes() == clean[0][j].tobytes() and got[1][j].tobytes() == clean[1][j].tobytes(), j
            assert got[2][j].tobytes() == clean[2][j].tobytes(), j
    cref = R.run_cuts(R.SitorRef(bank, [sel[j] for j in rows], W), z[rows])
    assert (cref[2] >= R.MARGIN).all(), cref[2]
    ref = R.run_cuts(R.SitorRef(bank, [sel[j] for j in rows], W), zp[rows])
    for k, j in enumerate(rows):
        assert got[1][j].shape == ref[1][k].shape, (j, got[1][j].shape, ref[1][k].shape)
        for key in ("start", "code", "flags"):
            assert np.array_equal(got[0][j][key], ref[0][k][key]), (j, key)
        for key in R.INT_STATUS:
            assert got[2][key][j] == ref[3][key][k], (j, key)
        fin = np.isfinite(ref[1][k]) & np.isfinite(got[1][j])
        assert np.array_equal(np.isnan(ref[1][k]), np.isnan(got[1][j])) and fin.sum() > fin.size // 2
        assert np.abs(got[1][j][fin].astype(np.float64) - ref[1][k][fin]).max() <= R.TOL_SITOR, j
        # RESTART: the second pass of the clean series reads as the clean run, n samples later
        back = both[0][j][both[0][j]["start"] >= n]
        assert back["code"].tobytes() == clean[0][j]["code"].tobytes() and back["flags"].tobytes() == clean[0][j]["flags"].tobytes(), j
        assert np.array_equal(back["start"], clean[0][j]["start"] + np.uint64(n)) and back["quality"].tobytes() == clean[0][j]["quality"].tobytes()
        assert both[1][j][len(got[1][j]):].tobytes() == clean[1][j].tobytes(), j
        assert both[2]["chars"][j] == got[2]["chars"][j] + clean[2]["chars"][j]
        assert both[2]["acc"][j] == clean[2]["acc"][j] and both[2]["reg"][j] == clean[2]["reg"][j]
    assert same_bits(run(pkg, torch.from_numpy(zp).to(dev), bank, sel, W), got)


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed (chars, counts,
    soft and nsoft still hold their canaries), the download on the null stream does not wait, and everything, read()
    included, has the bytes of the same batches on the null stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.sitor_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    full = R.bank16(W)
    bank = [full[2], full[1]]
    sel = [(j % 2, R.ON) for j in range(K)]
    x = np.stack([R.parity_row(j, 16, 3.0 / 32.0, 62000 + j) for j in range(K)])[:, :total]
    assert x.shape[1] == total
    scr = x.copy()
    scr[:, keep:] = x[:, keep:][:, ::-1]
    S.side_streams(dev, 1)

    def alloc(obj):
        bufs = [[S.Buf((K, obj.max_chars(b), 4), torch.int32, dev), S.Buf((K,), torch.int32, dev),
                 S.Buf((K, obj.max_syms(b)), torch.float32, dev), S.Buf((K,), torch.int32, dev)] for b in warm + main]
        torch.cuda.synchronize()
        return bufs

    def batches(obj, src, st, sizes, bufs, off, sync_each):
        views = []
        for b, bf in zip(sizes, bufs):
            views.append(obj.process(src[:, off:off + b], chars=bf[0].t, counts=bf[1].t, soft=bf[2].t, nsoft=bf[3].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    # the clean run
    real = torch.from_numpy(x).to(dev)
    obj = pkg.Sitor(bank, sel, W)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > K // 2 and sum(int(c[3].sum()) for c in clean) > 40 * K

    # the busy run
    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Sitor(bank, sel, W)
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
        counts, nsoft = w[1], w[3]
        assert S.same_bits(g[1], w[1]) and S.same_bits(g[3], w[3]), i
        for j in range(K):                                            # the written records (the rest is canary)
            assert S.same_bits(g[0][j, :counts[j]], w[0][j, :counts[j]]), (i, j)
            assert (g[0][j, counts[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
            assert S.same_bits(g[2][j, :nsoft[j]], w[2][j, :nsoft[j]]), (i, j)
            assert (g[2][j, nsoft[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
    assert reads.tobytes() == clean_read.tobytes()


# ---- one radio fact ----------------------------------------------------------------------------------------------------

def test_the_text_is_read_at_the_recorded_noise_level(pkg, dev):
    """tests/test_sitor_cpu.py's radio case on the device, a handful of its receivers: RADIO_TEXT in mode B behind 16
    phasing pairs at 16 and 40 samples per bit, the clock 200 ppm off either way, three seeds, noise sitor_ref.NOISE_DB
    below the tone: every one of the 12 receivers reads the whole message, in batches of 977 samples."""
    import torch
    bank, sel, z = R.radio_case(R.NOISE_DB, seeds=3)
    n = z.shape[1]
    cuts = [977] * (n // 977) + ([n % 977] if n % 977 else [])
    chars, soft, st = run(pkg, torch.from_numpy(z).to(dev), bank, sel, R.RADIO_W, cuts)
    bad = [j for j in range(len(sel)) if not R.reads(pkg.sitor_text(chars[j]), R.RADIO_TEXT)]
    assert not bad, (bad, pkg.sitor_text(chars[bad[0]]))
