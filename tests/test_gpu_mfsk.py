"""Mfsk (pddc_mfsk_*, k_mfsk) on the GPU against the numpy reference in double (tests/mfsk_ref.py).
quality and best: within mfsk_ref.TOL_MFSK, 7 x the float32 model's worst case on the parity test's very inputs
(tests/test_mfsk_cpu.py), never taken from k_mfsk.  Records (start, tone, second, flags), counts and the integer status
(symbols, acc, skip, tone_last): exactly the reference's for every receiver whose reference margin holds -- the least
quality of its strobes and the least |b[m] - b[m - 2 q]| / (b[m] + b[m - 2 q]) that is not exactly 0 are at least
mfsk_ref.MARGIN = 4 TOL_MFSK.  Only the 1024-receiver case may leave receivers out, at most a quarter of them; everywhere
else the margin is asserted for every receiver compared.  Against itself every output has the same bits however the
series is cut: no tolerance, no exclusions."""
import numpy as np
import pytest

import mfsk_ref as R
import stream_order as S

pytestmark = pytest.mark.gpu


def records(pkg, syms, counts):
    """the device's syms [nrx, cap, 4] int32 and counts -> one SYM array per receiver"""
    c = syms.cpu().numpy().view(pkg.mfsk_sym_dtype())[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


def run(pkg, z, bank, sel, W, cuts=None, before=None, pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh Mfsk in the given batches -> (one SYM array per
    receiver, best float32 [nrx, n], status); before(i, f) is called ahead of batch i; pad > 0: syms and best are views of
    tensors whose rows lie further apart than the batch needs, filled with a pattern that must survive behind the counts"""
    import torch
    f = pkg.Mfsk(bank, sel, W)
    nrx = z.shape[0]
    parts, bs, off = [[] for _ in range(nrx)], [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        cap = f.max_syms(b)
        assert cap == R.max_syms(bank, b)
        kw = {}
        if pad:
            kw = dict(syms=torch.full((nrx, cap + pad, 4), 0x5A5A5A5A, dtype=torch.int32, device=z.device),
                      best=torch.full((nrx, b + pad), -7.0, dtype=torch.float32, device=z.device)[:, :b + pad // 2])
        syms, counts, best = f.process(z[:, off:off + b], want_best=True, **kw)
        assert counts.shape == (nrx,) and best.shape == (nrx, b) and best.dtype == torch.float32
        recs = records(pkg, syms, counts)
        if pad:
            k = counts.cpu().numpy()
            raw = syms.cpu().numpy()
            assert all((raw[j, k[j]:] == 0x5A5A5A5A).all() for j in range(nrx)), i
            assert (kw["best"].cpu().numpy()[:, b:] == -7.0).all(), i
        for j, c in enumerate(recs):
            parts[j].append(c)
        bs.append(best.cpu().numpy())
        off += b
    assert off == z.shape[1]
    st = f.read()
    f.close()
    return [np.concatenate(q) for q in parts], np.concatenate(bs, axis=1), st


def same_bits(a, b):
    """two results of run() by their bytes"""
    return (len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
            and a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def against_reference(got, ref, rows, what, margin=True):
    """best of every receiver and sample and the qualities of every receiver in `rows` within TOL_MFSK, their records and
    status as the module's header says; the receivers outside `rows` are those whose margin does not hold: their strobes
    may fall elsewhere"""
    syms, best, st = got
    rsyms, rbest, rmargin, rst, _ = ref
    assert best.shape == rbest.shape
    worst = float(np.abs(best.astype(np.float64) - rbest).max())
    print(f"{what}: |best - ref| {worst:.2e} (TOL_MFSK {R.TOL_MFSK:.2e})")
    assert worst <= R.TOL_MFSK, (what, worst)
    worst = 0.0
    for j in rows:
        if margin:
            assert rmargin[j] >= R.MARGIN, (what, j, rmargin[j])
        assert syms[j].shape == rsyms[j].shape, (what, j, syms[j].shape, rsyms[j].shape)
        for k in ("start", "tone", "second", "flags"):
            assert np.array_equal(syms[j][k], rsyms[j][k]), (what, j, k, syms[j][k], rsyms[j][k])
        if rsyms[j].size:
            worst = max(worst, float(np.abs(syms[j]["quality"].astype(np.float64) - rsyms[j]["quality"]).max()))
        for k in ("symbols", "acc", "skip", "tone_last"):
            assert st[k][j] == rst[k][j], (what, j, k, st[k][j], rst[k][j])
        assert abs(float(st["q_last"][j]) - float(rst["q_last"][j])) <= R.TOL_MFSK, (what, j)
    print(f"{what}: |quality - ref| {worst:.2e} (TOL_MFSK {R.TOL_MFSK:.2e}), {len(rows)} of {len(syms)} receivers compared")
    assert worst <= R.TOL_MFSK, (what, worst)


_REFS = {}


def parity_ref(W, nrx):
    """the double reference of case(W, .), computed once for 9 and once for 1024 receivers: the smaller sets are the
    first rows of the nine"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _REFS:
        bank, sel, z = R.case(W, key[1])
        _REFS[key] = R.run_cuts(R.MfskRef(bank, sel, W), z)
    syms, best, margin, st, strobes = _REFS[key]
    return syms[:nrx], best[:nrx], margin[:nrx], st[:nrx], strobes[:nrx]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """mfsk_ref.case(W, nrx) for W = 1, 2, 16, 255, 256 (1024 receivers: 16 and 256), one batch: one tap and two taps with
    M = 2 and 3; banks of 16 modems with M = 2, 3, 8, 31 and 32 (the odd ones run the half pair), 8 and 16 samples per
    symbol, taps in the whole window, increments that are no power of two, steps 0, inc / 64, inc / 4 and inc, q = 1 and a
    quarter symbol, every fifth receiver REVERSE, noise 20 dB below.  Every receiver of the small sets is compared; of the
    1024 those whose margin holds, at least three quarters."""
    import torch
    for W in (R.BIG_WINDOWS if nrx == 1024 else R.WINDOWS):
        bank, sel, z = R.case(W, nrx)
        ref = parity_ref(W, nrx)
        rows = [j for j in range(nrx) if ref[2][j] >= R.MARGIN]
        assert len(rows) == nrx if nrx < 1024 else len(rows) >= nrx - nrx // 4, (W, len(rows))
        got = run(pkg, torch.from_numpy(z).to(dev), bank, sel, W)
        against_reference(got, ref, rows, f"nrx {nrx} W {W}")
        assert all(R.PARITY_SYMS <= got[0][j].size <= R.PARITY_SYMS + 6 for j in rows)


def test_the_slowest_modem(pkg, dev):
    """mfsk_ref.slow_case: q = 64 at inc = 2^24, 256 samples per symbol and 256 taps, M = 8, 5 receivers: the early sample
    lies 128 results back, the whole of what is kept in front of a tile.  One batch against the reference, and cut at every
    tile seam and 2 q behind one with the same bytes."""
    import torch
    bank, sel, z = R.slow_case()
    ref = R.run_cuts(R.MfskRef(bank, sel, 256), z)
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, 256)
    against_reference(one, ref, range(5), "slow")
    n, TT = z.shape[1], pkg.mfsk_tile_outputs()
    assert same_bits(run(pkg, zd, bank, sel, 256, [TT] * (n // TT) + ([n % TT] if n % TT else [])), one)
    assert same_bits(run(pkg, zd, bank, sel, 256, [TT + 128, 1, 127, n - TT - 256]), one)


@pytest.mark.parametrize("W", [2, 16, 256])
def test_bits_against_the_cut_and_the_company(pkg, dev, W):
    """9 receivers, one batch against every cut list of mfsk_ref.cut_lists (batches of 0 and 1, cuts on and beside the
    kernel's tile seams, forty batches of one sample, cuts just before strobe - 2 q, strobe - q, a strobe and the sample
    behind it): records, best and status have the same bytes.  With set_rx between batches (a RESTART, another modem with
    REVERSE, a receiver switched OFF) two cuts that share the change point have the same bytes.  A receiver's bytes are
    the same alone, among the nine and at index 517 among 1024 others, and with input, syms and best rows further apart
    than the batch needs."""
    import torch
    bank, sel, z = R.case(W, 9)
    n, TT = z.shape[1], pkg.mfsk_tile_outputs()
    zd = torch.from_numpy(z).to(dev)
    one = run(pkg, zd, bank, sel, W)
    ref = parity_ref(W, 9)
    against_reference(one, ref, range(9), f"W {W}")
    lists = R.cut_lists(n, TT, strobe=ref[4][0][20], q=bank[sel[0][0]][2])
    assert len(lists) == 4
    for cuts in lists:
        assert same_bits(run(pkg, zd, bank, sel, W, cuts), one), cuts

    def changes(at):
        def before(i, f):
            if i == at:
                f.set_rx(1, sel[1][0], R.ON | R.RESTART)
                f.set_rx(2, (sel[2][0] + 1) % len(bank), R.ON | R.REVERSE)
                f.set_rx(3, sel[3][0], 0)
        return before
    a = run(pkg, zd, bank, sel, W, [200, n - 200], changes(1))
    b = run(pkg, zd, bank, sel, W, [1, 199, 0, 63, n - 263], changes(3))
    assert same_bits(a, b) and not same_bits(a, one)
    for j in (2, 8):
        alone = run(pkg, zd[j:j + 1], bank, [sel[j]], W, lists[1])
        assert alone[0][0].tobytes() == one[0][j].tobytes() and alone[1][0].tobytes() == one[1][j].tobytes(), j
        assert alone[2][0].tobytes() == one[2][j].tobytes(), j
    big_bank, big_sel, big_z = R.case(W, 1024)
    assert len(big_bank) == len(bank) and big_z.shape[1] == n
    big_sel, big_z = list(big_sel), big_z.copy()
    big_sel[517], big_z[517] = sel[8], z[8]
    among = run(pkg, torch.from_numpy(big_z).to(dev), bank, big_sel, W, lists[0])
    assert among[0][517].tobytes() == one[0][8].tobytes() and among[1][517].tobytes() == one[1][8].tobytes()
    assert among[2][517].tobytes() == one[2][8].tobytes()
    wide = torch.zeros((9, n + 13), dtype=torch.complex64, device=dev)
    wide[:, :n] = zd
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    assert same_bits(run(pkg, view, bank, sel, W, lists[0], pad=6), one)
    assert same_bits(run(pkg, view, bank, sel, W), one)


# ---- receiver control --------------------------------------------------------------------------------------------------

def control_case():
    """7 receivers of the nine of case(16, 9) on its bank, three batches of 200, 200 and the remaining samples.  Receiver
    0 runs undisturbed; 1 is OFF throughout and its input row is NaN; 2 is OFF in the first batch and ON from the second;
    3 is restarted in front of the second batch; 4 goes to another modem with as many tones in front of the third batch
    and 5 is switched OFF there; 6 is REVERSE from the second batch on (no restart: the flag alone)."""
    bank, sel, z = R.case(16, 9)
    sel, z = list(sel[:7]), z[:7].copy()
    sel[1], sel[2] = (sel[1][0], 0), (sel[2][0], 0)
    z[1] = complex(np.nan, np.nan)
    other = next(b for b in range(len(bank)) if b != sel[4][0] and bank[b][0].shape[0] == bank[sel[4][0]][0].shape[0])

    def changes(at_b, at_c):
        def before(i, f):
            if i == at_b:
                f.set_rx(2, sel[2][0], R.ON)
                f.set_rx(3, sel[3][0], sel[3][1] | R.RESTART)
                f.set_rx(6, sel[6][0], sel[6][1] ^ R.REVERSE)
            if i == at_c:
                f.set_rx(4, other, R.ON)
                f.set_rx(5, sel[5][0], 0)
        return before
    return bank, sel, z, changes


def test_receiver_control_and_reset(pkg, dev):
    """control_case against the reference given the same changes, every receiver whose margin holds (the undisturbed one
    and the flag change among them).  The OFF receiver's NaN row is never read: count 0, best +0, status that of a fresh
    receiver.  The receiver switched ON reads as a fresh object fed the samples from there on, the starts aside, which
    count the object's samples.  RESTART and the modem change keep the counter.  Another cut with the same change points:
    the same bytes.  After reset the outputs repeat those after create; n = 0 sets counts to 0 and moves nothing."""
    import torch
    bank, sel, z, changes = control_case()
    W, n = 16, z.shape[1]
    cuts = [200, 200, n - 400]
    ref = R.run_cuts(R.MfskRef(bank, sel, W), z, cuts, before=changes(1, 2))
    zd = torch.from_numpy(z).to(dev)
    got = run(pkg, zd, bank, sel, W, cuts, before=changes(1, 2))
    rows = [j for j in range(7) if ref[2][j] >= R.MARGIN or j == 1]
    assert {0, 1, 6} <= set(rows) and len(rows) >= 5, rows
    against_reference(got, ref, rows, "control", margin=False)
    syms, best, st = got
    assert syms[1].size == 0 and not best[1].view(np.uint32).any() and not st[1:2].view(np.uint8).any()
    assert syms[2].size and syms[2]["start"].min() >= 200 - 8 and not best[2, :200].view(np.uint32).any()
    assert st["symbols"][5] == syms[5].size < syms[0].size and not best[5, 400:].view(np.uint32).any()
    fresh = run(pkg, zd[2:3, 200:], bank, [(sel[2][0], R.ON)], W)
    assert fresh[1][0].tobytes() == best[2, 200:].tobytes() and np.array_equal(fresh[0][0]["start"] + np.uint64(200), syms[2]["start"])
    assert fresh[0][0]["tone"].tobytes() == syms[2]["tone"].tobytes() and fresh[0][0]["quality"].tobytes() == syms[2]["quality"].tobytes()
    for j in (3, 4):
        assert st["symbols"][j] == syms[j].size >= syms[0].size - 3
    other = run(pkg, zd, bank, sel, W, [1, 199, 0, 63, 137, 30, n - 430], before=changes(3, 5))
    assert same_bits(other, got)
    # reset, and the empty batch
    f = pkg.Mfsk(bank, sel, W)
    assert not f.read().view(np.uint8).any()
    a = f.process(zd[:, :300], want_best=True)
    a = (records(pkg, a[0], a[1]), a[2].cpu().numpy())
    counts = torch.full((7,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    mid = f.read()
    f.process(zd[:, :0], counts=counts)
    assert not counts.cpu().numpy().any() and f.read().tobytes() == mid.tobytes()
    f.reset()
    assert not f.read().view(np.uint8).any()
    b = f.process(zd[:, :300], want_best=True)
    b = (records(pkg, b[0], b[1]), b[2].cpu().numpy())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and a[1].tobytes() == b[1].tobytes()
    assert f.read().tobytes() == mid.tobytes()
    f.close()


def test_capacity_and_refused_calls(pkg, dev):
    """sym_stride one below max_syms(n) is PDDC_ECAPACITY, as is a z or best stride below n, with nothing queued: syms,
    counts and best keep their fill; PDDC_EINVAL for misaligned or NULL pointers, a best that overlaps z and a bad set_rx,
    between the batches: the next good batch gives the bytes of an undisturbed run.  At inc = 2^29 with step = inc, on a
    series whose early sample always wins, the strobes lie D = 7 apart and a batch holds exactly max_syms(n) of them."""
    import torch
    W, nrx = 16, 5
    bank, sel, z = R.case(W, nrx)
    n = z.shape[1]
    cuts = [300, 500, n - 800]
    zd = torch.from_numpy(z).to(dev)
    clean = run(pkg, zd, bank, sel, W, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        cap = f.max_syms(b)
        assert cap == R.max_syms(bank, b) and cap > 1
        syms = torch.full((nrx, cap - 1, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        counts = torch.full((nrx,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        best = torch.full((nrx, b - 1), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], syms=syms, counts=counts)
        assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            f.process(zd[:, :b], counts=counts, best=best)
        assert e.value.code == pkg.PDDC_ECAPACITY
        for rx, modem, flags in ((-1, 0, 1), (nrx, 0, 1), (0, -1, 1), (0, len(bank), 1), (0, 0, 8), (0, 0, 0x100)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, modem, flags)
            assert e.value.code == pkg.PDDC_EINVAL
        sy = torch.zeros((nrx, cap, 4), dtype=torch.int32, device=dev)
        be = torch.full((nrx, b), 7.0, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_mfsk_process(f._h, *args, st)
        q = dict(z=zd.data_ptr(), s=sy.data_ptr(), k=counts.data_ptr(), b=be.data_ptr())
        assert call(q["z"], b, b - 1, q["s"], cap, q["k"], None, 0) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["s"], cap - 1, q["k"], None, 0) == pkg.PDDC_ECAPACITY
        assert call(q["z"], b, n, q["s"], cap, q["k"], q["b"], b - 1) == pkg.PDDC_ECAPACITY
        assert call(q["z"] + 4, b, n, q["s"], cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["s"] + 4, cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["s"], cap, q["k"] + 2, None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["s"], cap, q["k"], q["b"] + 2, b) == pkg.PDDC_EINVAL
        assert call(None, b, n, q["s"], cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, None, cap, q["k"], None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["s"], cap, None, None, 0) == pkg.PDDC_EINVAL
        assert call(q["z"], b, n, q["s"], cap, q["k"], q["z"] + 8 * b, 2 * n) == pkg.PDDC_EINVAL      # best inside z's rows
        torch.cuda.synchronize()
        assert (syms == 0x5A5A5A5A).all() and (counts == 0x5A5A5A5A).all() and (best == 7.0).all() and (be == 7.0).all() and not sy.any()

    assert same_bits(run(pkg, zd, bank, sel, W, cuts, before=disturb), clean)
    # the bound is reached: |z| falls along the series, so the early sample is the greater at every strobe
    bank1 = [(np.array([[1.0], [0.5]], np.complex64), 1 << 29, 1, 1 << 29)]
    ramp = np.linspace(2.0, 1.0, 1200)[None].astype(np.complex64)
    ref = R.run_cuts(R.MfskRef(bank1, [(0, R.ON)], 1), ramp)
    strobes = np.array(ref[4][0])
    assert R.distance(bank1) == 7 and (np.diff(strobes) == 7).all()
    f = pkg.Mfsk(bank1, [(0, R.ON)], 1)
    rd = torch.from_numpy(ramp).to(dev)
    first = int(strobes[0])
    off, sizes, full = first, list(range(0, 16)) + [255, 256, 257], 0
    f.process(rd[:, :first])
    got = []
    for b in sizes:
        rest = -(-b // 7) * 7 - b                                     # every batch of `sizes` begins on a strobe
        for size, counted in ((b, True), (rest, False)):
            cap = f.max_syms(size)
            syms = torch.full((1, max(cap, 1) + 2, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            _, counts = f.process(rd[:, off:off + size], syms=syms)
            k = int(counts.cpu().numpy()[0])
            assert k <= cap and (syms.cpu().numpy()[0, k:] == 0x5A5A5A5A).all(), (off, size, k, cap)
            if counted:
                assert k == cap == ((size - 1) // 7 + 1 if size else 0), (off, size, k, cap)
                full += 1
            got.append(records(pkg, syms, counts)[0])
            off += size
    f.close()
    got = np.concatenate(got)
    assert full == len(sizes) and np.array_equal(got["start"], ref[0][0]["start"][:got.size])


# ---- 2G ALE ------------------------------------------------------------------------------------------------------------

def test_ale_on_the_device(pkg, dev):
    """9 receivers at 9765.625 Hz, 78.125 samples per symbol, W = 80, ale_modem: ALE_LEAD_SYMS seeded tones for the clock
    to settle on, then the three-word call of mfsk_ref.ALE_CALL, each receiver at its own starting phase, its sender up to
    200 ppm off, noise 15 dB below, in batches of 977 samples: ale_words reads TO / TIS / DATA from every receiver's
    records, and ale_text joins them."""
    import torch
    m = pkg.ale_modem(R.ALE_RATE, 80)
    tones = list(np.random.default_rng(188).integers(0, 8, R.ALE_LEAD_SYMS)) + pkg.ale_encode(R.ALE_CALL)
    n = int(78.125 * (len(tones) + 3))
    rows = []
    for j in range(9):
        z = pkg.mfsk_encode(tones, m, R.ALE_RATE, lead=20.0 + 78.125 * j / 9.0, ppm=(j - 4) * 50.0, n=n)
        rng = np.random.default_rng(600 + j)
        rows.append(z + (10.0 ** (-15.0 / 20.0) / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    z = np.stack(rows).astype(np.complex64)
    cuts = [977] * (n // 977) + ([n % 977] if n % 977 else [])
    syms, best, st = run(pkg, torch.from_numpy(z).to(dev), [m], [(0, R.ON)] * 9, 80, cuts)
    for j in range(9):
        words = [w for w in pkg.ale_words(syms[j]) if w["split"] == 0]
        assert [(w["preamble"], w["chars"]) for w in words] == R.ALE_CALL, (j, words)
        assert pkg.ale_text(words) == "TO KK6 TIS OAM89"
        assert st["symbols"][j] == syms[j].size >= len(tones)


# ---- a busy side stream ------------------------------------------------------------------------------------------------

def test_on_a_busy_side_stream(pkg, dev):
    """stream_order's harness: 37 receivers, two warm-up batches on a side stream, then 100 ms of filler, the gate, the
    real input copied over a scrambled one behind the gate, and batches of TT - 1, 1 and 2 TT + 5 samples with explicit
    outputs and nothing synchronised.  The host runs ahead, no output is touched while the gate is closed (syms, counts
    and best still hold their canaries), the download on the null stream does not wait, and everything, read() included,
    has the bytes of the same batches on the null stream with a synchronise after each."""
    import torch
    W, K = 16, S.K
    TT = pkg.mfsk_tile_outputs()
    warm, main = [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]
    keep, total = sum(warm), sum(warm) + sum(main)
    bank, sel, x = R.case(W, 1024)
    sel, x = sel[:K], np.concatenate([x[:K], x[:K, ::-1]], axis=1)[:, :total]    # (any finite series will do here)
    assert x.shape[1] == total
    scr = x.copy()
    scr[:, keep:] = x[:, keep:][:, ::-1]
    S.side_streams(dev, 1)

    def alloc(obj):
        bufs = [[S.Buf((K, obj.max_syms(b), 4), torch.int32, dev), S.Buf((K,), torch.int32, dev), S.Buf((K, b), torch.float32, dev)]
                for b in warm + main]
        torch.cuda.synchronize()
        return bufs

    def batches(obj, src, st, sizes, bufs, off, sync_each):
        views = []
        for b, bf in zip(sizes, bufs):
            views.append(obj.process(src[:, off:off + b], syms=bf[0].t, counts=bf[1].t, best=bf[2].t, stream=st))
            off += b
            if sync_each:
                torch.cuda.synchronize()
        return views, off

    # the clean run
    real = torch.from_numpy(x).to(dev)
    obj = pkg.Mfsk(bank, sel, W)
    bufs = alloc(obj)
    vw, off = batches(obj, real, 0, warm, bufs[:2], 0, True)
    vm, _ = batches(obj, real, 0, main, bufs[2:], off, True)
    clean = [[S.host(t) for t in v] for v in vw + vm]
    clean_read = obj.read()
    obj.close()
    assert sum(int(c[1].sum()) for c in clean) > 40 * K

    # the busy run
    live = torch.from_numpy(scr).to(dev)
    obj = pkg.Mfsk(bank, sel, W)
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
        for j in range(K):                                            # the written records (the rest is canary)
            assert S.same_bits(g[0][j, :counts[j]], w[0][j, :counts[j]]), (i, j)
            assert (g[0][j, counts[j]:].view(np.uint8) == S.CANARY).all(), (i, j)
    assert reads.tobytes() == clean_read.tobytes()
