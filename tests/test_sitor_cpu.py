"""The SITOR decoder without a GPU: the numpy reference (tests/sitor_ref.py) against itself and against the facts of the
radio it is for.  TOL_SITOR and MARGIN are measured and asserted here, on the GPU tests' own inputs; the seeds of the small
sets, the cap on receivers below the margin and the noise level of the radio facts are checked on the reference alone.
Nothing here runs k_sitor."""
import difflib

import numpy as np

import sitor_ref as R


def test_the_table_and_the_helpers(pkg):
    """The M.476 table as the project holds it: 35 codes, all of weight four, all distinct -- every 7-bit word of weight four
    there is; the package's table is the reference's; sitor_encode gives the reference's slots and bits; sitor_modem the
    reference's modem; the dtypes are the header's records."""
    codes = list(R.LETTERS.values()) + list(R.OTHERS.values())
    assert len(codes) == 35 and len(set(codes)) == 35 and all(R.weight(c) == 4 and 0 <= c < 128 for c in codes)
    assert sorted(codes) == [c for c in range(128) if R.weight(c) == 4]
    assert pkg._SITOR_LETTERS == R.LETTERS and (pkg.SITOR_ALPHA, pkg.SITOR_BETA, pkg.SITOR_REPEAT) == (R.ALPHA, R.BETA, R.REPEAT)
    assert (pkg._SITOR_LTRS, pkg._SITOR_FIGS, pkg._SITOR_BLANK) == (R.LTRS, R.FIGS, R.BLANK)
    for text, ph in ((R.TEXT, 16), (R.RADIO_TEXT, 4), ("", 3), ("A", 0), ("1", 1)):
        a, b = pkg.sitor_encode(text, ph), R.encode(text, ph)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), text
        assert a[1].size == 7 * a[0].size and all(R.weight(c) == 4 for c in a[0])
    slots, _ = pkg.sitor_encode("AB", 2)
    assert list(slots) == [R.BETA, R.ALPHA, R.BETA, R.ALPHA, 0x47, R.ALPHA, 0x72, R.ALPHA, R.BETA, 0x47, R.BETA, 0x72, R.BETA, R.ALPHA]
    for W, sps in ((16, 16), (40, 40), (64, 16), (256, 100.0), (33, 8), (256, 1000.5)):
        a, b = pkg.sitor_modem(W, sps), R.modem(W, sps)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:], (W, sps)
        assert 1 <= a[2] <= 1 << 29 and a[3] == a[2] // 8 and a[4:] == (3, 4)
    assert pkg.sitor_modem(16, 8)[2] == 1 << 29 and pkg.sitor_modem(16, 16, step=5, lock=0, unlock=9)[3:] == (5, 0, 9)
    assert pkg.sitor_char_dtype() == R.CHAR and pkg.sitor_status_dtype() == R.STATUS and pkg.sitor_char_dtype().itemsize == 16
    assert pkg.sitor_status_dtype().itemsize == 32


def test_round_trip_through_the_framing(pkg):
    """sitor_encode -> bits -> the reference's framing -> sitor_text: every character of the table (letters, figures,
    space, CR, LF) comes back; with a DX or an RX copy damaged (one bit turned: weight three or five) in every slot of the
    message in turn it still reads; with both copies of a character damaged that character is U+FFFD and the rest
    reads; records dropped from the list do not shift the pairing; an empty list reads as nothing."""
    every = "".join(sorted(set(pkg._ITA2_LTRS + pkg._ITA2_FIGS) - set("\x00\x0e\x0f")))
    assert len(every) >= 55
    for text in (R.TEXT, every, "NNNN"):
        slots, bits = pkg.sitor_encode(text, 4)
        rec, f = R.frame_bits(bits)
        assert f.locked and len(rec) >= len(slots) - 4 and (rec["flags"] == R.VALID).all()
        assert pkg.sitor_text(rec) == text.upper()
    text = "CQ DE NAVTEX K"                                           # no shifts: a lost character costs itself alone
    slots, bits = pkg.sitor_encode(text, 4)
    clean, _ = R.frame_bits(bits)
    assert pkg.sitor_text(clean) == text
    first = 2 * 4                                                     # the first slot of the message
    for k in sorted(first + 2 * i + o for i in range(len(text)) for o in (0, 5)):     # every DX and every RX copy
        b = bits.copy()
        b[7 * k + k % 7] ^= 1
        rec, _ = R.frame_bits(b)
        assert len(rec) == len(clean) and (rec["flags"] == 0).sum() == 1
        assert pkg.sitor_text(rec) == text, k
    for i in range(len(text)):
        b = bits.copy()
        for k in (first + 2 * i, first + 2 * i + 5):
            b[7 * k + 3] ^= 1
        assert pkg.sitor_text(R.frame_bits(b)[0]) == text[:i] + "\ufffd" + text[i + 1:], i
    # records dropped from the list: the pairing goes by the start samples
    keep = np.ones(len(clean), bool)
    keep[[first + 1, first + 2, first + 3, first + 9]] = False
    assert pkg.sitor_text(clean[keep]) == text
    assert pkg.sitor_text(clean[:0]) == "" and pkg.sitor_text(clean[:1]) == ""


def test_the_reference_is_independent_of_the_cut():
    """The streaming reference against itself: case(16, 5) in one batch and in cut_lists' batches gives the same records,
    soft values and status; the float32 model's d at the strobes (model_d_at) is the streaming float32 model's soft."""
    bank, sel, z = R.case(16, 5)
    z = z[:, :1400]
    one = R.run_cuts(R.SitorRef(bank, sel, 16), z)
    strobe, trans, both = R.events(R.SitorRef(bank, sel[:1], 16), z[:1])
    for cuts in R.cut_lists(z.shape[1], 256, strobe, trans, both):
        got = R.run_cuts(R.SitorRef(bank, sel, 16), z, cuts)
        for j in range(5):
            assert got[0][j].tobytes() == one[0][j].tobytes() and np.array_equal(got[1][j], one[1][j]), (cuts, j)
        assert got[3].tobytes() == one[3].tobytes()
    r32 = R.SitorRef(bank, sel, 16, f32=True)
    chars, counts, soft, margin, where = r32.process(z, want_strobes=True)
    model = R.model_d_at(bank, sel, 16, z, where)
    for j in range(5):
        assert soft[j].dtype == np.float32 and soft[j].tobytes() == model[j].tobytes(), j
        assert np.array_equal(chars[j]["code"], one[0][j]["code"])


def test_float32_model_against_double(pkg):
    """The float32 model against the double reference on the GPU parity test's own inputs (sitor_ref's header): the worst
    |d_model - d_ref| at the strobes per window is the figure written into MODEL_WORST, TOL_SITOR is 7 x the largest,
    MARGIN 4 x that.  The same runs show what the GPU tests rely on: every receiver of the small sets keeps a margin of at
    least MARGIN, and of the 1024 at most a quarter fall below it."""
    worst = {}
    for nrx in (9, 1024):
        for W in (R.WINDOWS if nrx == 9 else R.BIG_WINDOWS):
            bank, sel, z = R.case(W, nrx)
            chars, counts, soft, margin, where = R.SitorRef(bank, sel, W).process(z, want_strobes=True)
            model = R.model_d_at(bank, sel, W, z, where)
            below = int((margin < R.MARGIN).sum())
            print(f"nrx {nrx} W {W}: least margin {margin.min():.3e} (MARGIN {R.MARGIN:.3e}), {below} below")
            assert below == 0 if nrx == 9 else below <= R.BELOW_CAP, (nrx, W, below)
            assert all(len(s) > 200 for s in soft)
            w = max(float(np.abs(model[j].astype(np.float64) - soft[j]).max()) for j in range(nrx))
            worst[W] = max(worst.get(W, 0.0), w)
            if W > 1:
                read = sum(R.reads(pkg.sitor_text(chars[j]), R.case_text(W, j)) for j in range(nrx))
                print(f"nrx {nrx} W {W}: {read} read their text")
                assert read >= nrx - nrx // 4
    for k, v in worst.items():
        print(f"W = {k}: worst |d_model32 - d_ref| at the strobes {v:.3e} (written {R.MODEL_WORST[k]:.3e})")
        assert abs(v - R.MODEL_WORST[k]) <= 0.0005 * R.MODEL_WORST[k] + 1e-12, k
    assert R.MODEL_WORST_SITOR == max(R.MODEL_WORST.values())
    assert R.TOL_SITOR == 7 * R.MODEL_WORST_SITOR and R.MARGIN == 4 * R.TOL_SITOR and R.BELOW_CAP == 1024 // 4


def test_margins_of_the_other_gpu_cases(pkg):
    """The cases of tests/test_gpu_sitor.py that compare every receiver, run on the reference alone: the tile seam lengths,
    the control case with its changes, the rows the non-finite test poisons, the refusal test's rows.  Every receiver
    keeps MARGIN, and the control case does what its text says: both change points lie inside a character, RESTART and the
    modem change lose it, the REVERSE stretch gives errors."""
    import test_gpu_sitor as G
    bank, sel, z = R.case(16, 5)
    for n in (255, 256, 257, 511, 513):
        assert (R.run_cuts(R.SitorRef(bank, sel, 16), z[:, :n])[2] >= R.MARGIN).all(), n
    bank, sel, z, changes = G.control_case()
    cuts = [1500, 1000, z.shape[1] - 2500]
    chars, soft, margin, st = R.run_cuts(R.SitorRef(bank, sel, 16), z, cuts, before=changes(1, 2))
    print("control margins", margin)
    rows = [0, 2, 3, 4, 5, 6, 7]
    assert (margin[rows] >= R.MARGIN).all(), margin
    full = R.run_cuts(R.SitorRef([bank[0]], [(0, R.ON)] * 8, 16), np.nan_to_num(z))
    for j, cut in ((3, cuts[0]), (4, cuts[0] + cuts[1])):
        s = full[0][j]["start"].astype(np.int64)
        assert ((s < cut) & (cut <= s + 96)).any(), (j, cut)          # the change falls between a character's first and last strobe
        assert len(chars[j]) < len(full[0][j]) and len(chars[j]) == st["chars"][j]
    assert st["errors"][7] > st["errors"][0] and chars[1].size == 0 and st["symbols"][1] == 0
    assert R.reads(pkg.sitor_text(chars[0]), R.parity_text(0))
    bank, sel, z, rows, cols = G.nonfinite_case(256)
    margin = R.run_cuts(R.SitorRef(bank, [sel[j] for j in rows], 16), z[rows])[2]
    print("non-finite rows' margins", margin, "columns", cols)
    assert (margin >= R.MARGIN).all() and len(cols) >= 9


def test_capacity_bounds_on_the_reference():
    """Strobes and records never exceed pddc_sitor_max_syms and pddc_sitor_max_chars over every window of a parity series
    and of the adversarial series (advancing_case: the decision alternates at every sample of a first half, the strobes
    read phasing and text); how near the bound that series comes: its strobes lie 6 or 7 samples apart against D = 4
    (behind the first, which the tie of sample 0 delays)."""
    bank, sel, z, sp = R.advancing_case()
    assert R.distance(bank) == 4
    r = R.SitorRef(bank, sel, 2)
    chars, counts, soft, margin, where = r.process(z, want_strobes=True)
    # the filters turn the keyed series into the decisions it was made from (sample 0: the tie of zero history reads mark)
    space = R.fsk_ref.FskRef([(bank[0][0], bank[0][1], 1, 5)], [(0, R.ON)], 2).discriminate(z)[0][0]
    assert np.array_equal(space[1:], sp[1:])
    gaps = np.diff(where[0])
    print(f"adversarial series: strobe distances {gaps.min()} .. {gaps.max()} against D = 4, {counts[0]} records")
    assert gaps.min() == 6 and gaps[1:].max() <= 7 and counts[0] > 20 and r.read()["locked"][0] == 1
    assert all(r == (R.VALID) for r in chars[0]["flags"][:20])
    ends = chars[0]["start"].astype(np.int64)                          # a record per seven strobes: the starts count like the emissions
    for n in (1, 2, 3, 4, 5, 6, 7, 28, 29, 255, 256, 257):
        for a in range(0, z.shape[1] - n):
            assert int(((where[0] >= a) & (where[0] < a + n)).sum()) <= R.max_syms(bank, n), (n, a)
            assert int(((ends >= a) & (ends < a + n)).sum()) <= R.max_chars(bank, n), (n, a)
    bank, sel, z = R.case(16, 9)
    chars, counts, soft, margin, where = R.SitorRef(bank, sel, 16).process(z, want_strobes=True)
    for j in range(9):
        for n in (1, 3, 4, 5, 16, 112, 255, 977):
            for a in range(0, z.shape[1] - n, 3):
                assert int(((where[j] >= a) & (where[j] < a + n)).sum()) <= R.max_syms(bank, n)
    assert R.max_syms(bank, 0) == 0 and R.max_chars(bank, 0) == 0 and R.max_chars(bank, 1) == 1
    assert R.max_syms(bank, 977) == 245 and R.max_chars(bank, 977) == 35


def test_radio_facts(pkg):
    """RADIO_TEXT in mode B behind 16 phasing pairs, 170 Hz shift at 100 baud, at 16 and 40 samples per bit, the clock 200
    ppm off either way, 20 seeds with five leads, 80 receivers, W = 40, step = inc / 8, lock 3, unlock 4; noise in the
    sample rate's bandwidth.  On the reference:
      NOISE_DB = 5: every receiver reads the whole message with the noise 5 dB below the tone; at 4 dB one does not.
      step = 0 at NOISE_DB: the fixed clock drifts 200 ppm x 1900 bits = 0.4 bit and a quarter of the receivers lose the
        message's end (58 of 80 read it whole).
      A receiver that joins mid-message (behind the phasing and ten characters): with lock = 0 it reads nothing, with
        lock = 3 it locks on three valid characters and reads the rest (75 of 80 read the last 14 characters).
      Without rule b (lock = 3 alone) 12 of 80 lock at a wrong bit phase on the phasing sequence and lose 5 to 9 characters
        of the message's beginning before four invalid characters unlock them."""
    def read(snr, rule_b=True, **kw):
        bank, sel, z = R.radio_case(snr, **kw)
        chars = R.SitorRef(bank, sel, R.RADIO_W, rule_b=rule_b).process(z)[0]
        return [pkg.sitor_text(c) for c in chars]

    def lost(t):
        blocks = difflib.SequenceMatcher(None, t, R.RADIO_TEXT, autojunk=False).get_matching_blocks()
        return len(R.RADIO_TEXT) - sum(b.size for b in blocks)

    texts = read(R.NOISE_DB)
    assert len(texts) == 80 and all(R.reads(t, R.RADIO_TEXT) for t in texts)
    worse = read(R.NOISE_DB - 1.0)
    print(f"noise {R.NOISE_DB - 1.0} dB down: {sum(R.reads(t, R.RADIO_TEXT) for t in worse)} of 80 read the message")
    assert not all(R.reads(t, R.RADIO_TEXT) for t in worse)
    fixed = read(R.NOISE_DB, step_div=0)
    whole = sum(R.reads(t, R.RADIO_TEXT) for t in fixed)
    print(f"step = 0: {whole} of 80 read the message; characters lost by the others: {sorted(lost(t) for t in fixed if not R.reads(t, R.RADIO_TEXT))}")
    assert whole <= 70
    cut = (32 + 21) * 7 + 3
    never, late = read(R.NOISE_DB, lock=0, cut_bits=cut), read(R.NOISE_DB, lock=3, cut_bits=cut)
    tail = R.RADIO_TEXT[-14:]
    print(f"joining mid-message: lock 0 reads {sum(t != '' for t in never)} texts, lock 3 reads the tail on {sum(tail in t for t in late)} of 80")
    assert all(t == "" for t in never) and sum(tail in t for t in late) >= 72
    plain = read(R.NOISE_DB, rule_b=False)
    cost = sorted(lost(t) for t in plain if not R.reads(t, R.RADIO_TEXT))
    print(f"without rule b: {len(cost)} of 80 lose characters: {cost}")
    assert len(cost) >= 5 and cost[0] >= 3
