"""What the references themselves do with non-finite samples (no GPU): the header's sentences checked by hand on a few
samples, the kind of damage per stage and poison value -- transient, healing or sticky; every assertion of
tests/test_gpu_nonfinite.py relies on one of them --, that rows without poison are untouched, and that the references'
edits for NaN (np.fmin / np.fmax, errstate, a NaN step) changed no bit on the inputs the other tests feed them."""
import warnings

import numpy as np
import pytest

import adapt_ref as AR
import blanker_ref as BR
import carrier_ref as CR
import channelizer_ref as HR
import demod_ref as DR
import eq_ref as ER
import nonfinite as NF
import rxfilter_ref as RR
import spectrum_ref as R
import squelch_ref as QR
import tuner_ref as TR
import test_gpu_nonfinite as G
from test_gpu_nonfinite import CASES, CLEAN, PARTS, ROWS, STAGES, case_ids, layout_columns, squelch_cases, values_of

F32 = np.float32
NAN, INF = NF.QNAN, F32(np.inf)


# ---- the helper module ----------------------------------------------------------------------------------------------

def test_helpers():
    """the fill pattern, plant, and the two comparisons: same_or_both_nan tells a NaN from a number, a sign of zero and
    an infinity's sign, takes NaNs of any sign and payload for one another and refuses to compare NaNs alone;
    clean_rows_identical refuses rows that are not finite"""
    f = NF.never_read((3, 5), np.float32)
    assert f.view(np.uint32).reshape(-1).tolist() == [0xFFFFFFFF, 0x7FC00000] * 7 + [0xFFFFFFFF] and np.isnan(f).all()
    assert np.isnan(NF.never_read((2, 3), np.complex64).view(F32)).all() and NF.never_read((2, 3), np.int16).shape == (2, 3)
    x = np.arange(12, dtype=F32).reshape(3, 4)
    y = NF.plant(x, [0, 2], [1, 3], NAN)
    assert np.isnan(y[[0, 2]][:, [1, 3]]).all() and np.isfinite(x).all() and np.array_equal(y[1], x[1])
    z = NF.plant(x.astype(np.complex64), [1], [2], INF, "im")
    assert z[1, 2].real == 6 and np.isposinf(z[1, 2].imag)
    assert NF.placements(256, 64, 773) == [0, 63, 255, 256, 515, 772] and NF.cuts_for(256, 773) == [1, 255, 1, 259, 0, 257]
    assert NF.placements(52, 64, 773, 104) == [0, 51, 52, 63, 104, 772] and NF.cuts_for(52, 773, 104) == [1, 51, 1, 52, 0, 668]
    assert NF.poisoned_rows(35) == [0, 16, 31, 34]
    a = np.array([1.0, np.nan, -0.0, np.inf], F32)
    other_nan = a.copy()
    other_nan.view(np.uint32)[1] = 0xFFC00001
    NF.same_or_both_nan(other_nan, a)
    for bad in ([1.0, 2.0, -0.0, np.inf], [1.0, np.nan, 0.0, np.inf], [1.0, np.nan, -0.0, -np.inf], [np.nan, np.nan, -0.0, np.inf]):
        with pytest.raises(AssertionError):
            NF.same_or_both_nan(np.array(bad, F32), a)
    with pytest.raises(AssertionError):
        NF.same_or_both_nan(np.array([np.nan], F32), np.array([np.nan], F32))
    NF.clean_rows_identical(a, a.copy(), [0, 2])
    with pytest.raises(AssertionError):
        NF.clean_rows_identical(a, a.copy(), [0, 1])
    with pytest.raises(AssertionError):
        NF.clean_rows_identical(np.array([0.0], F32), np.array([-0.0], F32), [0])


# ---- the header's sentences, by hand --------------------------------------------------------------------------------

def test_squelch_sentences_by_hand():
    """B = 1, attack 1, hang 2, R = 1, GATE, thresholds 4 / 2 (absolute), five samples of power 9, NaN, 9, 1, 1:
    block 0: closed, L = 9 >= 4: opens.  block 1: L = NaN, open: !(NaN >= 2) is true, run = 1 -- `L < tc` would say 0.
    block 2: L = 9: run = 0.  blocks 3, 4: L = 1 < 2: run = 1, 2: closes.  peak = fmaxf(peak, NaN) stays 9.
    And `c == 0: out = +0.0f whatever a is`: sample 0 is gated shut (c = 0) with a = NaN and gives +0 bits."""
    z = np.array([[3.0, NAN, 3.0, 1.0, 1.0]], np.complex64)
    a = np.array([[NAN, 5.0, NAN, 7.0, -8.0]], F32)
    out, lv, st, status, _ = QR.squelch_ref(z, a, [(4.0, 2.0, QR.GATE)], block=1, attack=1, hang=2, ramp=1)
    assert st.tolist() == [[1, 1, 1, 1, 0]]
    assert lv[0, 0] == 9 and np.isnan(lv[0, 1]) and lv[0, 2:].tolist() == [9, 1, 1]
    assert out.view(np.uint32)[0, 0] == 0                      # closed, a = NaN: +0
    assert out[0, 1] == 5 and np.isnan(out[0, 2]) and out[0, 3] == 7 and out[0, 4] == -8
    assert status["peak"][0] == 9 and status["level"][0] == 1 and status["opens"][0] == 1
    # one NaN block more and hang = 2 is reached by NaN blocks alone
    z2 = np.array([[3.0, NAN, NAN, 3.0]], np.complex64)
    st2 = QR.squelch_ref(z2, np.ones((1, 4), F32), [(4.0, 2.0, QR.GATE)], block=1, attack=1, hang=2, ramp=1)[2]
    assert st2.tolist() == [[1, 1, 0, 1]]
    # closed, a NaN level never opens and leaves the floor to f up
    z3 = np.array([[1.0, NAN, 1.0]], np.complex64)
    r3 = QR.squelch_ref(z3, np.ones((1, 3), F32), [(4.0, 2.0, QR.GATE)], block=1, attack=1, hang=1, ramp=1, up=2.0)
    assert not r3[2].any() and r3[3]["floor"][0] == 1.0 and not r3[0].view(np.uint32).any()


def test_blanker_sentences_by_hand():
    """B = 2, W = R = 0, thr 4, beta 1, cap 2.  `p > ref thr` with p = NaN is false: no trigger; with ref = inf it is
    false for every finite p.  A NaN block sum: x = fminf(NaN, ref cap) = ref cap, so ref doubles and stays finite.  An
    infinite first block (ref = 0: ref = L) makes ref = inf; the next block's x - ref = -inf gives ref = NaN, `ref > 0`
    is false and the block after that starts again from its own L."""
    par = dict(block=2, guard=0, ramp=0, beta=1.0, cap=2.0)
    z = np.array([[1.0, 1.0, NAN, 1.0, 1.0, 1.0, 3.0, 1.0]], np.complex64)
    out, st, r = BR.blanker_ref(z, [(4.0, BR.ON)], **par)
    assert not r.t[0, :6].any() and r.refs[0].tolist() == [0, 0, 1, 1, 2, 2, 1, 1] and r.t[0, 6] and st["triggers"][0] == 1
    assert np.isnan(out[0, 2]) and out.view(np.uint32)[0, 12:14].tolist() == [0, 0] and st["ref"][0] == 2.0
    zi = np.array([[INF, 1.0, 50.0, 1.0, 50.0, 1.0, 50.0, 1.0, 50.0, 1.0]], np.complex64)
    out, st, r = BR.blanker_ref(zi, [(4.0, BR.ON)], **par)
    assert np.isposinf(r.refs[0, 2:4]).all() and np.isnan(r.refs[0, 4:6]).all() and r.refs[0, 6] == F32(2501.0 / 2)
    assert not r.t[0, :8].any() and np.isfinite(st["ref"][0])


def test_demod_sentences_by_hand():
    """e = fmaxf(|NaN|, lambda e) = lambda e: the AGC's envelope steps over a NaN sample, one output is NaN and the next
    one is what it would have been after a sample of magnitude <= lambda e.  An infinite sample: e = inf, the gain
    target / inf = 0, and e stays inf (lambda inf): every later output is 0.  With the DC block the NaN is in y and
    stays there.  In double as in float32."""
    P = dict(rho=0.5, lam=0.5, target=1.0, gmax=100.0)
    z = np.array([[4.0, NAN, 1.0, 1.0]], np.complex64)
    for f32 in (False, True):
        r = DR.DemodRef([(DR.AM, 0, DR.AGC)], f32=f32, **P)
        out = r.process(z)
        assert r.e[0].tolist()[:1] == [4.0] and r.e[0, 1] == 2.0 and r.e[0, 2] == 1.0 and r.e[0, 3] == 1.0
        assert out[0, 0] == 1.0 and np.isnan(out[0, 1]) and out[0, 2] == 1.0 and out[0, 3] == 1.0
        zi = np.array([[4.0, INF, 1.0, 1.0]], np.complex64)
        r = DR.DemodRef([(DR.AM, 0, DR.AGC)], f32=f32, **P)
        out = r.process(zi)
        assert np.isposinf(r.e[0, 1:]).all() and np.isnan(out[0, 1]) and out[0, 2:].tolist() == [0.0, 0.0]
        out = DR.DemodRef([(DR.AM, 0, DR.DC)], f32=f32, **P).process(z)
        assert out[0, 0] == 4.0 and np.isnan(out[0, 1:]).all()
    # the issue's figure: AM + AGC, a NaN at output 10 of 50 gives exactly one NaN output
    zz = np.ones((1, 50), np.complex64)
    zz[0, 10] = NAN
    out = DR.demod_model_f32(zz, [(DR.AM, 0, DR.AGC)], **DR.PARAMS)
    assert np.flatnonzero(np.isnan(out[0])).tolist() == [10]


def test_carrier_sentences_by_hand():
    """A NaN sample: w and e are NaN; v = fminf(vmax, fmaxf(-vmax, NaN)) = -vmax; the step is NaN and adds 0 to theta;
    q = fmaf(gamma, |NaN| - q, q) is NaN and stays NaN, so locked reads 0.  The loop itself goes on from v = -vmax.
    An infinite sample: with one infinite part the angle is a finite number and q stays finite; with both parts infinite
    w is NaN and everything is as after a NaN."""
    z = np.array([[1.0 + 0.5j, 1.0 + 0.4j, NAN, 1.0 + 0.3j, 1.0 + 0.2j]], np.complex64)
    for f32 in (False, True):
        r = CR.CarrierRef([(CR.DSB, 0.25, 0.0625)], CR.hilbert(3), f32=f32, **CR.PARAMS)
        r.process(z[:, :2])
        before = r.read().copy()
        u = r.process(z[:, 2:3])
        st = r.read()
        assert np.isnan(u.view(r.ft)).all() and st["theta"][0] == before["theta"][0] and st["theta"][0] != 0
        assert st["freq"][0] == -F32(CR.PARAMS["vmax"]) and np.isnan(st["err"][0]) and st["locked"][0] == 0
        u = r.process(z[:, 3:])
        st = r.read()
        assert np.isfinite(u.view(r.ft)).all() and st["theta"][0] != before["theta"][0]
        assert -0.25 < st["freq"][0] < 0.25 and np.isnan(st["err"][0]) and st["locked"][0] == 0
        # an infinity, part by part, once theta is no longer 0 (c and s are ordinary numbers): one infinite part gives
        # w = (+-inf, +-inf), e is the finite angle of that and q stays finite; both parts infinite give
        # inf c - inf s = NaN, and q is NaN as after a NaN sample
        for bad, sticky in ((complex(np.inf, 0.3), False), (complex(1.0, -np.inf), False), (complex(np.inf, np.inf), True),
                            (complex(-np.inf, np.inf), True)):
            r = CR.CarrierRef([(CR.DSB, 0.25, 0.0625)], CR.hilbert(3), f32=f32, **CR.PARAMS)
            r.process(z[:, :2])
            assert r.read()["theta"][0] not in (0, 1 << 30, 1 << 31, 3 << 30)
            u = r.process(np.array([[bad]], np.complex64))
            st = r.read()
            assert not np.isfinite(u.view(r.ft)).any() and np.isnan(r.e[0, 0]) == sticky
            assert np.isnan(st["err"][0]) == sticky and (st["locked"][0] == 0 if sticky else np.isfinite(st["err"][0]))
            assert np.isfinite(r.process(z[:, 3:]).view(r.ft)).all() and np.isnan(r.read()["err"][0]) == sticky
        # ... and one infinite part against a phasor component that is exactly 0 (theta = 0: c = 1, s = 0): inf 0 is NaN
        r = CR.CarrierRef([(CR.DSB, 0.25, 0.0625)], CR.hilbert(3), f32=f32, **CR.PARAMS)
        r.process(np.array([[complex(np.inf, 0.3)]], np.complex64))
        assert np.isnan(r.e[0, 0]) and np.isnan(r.read()["err"][0])


def test_the_issues_figures():
    """adapt_ref, T = 16, D = 1, one NaN or one 1e25 at sample 300 of an NR row of 900: every later output is not finite
    (599 of 599).  blanker_ref, (32, 2, 4), thr 16, ON, one NaN at sample 100: exactly one output changes (106) and ref
    recovers; one Inf: it triggers, 2 D + 1 = 13 outputs differ, all stay finite."""
    x = AR.audio_series(1, 900, 3)
    for v in (NAN, F32(1e25)):
        out = AR.adapt_ref(NF.plant(x, [0], [300], v), [(AR.NR, 0.5, 0.0)], 16, 1)[0]
        assert np.isfinite(out[0, :301]).all() and not np.isfinite(out[0, 301:]).any() and out[0, 301:].size == 599
    z = BR.impulse_series(1, 400, 5)[:, :400] * F32(0.0) + (1.0 + 1.0j)
    z = z.astype(np.complex64)
    clean = BR.blanker_ref(z, [(16.0, BR.ON)], **BR.params(32, 2, 4))
    got = BR.blanker_ref(NF.plant(z, [0], [100], NAN), [(16.0, BR.ON)], **BR.params(32, 2, 4))
    diff = np.flatnonzero((BR.bits(got[0]) != BR.bits(clean[0])).reshape(400, 2).any(axis=1))
    assert diff.tolist() == [106] and np.isfinite(got[1]["ref"][0]) and got[1]["triggers"][0] == 0
    got = BR.blanker_ref(NF.plant(z, [0], [100], INF), [(16.0, BR.ON)], **BR.params(32, 2, 4))
    diff = np.flatnonzero((BR.bits(got[0]) != BR.bits(clean[0])).reshape(400, 2).any(axis=1))
    assert diff.tolist() == list(range(100, 113)) and np.isfinite(got[0].view(F32)).all() and got[1]["triggers"][0] == 1


# ---- the kinds, stage by stage --------------------------------------------------------------------------------------

def changed(got, clean):
    """per output position (axis 1) whether any word of it differs, NaNs of any payload counted as equal"""
    g = np.ascontiguousarray(got).view(F32).reshape(got.shape[0], got.shape[1], -1)
    c = np.ascontiguousarray(clean).view(F32).reshape(g.shape)
    same = (g.view(np.uint32) == c.view(np.uint32)) | (np.isnan(g) & np.isnan(c))
    return ~same.all(axis=2)


def differs(got, clean):
    """any word differs, NaNs of any payload counted as equal"""
    g, c = np.ascontiguousarray(got), np.ascontiguousarray(clean)
    if g.dtype not in (np.float32, np.complex64):
        return not np.array_equal(g, c)
    g, c = g.view(F32), c.view(F32)
    return bool(((g.view(np.uint32) != c.view(np.uint32)) & ~(np.isnan(g) & np.isnan(c))).any())


def finite(x):
    x = np.ascontiguousarray(x)
    return np.isfinite(x.view(F32) if x.dtype in (np.float32, np.complex64) else x.astype(np.float64))


# what include/perseus_ddc.h says under "Non-finite samples", per stage
KINDS = {"rxfilter": "transient", "audio": "transient", "scope": "transient", "blanker": "healing", "squelch": "healing",
         "demod": "sticky", "carrier": "sticky", "adapt": "sticky"}


KIND_CASES = [(st, v) for st in STAGES if st.id.split("-")[0] in KINDS for v in values_of(st)]      # (the six later stages: below)


@pytest.mark.parametrize("st,value", KIND_CASES, ids=[f"{st.id}-{v}" for st, v in KIND_CASES])
def test_kinds(pkg, st, value):
    """One poisoned sample at column TT (Audio: the input on the tile edge) of rows 0, 16, 31, 34, the reference's outputs
    against its outputs on the clean series; the bit-exact stages also with 1e25 (its square overflows: as an infinity)
    and 2^-80 (ordinary data).  transient (RxFilter, Audio, Scope): the outputs whose window holds the sample change,
    no other.  healing (Blanker, Squelch): outputs and status are finite again behind the batch without any action (the
    squelch's peak after an infinite level excepted: sticky).  sticky: Demod's DC block keeps the NaN and its AGC
    envelope the infinity (gain 0 from then on); Carrier's q stays NaN and locked 0 while theta, v and the outputs go
    on -- after a NaN and after a sample with both parts infinite, not after one with one infinite part --; Adapt's
    weights stay NaN.  Rows without poison are untouched in the reference."""
    TT, n = st.edge(pkg), st.n(pkg)
    xs = st.inputs(n)
    ps = st.poison(xs, NF.POISON_EXACT[value], [[TT]] * 4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # the references take such input without a warning
        clean, got = st.ref(xs), st.ref(ps)
    for g, c in zip(got[0] + got[1], clean[0] + clean[1]):
        NF.clean_rows_identical(g, c, CLEAN, (st.id, value, "rows without poison"))
    kind = KINDS[st.id.split("-")[0]]
    out, cout = got[0][0], clean[0][0]
    ch = changed(out, cout)
    first = st.outputs_before(TT)
    assert not ch[:, :first].any()
    if kind == "transient":
        for r in ROWS:
            span = np.asarray(list(st.nan_span(TT, n)))
            assert np.flatnonzero(ch[r]).tolist() == span.tolist(), (st.id, value, r)
    elif kind == "healing":
        for r in ROWS:
            seen = any(differs(g[r], c[r]) for g, c in zip(got[0] + got[1], clean[0] + clean[1]))
            assert seen and finite(out[r, -50:]).all(), (st.id, value, r)
        for name, s in zip(st.status_names, got[1]):
            if name == "peak" and value in ("+inf", "-inf", "huge"):
                # the rows whose z holds the value (SquelchStage.poison: a finite value goes into every row's z)
                assert np.isposinf(s[ROWS if value == "huge" else ROWS[:2]]).all()
            else:
                assert finite(s[ROWS]).all(), (st.id, value, name)
    elif st.id == "demod":
        f = finite(out)
        dc = [r for r in ROWS if st.rx[r][2] & DR.DC]
        agc_only = [r for r in ROWS if st.rx[r][2] == DR.AGC]
        plain = [r for r in ROWS if st.rx[r][2] == 0]
        assert dc and agc_only and plain
        assert not f[dc, TT:].any()                                                     # the DC block: y is NaN for good
        assert not f[plain, TT].any() and f[plain, TT + 2:].all()                       # FM: outputs TT and TT + 1
        if value == "nan":
            assert [np.flatnonzero(~f[r]).tolist() for r in agc_only] == [[TT]] * len(agc_only)    # fmaxf drops it
            # ... and the gain is not stuck: |y| <= e, so |a| <= target, as on any clean row
            assert (np.abs(out[agc_only, TT + 1:]) <= F32(DR.PARAMS["target"]) * F32(1.000001)).all()
        else:
            assert not f[agc_only, TT].any() and not out[agc_only, TT + 1:].any()       # e = inf: the gain is 0
    elif st.id.startswith("carrier"):
        theta, freq, err, locked = got[1]
        on = [r for r in ROWS if st.rx[r][0] != CR.OFF]
        off = [r for r in ROWS if st.rx[r][0] == CR.OFF]
        assert len(on) == 3 and len(off) == 1
        assert finite(freq[on]).all()
        if value == "nan":
            assert np.isnan(err[on]).all() and not locked[on].any()
        else:
            # ONE infinite part (rows 0: re, 16: im): w = (+-inf, +-inf), whose angle is a finite number, q stays finite.
            # BOTH parts infinite (row 34): inf c - inf s is NaN for ordinary c and s, and q is NaN as after a NaN.
            one = [r for r, part in zip(ROWS, PARTS) if part != "both" and r in on]
            both = [r for r, part in zip(ROWS, PARTS) if part == "both" and r in on]
            assert one == [0, 16] and both == [34]
            assert finite(err[one]).all() and np.isnan(err[both]).all() and not locked[both].any()
            assert np.array_equal(locked[one] == 1, err[one] < F32(CR.PARAMS["lock_thr"]))
        assert finite(out[on, TT + st.L:]).all() and not finite(out[on, TT]).reshape(-1, 2).all(axis=1).any()
        assert np.array_equal(NF.words(out[off]), NF.words(ps[0][off])) and locked[off].all()
    else:
        assert st.id.startswith("adapt")
        on = [r for r in ROWS if st.rx[r][0] != AR.OFF]
        assert len(on) == 3
        if value == "tiny":                                                              # ordinary data: nothing sticks
            assert finite(got[1][0]).all() and finite(out).all() and ch[on].any(axis=1).all()
        else:
            assert not finite(got[1][0][on]).any()                                       # the weights
            assert not finite(out[on, TT + st.D + 1:]).any()


@pytest.mark.parametrize("st,value,layout", CASES, ids=case_ids)
def test_gpu_cases_preconditions(pkg, st, value, layout):
    """Every case of the GPU file through the reference: it takes the input without a warning, the rows without poison
    are untouched, every poisoned row's output differs from the clean one, and -- same_or_both_nan needs it -- no
    poisoned output or status array is NaN throughout.  The cut reference equals the uncut one."""
    TT, n = st.edge(pkg), st.n(pkg)
    xs = st.inputs(n)
    cols = layout_columns(st, pkg, layout)
    assert sorted(set(sum(cols, []))) == (st.columns(pkg) if layout else sorted({0, max(st.H - 1, 0), TT - 1, TT}))
    ps = st.poison(xs, NF.POISON_EXACT[value], cols)
    for x, p in zip(xs, ps):
        assert np.array_equal(NF.words(x[CLEAN]), NF.words(p[CLEAN]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clean, got, cut = st.ref(xs), st.ref(ps), st.ref(ps, st.cuts(pkg))
    for g, c, k in zip(got[0] + got[1], clean[0] + clean[1], cut[0] + cut[1]):
        NF.clean_rows_identical(g, c, CLEAN, (st.id, value, layout))
        if g.dtype in (np.float32, np.complex64):
            assert not np.isnan(np.ascontiguousarray(g[ROWS]).view(F32)).all()
            NF.same_or_both_nan(k[ROWS], g[ROWS], (st.id, "the reference in cuts"))
    if value != "tiny":
        # the poison is seen: some output or status value of the row differs -- unless its first poisoned sample is so
        # late that it lies in the carried record alone (what the cut and reset tests are about)
        for r, cs in zip(ROWS, cols):
            seen = any(differs(g[r], c[r]) for g, c in zip(got[0] + got[1], clean[0] + clean[1]))
            # (... or the row is a decoder's OFF row; or the stage is Psk with a window of 2, which shows its filter at
            # the three samples a strobe looks at alone: two poisoned outputs may pass between them)
            assert seen or min(cs) + max(st.H, 1) >= n or r in st.unseen or st.sparse, (st.id, value, layout, r)


def test_squelch_designed_rows():
    """the designed inputs of test_b_squelch_gate_and_count show the gate in the states that test needs"""
    z, a, rx, par = squelch_cases(773)
    out, lv, st, status, _ = QR.squelch_ref(z, a, rx, **QR.params(*par))
    assert not st[0].any() and not out[0].view(np.uint32).any() and np.isnan(a[0, 100:300]).all()
    assert st[1, 5:8].tolist() == [1, 1, 0] and np.isnan(lv[1, 6]) and st[2, 5:9].all() and np.isnan(lv[2, 6]) and st[3, 2:].all()
    assert np.isfinite(out[3]).all() and np.isfinite(status["level"]).all()


# ---- the six later stages: Eq, Denoise, Fsk, Morse, Psk and the mixer ------------------------------------------------

NEW = [st for st in STAGES if st.id.split("-")[0] not in KINDS]


def test_the_table_holds_the_later_stages():
    assert [st.id for st in NEW] == ["eq-S1", "eq-S8", "denoise-256-64", "denoise-1024-256", "fsk-W2", "fsk-W256", "morse-W2",
                                     "morse-W256", "psk-W2", "psk-W256"]
    for st in G.DECODERS:
        assert len(st.bank) == 2 and {s[0] for s in st.sel} == {0, 1} and [r for r in ROWS if not st.sel[r][1] & 1] == [31]
    for st in G.EQS:
        assert [len(st.rx[r]) for r in ROWS].count(0) == 1 and max(len(st.rx[r]) for r in ROWS) == st.S
    for st in G.DENOISES:
        assert [(st.rx[r][0], len(st.rx[r]) > 4) for r in ROWS] == [(1, False), (1, False), (0, False), (1, True)]


@pytest.mark.parametrize("st", NEW, ids=G.ids)
def test_new_stages_clean_runs_and_reset(pkg, st):
    """Every new adapter's reference on its own clean series: finite on every row, records on most rows (the decoders
    decode something), the same in cuts; and after a batch that leaves a NaN in every row's record (test C's input)
    reset() gives a fresh reference's bits."""
    n = st.n(pkg)
    xs = st.inputs(n)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clean = st.ref(xs)
    for v in clean[0] + clean[1]:
        assert finite(v).all() if v.dtype in NF.FLOATS else True, st.id
    if st.kinds:
        counts = clean[0][1]
        assert (counts[[j for j in range(G.K) if j != 31]] >= 3).all() and counts[31] == 0, (st.id, counts)
    poisoned = G.all_rows_poisoned(st, xs, n)
    assert all(np.isnan(NF.parts(p)[:, -1:]).all() for p in poisoned)
    if isinstance(st, G.DecoderStage):
        r = st.reference(True)
        first = st.R.run_cuts(r, poisoned[0])
        r.reset()
        again, fresh = st.R.run_cuts(r, xs[0]), st.R.run_cuts(st.reference(True), xs[0])
        for a, b in zip(again[0], fresh[0]):
            assert a.tobytes() == b.tobytes()
        assert again[3].tobytes() == fresh[3].tobytes() and np.array_equal(NF.words(np.asarray(again[1][0])), NF.words(np.asarray(fresh[1][0])))
        return
    r = ER.EqRef(st.rx, st.S) if isinstance(st, G.EqStage) else st.stream()
    r.process(poisoned[0])
    if isinstance(st, G.EqStage):                                  # the record that reset() has to keep out
        assert all(not np.isfinite(r.state[j, :len(st.rx[j])]).all(axis=1).any() for j in range(G.K))
    else:
        on = [j for j in range(G.K) if len(st.rx[j]) < 5]          # (HOLD keeps S and N)
        assert np.isnan(r.st[0][on]).all() and np.isnan(r.st[1][on]).all() and np.isnan(r.st[2]).all()
        assert np.isnan(r.sums).any(axis=1).all() and np.isnan(r.inputs).any(axis=1).all()
    r.reset()
    out = r.process(xs[0])
    state = r.state if isinstance(st, G.EqStage) else r.noise()
    assert np.array_equal(NF.words(out.astype(np.float32)), NF.words(clean[0][0])) and np.array_equal(NF.words(state), NF.words(clean[1][0]))


@pytest.mark.parametrize("st,value,layout", G.DECODER_CASES, ids=[f"{st.id}-{v}-{layout}" for st, v, layout in G.DECODER_CASES])
def test_decoder_cases_leave_enough_to_compare(pkg, st, value, layout):
    """test_b_poisoned_rows_of_the_decoders' conditions on the references alone: on every case's poisoned series the
    float32 model decides as the double reference does -- records, counts, strobes, integer status, on every row -- and
    is within the file's tolerance of it wherever the double reference is finite, which is more than half of every row's
    samples and strobes (decoder_rows_against asserts the share).  The series were chosen on this."""
    xs = st.inputs(st.n(pkg))
    ps = st.poison(xs, NF.POISON[value], layout_columns(st, pkg, layout))
    e = G.decoder_rows_against(st, st.ref(ps), st.ref(ps, f32=False), range(G.K), (st.id, value, layout))
    print(f"{st.id} {value} {layout}: the model's largest error is {e:.3f} of the tolerance")


def model_run(st, pkg, dev, xs, cuts=None, obj=None, before=None, in_place=False, rev=False):
    """test_gpu_nonfinite.run with the float32 model (Eq: the reference) in the device's place"""
    assert obj is None and not in_place and not rev
    if before is None:
        return st.ref(xs, cuts)
    s, outs, off = st.stream(), [], 0                              # (Denoise alone has a hook here)
    for i, b in enumerate(cuts):
        before(i, s)
        outs.append(s.process(xs[0][:, off:off + b]))
        off += b
    return (np.concatenate(outs, axis=1).astype(np.float32),), (s.noise(),)


DESIGNED = [(f, st) for f, sts in ((G.test_b_designed_denoise_one_nan, G.DENOISES), (G.test_b_designed_denoise_restart_needs_a_clean_frame, G.DENOISES),
                                   (G.test_b_designed_morse_mark_and_gap, [s for s in G.DECODERS if s.name == "morse"]),
                                   (G.test_b_designed_fsk_window, [s for s in G.DECODERS if s.name == "fsk"]),
                                   (G.test_b_designed_psk_nan_strobes, [s for s in G.DECODERS if s.name == "psk"])) for st in sts]


def stand_in(monkeypatch, pkg):
    monkeypatch.setattr(G, "run", model_run)
    monkeypatch.setattr(G, "clean_run", lambda st, pkg, dev: (st.inputs(st.n(pkg)), st.ref(st.inputs(st.n(pkg)))))
    monkeypatch.setattr(G, "mixer_run", lambda pkg, dev, a, gains, limit, cuts=None, obj=None, changes=(): G.mixer_ref(pkg, a, gains, limit, changes, cuts)[0])


@pytest.mark.parametrize("f,st", DESIGNED, ids=[f"{f.__name__[16:]}-{st.id}" for f, st in DESIGNED])
def test_designed_tests_on_the_references(monkeypatch, pkg, f, st):
    """The designed GPU tests of the header's sentences, run with the float32 model in the device's place: every
    assertion they make of the reference before the device is asked -- the NaN spans, what sticks and what heals, +0
    where the header says +0 -- holds here, without a GPU."""
    stand_in(monkeypatch, pkg)
    f(pkg, None, st)


@pytest.mark.parametrize("value", list(NF.POISON))
@pytest.mark.parametrize("st", G.EQS, ids=G.ids)
def test_designed_eq_on_the_reference(monkeypatch, pkg, st, value):
    stand_in(monkeypatch, pkg)
    G.test_b_designed_eq_is_sticky(pkg, None, st, value)


@pytest.mark.parametrize("value", list(NF.POISON))
@pytest.mark.parametrize("limit", G.MIX_LIMITS, ids=G.mix_ids)
def test_mixer_isolation_on_the_reference(monkeypatch, pkg, limit, value):
    """test_e_mixer_isolation_and_the_limiter's assertions on mixer_ref: E = 0 for the blocks k - 1 and k, the recovery by
    rel, -ceil (block 0: +-ceil), min_gain 0, |out| <= ceil, and which indices differ from the clean run"""
    stand_in(monkeypatch, pkg)
    G.test_e_mixer_isolation_and_the_limiter(pkg, None, limit, value)


def test_mixer_reference_reset():
    """mixer_ref after test_e_mixer_reset_after_poison's batch (a NaN in every row's last sample, which the held block
    keeps, an infinity that leaves E = 0 and the peak inf, ramps under way): reset() gives a fresh reference's bits with
    the gains the set_rx calls left"""
    import importlib
    pkg = importlib.import_module("libperseus-sdr_amd")
    n, a, g, ch, after = G.mixer_case(pkg)
    for limit in G.MIX_LIMITS:
        ref = G.mixer_ref(pkg, G.mixer_bad_batch(n, a, g, ch), g, limit, ch)[1]
        carried = ref.read()
        assert np.isposinf(carried["peak"]).all() and (limit is None or (not carried["gain"].any() and np.isnan(ref.lim.held).any()))
        ref.reset()
        f, p = ref.process(a)
        st = ref.read()
        want = G.mixer_ref(pkg, a, after, limit)[0]
        assert np.array_equal(NF.words(f), NF.words(want[0])) and np.array_equal(p, want[1]) and finite(f).all()
        assert all(np.array_equal(NF.words(st[name]), NF.words(w)) for name, w in zip(G.MR.STATUS.names, want[2]))


# ---- the references' edits changed no bit ---------------------------------------------------------------------------

class OldNumpy:
    """numpy as the references used it before their edits: np.maximum / np.minimum where they now say np.fmax / np.fmin,
    and an errstate that ignores what it ignored then"""

    def __init__(self, errstate_keys):
        self.keys = errstate_keys

    def __getattr__(self, name):
        return getattr(np, name)

    fmax = staticmethod(np.maximum)                # the old expression; the new one is np.fmax
    fmin = staticmethod(np.minimum)                # the old expression; the new one is np.fmin

    def errstate(self, **kw):
        return np.errstate(**{k: v for k, v in kw.items() if k in self.keys})


@pytest.fixture(scope="module")
def tuner_outputs(O):
    """the demod tests' input: the tuner reference's outputs on the 2^19-sample LCG stream, rounded to complex64"""
    x = R.to_complex(O, O.lcg_bytes(6 << 19, 12345))
    M, hop, T, Rd = 1024, 512, 64, 4
    y = HR.channelizer_ref(x, M, hop, TR.kaiser_prototype_wide(M, 4))
    return TR.tuner_ref(y, M, hop, TR.receiver_set(M, 1024), TR.kaiser_lowpass(T, Rd), Rd).astype(np.complex64)


def words64(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype in (np.float64, np.complex128) else NF.words(x)


def test_edited_references_give_the_old_bits(monkeypatch, tuner_outputs):
    """demod_ref, carrier_ref and adapt_ref with numpy as they used it before (np.maximum / np.minimum, the old errstate,
    warnings raised as errors: finite data never met what is now ignored) against themselves as they are, on the inputs
    the existing tests feed them -- the demod tests' tuner outputs and their receivers, am_carriers(1024, 3000) with the
    carrier tests' receivers, AR.gpu_series() -- in double and in float32: not one differing bit.  carrier_ref and
    rxfilter_ref now put re and im side by side where they wrote re + 1j im: the old expression gives the same bits on
    every value met here."""
    def both(module, make, keys=()):
        new = make()
        with monkeypatch.context() as m, warnings.catch_warnings():
            warnings.simplefilter("error")
            m.setattr(module, "np", OldNumpy(keys))
            old = make()
        assert len(new) == len(old)
        for a, b in zip(new, old):
            assert a.dtype == b.dtype and np.array_equal(words64(a), words64(b))
        return new

    z = tuner_outputs
    for f32 in (False, True):
        rx = DR.interleaved_rx(1024)
        both(DR, lambda: (DR.DemodRef(rx, f32=f32, **DR.PARAMS).process(z),), ("divide",))
        for mode in DR.MODES:
            rx = [(mode, 77777 * (j + 1), DR.FLAG_SETS[j % 4]) for j in range(1024)]
            both(DR, lambda: (DR.DemodRef(rx, f32=f32, **DR.PARAMS).process(z),), ("divide",))
    zc = CR.am_carriers(1024, 3000)[0]
    for f32, L in ((False, 31), (True, 3), (True, 255)):
        def carrier():
            r = CR.CarrierRef(CR.interleaved_rx(1024), CR.hilbert(L), f32=f32, **CR.PARAMS)
            u = r.process(zc)
            st = r.read()
            assert np.isfinite(r.e).all()
            return (u, r.e) + tuple(st[name] for name in CR.STATUS.names)
        u = both(CR, carrier)[0]
        old = (u.real + 1j * u.imag).astype(u.dtype)                 # the old expression; the new one sets the two parts
        assert np.array_equal(words64(old), words64(u))
    x = AR.gpu_series()
    T, D = AR.GPU_SETS[0]
    both(AR, lambda: AR.adapt_ref(x, AR.interleaved_rx(1024), T, D)[:2], ("under",))      # all K0 rows, as test_gpu_adapt.py
    for T, D in AR.GPU_SETS[1:]:
        both(AR, lambda: AR.adapt_ref(x[:37], AR.interleaved_rx(37), T, D)[:2], ("under",))
    for nrx, (B, T) in ((9, (3, 2)), (9, (4, 64)), (5, (5, 256))):
        zz = RR.parity_inputs(nrx)
        out = RR.rxfilter_model32(zz, RR.parity_bank(B, T), RR.select(nrx, B))
        old = out.real + 1j * out.imag                               # the old expression
        assert np.array_equal(words64(old), words64(out))
