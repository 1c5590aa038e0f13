"""Non-finite samples through the eight per-receiver stages (RxFilter, Blanker, Adapt, Demod, Carrier, Squelch, Audio,
Scope) on the GPU, row by row: what one bad sample does, that it stays inside its own row, and how the caller gets the
row back (include/perseus_ddc.h, "Non-finite samples" under every stage).  One table of stage adapters, STAGES; every
test is parametrised over it.  K = 35 receivers (2 16 + 3: a partial last group for blocks of 2, 4 and 16 receivers),
n = 3 TT + 5 samples; rows 0, 16, 31 and 34 are poisoned, all others stay clean.  Every comparison is equality of bits
(nonfinite.clean_rows_identical), equality of bits and of NaN positions (nonfinite.same_or_both_nan, on poisoned rows
of the bit-exact stages only) or equality of NaN positions; there are no tolerances.  What the references themselves do
with these inputs -- the preconditions -- is asserted in tests/test_nonfinite_cpu.py."""
import numpy as np
import pytest

import adapt_ref as AR
import audio_ref as UR
import blanker_ref as BR
import carrier_ref as CR
import demod_ref as DR
import nonfinite as NF
import rxfilter_ref as RR
import scope_ref as SR
import squelch_ref as QR

pytestmark = pytest.mark.gpu
K = 35
ROWS = NF.poisoned_rows(K)                                   # 0, 16, 31, 34
CLEAN = [j for j in range(K) if j not in ROWS]
PARTS = ("re", "im", "both", "both")                          # of a complex sample, per poisoned row


def noise(K, n, seed):
    """complex64 [K, n], unit normal components"""
    w = np.random.default_rng(seed).standard_normal((K, n, 2), dtype=np.float32)
    return np.ascontiguousarray(w).view(np.complex64)[..., 0]


class Stage:
    """One stage at one setting.  xs: the tuple of its input arrays [K, n] (two for the squelch).  outs: the tuple of
    its output arrays, concatenated over the batches along axis 1.  status: a tuple of arrays [K, ...] of what read()
    returns (empty where the stage has no read).  rev: the receivers in reversed order."""
    exact = False                 # bit-exact against its reference (otherwise the reference is the float32 model)
    in_place = None               # the index of the input an output may overwrite
    fir = False                   # no memory but the last inputs: the NaN set is exact and everything else is clean
    tile = None                   # the package's tile getter
    TT0 = None                    # ... or the tile itself where there is no getter
    status_names = ()

    def TT(self, pkg):
        return self.TT0 or int(getattr(pkg, self.tile)())

    def n(self, pkg):
        return 3 * self.TT(pkg) + 5

    def edge(self, pkg):
        """the input column of the first output of the walk's second tile: TT where a tile counts inputs"""
        return self.TT(pkg)

    def far(self, pkg):
        """the input column of output 2 TT + 3"""
        return 2 * self.TT(pkg) + 3

    def columns(self, pkg):
        return NF.placements(self.edge(pkg), self.H, self.n(pkg), self.far(pkg))

    def cuts(self, pkg):
        return NF.cuts_for(self.edge(pkg), self.n(pkg), self.far(pkg))

    def counts(self, obj, b):
        return (b,)

    def status(self, obj):
        return ()

    def poison(self, xs, value, cols_per_row):
        """xs with `value` planted in input 0: row ROWS[i] at the columns cols_per_row[i]"""
        x = xs[0]
        for r, cols, part in zip(ROWS, cols_per_row, PARTS):
            if len(cols):
                x = NF.plant(x, [r], cols, value, part)
        return (x,) + tuple(xs[1:])

    def outputs_before(self, col):
        """how many outputs (along axis 1 of output 0) are made of inputs before `col` alone"""
        return col

    def pick(self, rx, rev):
        return list(rx)[::-1] if rev else list(rx)


class RxFilterStage(Stage):
    tile, fir, out_dtypes = "rxfilter_tile_outputs", True, (np.complex64,)

    def __init__(self, T):
        self.T = self.H = T
        self.id = f"rxfilter-T{T}"
        self.bank = RR.parity_bank(3, T).copy()
        if T >= 2:
            self.bank[1, T // 2:] = 0.0                       # a shorter filter padded with zeros: those taps run too
        self.sel = RR.select(K, 3)

    def inputs(self, n):
        v = np.random.default_rng(1000 + self.T).uniform(-1.0, 1.0, (K, n, 2)).astype(np.float32)
        return (np.ascontiguousarray(v).view(np.complex64)[..., 0],)

    def make(self, pkg, rev=False):
        return pkg.RxFilter(self.bank, self.pick(self.sel, rev))

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=bufs[0] if bufs else None),)

    def ref(self, xs, cuts=None):
        return (RR.rxfilter_model32(xs[0], self.bank, self.sel, cuts).astype(np.complex64),), ()

    def nan_span(self, col, n):
        """the outputs whose window holds input col: col .. col + T - 1, zero-valued taps included"""
        return range(col, min(col + self.T, n))


class AudioStage(Stage):
    # k_audio's tile is 256 OUTPUTS (test_gpu_audio.py: there is no getter), about 52 inputs at this ratio: n is 3 TT + 5
    # inputs as for the other TT = 256 stages (some 15 tiles), and the columns and cuts that stand on a tile edge are
    # the inputs of outputs TT - 1, TT and 2 TT + 3 (edge, far)
    TT0, fir, out_dtypes = 256, True, (np.float32, np.int16)
    L, M = 3072, 625

    def __init__(self, P, T):
        self.P, self.T, self.H = P, T, T
        self.id = f"audio-T{T}"
        self.g = UR.parity_prototype(self.L, self.M, P, T)

    def edge(self, pkg):
        (nk, _, _), _ = UR.positions(self.L, self.M, self.P, self.TT0 - 1, 2)
        assert nk[1] == nk[0] + 1                              # outputs TT - 1 and TT read up to neighbouring inputs
        return int(nk[1])

    def far(self, pkg):
        return int(UR.positions(self.L, self.M, self.P, 2 * self.TT0 + 3, 1)[0][0][0])

    def inputs(self, n):
        return (np.random.default_rng(2000 + self.T).uniform(-1.0, 1.0, (K, n)).astype(np.float32),)

    def make(self, pkg, rev=False):
        return pkg.Audio(K, self.L, self.M, self.P, self.T, self.g)

    def counts(self, obj, b):
        return (obj.next_outputs(b),) * 2

    def process(self, obj, xs, bufs=None, in_place=False):
        if bufs:
            return tuple(obj.process(xs[0], out_f32=bufs[0], out_i16=bufs[1]))
        return tuple(obj.process(xs[0], f32=True, i16=True))

    def ref(self, xs, cuts=None):
        y = UR.audio_model32(xs[0], self.L, self.M, self.P, self.T, self.g, cuts)
        return (y, UR.pcm_ref(y)), ()

    def outputs_before(self, col):
        return UR.outputs(self.L, self.M, 0, col)

    def nan_span(self, col, n):
        """the outputs k whose T taps x[n_k - T + 1 .. n_k] hold input col (positions from audio_ref)"""
        count = UR.outputs(self.L, self.M, 0, n)
        (nk, _, _), _ = UR.positions(self.L, self.M, self.P, 0, count)
        return np.flatnonzero((nk - self.T + 1 <= col) & (col <= nk))


class ScopeStage(Stage):
    fir, out_dtypes = True, (np.float32,)

    def __init__(self, nfft, hop):
        self.nfft, self.hop, self.avg, self.H, self.TT0 = nfft, hop, 1, nfft, nfft
        self.id = f"scope-{nfft}-{hop}"
        self.window = SR.hann(nfft)

    def inputs(self, n):
        return (0.1 * noise(K, n, 3000),)

    def make(self, pkg, rev=False, rows=None):
        return pkg.Scope(K, list(range(K)) if rows is None else rows, self.nfft, self.hop, self.avg, self.window)

    def counts(self, obj, b):
        return (obj.next_lines(b),)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=bufs[0] if bufs else None),)

    def ref(self, xs, cuts=None):
        return (SR.scope_model_f32(xs[0], self.nfft, self.hop, self.avg, self.window),), ()

    def outputs_before(self, col):
        return SR.nseg_of(col, self.nfft, self.hop)

    def nan_span(self, col, n):
        """the lines (avg 1: the segments) s with s hop <= col < s hop + nfft"""
        s = np.arange(SR.nseg_of(n, self.nfft, self.hop))
        return s[(s * self.hop <= col) & (col < s * self.hop + self.nfft)]

    def restart(self, obj, j):
        obj.set_slot(j, (j + 1) % K)

    def restarted(self, pkg):
        return self.make(pkg, rows=[(j + 1) % K for j in range(K)])


class DemodStage(Stage):
    tile, H, id, out_dtypes = "demod_tile_outputs", 1, "demod", (np.float32,)

    def __init__(self):
        rx = DR.interleaved_rx(K)
        # rows 28 .. 31 without a post stage: one group of four on the kernel's other walk, row 31 poisoned
        rx = [(m, w, 0) if 28 <= j < 32 else (m, w, f) for j, (m, w, f) in enumerate(rx)]
        # the poisoned rows between them: every mode, the DC block and the AGC alone and together, and none
        for r, mode, flags in zip(ROWS, (DR.SSB, DR.AM, DR.FM, DR.FM), (DR.DC | DR.AGC, DR.AGC, 0, DR.DC)):
            rx[r] = (mode, rx[r][1], flags)
        self.rx = rx

    def inputs(self, n):
        return (noise(K, n, 4000),)

    def make(self, pkg, rev=False, rx=None):
        P = DR.PARAMS
        return pkg.Demod(self.pick(rx or self.rx, rev), rho=P["rho"], lam=P["lam"], target=P["target"], gmax=P["gmax"])

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=bufs[0] if bufs else None),)

    def ref(self, xs, cuts=None):
        return (DR.run_cuts(DR.DemodRef(self.rx, f32=True, **DR.PARAMS), xs[0], cuts),), ()

    def other(self):
        """another mode for every receiver, the word 0 (so that nothing depends on m), the same flags"""
        return [((m + 1) % 3, 0, f) for m, _, f in self.rx]

    def restart(self, obj, j):
        obj.set_rx(j, *self.other()[j])

    def restarted(self, pkg):
        return self.make(pkg, rx=self.other())


class CarrierStage(Stage):
    tile, in_place, out_dtypes = "carrier_tile_outputs", 0, (np.complex64,)
    status_names = CR.STATUS.names

    def __init__(self, L):
        self.L = self.H = L
        self.id = f"carrier-L{L}"
        self.rx = CR.interleaved_rx(K + 1)[1:]                # row j has mode (j + 1) mod 4: DSB, DSB, OFF, LSB poisoned

    def inputs(self, n):
        return (CR.am_carriers(K, n)[0],)

    def make(self, pkg, rev=False, rx=None):
        return pkg.Carrier(self.pick(rx or self.rx, rev), CR.hilbert(self.L), **CR.PARAMS)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=xs[0] if in_place else bufs[0] if bufs else None),)

    def status(self, obj):
        st = obj.read()
        return tuple(st[name].copy() for name in self.status_names)

    def ref(self, xs, cuts=None):
        r = CR.CarrierRef(self.rx, CR.hilbert(self.L), f32=True, **CR.PARAMS)
        u = CR.run_cuts(r, xs[0], cuts)
        st = r.read()
        return (u,), tuple(st[name].copy() for name in self.status_names)

    def other(self):
        return [((m + 1) % 4, kp, ki) for m, kp, ki in self.rx]

    def restart(self, obj, j):
        obj.set_rx(j, *self.other()[j])

    def restarted(self, pkg):
        return self.make(pkg, rx=self.other())


class SquelchStage(Stage):
    tile, in_place, exact, id = "squelch_tile_outputs", 1, True, "squelch"
    out_dtypes = (np.float32, np.float32, np.uint8)
    status_names = QR.STATUS.names
    par = (48, 2, 3, 37)

    def __init__(self):
        self.H = self.par[0]
        self.rx = QR.interleaved_rx(K)
        # the poisoned rows: z into a relative and an absolute gated receiver, a into a gated one (thresholds below the
        # series' quiet power: closed for its first two blocks, open from then on) and an ungated one
        for r, rx in zip(ROWS, ((60.0, 20.0, QR.GATE | QR.RELATIVE), (0.5, 0.125, QR.GATE), (0.001, 0.0005, QR.GATE), (0.5, 0.125, 0))):
            self.rx[r] = rx

    def inputs(self, n):
        return QR.keyed_series(K, n, 11), QR.audio_series(K, n, 12)

    def poison(self, xs, value, cols_per_row):
        """z on rows 0 and 16 (the level), a on rows 31 and 34 (the gated audio), z too where the value is no NaN or
        infinity: a huge or tiny a is ordinary data"""
        z, a = xs
        for i, (r, cols, part) in enumerate(zip(ROWS, cols_per_row, PARTS)):
            if not len(cols):
                continue
            if i < 2 or np.isfinite(value):
                z = NF.plant(z, [r], cols, value, part)
            else:
                a = NF.plant(a, [r], cols, value)
        return z, a

    def make(self, pkg, rev=False):
        B, attack, hang, R = self.par
        return pkg.Squelch(self.pick(self.rx, rev), B, attack, hang, R, up=QR.UP)

    def counts(self, obj, b):
        return (b, obj.next_blocks(b), obj.next_blocks(b))

    def process(self, obj, xs, bufs=None, in_place=False):
        if bufs:
            return tuple(obj.process(xs[0], xs[1], out=bufs[0], levels=bufs[1], states=bufs[2]))
        return tuple(obj.process(xs[0], xs[1], out=xs[1] if in_place else None))

    def status(self, obj):
        st = obj.read()
        return tuple(st[name].copy() for name in self.status_names)

    def ref(self, xs, cuts=None):
        r = QR.SquelchRef(self.rx, **QR.params(*self.par))
        outs = QR.run_cuts(r, xs[0], xs[1], cuts or [xs[0].shape[1]])
        st = r.read()
        return outs, tuple(st[name].copy() for name in self.status_names)


class AdaptStage(Stage):
    tile, in_place, exact, out_dtypes = "adapt_tile_outputs", 0, True, (np.float32,)
    status_names = ("weights",)

    def __init__(self, T, D):
        self.T, self.D, self.H = T, D, D + T - 1
        self.id = f"adapt-T{T}-D{D}"
        self.rx = AR.interleaved_rx(K)                        # the poisoned rows: OFF, NR, NR and (set here) NOTCH
        self.rx[ROWS[2]] = (AR.NOTCH,) + self.rx[ROWS[2]][1:]

    def inputs(self, n):
        return (AR.audio_series(K, n, 21),)

    def make(self, pkg, rev=False):
        return pkg.Adapt(self.pick(self.rx, rev), self.T, self.D, eps=AR.EPS)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=xs[0] if in_place else bufs[0] if bufs else None),)

    def status(self, obj):
        return (obj.read_weights(),)

    def ref(self, xs, cuts=None):
        r = AR.AdaptRef(self.rx, self.T, self.D)
        return (AR.run_cuts(r, xs[0], cuts),), (r.weights.copy(),)

    def restart(self, obj, j):
        obj.set_rx(j, *self.rx[j], AR.RESTART)


class BlankerStage(Stage):
    tile, exact, out_dtypes = "blanker_tile_outputs", True, (np.complex64,)
    status_names = BR.STATUS.names

    def __init__(self, B, W, R):
        self.par, self.H = (B, W, R), W + R
        self.id = f"blanker-D{W + R}"
        self.rx = BR.interleaved_rx(K)                        # the poisoned rows: ON, ON, OFF (set here), ON
        self.rx[ROWS[2]] = (self.rx[ROWS[2]][0], 0)

    def inputs(self, n):
        return (BR.impulse_series(K, n, 21),)

    def make(self, pkg, rev=False):
        B, W, R = self.par
        return pkg.Blanker(self.pick(self.rx, rev), B, W, R, beta=BR.BETA, cap=BR.CAP)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=bufs[0] if bufs else None),)

    def status(self, obj):
        st = obj.read()
        return tuple(st[name].copy() for name in self.status_names)

    def ref(self, xs, cuts=None):
        r = BR.BlankerRef(self.rx, **BR.params(*self.par))
        out = BR.run_cuts(r, xs[0], cuts or [xs[0].shape[1]])
        st = r.read()
        return (out,), tuple(st[name].copy() for name in self.status_names)


# the small and the large end of every stage's taps / delays (test D's list); the blanker also at the issue's (32, 2, 4)
STAGES = [RxFilterStage(1), RxFilterStage(2), RxFilterStage(256), AudioStage(32, 1), AudioStage(128, 64), ScopeStage(256, 16),
          DemodStage(), CarrierStage(3), CarrierStage(255), SquelchStage(), AdaptStage(16, 1), AdaptStage(128, 256),
          BlankerStage(32, 0, 0), BlankerStage(32, 2, 4), BlankerStage(32, 128, 128)]
BY_ID = {st.id: st for st in STAGES}
ids = lambda st: st.id if isinstance(st, Stage) else str(st)


def layout_columns(st, pkg, layout):
    """the columns of every poisoned row, so that each standard placement is the FIRST poison of some row: layout 0 has
    0 | H - 1 | TT - 1 | TT on rows 0, 16, 31, 34, layout 1 has 2 TT + 3 | n - 1 | all of them | TT - 1 and n - 1 (TT and
    2 TT + 3 as input columns: Stage.edge, Stage.far)"""
    E, n = st.edge(pkg), st.n(pkg)
    if layout == 0:
        return [[0], [max(st.H - 1, 0)], [E - 1], [E]]
    return [[st.far(pkg)], [n - 1], st.columns(pkg), [E - 1, n - 1]]


def values_of(st):
    return list(NF.POISON_EXACT if st.exact else NF.POISON)


CASES = [(st, v, layout) for st in STAGES for v in values_of(st) for layout in (0, 1)]
case_ids = [f"{st.id}-{v}-{layout}" for st, v, layout in CASES]


def upload(xs, dev):
    import torch
    return [torch.from_numpy(np.array(x, copy=True, order="C")).to(dev) for x in xs]          # never the host array itself


def run(st, pkg, dev, xs, cuts=None, obj=None, before=None, in_place=False, rev=False):
    """all of xs through `obj` (default: a fresh object, closed afterwards) in the given batches -> (outs, status), numpy;
    before(i, obj) is called ahead of batch i"""
    own = obj is None
    if own:
        obj = st.make(pkg, rev=rev)
    xd = upload(xs, dev)
    n = xs[0].shape[1]
    parts, off = [], 0
    for i, b in enumerate(cuts or [n]):
        if before:
            before(i, obj)
        due = st.counts(obj, b)
        o = st.process(obj, [x[:, off:off + b] for x in xd], in_place=in_place)
        assert len(o) == len(due) and all(t.shape[0] == K and t.shape[1] == d for t, d in zip(o, due)), (st.id, i, b)
        parts.append([t.cpu().numpy() for t in o])
        off += b
    assert off == n
    status = st.status(obj)
    if own:
        obj.close()
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(len(parts[0]))), status


def flip(r):
    return tuple(tuple(v[::-1] for v in part) for part in r)


_clean, _runs = {}, {}


def clean_run(st, pkg, dev):
    """(the clean inputs, the device's run of them in one batch), once per stage; the run in cuts has its bits"""
    if st.id not in _clean:
        xs = st.inputs(st.n(pkg))
        one = run(st, pkg, dev, xs)
        cut = run(st, pkg, dev, xs, st.cuts(pkg))
        for a, b in zip(one[0] + one[1], cut[0] + cut[1]):
            NF.clean_rows_identical(b, a, np.arange(K), (st.id, "the clean run against its cut"))
        _clean[st.id] = (xs, one)
    return _clean[st.id]


def poisoned_run(st, pkg, dev, value, layout):
    """(the poisoned inputs, their columns per row, the device's run in one batch, in cuts), once per case"""
    key = (st.id, value, layout)
    if key not in _runs:
        xs, _ = clean_run(st, pkg, dev)
        cols = layout_columns(st, pkg, layout)
        ps = st.poison(xs, NF.POISON_EXACT[value], cols)
        one = run(st, pkg, dev, ps)
        cut = run(st, pkg, dev, ps, st.cuts(pkg))
        _runs[key] = (ps, cols, one, cut)
    return _runs[key]


def flat(r):
    return r[0] + r[1]


# ---- A. isolation ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("st,value,layout", CASES, ids=case_ids)
def test_a_poisoned_row_leaves_the_others_alone(pkg, dev, st, value, layout):
    """Rows 0, 16, 31 and 34 poisoned: every other row's outputs and status / carried values have exactly the bits of
    the run of the clean input -- in one batch, in cuts (1 | TT - 1 | 1 | TT + 3 | 0 | rest), in place where the stage
    allows it, and with the receivers in reversed order."""
    _, clean = clean_run(st, pkg, dev)
    ps, _, one, cut = poisoned_run(st, pkg, dev, value, layout)
    cuts = st.cuts(pkg)
    runs = {"one batch": one, "cut": cut}
    if st.in_place is not None:
        runs["in place"] = run(st, pkg, dev, ps, cuts, in_place=True)
    runs["reversed"] = flip(run(st, pkg, dev, tuple(x[::-1] for x in ps), cuts[::-1], rev=True))
    for what, got in runs.items():
        assert len(flat(got)) == len(flat(clean))
        for i, (g, c) in enumerate(zip(flat(got), flat(clean))):
            NF.clean_rows_identical(g, c, CLEAN, (st.id, value, layout, what, i))


# ---- B. the poisoned rows themselves --------------------------------------------------------------------------------

EXACT_CASES = [c for c in CASES if c[0].exact]
MODEL_CASES = [(st, layout) for st in STAGES if not st.exact for layout in (0, 1)]


@pytest.mark.parametrize("st,value,layout", EXACT_CASES, ids=[i for i, c in zip(case_ids, CASES) if c[0].exact])
def test_b_poisoned_rows_of_the_exact_stages(pkg, dev, st, value, layout):
    """Blanker, Squelch, Adapt: the poisoned rows' outputs and status have the reference's bits wherever the reference
    has no NaN, and NaN exactly where it has one; the cut run against the run in one batch in the same way."""
    ps, _, one, cut = poisoned_run(st, pkg, dev, value, layout)
    want = st.ref(ps)
    for i, (g, c, w) in enumerate(zip(flat(one), flat(cut), flat(want))):
        NF.same_or_both_nan(g[ROWS], w[ROWS].astype(g.dtype), (st.id, value, layout, "reference", i))
        NF.same_or_both_nan(c[ROWS], g[ROWS], (st.id, value, layout, "cut", i))


def nan_rows(x):
    """per row the set of positions (along axis 1) that hold a NaN in any part or bin"""
    x = np.ascontiguousarray(x)
    m = np.isnan(x.view(np.float32).reshape(x.shape[0], x.shape[1], -1)).any(axis=2)
    return [set(np.flatnonzero(r).tolist()) for r in m]


@pytest.mark.parametrize("st,layout", MODEL_CASES, ids=[f"{st.id}-{layout}" for st, layout in MODEL_CASES])
def test_b_poisoned_rows_of_the_model_stages(pkg, dev, st, layout):
    """RxFilter, Audio, Scope, Demod, Carrier with a NaN: the NaN positions are the float32 model's, part by part; every
    output made of the samples before a row's first NaN has the clean run's bits.  RxFilter, Audio, Scope have no other
    memory than their inputs: the NaN set is exactly the outputs whose window holds a poisoned sample, all of them, and
    every other output has the clean run's bits again.  The cut run has the NaN positions and the bits of the run in one
    batch."""
    _, clean = clean_run(st, pkg, dev)
    ps, cols, one, cut = poisoned_run(st, pkg, dev, "nan", layout)
    want = st.ref(ps)
    n = st.n(pkg)
    for i, (g, c, w) in enumerate(zip(flat(one), flat(cut), flat(want))):
        if g.dtype in (np.float32, np.complex64):
            gn, wn = np.isnan(np.ascontiguousarray(g).view(np.float32)), np.isnan(np.ascontiguousarray(w).view(np.float32))
            assert np.array_equal(gn, wn), (st.id, layout, i, "NaN positions", np.argwhere(gn != wn)[:4].tolist())
        NF.same_or_both_nan(c[ROWS], g[ROWS], (st.id, layout, "cut", i))
    for r, cs in zip(ROWS, cols):
        before = st.outputs_before(min(cs))
        for i, (g, cl) in enumerate(zip(one[0], clean[0])):
            assert np.array_equal(NF.words(g[r, :before]), NF.words(cl[r, :before])), (st.id, layout, r, i, "before")
        if st.fir:
            span = set()
            for col in cs:
                span |= set(int(v) for v in st.nan_span(col, n))
            found = nan_rows(one[0][0])[r]
            assert found == span and (span or min(cs) == n - 1), (st.id, layout, r, sorted(found ^ span)[:6])
            keep = np.array(sorted(set(range(one[0][0].shape[1])) - span), dtype=np.int64)
            for i, (g, cl) in enumerate(zip(one[0], clean[0])):
                assert np.array_equal(NF.words(g[r, keep]), NF.words(cl[r, keep])), (st.id, layout, r, i, "behind the NaNs")


@pytest.mark.parametrize("L", [3, 255])
def test_b_a_nan_step_adds_nothing_to_theta(pkg, dev, L):
    """Carrier, a NaN in the last sample of rows 0, 16, 31, 34: theta behind the batch is theta behind the n - 1 clean
    samples before it, to the bit -- the NaN step added 0 --, freq is -vmax (fmaxf and fminf drop the NaN), err is NaN
    and locked is 0; an OFF receiver's loop is not run and keeps its zeros.  In cuts as in one batch."""
    st = BY_ID[f"carrier-L{L}"]
    n = st.n(pkg)
    xs, clean = clean_run(st, pkg, dev)
    short = run(st, pkg, dev, (xs[0][:, :n - 1],))[1]
    ps = st.poison(xs, NF.QNAN, [[n - 1]] * 4)
    for cuts in (None, st.cuts(pkg)):
        theta, freq, err, locked = run(st, pkg, dev, ps, cuts)[1]
        assert np.array_equal(theta[ROWS], short[0][ROWS]), (L, cuts, theta[ROWS], short[0][ROWS])
        for r in ROWS:
            if st.rx[r][0] == CR.OFF:
                assert theta[r] == 0 and freq[r] == 0 and err[r] == 0 and locked[r] == 1
            else:
                assert freq[r] == -np.float32(CR.PARAMS["vmax"]) and np.isnan(err[r]) and locked[r] == 0, (L, r)
        for v, w in zip((theta, freq, err, locked), clean[1]):
            NF.clean_rows_identical(v, w, CLEAN, (L, "clean rows"))
    assert any(st.rx[r][0] != CR.OFF for r in ROWS)


@pytest.mark.parametrize("value", ["+inf", "-inf"])
@pytest.mark.parametrize("L", [3, 255])
def test_b_carrier_infinity_part_by_part(pkg, dev, L, value):
    """Carrier, an infinity at column TT (theta is an ordinary word there) in re of row 0, in im of row 16 (both DSB)
    and in both parts of row 34 (LSB).  One infinite part: w is (+-inf, +-inf), its angle a finite number, err behind
    the batch is finite and locked is the comparison.  Both parts: inf c - inf s is NaN, err is NaN and locked 0, as
    after a NaN.  The float32 model shows this (asserted) before the device is asked."""
    st = BY_ID[f"carrier-L{L}"]
    assert [st.rx[r][0] for r in ROWS] == [CR.DSB, CR.DSB, CR.OFF, CR.LSB] and PARTS[:2] == ("re", "im") and PARTS[3] == "both"
    xs, _ = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.POISON[value], [[st.edge(pkg)]] * 4)
    thr = np.float32(CR.PARAMS["lock_thr"])
    for _, (theta, freq, err, locked) in (st.ref(ps), run(st, pkg, dev, ps), run(st, pkg, dev, ps, st.cuts(pkg))):
        assert np.isfinite(err[[0, 16]]).all() and np.array_equal(locked[[0, 16]] == 1, err[[0, 16]] < thr)
        assert np.isnan(err[34]) and locked[34] == 0 and np.isfinite(freq[ROWS]).all()
        assert err[31] == 0 and locked[31] == 1                       # OFF: the loop is not run


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_b_demod_post_stage(pkg, dev, value):
    """Demod, one poisoned sample at column TT of rows 0 (SSB, DC block and AGC), 16 (AM, AGC), 31 (FM, plain) and 34
    (FM, DC block).  The DC block keeps the NaN: every output from TT on is NaN (behind an infinity: not finite, on the
    SSB row).  The plain FM row has two NaN outputs.  The AGC alone steps over a NaN --
    e = fmaxf(NaN, lambda e) -- with one NaN output, and the outputs behind it are within TOL_DEMOD of the float32
    model and no larger than the target: the gain is not stuck.  Behind an infinity e = inf: the gain is 0 and every
    later output of the AGC row is 0.  The float32 model shows each of these (asserted) before the device is asked."""
    st = BY_ID["demod"]
    TT, n = st.TT(pkg), st.n(pkg)
    assert [st.rx[r][2] for r in ROWS] == [DR.DC | DR.AGC, DR.AGC, 0, DR.DC] and st.rx[16][0] == DR.AM
    xs, _ = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.POISON[value], [[TT]] * 4)
    want = st.ref(ps)[0][0]
    got = run(st, pkg, dev, ps)[0][0]
    target = np.float32(DR.PARAMS["target"])
    for out in (want, got):
        f = np.isfinite(out)
        assert f[ROWS, :TT].all() and not f[0, TT:].any() and not f[16, TT] and f[16, TT + 1:].all()
        if value == "nan":                     # (the angle of an infinite FM product may be a finite number)
            assert not f[34, TT:].any() and not f[31, TT:TT + 2].any() and f[31, TT + 2:].all()
            assert (np.abs(out[16, TT + 1:]) <= target * np.float32(1.000001)).all() and out[16, TT + 1:].any()
        else:
            assert not out[16, TT + 1:].any()
    if value == "nan":
        keep = np.isfinite(want[16])
        e = float(np.max(np.abs(got[16, keep].astype(np.float64) - want[16, keep])) / np.max(np.abs(want[16, keep])))
        print(f"demod AM + AGC behind a NaN: err {e:.2e} (TOL {DR.TOL_DEMOD[DR.AM]:.2e})")
        assert e <= DR.TOL_DEMOD[DR.AM]


def squelch_cases(n):
    """Two designed squelch inputs, [4, n] each, B = 48, attack 2, hang 2, GATE, absolute thresholds 0.5 / 0.125:
    row 0 quiet throughout (the gate stays closed) with NaN audio over samples 100 .. 299;
    row 1 loud throughout with a NaN in z in block 6 and a quiet block 7: the NaN block counts towards hang;
    row 2 loud throughout with a NaN in z in block 6 alone: one count, reset by block 7;
    row 3 loud throughout, clean."""
    B = 48
    z = noise(4, n, 77)
    a = QR.audio_series(4, n, 78)
    z[0] *= np.float32(0.03)
    z[1, 7 * B:8 * B] *= np.float32(0.03)
    a = NF.plant(a, [0], np.arange(100, 300), NF.QNAN)
    z = NF.plant(z, [1, 2], [6 * B + 5], NF.QNAN, "re")
    rx = [(0.5, 0.125, QR.GATE)] * 4
    return z, a, rx, (B, 2, 2, 37)


def test_b_squelch_gate_and_count(pkg, dev):
    """The header's `c == 0: out = +0.0f whatever a is` and `run = !(L >= tc) ? run + 1 : 0` on the designed rows of
    squelch_cases(): the closed row's out is +0 bits throughout its NaN audio, the NaN block of row 1 counts towards
    hang (it closes behind block 7), that of row 2 does not close.  The reference shows the gate in those states; the
    device's out, levels, states and status are the reference's."""
    import torch
    st = BY_ID["squelch"]
    n = st.n(pkg)
    z, a, rx, par = squelch_cases(n)
    want = QR.squelch_ref(z, a, rx, **QR.params(*par))
    states = want[2]
    assert not states[0].any() and not want[0][0].view(np.uint32).any()
    assert states[1, 5] == 1 and states[1, 6] == 1 and states[1, 7] == 0 and np.isnan(want[1][1, 6])
    assert states[2, 5:9].all() and np.isnan(want[1][2, 6]) and states[3, 5:].all()
    for cuts in ([n], [100, 150, 6 * 48 + 5 - 250, 1, n - 6 * 48 - 6]):
        s = pkg.Squelch(rx, *par, up=QR.UP)
        zd, ad = upload((z, a), dev)
        outs, off = [], 0
        for b in cuts:
            outs.append([t.cpu().numpy() for t in s.process(zd[:, off:off + b], ad[:, off:off + b])])
            off += b
        status = s.read()
        s.close()
        got = tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3))
        assert not got[0][0].view(np.uint32).any(), "a closed gate's out is +0 whatever a is"
        for i in range(3):
            NF.same_or_both_nan(got[i], want[i], ("squelch designed", cuts, i))
        for name in QR.STATUS.names:
            NF.same_or_both_nan(status[name], want[3][name], ("squelch designed", cuts, name))


# ---- C. getting the row back ----------------------------------------------------------------------------------------

def all_rows_poisoned(st, xs, n):
    """a NaN in the last sample of every row (of every input), so that every carried record holds it"""
    return tuple(NF.plant(x, np.arange(K), [n - 1], NF.QNAN) for x in xs)


@pytest.mark.parametrize("st", STAGES, ids=ids)
def test_c_reset_after_poison(pkg, dev, st):
    """A batch that leaves a NaN in every row's carried record, reset(), the clean series: outputs and status have the
    bits of a freshly created object's -- nothing on the device is cleared from the host, so the old record is kept out
    by a select."""
    xs, clean = clean_run(st, pkg, dev)
    n = st.n(pkg)
    obj = st.make(pkg)
    run(st, pkg, dev, all_rows_poisoned(st, xs, n), obj=obj)
    obj.reset()
    got = run(st, pkg, dev, xs, obj=obj)
    obj.close()
    for i, (g, c) in enumerate(zip(flat(got), flat(clean))):
        NF.clean_rows_identical(g, c, np.arange(K), (st.id, "after reset", i))


RESTARTS = [st for st in STAGES if hasattr(st, "restarted")]


@pytest.mark.parametrize("st", RESTARTS, ids=ids)
def test_c_restart_after_poison(pkg, dev, st):
    """Demod and Carrier: set_rx to another mode; Scope: set_slot to another row.  After a batch that leaves a NaN in
    every carried record the restarted receivers have the bits of an object created with the new settings at that sample
    (Scope: of one fed zeros until then, the segment grid goes on); with only the poisoned rows 0, 16, 31, 34 restarted,
    the rows that were not touched keep the bits of a run without the restart."""
    xs, _ = clean_run(st, pkg, dev)
    n = st.n(pkg)
    poisoned = all_rows_poisoned(st, xs, n)
    tail = tuple(x[:, :n // 2] for x in xs)
    obj = st.make(pkg)
    run(st, pkg, dev, poisoned, obj=obj)
    for j in range(K):
        st.restart(obj, j)
    got = run(st, pkg, dev, tail, obj=obj)
    obj.close()
    fresh = st.restarted(pkg)
    if isinstance(st, ScopeStage):
        run(st, pkg, dev, tuple(np.zeros_like(x) for x in xs), obj=fresh)
    want = run(st, pkg, dev, tail, obj=fresh)
    fresh.close()
    for i, (g, w) in enumerate(zip(flat(got), flat(want))):
        NF.clean_rows_identical(g, w, np.arange(K), (st.id, "restarted", i))
    # the poisoned rows alone
    some = st.poison(xs, NF.QNAN, [[n - 1]] * 4)
    plain = st.make(pkg)
    run(st, pkg, dev, some, obj=plain)
    keep = run(st, pkg, dev, tail, obj=plain)
    plain.close()
    obj = st.make(pkg)
    run(st, pkg, dev, some, obj=obj)
    for j in ROWS:
        st.restart(obj, j)
    got2 = run(st, pkg, dev, tail, obj=obj)
    obj.close()
    for i, (g, w, f) in enumerate(zip(flat(got2), flat(keep), flat(got))):
        NF.clean_rows_identical(g, w, CLEAN, (st.id, "not touched", i))
        NF.clean_rows_identical(g, f, ROWS, (st.id, "restarted alone", i))


@pytest.mark.parametrize("st", [s for s in STAGES if isinstance(s, AdaptStage)], ids=ids)
def test_c_adapt_restart_needs_a_clean_history(pkg, dev, st):
    """PDDC_ADAPT_RESTART zeroes the weights only.  A NaN in sample p, then H = D + T - 1 clean samples, then RESTART:
    from there on the row has the bits of an object fed the clean series and restarted at the same sample.  RESTART one
    sample sooner: the NaN is still inside the window, the weights are poisoned again -- in the reference (asserted) and
    on the device alike."""
    xs, _ = clean_run(st, pkg, dev)
    n, H = st.n(pkg), st.H
    p = 40
    assert p + 1 + H + 50 <= n
    on = [r for r in ROWS if st.rx[r][0] != AR.OFF]
    assert len(on) >= 2 and len(on) < len(ROWS)
    ps = st.poison(xs, NF.QNAN, [[p]] * 4)

    def restarted(data, at, rows):
        def before(i, obj):
            if i == 1:
                for j in rows:
                    st.restart(obj, j)
        return run(st, pkg, dev, data, [at, n - at], before=before)

    def reference(at):
        r = AR.AdaptRef(st.rx, st.T, st.D)
        head = r.process(ps[0][:, :at])
        for j in ROWS:
            r.set_rx(j, *st.rx[j], AR.RESTART)
        return np.concatenate([head, r.process(ps[0][:, at:])], axis=1), r.weights.copy()

    late, soon = p + 1 + H, p + H
    got, want = restarted(ps, late, ROWS), reference(late)
    clean = restarted(xs, late, ROWS)
    assert np.isfinite(want[0][ROWS, late:]).all() and np.isfinite(want[1]).all()
    assert not np.isfinite(want[0][on, late - 1]).any()
    NF.clean_rows_identical(got[0][0][:, late:], clean[0][0][:, late:], np.arange(K), (st.id, "recovered"))
    NF.clean_rows_identical(got[1][0], clean[1][0], np.arange(K), (st.id, "recovered weights"))
    NF.same_or_both_nan(got[0][0][ROWS], want[0][ROWS], (st.id, "late"))
    got, want = restarted(ps, soon, ROWS), reference(soon)
    assert not np.isfinite(want[0][on, soon:]).any() and not np.isfinite(want[1][on]).any()
    NF.same_or_both_nan(got[0][0][ROWS], want[0][ROWS], (st.id, "soon"))
    NF.same_or_both_nan(got[1][0][ROWS], want[1][ROWS], (st.id, "soon, weights"))
    NF.clean_rows_identical(got[0][0], clean[0][0], CLEAN, (st.id, "soon, the other rows"))


HEALING = [st for st in STAGES if isinstance(st, (BlankerStage, SquelchStage))]


@pytest.mark.parametrize("value", list(NF.POISON))
@pytest.mark.parametrize("st", HEALING, ids=ids)
def test_c_healing_without_the_caller(pkg, dev, st, value):
    """Blanker and Squelch with one poisoned sample per row (columns 0, H - 1, TT - 1, TT) and no action of the caller: the
    reference's outputs are finite again from some output on and its ref / level / floor are finite behind the batch; the
    device has the reference's bits from that output on and in the status.  The squelch's peak is inf behind an infinity:
    sticky by definition (fmaxf), until read(clear_peak)."""
    ps, cols, one, _ = poisoned_run(st, pkg, dev, value, 0)
    assert cols[3] == [st.edge(pkg)]
    want = st.ref(ps)
    for r in ROWS:
        for g, w in zip(one[0], want[0]):
            if g.dtype == np.uint8:
                continue
            bad = np.flatnonzero(~np.isfinite(np.ascontiguousarray(w[r]).view(np.float32).reshape(w.shape[1], -1)).all(axis=1))
            first = int(bad[-1]) + 1 if bad.size else 0
            assert first < w.shape[1], (st.id, value, r, "the reference does not heal")
            assert np.array_equal(NF.words(g[r, first:]), NF.words(w[r, first:])), (st.id, value, r, first)
    for name, g, w in zip(st.status_names, one[1], want[1]):
        if name == "peak" and value != "nan":
            planted = [r for r in ROWS[:2]]                  # z is poisoned on rows 0 and 16 (SquelchStage.poison)
            assert np.isposinf(w[planted]).all() and np.isposinf(g[planted]).all(), (st.id, value, "peak")
        else:
            assert np.isfinite(w[ROWS].astype(np.float64)).all(), (st.id, value, name, "the reference does not heal")
        assert np.array_equal(NF.words(g[ROWS]), NF.words(w[ROWS].astype(g.dtype))), (st.id, value, name)


# ---- D. poisoned surroundings ---------------------------------------------------------------------------------------

def framed(shape, dtype, dev, pad, spare=2):
    """a device buffer [spare + K + spare, shape[1] + pad, ...] of the never-read pattern -> (the buffer, its host copy,
    the view of the K rows in the middle, full width)"""
    import torch
    full = (K + 2 * spare, shape[1] + pad) + tuple(shape[2:])
    host = NF.never_read(full, dtype)
    if np.dtype(dtype) == np.complex64:
        buf = torch.view_as_complex(torch.from_numpy(host.view(np.float32).reshape(full + (2,))).to(dev))
    else:
        buf = torch.from_numpy(host).to(dev)
    return buf, host, buf[spare:spare + K]


def host_words(t):
    import torch
    t = t.cpu()
    if t.dtype == torch.complex64:
        t = torch.view_as_real(t)
    return NF.words(t.contiguous().numpy())


@pytest.mark.parametrize("st", STAGES, ids=ids)
def test_d_poisoned_surroundings(pkg, dev, st):
    """Clean data, poison everywhere else.  The inputs are views of a buffer with row stride n + 37 and two spare rows
    above and below, padding and spare rows filled with 0xFFFFFFFF / 0x7FC00000; the outputs are views of buffers
    prefilled with the same pattern (row stride count + 11, spare rows; the scope's lines: spare slots and spare lines).
    Batches of 0, 1, 2, H - 1, H, TT - 1, TT, TT + 1 and the rest.  Outputs and status have the bits of the contiguous
    run in one batch; the outputs' padding and spare rows keep their fill; the input buffer is intact.  Any over-read
    turns into a NaN here."""
    TT, H = st.edge(pkg), st.H                                  # (Audio: the input column on the tile edge)
    cuts = [0, 1, 2, max(H - 1, 0), H, TT - 1, TT, TT + 1]
    n = max(st.n(pkg), sum(cuts) + 7)
    cuts.append(n - sum(cuts))
    xs = st.inputs(n)
    want = run(st, pkg, dev, xs)
    frames = []
    for x in xs:
        buf, host, view = framed(x.shape, x.dtype, dev, 37)
        view[:, :n] = upload((x,), dev)[0]
        host[2:2 + K, :n] = x
        frames.append((buf, host, view))
    obj = st.make(pkg)
    parts, off = [], 0
    for b in cuts:
        due = st.counts(obj, b)
        outs = [framed((K, d) + ((st.nfft,) if isinstance(st, ScopeStage) else ()), dt, dev, 3 if isinstance(st, ScopeStage) else 11)
                for d, dt in zip(due, st.out_dtypes)]
        o = st.process(obj, [f[2][:, off:off + b] for f in frames], bufs=[f[2] for f in outs])
        part = []
        for t, d, (buf, host, view) in zip(o, due, outs):
            assert t.shape[1] == d
            part.append(t.cpu().numpy())
            after = host_words(buf)
            filled = NF.words(host).copy().reshape(after.shape)
            mask = np.ones(after.shape, bool)
            mask[2:2 + K, :d] = False
            assert np.array_equal(after[mask], filled[mask]), (st.id, b, "an output's surroundings were written")
        parts.append(part)
        off += b
    status = st.status(obj)
    obj.close()
    got = tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(len(parts[0]))), status
    for i, (g, w) in enumerate(zip(flat(got), flat(want))):
        NF.clean_rows_identical(g, w, np.arange(K), (st.id, "surroundings", i))
    for buf, host, _ in frames:
        assert np.array_equal(host_words(buf), NF.words(host).reshape(host_words(buf).shape)), (st.id, "the input buffer changed")
