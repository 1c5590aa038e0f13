"""Non-finite samples through the thirteen per-receiver stages (RxFilter, Blanker, Adapt, Demod, Carrier, Squelch, Audio,
Scope, Eq, Denoise, Fsk, Morse, Psk) on the GPU, row by row: what one bad sample does, that it stays inside its own row,
and how the caller gets the row back (include/perseus_ddc.h, "Non-finite samples" under every stage).  One table of
stage adapters, STAGES; every test is parametrised over it.  K = 35 receivers (2 16 + 3: a partial last group for blocks
of 2, 4 and 16 receivers), n = 3 TT + 5 samples; rows 0, 16, 31 and 34 are poisoned, all others stay clean.  The
decoders' records are ragged (chars trimmed by counts, Psk's sym by nsym): run() gathers them row by row and compares
them by their words, a cell at or behind a count is nobody's.  Every comparison is equality of bits
(nonfinite.clean_rows_identical), equality of bits and of NaN positions (nonfinite.same_or_both_nan, on poisoned rows
of the bit-exact stages only) or equality of NaN positions; the only tolerances are those the reference files carry from
their own float32 models (TOL_DEMOD, TOL_DENOISE, TOL_FSK, TOL_MORSE, TOL_PSK), on soft values of poisoned rows against
the double reference, where that is finite.  Section E is the mixer's, where the rows meet: isolation is per sample index
and per bus.  What the references themselves do with these inputs -- the preconditions -- is asserted in
tests/test_nonfinite_cpu.py, which also runs the designed tests with the float32 models in the device's place."""
import numpy as np
import pytest

import adapt_ref as AR
import audio_ref as UR
import blanker_ref as BR
import carrier_ref as CR
import demod_ref as DR
import denoise_ref as NR
import eq_ref as ER
import fsk_ref as FR
import mixer_ref as MR
import morse_ref as OR
import nonfinite as NF
import psk_ref as PR
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
    kinds = None                  # per output of process(): "dense" [K, b, ...] (all of them unless given), "ragged" (a
    #                               record buffer [K, capacity, ...]) with its "count" [K] behind it: run() gathers row j's
    #                               first count[j] records, batch by batch, and gives them as nonfinite.dense()
    tails = None                  # per output the shape behind [K, capacity] (the decoders' records)
    counters = ()                 # the status names that count since create: a restart leaves them
    unseen = ()                   # the poisoned rows that show nothing of their input (a decoder's OFF row)
    sparse = False                # the outputs look at some samples only (Psk: the strobes'), a short window may pass unseen
    heal = 0                      # good samples a row needs in front of a restart
    restart_on_clean = False      # a restarted row is compared with: a fresh object (False), or -- where sample indices
    #                               or a frame grid go on across a restart -- an object fed the clean series and
    #                               restarted at the same sample

    def carried(self, n):
        """the columns whose poison is in the carried record behind a batch of n"""
        return [n - 1]

    def recovered(self, fed):
        """the tail's first output that is a restarted receiver's, restarted after `fed` samples"""
        return 0

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


class EqStage(Stage):
    tile, in_place, exact, out_dtypes = "eq_tile_outputs", 0, True, (np.float32,)
    status_names = ("state",)

    def __init__(self, S):
        self.S = self.H = S
        self.id = f"eq-S{S}"
        self.rx = ER.interleaved_rx(K, S, first=200)
        p = ER.pool()
        # the poisoned rows: an empty cascade on row 16 (the words pass, there are no states), 1 .. S sections on the others
        for r, ns in zip(ROWS, (max(S // 2, 1), 0, 1, S)):
            self.rx[r] = [p[(r + 2 * s) % len(p)] for s in range(ns)]

    def inputs(self, n):
        return (AR.audio_series(K, n, 33),)

    def make(self, pkg, rev=False):
        return pkg.Eq(self.pick(self.rx, rev), self.S)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=xs[0] if in_place else bufs[0] if bufs else None),)

    def status(self, obj):
        return (obj.read_state(),)

    def ref(self, xs, cuts=None):
        r = ER.EqRef(self.rx, self.S)
        return (AR.run_cuts(r, xs[0], cuts),), (r.state.copy(),)

    def restart(self, obj, j):
        obj.set_rx(j, self.rx[j], ER.RESTART)

    def restarted(self, pkg):
        return self.make(pkg)


class DenoiseStage(Stage):
    # the tile is pddc_denoise_tile_frames() frames of hop samples.  TT, the column the placements and cuts stand on, is
    # the first tile seam at or behind the delay nfft: the input of the first output that is not 0 by definition; H is the
    # hop, so that the ladder has batches that complete no frame and exactly one
    out_dtypes, status_names, restart_on_clean = (np.float32,), ("noise",), True

    def __init__(self, nfft, hop):
        self.nfft, self.hop, self.H, self.heal = nfft, hop, hop, nfft
        self.id = f"denoise-{nfft}-{hop}"
        self.w = NR.window(nfft, hop)
        self.rx = NR.receivers(K)
        # the poisoned rows between them: NR, NR with HOLD, OFF, NR
        # (HOLD on row 34, whose first poison is never in frame 0: a first frame sets N whatever HOLD says)
        for r, rx in zip(ROWS, ((NR.NR, 2.0, 0.1, 0.98), (NR.NR, 1.5, 0.1, 0.7), (NR.OFF, 2.0, 0.1, 0.98), (NR.NR, 2.0, 0.05, 0.98, NR.HOLD))):
            self.rx[r] = rx

    def carried(self, n):
        """the last sample (in the inputs of the open frames alone) and one a hop earlier: frames that hold it are
        complete, so S, N, A, the overlap sums and the finished values not yet given out hold it too"""
        return [n - 1 - self.hop, n - 1]

    def TT(self, pkg):
        step = int(pkg.denoise_tile_frames()) * self.hop
        return -(-self.nfft // step) * step

    def inputs(self, n):
        return (NR.rows(K, n, 7),)

    def make(self, pkg, rev=False):
        return pkg.Denoise(self.pick(self.rx, rev), self.nfft, self.hop, self.w, **NR.DEFAULTS)

    def process(self, obj, xs, bufs=None, in_place=False):
        return (obj.process(xs[0], out=bufs[0] if bufs else None),)

    def status(self, obj):
        return (obj.read_noise(),)

    def stream(self):
        return NR.Stream(self.nfft, self.hop, self.w, self.rx, np.float32)

    def ref(self, xs, cuts=None):
        s = self.stream()
        return (AR.run_cuts(s, xs[0], cuts).astype(np.float32),), (s.noise(),)

    def restart(self, obj, j):
        r = self.rx[j]
        obj.set_rx(j, *r[:4], (r[4] if len(r) > 4 else 0) | NR.RESTART)

    def recovered(self, fed):
        """the restart makes frame q = fed div hop, the next one completed, a first frame: out index q hop + nfft"""
        return fed // self.hop * self.hop + self.nfft - fed


class DecoderStage(Stage):
    """Fsk, Morse, Psk: W taps, a bank of two modems / keyers, receiver j on the one of j mod 2; row 31 is OFF.  The
    records are ragged (chars trimmed by counts, Psk's sym by nsym); the soft values d and p come one per sample."""
    restart_on_clean = True
    unseen = (ROWS[2],)

    def __init__(self, W):
        self.W = self.H = W
        self.id = f"{self.name}-W{W}"
        self.setup()
        self.sel[ROWS[2]] = (self.sel[ROWS[2]][0], 0)                  # OFF: nothing of z is read

    def carried(self, n):
        """the last sample, and one W / 2 earlier: the second has reached the carried OUTPUTS too where there are any"""
        return sorted({n - 1 - max(self.W // 2, 1), n - 1})

    def make(self, pkg, rev=False):
        return getattr(pkg, self.name.capitalize())(self.bank, self.pick(self.sel, rev), self.W, **self.params)

    def status(self, obj):
        st = obj.read()
        return tuple(st[name].copy() for name in self.status_names)

    def restart(self, obj, j):
        obj.set_rx(j, self.sel[j][0], self.sel[j][1] | self.R.RESTART)

    def reference(self, f32):
        return self.Ref(self.bank, self.sel, self.W, f32=f32, **self.params)

    def ref(self, xs, cuts=None, f32=True):
        """the float32 model (f32 False: the double reference) in run()'s form"""
        r = self.reference(f32)
        got = self.R.run_cuts(r, xs[0], cuts)
        n = xs[0].shape[1]
        chars = NF.record_words(got[0])
        outs = [NF.dense(chars, n), np.array([c.shape[0] for c in chars], np.int32)]
        if self.name == "psk":
            sym = [np.asarray(s, np.float64).astype(np.float32).reshape(-1, 2) for s in got[1]]
            outs += [NF.dense(sym, n), np.array([s.shape[0] for s in sym], np.int32)]
        else:
            outs.append(np.asarray(got[1], np.float64).astype(np.float32))
        st = got[3]
        return tuple(outs), tuple(st[name].copy() for name in self.status_names)


class FskStage(DecoderStage):
    name, tile, R, Ref, params = "fsk", "fsk_tile_outputs", FR, FR.FskRef, {}
    kinds, tails, out_dtypes = ("ragged", "count", "dense"), ((4,), (), ()), (np.int32, np.int32, np.float32)
    status_names, counters = FR.STATUS.names, ("chars", "framing", "false_starts")

    def setup(self):
        W = self.W
        if W == 2:                                                     # 4 samples per bit, 8 data bits, tones at +-1/4
            m = FR.modem(4.0, 1.0, 1.0, -1.0, 2, 8)
            self.bank, self.sig = [m, (m[0], m[1], (1 << 30) - 77777, 8)], (4, 8, 0.25, -0.25, 20.0)
        else:                                                          # 16 samples per bit, 5 data bits, tailed windows
            self.bank = [FR.tailed_modem(W, 100 * W), FR.tailed_modem(W, 100 * W + 1, (1 << 28) - 9973)]
            self.sig = (FR.SPS, 5, FR.MARK, FR.SPACE, 16.0)
        self.sel = [(j % 2, FR.ON | (FR.REVERSE if j % 5 == 3 else 0)) for j in range(K)]

    def inputs(self, n):
        sps, nbits, mark, space, snr = self.sig
        nch = n // int(sps * (nbits + 2.5)) + 1
        rows = []
        for j in range(K):
            codes = [(37 * j + 11 * i + 5) % (1 << nbits) for i in range(nch)]
            rows.append(FR.two_tone(FR.keying(codes, nbits=nbits, sps=sps)[:n], mark, space, snr, 81000 + j, n))
        return (np.stack(rows),)

    def counts(self, obj, b):
        return (obj.max_chars(b), None, b)

    def process(self, obj, xs, bufs=None, in_place=False):
        if bufs:
            return tuple(obj.process(xs[0], chars=bufs[0], counts=bufs[1], d=bufs[2]))
        return tuple(obj.process(xs[0], want_d=True))


class MorseStage(DecoderStage):
    name, tile, R, Ref, params = "morse", "morse_tile_outputs", OR, OR.MorseRef, OR.CASE_PARAMS
    kinds, tails, out_dtypes = ("ragged", "count", "dense"), ((4,), (), ()), (np.int32, np.int32, np.float32)
    status_names, counters = OR.STATUS.names, ("chars", "marks")

    def setup(self):
        W = self.W
        if W == 2:                                                     # 4 samples per dot
            h, two = np.full(2, 0.5, np.float32), OR.two_of(OR.FAST_SPD)
            self.bank, self.spd = [(h, two, 512, 4 * two, 0), (h, two, 512, 4 * two, 2)], OR.FAST_SPD
        else:                                                          # 16 samples per dot; the second keyer starts off speed
            self.bank, self.spd = [OR.tailed_keyer(W, 100 * W), OR.tailed_keyer(W, 100 * W + 1, speed=0.4, shift=3)], OR.SPD
        self.sel = [(j % 2, OR.ON | (OR.FIXED if j % 4 == 2 else 0)) for j in range(K)]

    def line(self, j, n):
        """receiver j's key line: "VV" and words of three characters, as many as n samples hold"""
        text = "VV " + " ".join(OR.PARITY_TEXTS[(j + i) % len(OR.PARITY_TEXTS)].strip() for i in range(14))
        line = OR.keying(text, self.spd, OR.LEAD * self.spd // OR.SPD)
        assert line.size >= n
        return line[:n]

    def inputs(self, n):
        return (np.stack([OR.keyed_carrier(self.line(j, n), 30.0, 82000 + j, n, (j % 5 - 2) / 2048.0) for j in range(K)]),)

    def counts(self, obj, b):
        return (obj.max_chars(b), None, b)

    def process(self, obj, xs, bufs=None, in_place=False):
        if bufs:
            return tuple(obj.process(xs[0], chars=bufs[0], counts=bufs[1], p=bufs[2]))
        return tuple(obj.process(xs[0], want_p=True))


class PskStage(DecoderStage):
    name, tile, R, Ref, params = "psk", "psk_tile_outputs", PR, PR.PskRef, {}
    kinds, tails = ("ragged", "count", "ragged", "count"), ((4,), (), (2,), ())
    out_dtypes = (np.int32, np.int32, np.float32, np.int32)
    status_names, counters = PR.STATUS.names, ("chars", "symbols")

    def setup(self):
        W = self.W
        if W == 2:                                                     # 8 samples per symbol
            h = np.full(2, 0.5, np.float32)
            self.bank, self.sps, self.sparse = [(h, 1 << 29, 1, 1 << 25), (h, 1 << 29, 2, 1 << 27)], 8, True
        else:                                                          # 16 samples per symbol; the second modem's clock is fixed
            self.bank, self.sps = [PR.tailed_modem(W, 16, 100 * W), PR.tailed_modem(W, 16, 100 * W + 1, step=0, q=2)], 16
        self.sel = [(j % 2, PR.ON) for j in range(K)]

    def inputs(self, n):
        sps, rows = self.sps, []
        for j in range(K):
            text = PR.bits_of(PR.PARITY_TEXTS[j % len(PR.PARITY_TEXTS)] + " " + PR.PARITY_TEXTS[(j + 4) % len(PR.PARITY_TEXTS)])
            bits = ([0] * 6 + text * (n // (sps * len(text)) + 1))[:n // sps + 2]
            rows.append(PR.bpsk(bits, sps, n, lead=sps, snr_db=PR.PARITY_SNR, seed=83000 + j, freq=(j % 5 - 2) / 8192.0,
                                ppm=(j % 7 - 3) * 100.0, phase=(j % 8) / 8.0))
        return (np.stack(rows),)

    def counts(self, obj, b):
        return (obj.max_chars(b), None, obj.max_syms(b), None)

    def process(self, obj, xs, bufs=None, in_place=False):
        if bufs:
            return tuple(obj.process(xs[0], chars=bufs[0], counts=bufs[1], sym=bufs[2], nsym=bufs[3]))
        return tuple(obj.process(xs[0], want_sym=True))


# the small and the large end of every stage's taps / delays (test D's list); the blanker also at the issue's (32, 2, 4)
STAGES = [RxFilterStage(1), RxFilterStage(2), RxFilterStage(256), AudioStage(32, 1), AudioStage(128, 64), ScopeStage(256, 16),
          DemodStage(), CarrierStage(3), CarrierStage(255), SquelchStage(), AdaptStage(16, 1), AdaptStage(128, 256),
          BlankerStage(32, 0, 0), BlankerStage(32, 2, 4), BlankerStage(32, 128, 128),
          EqStage(1), EqStage(8), DenoiseStage(256, 64), DenoiseStage(1024, 256), FskStage(2), FskStage(256),
          MorseStage(2), MorseStage(256), PskStage(2), PskStage(256)]
DECODERS = [st for st in STAGES if isinstance(st, DecoderStage)]
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


def collect(st, o, due, what):
    """one batch's outputs as numpy: a dense one [K, due, ...] as it is; a record buffer as the list of the records
    written per row, at most the bound `due` of them; a count [K] as it is"""
    kinds = st.kinds or ("dense",) * len(o)
    assert len(o) == len(due) == len(kinds), what
    part = []
    for i, (t, d, kind) in enumerate(zip(o, due, kinds)):
        if kind == "dense":
            assert t.shape[0] == K and t.shape[1] == d, what
            part.append(t.cpu().numpy())
        elif kind == "ragged":
            assert kinds[i + 1] == "count" and t.shape[0] == K and t.shape[1] >= d, what
            counts = o[i + 1].cpu().numpy()
            assert (counts <= d).all(), (what, "more records than the bound", counts.max(), d)
            part.append(NF.gather(t.cpu().numpy(), counts))
        else:
            assert tuple(t.shape) == (K,), what
            part.append(t.cpu().numpy())
    return part


def join(st, parts, n):
    """the batches' collect()s as one: dense outputs concatenated along axis 1, the records of a row one behind the other
    (as nonfinite.dense of width n: no batch of n samples holds more), the counts added"""
    kinds = st.kinds or ("dense",) * len(parts[0])
    outs = []
    for i, kind in enumerate(kinds):
        col = [p[i] for p in parts]
        if kind == "dense":
            outs.append(np.concatenate(col, axis=1))
        elif kind == "ragged":
            outs.append(NF.dense([np.concatenate([c[j] for c in col]) for j in range(K)], n))
        else:
            outs.append(np.sum(col, axis=0, dtype=col[0].dtype))
    return tuple(outs)


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
        parts.append(collect(st, o, due, (st.id, i, b)))
        off += b
    assert off == n
    status = st.status(obj)
    if own:
        obj.close()
    return join(st, parts, n), status


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
    """Blanker, Squelch, Adapt, Eq: the poisoned rows' outputs and status (Eq: the binary64 states) have the reference's
    bits wherever the reference has no NaN, and NaN exactly where it has one; the cut run against the run in one batch in
    the same way."""
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


_before = {}


def made_before(st, pkg, dev, xs, col):
    """per output: how many of its values along axis 1 are made of the inputs before column `col` alone -- a number, or
    for a record buffer one per row: the records the device has emitted once the clean series' first `col` samples are in
    (the count itself, a total, has none: 0)"""
    if not st.kinds:
        return [st.outputs_before(col)] * len(st.out_dtypes)
    if (st.id, col) not in _before:
        head = run(st, pkg, dev, tuple(x[:, :col] for x in xs))[0] if col else None
        _before[st.id, col] = [col if kind == "dense" else 0 if kind == "count" or not col else head[i + 1]
                               for i, kind in enumerate(st.kinds)]
    return _before[st.id, col]


@pytest.mark.parametrize("st,layout", MODEL_CASES, ids=[f"{st.id}-{layout}" for st, layout in MODEL_CASES])
def test_b_poisoned_rows_of_the_model_stages(pkg, dev, st, layout):
    """RxFilter, Audio, Scope, Demod, Carrier, Denoise, Fsk, Morse, Psk with a NaN: the NaN positions are the float32
    model's, part by part (the decoders' d, p and (d, x) pairs have none: a NaN reads as +0 there); every output made of
    the samples before a row's first NaN -- of a decoder's records those the device has emitted by then (made_before) --
    has the clean run's bits.  RxFilter, Audio, Scope have no other
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
    xs, _ = clean_run(st, pkg, dev)
    for r, cs in zip(ROWS, cols):
        before = made_before(st, pkg, dev, xs, min(cs))
        for i, (g, cl) in enumerate(zip(one[0], clean[0])):
            if g.ndim == 1:                                     # (a count)
                continue
            k = before[i] if np.ndim(before[i]) == 0 else before[i][r]
            assert np.array_equal(NF.words(g[r, :k]), NF.words(cl[r, :k])), (st.id, layout, r, i, "before")
        if st.fir:
            span = set()
            for col in cs:
                span |= set(int(v) for v in st.nan_span(col, n))
            found = nan_rows(one[0][0])[r]
            assert found == span and (span or min(cs) == n - 1), (st.id, layout, r, sorted(found ^ span)[:6])
            keep = np.array(sorted(set(range(one[0][0].shape[1])) - span), dtype=np.int64)
            for i, (g, cl) in enumerate(zip(one[0], clean[0])):
                assert np.array_equal(NF.words(g[r, keep]), NF.words(cl[r, keep])), (st.id, layout, r, i, "behind the NaNs")


def decoder_rows_against(st, got, want, rows, what):
    """`got` against the double reference `want` (both in run()'s form) on `rows`.  Records: start, code, flags / nel /
    nbits -- the first three words -- and Morse's `two` exactly, a float quality within the reference file's tolerance;
    counts, nsym and the integer status exactly.  Soft values (d, p, the (d, x) pairs, the float status) within that
    tolerance -- Morse's p, pk and fl relative to the row's largest finite p, as in test_gpu_morse.py -- wherever the
    reference is finite, which must be more than half of every row's samples / strobes: the share left out is a
    condition, not a result.  -> the largest error met, in units of the tolerance"""
    tol, worst = getattr(st.R, "TOL_" + st.name.upper()), 0.0
    scale = np.ones(K)
    if st.name == "morse":
        p = want[0][2].astype(np.float64)
        scale = np.where(np.isfinite(p), p, 0.0).max(axis=1)
        scale[scale == 0] = 1.0                                 # (an OFF row)
    nout = len(st.kinds)

    def soft(gv, wv, r, known, where):
        """known: how many of the leading positions hold values (None: a status word or a quality, no share is asked)"""
        nonlocal worst
        fin = np.isfinite(wv.astype(np.float64))
        if known is not None:
            whole = fin.reshape(wv.shape[0], -1).all(axis=1)[:known]
            assert whole.sum() * 2 > known or not known, (what, where, r, "the reference leaves too little to compare", int(whole.sum()), known)
        if fin.any():
            e = float(np.abs(gv.astype(np.float64) - wv)[fin].max()) / (tol * scale[r])
            worst = max(worst, e)
            assert e <= 1.0, (what, where, r, e)

    for i, (g, w) in enumerate(zip(flat(got), flat(want))):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
        kind = st.kinds[i] if i < nout else "status"
        for r in rows:
            if g.dtype != np.float32 and kind != "ragged":      # counts, nsym, the integer status
                assert np.array_equal(g[r], w[r]), (what, i, kind, r, g[r], w[r])
            elif g.dtype != np.float32:                         # records
                assert np.array_equal(g[r, :, :3], w[r, :, :3]), (what, "records", r, np.argwhere(g[r, :, :3] != w[r, :, :3])[:3].tolist())
                if st.name == "morse":
                    assert np.array_equal(g[r, :, 3], w[r, :, 3]), (what, "two", r)
                else:
                    soft(g[r, :, 3].copy().view(np.float32), w[r, :, 3].copy().view(np.float32), r, None, "quality")
            elif kind == "ragged":                              # Psk's (d, x) pairs: the strobes the reference has
                soft(g[r], w[r], r, int(want[0][i + 1][r]), "sym")
            elif kind == "dense":
                soft(g[r], w[r], r, w.shape[1], "soft")
            else:
                soft(np.atleast_1d(g[r]), np.atleast_1d(w[r]), r, None, st.status_names[i - nout])
    return worst


DECODER_CASES = [(st, v, layout) for st in DECODERS for v in NF.POISON for layout in (0, 1)]


@pytest.mark.parametrize("st,value,layout", DECODER_CASES, ids=[f"{st.id}-{v}-{layout}" for st, v, layout in DECODER_CASES])
def test_b_poisoned_rows_of_the_decoders(pkg, dev, st, value, layout):
    """Fsk, Morse, Psk: a poisoned row's records, counts, strobe counts and integer status are the double reference's of
    the poisoned series, exactly; its soft values are within TOL_FSK / TOL_MORSE / TOL_PSK of it wherever it is finite
    (decoder_rows_against; tests/test_nonfinite_cpu.py asserts that the reference leaves more than half of every row to
    compare and that its float32 model decides as it does on these very series).  The clean rows too."""
    ps, _, one, cut = poisoned_run(st, pkg, dev, value, layout)
    want = st.ref(ps, f32=False)
    e = decoder_rows_against(st, one, want, range(K), (st.id, value, layout))
    print(f"{st.id} {value} {layout}: the largest error is {e:.3f} of the tolerance")
    for i, (c, g) in enumerate(zip(flat(cut), flat(one))):
        NF.same_or_both_nan(c[ROWS], g[ROWS], (st.id, value, layout, "cut", i))


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


EQS = [st for st in STAGES if isinstance(st, EqStage)]
DENOISES = [st for st in STAGES if isinstance(st, DenoiseStage)]


@pytest.mark.parametrize("value", list(NF.POISON))
@pytest.mark.parametrize("st", EQS, ids=ids)
def test_b_designed_eq_is_sticky(pkg, dev, st, value):
    """Eq, "states that are not finite stay so ... and every output after it is not finite.  OFF passes the words and has
    no states": one NaN or infinity at column TT.  A row with sections is not finite from that sample to the end, and so
    are its states behind the batch; row 16, the empty cascade, is its input word for word.  The reference shows it
    (asserted) before the device is asked; in cuts as in one batch."""
    TT = st.edge(pkg)
    xs, _ = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.POISON[value], [[TT]] * 4)
    on = [r for r in ROWS if st.rx[r]]
    off = [r for r in ROWS if not st.rx[r]]
    assert len(on) == 3 and off == [16]
    for (out,), (state,) in (st.ref(ps), run(st, pkg, dev, ps), run(st, pkg, dev, ps, st.cuts(pkg))):
        assert np.isfinite(out[on, :TT]).all() and not np.isfinite(out[on, TT:]).any()
        for r in on:
            assert not np.isfinite(state[r, :len(st.rx[r])]).all(axis=1).any(), (st.id, value, r, state[r])
        assert np.array_equal(NF.words(out[off]), NF.words(ps[0][off])) and not NF.words(state[off]).any()


def denoise_frames(st, c):
    """the frames that hold sample c, and the first out index behind everything they reach: frame q holds the inputs
    (q + 1) hop - nfft .. (q + 1) hop - 1, its term reaches y up to (q + 1) hop - 1, and out[m] = y[m - nfft]"""
    first = c // st.hop
    last = first + st.nfft // st.hop - 1
    return first, last, (last + 1) * st.hop + st.nfft


@pytest.mark.parametrize("st", DENOISES, ids=ids)
def test_b_designed_denoise_one_nan(pkg, dev, st):
    """Denoise, "N stays NaN (read_noise shows it) when good samples follow ... the output is finite again, the input
    through the floor gain (through 1 with OFF)" and "Under HOLD S and N are not touched and A alone is lost, for one
    frame": one NaN at column hop + 5 (not in frame 0) of rows 0 and 16 (NR), 31 (OFF) and 34 (NR with HOLD).  The outputs the R frames
    that hold it reach are NaN, every output behind them is finite.  Rows 0, 16, 31: every bin of N is NaN behind the
    batch, and the finite outputs are gmin (OFF: 1) times the input nfft samples ago, to 1e-5 of the row's largest sample
    (G = gmin in every bin; what is left is the windows' squares summing to 1 and a handful of float32 roundings per
    value, some 2^-21 each).  Row 34: N has the bits of the clean run's (HOLD never touches it behind the first frame),
    and the outputs are finite from the same index on.  The float32 model shows all of it (asserted); the device has the
    model's NaN positions, N as said, and finite outputs within TOL_DENOISE of the model's."""
    c = st.hop + 5
    xs, clean = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.QNAN, [[c]] * 4)
    first, last, m0 = denoise_frames(st, c)
    n = st.n(pkg)
    assert m0 + 100 <= n and [len(st.rx[r]) > 4 and bool(st.rx[r][4] & NR.HOLD) for r in ROWS] == [False, False, False, True]
    want = st.ref(ps)
    model_clean = st.ref(xs)
    x = xs[0].astype(np.float64)
    for what, ((out,), (N,)), clean_N in (("model", want, model_clean[1][0]), ("device", run(st, pkg, dev, ps), clean[1][0]),
                                          ("device, cut", run(st, pkg, dev, ps, st.cuts(pkg)), clean[1][0])):
        f = np.isfinite(out)
        lo = max((first + 1) * st.hop, st.nfft)                 # (out[m] = 0 for m < nfft)
        assert f[ROWS, :lo].all() and not f[ROWS, lo:m0].any() and f[ROWS, m0:].all(), what
        assert np.isnan(N[ROWS[:3]]).all(), what
        assert np.isfinite(clean_N[34]).all() and np.array_equal(NF.words(N[34]), NF.words(clean_N[34])), what
        for r in ROWS[:3]:
            g = 1.0 if st.rx[r][0] == NR.OFF else float(np.float32(st.rx[r][2]))
            e = np.abs(out[r, m0:] - g * x[r, m0 - st.nfft:n - st.nfft]).max() / np.abs(x[r]).max()
            assert e <= 1e-5, (what, r, e)
        if what != "model":
            assert np.array_equal(np.isnan(out), np.isnan(want[0][0])), what
            e = NR.metric(out[ROWS, m0:], want[0][0][ROWS, m0:])
            print(f"{st.id} behind a NaN, {what}: {e:.2e} (TOL_DENOISE {NR.TOL_DENOISE:.2e})")
            assert e <= NR.TOL_DENOISE, (what, e)
            NF.clean_rows_identical(out, clean[0][0], CLEAN, (st.id, what, "the other rows"))


@pytest.mark.parametrize("st", DENOISES, ids=ids)
def test_b_designed_denoise_restart_needs_a_clean_frame(pkg, dev, st):
    """Denoise, "the caller feeds nfft good samples and then calls set_rx with PDDC_DENOISE_RESTART; the next completed
    frame q holds good samples only and is a first frame, and from out index q hop + nfft on ... the row is that of a
    receiver restarted there".  A NaN in sample p = j hop - nfft, the first sample of frame j - 1 (j = R + 3).  RESTART
    behind j hop samples: frame j is the first frame and holds good samples only; from out index j hop + nfft on outputs
    and N have the bits of an object fed the clean series and restarted at the same sample.  RESTART one sample sooner,
    behind j hop - 1: the next completed frame is j - 1, it holds the NaN, and a first frame takes S = N = P: N is NaN
    again -- in the float32 model (asserted) and on the device alike.  The shape of
    test_c_adapt_restart_needs_a_clean_history."""
    hop, nfft = st.hop, st.nfft
    j = nfft // hop + 3
    p, late, soon = j * hop - nfft, j * hop, j * hop - 1
    n = st.n(pkg)
    xs, _ = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.QNAN, [[p]] * 4)
    start = late + nfft
    assert start + 50 <= n

    def restarted(data, at):
        def before(i, obj):
            if i == 1:
                for r in ROWS:
                    st.restart(obj, r)
        return run(st, pkg, dev, data, [at, n - at], before=before)

    def model(data, at):
        s = st.stream()
        head = s.process(data[0][:, :at])
        for r in ROWS:
            rx = st.rx[r]
            s.set_rx(r, *rx[:4], (rx[4] if len(rx) > 4 else 0) | NR.RESTART)
        return np.concatenate([head, s.process(data[0][:, at:])], axis=1).astype(np.float32), s.noise()

    want, want_clean = model(ps, late), model(xs, late)
    assert np.array_equal(NF.words(want[0][:, start:]), NF.words(want_clean[0][:, start:])) and np.isfinite(want[1]).all()
    assert np.array_equal(NF.words(want[1]), NF.words(want_clean[1])) and not np.isfinite(want[0][ROWS, start - 1]).any()
    got, clean = restarted(ps, late), restarted(xs, late)
    NF.clean_rows_identical(got[0][0][:, start:], clean[0][0][:, start:], np.arange(K), (st.id, "recovered"))
    NF.clean_rows_identical(got[1][0], clean[1][0], np.arange(K), (st.id, "recovered, N"))
    assert np.array_equal(np.isnan(got[0][0]), np.isnan(want[0])), (st.id, "late, NaN positions")
    want = model(ps, soon)
    assert np.isnan(want[1][ROWS]).all()
    got = restarted(ps, soon)
    assert np.isnan(got[1][0][ROWS]).all(), (st.id, "soon: N")
    assert np.array_equal(np.isnan(got[0][0]), np.isnan(want[0])), (st.id, "soon, NaN positions")
    NF.clean_rows_identical(got[0][0], restarted(xs, soon)[0][0], CLEAN, (st.id, "soon, the other rows"))


def run_of(line, value, least, after):
    """the middle of the first run of `value` in the boolean line that is at least `least` long and begins behind `after`"""
    i = after
    while i < line.size:
        if line[i] == value and line[i - 1] != value:
            k = i
            while k < line.size and line[k] == value:
                k += 1
            if k - i >= least and k < line.size:
                return (i + k) // 2
            i = k
        else:
            i += 1
    raise AssertionError("no such run")


@pytest.mark.parametrize("st", [s for s in DECODERS if s.name == "morse"], ids=ids)
def test_b_designed_morse_mark_and_gap(pkg, dev, st):
    """Morse, "a NaN or an infinity in the window reads as no signal, nothing non-finite reaches a tracker, and nothing
    is left behind once the sample has left the window": a NaN, +inf and -inf in the middle of a dash and another of them
    in the middle of a character gap, on rows 0, 16 and 34 (31 is OFF).  In the float32 model p is +0 over exactly the W
    outputs behind each (the two spans may meet) and finite everywhere, and pk, fl and the status are finite; the device's p is +0 there, its
    status (chars, marks, two, nel, key, pk, fl) and its records have the model's bits -- one float32 operation
    sequence, so no tolerance is asked -- and the other rows have the clean run's."""
    n, W = st.n(pkg), st.W
    xs, clean = clean_run(st, pkg, dev)
    z = xs[0]
    values = {0: (NF.QNAN, np.float32(np.inf)), 16: (np.float32(np.inf), NF.QNAN), 34: (np.float32(-np.inf), NF.QNAN)}
    cols = {}
    for r, (in_mark, in_gap) in values.items():
        line = st.line(r, n)
        mark = run_of(line, True, 3 * st.spd, 100)
        gap = run_of(line, False, 3 * st.spd, 100)
        assert gap + W < n - 1
        cols[r] = (mark, gap)
        z = NF.plant(NF.plant(z, [r], [mark], in_mark, "re" if r else "both"), [r], [gap], in_gap, "im" if r else "both")
    want = st.ref((z,))
    for what, (outs, status) in (("model", want), ("device", run(st, pkg, dev, (z,))), ("device, cut", run(st, pkg, dev, (z,), st.cuts(pkg)))):
        p = outs[2]
        assert np.isfinite(p).all(), what
        for r, cs in cols.items():
            span = np.zeros(n, bool)
            for c in cs:
                span[c:c + W] = True
            assert not NF.words(p[r, span]).any() and (p[r, ~span] > 0).all(), (what, r, cs)
        for name, s in zip(st.status_names, status):
            assert np.isfinite(s.astype(np.float64)).all(), (what, name)
        if what != "model":
            for i, (g, w) in enumerate(zip(outs[:2] + status, want[0][:2] + want[1])):
                assert g.dtype == w.dtype and np.array_equal(NF.words(g[ROWS]), NF.words(w[ROWS])), (st.id, what, i)
            for g, c in zip(outs + status, flat(clean)):
                NF.clean_rows_identical(g, c, CLEAN, (st.id, what, "the other rows"))
    assert any(want[1][st.status_names.index("marks")][r] > 0 for r in cols)


@pytest.mark.parametrize("st", [s for s in DECODERS if s.name == "fsk"], ids=ids)
def test_b_designed_fsk_window(pkg, dev, st):
    """Fsk, "while a NaN is in the window, pm or ps and with it s is NaN, so d = +0 and the sample reads mark ...
    Nothing is left behind once the sample has left the window": a NaN at column TT - 3 of rows 0, 16 and 34 (31 is OFF).
    d is +0, by its bits, over exactly the W outputs TT - 3 .. TT - 4 + W, whose windows straddle the tile seam, and
    every other d has the clean run's bits: d is a function of its window alone.  The float32 model shows it (asserted,
    with the clean d not 0 at either end of the span); in cuts as in one batch."""
    W, c = st.W, st.edge(pkg) - 3
    xs, clean = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.QNAN, [[c]] * 4)
    on = [r for r in ROWS if st.sel[r][1] & FR.ON]
    assert on == [0, 16, 34]
    model_clean = st.ref(xs)[0][2]
    for what, (outs, _), cl in (("model", st.ref(ps), model_clean), ("device", run(st, pkg, dev, ps), clean[0][2]),
                                ("device, cut", run(st, pkg, dev, ps, st.cuts(pkg)), clean[0][2])):
        d = outs[2]
        assert cl[on, c].all() and cl[on, c + W - 1].all(), "the clean d is 0 there anyway"
        assert not NF.words(d[on, c:c + W]).any(), (st.id, what, "d is not +0 in the window")
        keep = np.r_[0:c, c + W:d.shape[1]]
        assert np.array_equal(NF.words(d[:, keep]), NF.words(cl[:, keep])), (st.id, what, "d outside the window")
        assert not NF.words(d[31]).any()


@pytest.mark.parametrize("st", [s for s in DECODERS if s.name == "psk"], ids=ids)
def test_b_designed_psk_nan_strobes(pkg, dev, st):
    """Psk, "bit = dot > 0: ... a NaN reads as 0, the idle bit" and "A NaN moves nothing": a NaN at column TT - 3 of rows
    0, 16 and 34.  In the double reference the strobes whose pair holds the NaN give (d, x) = (+0, +0) -- s is NaN, so
    s > 0 fails --, there are such strobes, and every other pair is finite.  The device has (+0, +0), by the bits, at the
    same strobes; its acc, symbols, reg and chars behind the batch are the reference's (a clock that moved on a NaN
    comparison would show in acc), d_last and x_last are within TOL_PSK."""
    c = st.edge(pkg) - 3
    xs, _ = clean_run(st, pkg, dev)
    ps = st.poison(xs, NF.QNAN, [[c]] * 4)
    on = [0, 16, 34]
    want = st.ref(ps, f32=False)
    wsym, wn = want[0][2], want[0][3]
    assert np.isfinite(wsym).all()
    zero = {r: [k for k in range(1, wn[r]) if not NF.words(wsym[r, k]).any()] for r in on}
    assert all(zero[r] for r in on), zero
    for what, got in (("device", run(st, pkg, dev, ps)), ("device, cut", run(st, pkg, dev, ps, st.cuts(pkg)))):
        sym, ns = got[0][2], got[0][3]
        assert np.array_equal(ns, wn), (st.id, what)
        for r in on:
            assert not NF.words(sym[r, zero[r]]).any(), (st.id, what, r, "a NaN strobe's pair is not (+0, +0)")
            assert np.isfinite(sym[r]).all()
        for name, g, w in zip(st.status_names, got[1], want[1]):
            if name in ("d_last", "x_last"):
                assert np.abs(g[on].astype(np.float64) - w[on]).max() <= PR.TOL_PSK, (st.id, what, name)
            else:
                assert np.array_equal(g[on], w[on]), (st.id, what, name, g[on], w[on])


# ---- C. getting the row back ----------------------------------------------------------------------------------------

def all_rows_poisoned(st, xs, n):
    """a NaN in the last sample of every row (of every input), so that every carried record holds it; for the decoders
    one W / 2 samples earlier too, which the carried filter outputs hold (Stage.carried)"""
    return tuple(NF.plant(x, np.arange(K), st.carried(n), NF.QNAN) for x in xs)


@pytest.mark.parametrize("st", STAGES, ids=ids)
def test_c_reset_after_poison(pkg, dev, st):
    """A batch that leaves a NaN in every row's carried record (the decoders: in the carried inputs and, from a second
    NaN W / 2 samples earlier, in the carried filter outputs; Denoise: in the inputs of the open frames; Eq: in the
    binary64 states), reset(), the clean series: outputs, records, counts and status have the bits of a freshly created
    object's -- nothing on the device is cleared from the host, so the old record is kept out by a select."""
    xs, clean = clean_run(st, pkg, dev)
    n = st.n(pkg)
    obj = st.make(pkg)
    run(st, pkg, dev, all_rows_poisoned(st, xs, n), obj=obj)
    obj.reset()
    got = run(st, pkg, dev, xs, obj=obj)
    obj.close()
    for i, (g, c) in enumerate(zip(flat(got), flat(clean))):
        NF.clean_rows_identical(g, c, np.arange(K), (st.id, "after reset", i))


RESTARTS = [st for st in STAGES if hasattr(st, "restarted") or st.restart_on_clean]


def restarted_run(st, pkg, dev, head, good, tail, rows):
    """head, then st.heal samples of `good` (Denoise: the NaN has to leave the frames first), the restart of `rows`, the
    tail -> the tail's (outputs from st.recovered() on, status), the status' counters as the tail's increments: a restart
    leaves them"""
    obj = st.make(pkg)
    run(st, pkg, dev, head, obj=obj)
    fed = head[0].shape[1] + st.heal
    if st.heal:
        run(st, pkg, dev, tuple(x[:, :st.heal] for x in good), obj=obj)
    base = st.status(obj) if st.counters else ()
    for j in rows:
        st.restart(obj, j)
    outs, status = run(st, pkg, dev, tail, obj=obj)
    obj.close()
    first = st.recovered(fed)
    assert 0 <= first <= tail[0].shape[1] - 100, (st.id, first)
    if st.counters:
        status = tuple(s - b if name in st.counters else s for name, s, b in zip(st.status_names, status, base))
    return tuple(o[:, first:] for o in outs) if first else outs, status


@pytest.mark.parametrize("st", RESTARTS, ids=ids)
def test_c_restart_after_poison(pkg, dev, st):
    """Demod and Carrier: set_rx to another mode; Scope: set_slot to another row; Eq, Denoise, Fsk, Morse, Psk: set_rx
    with the stage's RESTART flag.  After a batch that leaves a NaN in every carried record the restarted receivers have
    the bits of an object created with the new settings at that sample (Scope: of one fed zeros until then, the segment
    grid goes on; the decoders, whose records hold sample indices, and Denoise, whose frame grid goes on: of one fed the
    clean series until then and restarted at the same sample; Denoise restarts behind nfft good samples, as its header
    asks, and is compared from out index q hop + nfft on); with only the poisoned rows 0, 16, 31, 34 restarted, the rows
    that were not touched keep the bits of a run without the restart."""
    xs, _ = clean_run(st, pkg, dev)
    n = st.n(pkg)
    poisoned = all_rows_poisoned(st, xs, n)
    tail = tuple(x[:, :n // 2] for x in xs)
    got = restarted_run(st, pkg, dev, poisoned, xs, tail, range(K))
    if st.restart_on_clean:
        want = restarted_run(st, pkg, dev, xs, xs, tail, range(K))
    else:
        fresh = st.restarted(pkg)
        if isinstance(st, ScopeStage):
            run(st, pkg, dev, tuple(np.zeros_like(x) for x in xs), obj=fresh)
        want = run(st, pkg, dev, tail, obj=fresh)
        fresh.close()
    for i, (g, w) in enumerate(zip(flat(got), flat(want))):
        NF.clean_rows_identical(g, w, np.arange(K), (st.id, "restarted", i))
    # the poisoned rows alone
    some = st.poison(xs, NF.QNAN, [[n - 1]] * 4)
    keep = restarted_run(st, pkg, dev, some, xs, tail, ())
    got2 = restarted_run(st, pkg, dev, some, xs, tail, ROWS)
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

def framed(shape, dtype, dev, pad, spare=2, rows=K):
    """a device buffer [spare + rows + spare, shape[1] + pad, ...] of the never-read pattern -> (the buffer, its host
    copy, the view of the rows in the middle, full width)"""
    import torch
    full = (rows + 2 * spare,) + ((shape[1] + pad,) + tuple(shape[2:]) if len(shape) > 1 else ())      # (a count: [K])
    host = NF.never_read(full, dtype)
    if np.dtype(dtype) == np.complex64:
        buf = torch.view_as_complex(torch.from_numpy(host.view(np.float32).reshape(full + (2,))).to(dev))
    else:
        buf = torch.from_numpy(host).to(dev)
    return buf, host, buf[spare:spare + rows]


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
    turns into a NaN here.  The decoders' chars, counts, sym, nsym and d / p all go into such buffers: of a record buffer
    every cell at or behind counts[j] / nsym[j] keeps its fill too -- lane 0 writes the records as they come -- and the
    counts are written for the K rows alone, in the batch of 0 as well."""
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
    kinds = st.kinds or ("dense",) * len(st.out_dtypes)
    parts, off = [], 0
    for b in cuts:
        due = st.counts(obj, b)
        outs = [framed((K,) if kind == "count" else (K, d) + ((st.nfft,) if isinstance(st, ScopeStage) else st.tails[i] if st.tails else ()),
                       dt, dev, 3 if isinstance(st, ScopeStage) else 11)
                for i, (d, dt, kind) in enumerate(zip(due, st.out_dtypes, kinds))]
        o = st.process(obj, [f[2][:, off:off + b] for f in frames], bufs=[f[2] for f in outs])
        part = collect(st, o, due, (st.id, b))
        for i, (d, kind, (buf, host, view)) in enumerate(zip(due, kinds, outs)):
            after = host_words(buf)
            filled = NF.words(host).copy().reshape(after.shape)
            mask = np.ones(after.shape, bool)
            if kind == "dense":
                mask[2:2 + K, :d] = False
            elif kind == "ragged":                              # the records written, and not a cell at or behind the count
                for j, c in enumerate(part[i + 1]):
                    mask[2 + j, :c] = False
            else:
                mask[2:2 + K] = False
            assert np.array_equal(after[mask], filled[mask]), (st.id, b, i, "an output's surroundings were written")
        parts.append(part)
        off += b
    status = st.status(obj)
    obj.close()
    got = join(st, parts, n), status
    for i, (g, w) in enumerate(zip(flat(got), flat(want))):
        NF.clean_rows_identical(g, w, np.arange(K), (st.id, "surroundings", i))
    for buf, host, _ in frames:
        assert np.array_equal(host_words(buf), NF.words(host).reshape(host_words(buf).shape)), (st.id, "the input buffer changed")


# ---- E. the mixer: rows meet, so isolation is per sample index and per bus ------------------------------------------

MIX_K, MIX_Q, MIX_LB, MIX_R = 37, 2, 48, 4000
MIX_LIMITS = [None, (MIX_LB, MR.CEIL, MR.REL)]
mix_ids = lambda v: "plain" if v is None else f"Lb{v[0]}" if isinstance(v, tuple) else str(v)


def mixer_case(pkg):
    """n = 8 Lb + 3 TT + 5 samples of the mixer tests' series for K = 37, the interleaved gains (every third receiver
    silent), and set_rx calls ahead of the first batch whose ramps (R = 4000) no batch here completes -> (n, a, gains,
    changes, the gains once every change is taken: what reset() leaves)"""
    n = 8 * MIX_LB + 3 * pkg.mixer_tile_outputs() + 5
    g = MR.interleaved_gains(MIX_K, MIX_Q)
    ch = MR.one_shot_changes(MIX_K, MIX_Q, g)
    after = g.copy()
    for j, gg in ch:
        after[j] = gg
    return n, QR.audio_series(MIX_K, n, MR.SERIES_SEED), g, ch, after


def mixer_run(pkg, dev, a, gains, limit, cuts=None, obj=None, changes=()):
    """all of a through `obj` (default: a fresh Mixer with `changes` set ahead, closed afterwards) -> (f32 [Q, count],
    i16 [count, Q], (peak, gain, min_gain))"""
    import torch
    own = obj is None
    if own:
        obj = pkg.Mixer(gains, MIX_R, limit=limit)
        for j, gg in changes:
            obj.set_rx(j, gg)
    ad = upload((a,), dev)[0]
    fs, ps, off = [], [], 0
    for b in cuts or [a.shape[1]]:
        due = obj.next_outputs(b)
        f, p = obj.process(ad[:, off:off + b], f32=True, i16=True)
        assert f.shape == (MIX_Q, due) and p.shape == (due, MIX_Q)
        fs.append(f)
        ps.append(p)
        off += b
    assert off == a.shape[1]
    st = obj.read()
    if own:
        obj.close()
    return torch.cat(fs, dim=1).cpu().numpy(), torch.cat(ps, dim=0).cpu().numpy(), tuple(st[name].copy() for name in MR.STATUS.names)


def mixer_ref(pkg, a, gains, limit, changes=(), cuts=None):
    """-> (the same triple from mixer_ref.MixerRef, the MixerRef)"""
    ref = MR.MixerRef(gains, MIX_R, limit, chunk=pkg.mixer_chunk())
    for j, gg in changes:
        ref.set_rx(j, gg)
    f, p = MR.run_cuts(ref, a, cuts or [a.shape[1]])
    st = ref.read()
    return (f, p, tuple(st[name].copy() for name in MR.STATUS.names)), ref


def mixer_columns(pkg, n):
    TT = pkg.mixer_tile_outputs()
    return NF.placements(TT, MIX_LB, n), NF.cuts_for(TT, n)


def mixer_same(got, want, what):
    for i, (g, w) in enumerate(zip(got[:2] + got[2], want[:2] + want[2])):
        NF.same_or_both_nan(g, w, (what, i))


@pytest.mark.parametrize("value", list(NF.POISON))
@pytest.mark.parametrize("limit", MIX_LIMITS, ids=mix_ids)
def test_e_mixer_isolation_and_the_limiter(pkg, dev, limit, value):
    """One active receiver (every gain of it non-zero) poisoned at each standard column in turn -- 0, Lb - 1, TT - 1, TT,
    2 TT + 3, n - 1 --, in one batch and in the cuts of cuts_for; ramps are under way throughout.  Every output and the
    status have the reference's bits (NaN where it has NaN).  Without the limiter only that index of the buses differs
    from the clean run, and it is not finite.  With the limiter a NaN changes no gain and leaves as -ceil; an infinity in
    block k makes E = 0 for the blocks k - 1 and k ("m is Inf for the blocks k - 1 and k, so t = 0 and E = 0 there"),
    the sample leaves as -ceil (in block 0, which ramps down from E[-1] = 1, as +-ceil by its sign), E is in (0, rel] for block k + 1 and no smaller in block k + 2 unless the block's own
    peak asks for less ("From block k + 1 on E recovers by rel per block"), min_gain is 0, |out| <= ceil everywhere and
    no output is NaN ("Nothing sticks").  The reference shows each of these (asserted) before the device is compared."""
    n, a, g, ch, _ = mixer_case(pkg)
    cols, cuts = mixer_columns(pkg, n)
    j = next(j for j in range(MIX_K) if g[j].all() and not any(c[0] == j for c in ch))
    clean, _ = mixer_ref(pkg, a, g, limit, ch)
    y = np.abs(clean[0] if limit is None else mixer_ref(pkg, a, g, None, ch)[0][0])
    Lb, ceil, rel = MIX_LB, np.float32(MR.CEIL), np.float32(MR.REL)
    for col in cols:
        x = NF.plant(a, [j], [col], NF.POISON[value])
        want, ref = mixer_ref(pkg, x, g, limit, ch)
        count = want[0].shape[1]
        diff = np.flatnonzero((NF.words(want[0]) != NF.words(clean[0])).any(axis=0))
        if limit is None:
            assert diff.tolist() == [col] and not np.isfinite(want[0][:, col]).any(), (value, col, diff)
        else:
            assert np.isfinite(want[0]).all() and (np.abs(want[0]) <= ceil).all()
            if col < count and value != "nan" and col < Lb - 1:
                # block 0 ramps down from E[-1] = 1: g > 0 at every sample but its last, so the infinity is clamped
                assert (np.abs(want[0][:, col]) == ceil).all(), (value, col)
            elif col < count:
                assert (want[0][:, col] == -ceil).all(), (value, col)
            E, k = np.array(ref.lim.gains), col // Lb                          # [blocks written, Q]
            zero = [b for b in (k - 1, k) if 0 <= b < len(E)]
            if value == "nan" or not zero:
                # a NaN changes no block peak (unless the sample it replaces was one), an infinity in a block that no
                # written block looks at changes no gain yet: the poisoned index alone differs, if it was written
                if not (y[:, col] == y[:, k * Lb:(k + 1) * Lb].max(axis=1)).any():
                    assert diff.tolist() == ([col] if col < count else []), (value, col, diff)
                    assert all(np.array_equal(NF.words(w), NF.words(c)) for w, c in zip(want[2][1:], clean[2][1:]))
            else:
                assert not E[zero].any(), (value, col, E[zero])
                assert (want[2][2] == 0).all() and np.array_equal(want[2][1], E[-1])
                if k + 1 < len(E):
                    assert (E[k + 1] > 0).all() and (E[k + 1] <= rel).all(), (value, col, E[k + 1])
                if k + 2 < len(E):
                    step = MR.fma(rel, np.float32(1) - E[k + 1], E[k + 1])
                    assert ((E[k + 2] == step) | ((E[k + 2] < step) & (E[k + 2] > 0))).all() and (step > E[k + 1]).all()
        for cut in (None, cuts):
            mixer_same(mixer_run(pkg, dev, x, g, limit, cut, changes=ch), want, ("mixer", mix_ids(limit), value, col, cut))


def mixer_bad_batch(n, a, g, ch):
    """a with a NaN in the last sample of every row and +inf in an active receiver in the last block the limiter writes
    (n div Lb - 2): behind it the held block holds the NaN, the latest E and min_gain are 0 and the peak is inf"""
    j = next(j for j in range(MIX_K) if g[j].all() and not any(c[0] == j for c in ch))
    return NF.plant(NF.plant(a, np.arange(MIX_K), [n - 1], NF.QNAN), [j], [(n // MIX_LB - 2) * MIX_LB + 5], np.float32(np.inf))


@pytest.mark.parametrize("limit", MIX_LIMITS, ids=mix_ids)
def test_e_mixer_reset_after_poison(pkg, dev, limit):
    """A batch with a NaN in the last sample of every row and an infinity two blocks earlier, the ramps of the set_rx
    calls ahead of it not yet over: the held block (with the limiter) holds the NaN, E and min_gain are 0, the peak is
    inf and the ramps are under way.  reset(), the clean series: outputs and read() have the bits of a freshly created
    object's with the gains reset() leaves, which are the reference's."""
    n, a, g, ch, after = mixer_case(pkg)
    bad = mixer_bad_batch(n, a, g, ch)
    obj = pkg.Mixer(g, MIX_R, limit=limit)
    for j, gg in ch:
        obj.set_rx(j, gg)
    first = mixer_run(pkg, dev, bad, g, limit, obj=obj)
    assert np.isnan(first[0][:, -1]).all() if limit is None else first[0].shape[1] == MIX_LB * (n // MIX_LB - 1)
    assert np.isposinf(first[2][0]).all() and (limit is None or (not first[2][1].any() and not first[2][2].any())), first[2]
    obj.reset()
    got = mixer_run(pkg, dev, a, g, limit, obj=obj)
    obj.close()
    fresh = mixer_run(pkg, dev, a, after, limit)
    want, _ = mixer_ref(pkg, a, after, limit)
    for i, (v, f, w) in enumerate(zip(got[:2] + got[2], fresh[:2] + fresh[2], want[:2] + want[2])):
        assert np.isfinite(f.astype(np.float64)).all() and np.array_equal(NF.words(v), NF.words(f)), ("mixer", mix_ids(limit), "after reset", i)
        assert np.array_equal(NF.words(f), NF.words(w)), ("mixer", mix_ids(limit), "fresh against the reference", i)


@pytest.mark.parametrize("limit", MIX_LIMITS, ids=mix_ids)
def test_e_mixer_poisoned_surroundings(pkg, dev, limit):
    """Clean data, poison everywhere else.  a is a view of a buffer with row stride n + 37 and two spare rows above and
    below, padding and spare rows filled with 0xFFFFFFFF / 0x7FC00000; a silent receiver's row holds nothing but that
    pattern ("it is not read").  f32 goes planar into a buffer of that pattern with row stride count + 11 and spare
    rows, i16 interleaved into the middle of one with three spare frames in front and eight behind.  Batches of 0, 1, 2,
    Lb - 1, Lb, TT - 1, TT, TT + 1 and the rest in one object: several complete no block and write nothing.  Outputs and
    status have the bits of the contiguous run in one batch; every cell outside the counts keeps its fill; the input
    buffer is intact."""
    import torch
    n, a, g, ch, _ = mixer_case(pkg)
    TT, Lb = pkg.mixer_tile_outputs(), MIX_LB
    cuts = [0, 1, 2, Lb - 1, Lb, TT - 1, TT, TT + 1]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    silent = next(j for j in range(MIX_K) if not g[j].any() and not any(c[0] == j for c in ch))
    want = mixer_run(pkg, dev, a, g, limit, changes=ch)
    x = a.copy()
    x[silent] = NF.never_read((n,), np.float32)
    buf, host, view = framed(x.shape, x.dtype, dev, 37, rows=MIX_K)
    view[:, :n] = upload((x,), dev)[0]
    host[2:2 + MIX_K, :n] = x
    obj = pkg.Mixer(g, MIX_R, limit=limit)
    for j, gg in ch:
        obj.set_rx(j, gg)
    fs, ps, off = [], [], 0
    for b in cuts:
        due = obj.next_outputs(b)
        fbuf, fhost, fview = framed((MIX_Q, due), np.float32, dev, 11, rows=MIX_Q)
        ihost = NF.never_read((3 + due + 8, MIX_Q), np.int16)
        ibuf = torch.from_numpy(ihost.copy()).to(dev)
        f, p = obj.process(view[:, off:off + b], out_f32=fview, out_i16=ibuf[3:])
        assert f.shape == (MIX_Q, due) and p.shape == (due, MIX_Q)
        fs.append(f.cpu().numpy())
        ps.append(p.cpu().numpy())
        mask = np.ones(fhost.shape, bool)
        mask[2:2 + MIX_Q, :due] = False
        assert np.array_equal(host_words(fbuf)[mask], NF.words(fhost)[mask]), ("mixer", b, "f32's surroundings were written")
        mask = np.ones(ihost.shape, bool)
        mask[3:3 + due] = False
        assert np.array_equal(ibuf.cpu().numpy()[mask], ihost[mask]), ("mixer", b, "i16's surroundings were written")
        off += b
    st = obj.read()
    obj.close()
    got = (np.concatenate(fs, axis=1), np.concatenate(ps, axis=0), tuple(st[name].copy() for name in MR.STATUS.names))
    for i, (v, w) in enumerate(zip(got[:2] + got[2], want[:2] + want[2])):
        assert np.isfinite(w.astype(np.float64)).all() and np.array_equal(NF.words(v), NF.words(w)), ("mixer", mix_ids(limit), "surroundings", i)
    assert np.array_equal(host_words(buf), NF.words(host)), ("mixer", "the input buffer changed")
