"""What tests/test_gpu_stream_order.py shares: the harness that keeps a side stream busy behind a gate, the canary
buffers, and one adapter per stream object (OBJECTS) with its settings, input series, batch sizes, parameter changes and
double reference.  A plain module: no fixtures.  Nothing here asserts on the code under test except reference(), which
compares a run with the object's own reference at the tolerance that reference's file already carries.

The harness in four pieces (the test module's header says what each one is for):
  Buf       an output tensor over a byte buffer filled with CANARY, allocated up front on the null stream
  side_streams  the side streams: torch streams that were tried and do not share the null stream's hardware queue
  occupy    the filler: ordinary elementwise kernels on the side stream that finish by themselves, as many as fill
            the asked milliseconds (their duration is measured once per session with events)
  scrambled the series the object's input tensor holds until the real one is copied over it behind the gate
  Runner    walks a list of steps -- ("batch", size), ("change", k), ("tail",), ("reset",) -- through an object on a
            given stream with explicit out= tensors; with sync_each it is the clean run (null stream, a device
            synchronise after every call)
"""
import math
import types

import numpy as np

import adapt_ref as AR
import audio_ref as UR
import blanker_ref as BR
import carrier_ref as CR
import channelizer_ref as HR
import demod_ref as DR
import rxfilter_ref as RR
import scope_ref as SR
import spectrum_ref as PR
import squelch_ref as QR
import tuner_ref as TR

CANARY = 0xA5
K = 37                                  # 2 x 16 + 5: a partial last group for blocks of 4 and of 16 receivers
FIR_TOL = 1e-6                          # the pipeline's, as in tests/test_gpu_parity.py and the other pipeline tests
SPECTRUM_TOL = 1e-5                     # tests/test_gpu_spectrum.py's TOL
FREG = 381178347
TILE = 8192                             # samples per tile of k_fir_i8x


# ---- buffers and comparisons ----------------------------------------------------------------------------------------

class Buf:
    """An output tensor `t` of `shape` and torch dtype `dtype` over `raw`, bytes filled with CANARY."""

    def __init__(self, shape, dtype, dev):
        import torch
        self.shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(self.shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((nbytes,), CANARY, dtype=torch.uint8, device=dev)
        self.t = self.raw.view(dtype).view(self.shape)

    def untouched(self):
        """downloads on the current stream; every byte is still the canary"""
        return bool((self.raw.cpu() == CANARY).all())


def host(t):
    """a device view -> numpy (complex64 stays complex64)"""
    return t.contiguous().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def assert_same(got, want, what):
    """two results of Runner.go (lists over steps of lists over outputs, numpy) by their bytes"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, i)
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.size or not b.size, (what, i, j, "empty")
            assert same_bits(a, b), (what, f"step {i} output {j}", a.shape, b.shape)


def upload(xs, dev):
    import torch
    return [torch.from_numpy(np.array(x, copy=True, order="C")).to(dev) for x in xs]


def scrambled(ad, xs, keep):
    """xs with everything behind the first `keep` time units reversed in time: other finite, valid values of the same
    kind, so a launch that reads them computes something else and faults nothing"""
    out = []
    for x in xs:
        y = np.array(x, copy=True)
        if ad.axis == 1:
            y[:, keep:] = x[:, keep:][:, ::-1]
        else:
            y[keep * ad.unit:] = x[keep * ad.unit:][::-1]
        out.append(y)
    return out


# ---- the filler -----------------------------------------------------------------------------------------------------

_FILL = {}


def _filler(dev):
    """(a 256 MiB tensor, the milliseconds one in-place add on it takes), measured once with events"""
    import torch
    if "x" not in _FILL:
        x = torch.zeros(1 << 26, dtype=torch.float32, device=dev)
        for _ in range(3):
            x.add_(1.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            x.add_(1.0)
        e1.record()
        torch.cuda.synchronize()
        _FILL["x"], _FILL["ms"] = x, max(e0.elapsed_time(e1) / 20.0, 1e-3)
    return _FILL["x"], _FILL["ms"]


_SIDE = []


def side_streams(dev, n=1):
    """n of torch's streams whose work does not hold up the null stream, the same ones every time.  A torch.cuda.Stream
    does not synchronise with the null stream, but the runtime puts its streams onto a few hardware queues (four unless
    GPU_MAX_HW_QUEUES says otherwise), and a stream that got the null stream's queue keeps a download on the null stream
    waiting behind its own kernels: the queue's doing, not the library's (measured: 2 of the first 12 pool streams,
    NOTEBOOK.md).  Those are found by trying -- 10 ms of filler, a small download, was the gate still closed -- and left
    out."""
    import torch
    if not _SIDE:
        tiny = torch.zeros(1024, device=dev)
        _filler(dev)
        torch.cuda.synchronize()
        for _ in range(16):
            s = torch.cuda.Stream(device=dev)
            gate = occupy(s, dev, 10.0)
            tiny.cpu()
            free = not gate.query()
            s.synchronize()
            if free:
                _SIDE.append(s)
            if len(_SIDE) == 2:
                break
    assert len(_SIDE) >= n, "no stream that leaves the null stream alone"
    return _SIDE[:n]


def occupy(side, dev, ms):
    """`ms` milliseconds (at most 1000) of elementwise kernels on `side`, then the gate: an event recorded behind them.
    Call _filler(dev) before the test's allocations are synchronised, so that nothing is allocated here."""
    import torch
    assert 0 < ms <= 1000.0
    x, per = _filler(dev)
    with torch.cuda.stream(side):
        for _ in range(max(1, math.ceil(ms / per))):
            x.add_(1.0)
    gate = torch.cuda.Event()
    gate.record(side)
    return gate


# ---- steps ----------------------------------------------------------------------------------------------------------

class Plan:
    """the sizes of an object's outputs step by step, from host arithmetic alone: `before` counts the time units taken"""

    def __init__(self):
        self.before = 0


def allocate(ad, env, steps):
    """one list of Buf per step (None where a step writes nothing), all allocated here"""
    plan = ad.plan()
    bufs = []
    for s in steps:
        if s[0] == "batch":
            bufs.append([Buf(sh, dt, env.dev) for sh, dt in ad.out_specs(env, plan, s[1])])
            plan.before += s[1]
        elif s[0] == "tail":
            bufs.append([Buf(sh, dt, env.dev) for sh, dt in ad.tail_specs(env, plan)])
        else:
            if s[0] == "change":
                ad.plan_change(plan, s[1])
            elif s[0] == "reset":
                plan.before = 0
            bufs.append(None)
    return bufs


class Runner:
    def __init__(self, ad, env, obj, xs, st, sync_each=False):
        self.ad, self.env, self.obj, self.xs, self.st, self.sync_each, self.off = ad, env, obj, xs, st, sync_each, 0

    def take(self, b):
        ad = self.ad
        if ad.axis == 1:
            return [x[:, self.off:self.off + b] for x in self.xs]
        return [x[self.off * ad.unit:(self.off + b) * ad.unit] for x in self.xs]

    def go(self, steps, bufs):
        """-> the views of what the batch and tail steps wrote, in order; nothing is downloaded here"""
        import torch
        views = []
        for s, bf in zip(steps, bufs):
            if s[0] == "batch":
                views.append(self.ad.process(self.env, self.obj, self.take(s[1]), bf, self.st))
                self.off += s[1]
            elif s[0] == "tail":
                views.append(self.ad.tail(self.env, self.obj, bf, self.st))
            elif s[0] == "change":
                self.ad.change(self.obj, s[1])
            elif s[0] == "reset":
                self.obj.reset()
                self.off = 0
            if self.sync_each:
                torch.cuda.synchronize()
        return views


def batches(sizes):
    return [("batch", int(b)) for b in sizes]


def cat(parts, i, axis):
    return np.concatenate([p[i] for p in parts], axis=axis)


def rows_of(k, nrx):
    """the receivers change k touches: 0, 5, 16, last | 5, 16, 17, 31 | 0, 20, last (those below nrx)"""
    sets = ((0, 5, 16, nrx - 1), (5, 16, 17, 31), (0, 20, nrx - 1))
    return sorted({j for j in sets[k % 3] if 0 <= j < nrx})


def uniform_complex(nrx, n, seed):
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, (nrx, n, 2)).astype(np.float32)
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]


def normal_complex(nrx, n, seed):
    w = np.random.default_rng(seed).standard_normal((nrx, n, 2), dtype=np.float32)
    return np.ascontiguousarray(w).view(np.complex64)[..., 0]


# ---- the objects ----------------------------------------------------------------------------------------------------

class Obj:
    """One object type at one setting.  Time runs along `axis` of every input, `unit` items per time unit (6 bytes per
    packed sample).  sizes() -> (the two warm-up batches, the batches of case A); out_specs / tail_specs say what a step
    writes; process / tail issue it on stream `st` into the given Bufs and return the views that hold the results; read
    is the object's own blocking read(); reference asserts on a clean run of case A."""
    axis, unit, nrx = 1, 1, K
    tile = None                       # the package's tile getter

    def plan(self):
        return Plan()

    def TT(self, env):
        return int(getattr(env.pkg, self.tile)())

    def sizes(self, env):
        TT = self.TT(env)
        return [TT + 3, 7], [TT - 1, 1, 2 * TT + 5]

    def b_steps(self, env):
        """case B: a change in front of each of the three batches"""
        main = self.sizes(env)[1]
        return [s for k, b in enumerate(main) for s in (("change", k), ("batch", b))]

    def tail_specs(self, env, plan):
        return []

    def tail(self, env, obj, bufs, st):
        return []

    def plan_change(self, plan, k):
        pass

    def change(self, obj, k):
        pass

    def read(self, obj, st):
        return ()


class BlankerObj(Obj):
    id, tile, par = "blanker", "blanker_tile_outputs", (48, 3, 5)

    def __init__(self):
        self.rx = BR.interleaved_rx(self.nrx)

    def inputs(self, env, n):
        return (BR.impulse_series(self.nrx, n, 21),)

    def make(self, env):
        B, W, R = self.par
        return env.pkg.Blanker(self.rx, B, W, R, beta=BR.BETA, cap=BR.CAP)

    def out_specs(self, env, plan, b):
        import torch
        return [((self.nrx, b), torch.complex64)]

    def process(self, env, obj, xs, bufs, st):
        return [obj.process(xs[0], out=bufs[0].t, stream=st)]

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, BR.THRESHOLDS[(j + k + 1) % 6], BR.ON if (j + k) % 2 else 0)

    def read(self, obj, st):
        return (obj.read(stream=st),)

    def reference(self, env, xs, parts, reads):
        r = BR.BlankerRef(self.rx, **BR.params(*self.par))
        want = r.process(xs[0])
        assert same_bits(cat(parts, 0, 1), want), "blanker: out against the reference's bits"
        st = r.read()
        for name in BR.STATUS.names:
            assert np.array_equal(reads[0][name], st[name].astype(reads[0][name].dtype)), ("blanker status", name)


class RxFilterObj(Obj):
    id, tile, B, T = "rxfilter", "rxfilter_tile_outputs", 4, 64

    def __init__(self):
        self.bank, self.sel = RR.parity_bank(self.B, self.T), RR.select(self.nrx, self.B)

    def inputs(self, env, n):
        return (uniform_complex(self.nrx, n, 1064),)         # re, im uniform in [-1, 1]: what TOL_RXFILTER was measured on

    def make(self, env):
        return env.pkg.RxFilter(self.bank, self.sel)

    out_specs = BlankerObj.out_specs
    process = BlankerObj.process

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, (self.sel[j] + k + 1) % self.B)

    def reference(self, env, xs, parts, reads):
        assert (self.B, self.T) in RR.SHAPES and float(np.max(np.abs(xs[0].view(np.float32)))) <= 1.0
        ref = RR.rxfilter_ref(xs[0], self.bank, self.sel)
        e = float(np.max(np.abs(cat(parts, 0, 1).astype(np.complex128) - ref)))
        print(f"stream order, rxfilter: err {e:.2e} (TOL_RXFILTER {RR.TOL_RXFILTER:.2e})")
        assert e <= RR.TOL_RXFILTER


class CarrierObj(Obj):
    tile, L = "carrier_tile_outputs", 31

    def __init__(self, nrx=K):
        self.nrx, self.id = nrx, "carrier" if nrx == K else f"carrier-k{nrx}"
        self.rx = CR.interleaved_rx(nrx + 1)[1:]             # receiver 0 has a loop (DSB), also when it is the only one

    def inputs(self, env, n):
        return (CR.am_carriers(self.nrx, n)[0],)

    def make(self, env):
        return env.pkg.Carrier(self.rx, CR.hilbert(self.L), **CR.PARAMS)

    out_specs = BlankerObj.out_specs
    process = BlankerObj.process

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, (self.rx[j][0] + k + 1) % 4, *CR.loop_gains(CR.BANDWIDTHS[(j + k) % 3]))

    read = BlankerObj.read

    def reference(self, env, xs, parts, reads):
        ref = CR.CarrierRef(self.rx, CR.hilbert(self.L), **CR.PARAMS)
        want = ref.process(xs[0])
        assert np.abs(ref.e).max() < CR.E_MAX                 # the reference's own precondition (test_carrier_cpu.py)
        u, st, rd = cat(parts, 0, 1), reads[0], ref.read()
        modes = np.array([r[0] for r in self.rx])
        for m in CR.MODES:
            rows = np.flatnonzero(modes == m)
            if not rows.size:
                continue
            tol = CR.TOL_CARRIER[m]
            if m == CR.OFF:
                assert same_bits(u[rows], xs[0][rows]), "carrier: OFF passes z"
            e = float(CR.err_rows(u[rows], want[rows]).max())
            print(f"stream order, {self.id} {CR.MODE_NAMES[m]}: err {e:.2e} (TOL_CARRIER {tol:.2e})")
            assert e <= tol, (m, e)
            dth = int(np.abs(CR.theta_diff(st["theta"][rows], rd["theta"][rows])).max())
            assert dth <= tol / (2.0 * np.pi) * 2.0 ** 32, (m, dth)
            turn = tol / np.pi
            assert float(np.abs(st["freq"][rows].astype(np.float64) - ref.v[rows]).max()) <= turn
            assert float(np.abs(st["err"][rows].astype(np.float64) - ref.q[rows]).max()) <= turn


class DemodObj(Obj):
    id, tile = "demod", "demod_tile_outputs"

    def __init__(self):
        self.rx = DR.interleaved_rx(self.nrx)

    def inputs(self, env, n):
        return (normal_complex(self.nrx, n, 99),)             # unit normal parts, as tests/test_gpu_demod.py's random_series

    def make(self, env):
        return env.pkg.Demod(self.rx, **DR.PARAMS)

    def out_specs(self, env, plan, b):
        import torch
        return [((self.nrx, b), torch.float32)]

    process = BlankerObj.process

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, (self.rx[j][0] + k + 1) % 3, 0x01234567 * (k + 1), DR.FLAG_SETS[(j + k) % 4])

    def reference(self, env, xs, parts, reads):
        ref = DR.demod_ref(xs[0], self.rx, **DR.PARAMS)
        for m, e in DR.err_by_mode(cat(parts, 0, 1), ref, self.rx).items():
            print(f"stream order, demod {DR.MODE_NAMES[m]}: err {e:.2e} (TOL_DEMOD {DR.TOL_DEMOD[m]:.2e})")
            assert e <= DR.TOL_DEMOD[m], (m, e)


class AdaptObj(Obj):
    id, tile, T, D = "adapt", "adapt_tile_outputs", 32, 7

    def __init__(self):
        assert (self.T, self.D) in AR.GPU_SETS
        self.rx = AR.interleaved_rx(self.nrx)

    def inputs(self, env, n):
        x = AR.gpu_series()                                   # (its preconditions: tests/test_adapt_cpu.py)
        assert n <= x.shape[1]
        return (np.ascontiguousarray(x[:self.nrx, :n]),)

    def make(self, env):
        return env.pkg.Adapt(self.rx, self.T, self.D, eps=AR.EPS)

    out_specs = DemodObj.out_specs
    process = BlankerObj.process

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, AR.MODES[(j + k + 1) % 3], AR.MUS[(j + k) % 5], AR.LEAKS[(j + k) % 4], AR.RESTART if k == 1 else 0)

    def read(self, obj, st):
        return (obj.read_weights(stream=st),)

    def reference(self, env, xs, parts, reads):
        r = AR.AdaptRef(self.rx, self.T, self.D)
        want = r.process(xs[0])
        assert same_bits(cat(parts, 0, 1), want), "adapt: out against the reference's bits"
        assert same_bits(reads[0], r.weights), "adapt: weights against the reference's bits"


class SquelchObj(Obj):
    id, tile, par = "squelch", "squelch_tile_outputs", (48, 2, 3, 37)

    def __init__(self):
        self.rx = QR.interleaved_rx(self.nrx)
        self.other = QR.interleaved_rx(self.nrx + 8)

    def inputs(self, env, n):
        return QR.keyed_series(self.nrx, n, 11), QR.audio_series(self.nrx, n, 12)

    def make(self, env):
        B, attack, hang, R = self.par
        return env.pkg.Squelch(self.rx, B, attack, hang, R, up=QR.UP)

    def out_specs(self, env, plan, b):
        import torch
        nb = env.pkg.squelch_blocks(self.par[0], plan.before, b)
        return [((self.nrx, b), torch.float32), ((self.nrx, nb), torch.float32), ((self.nrx, nb), torch.uint8)]

    def process(self, env, obj, xs, bufs, st):
        return list(obj.process(xs[0], xs[1], out=bufs[0].t, levels=bufs[1].t, states=bufs[2].t, stream=st))

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_rx(j, *self.other[j + k + 1])

    def read(self, obj, st):
        return (obj.read(stream=st),)

    def reference(self, env, xs, parts, reads):
        r = QR.SquelchRef(self.rx, **QR.params(*self.par))
        want = r.process(xs[0], xs[1])
        for i in range(3):
            assert same_bits(cat(parts, i, 1), want[i]), ("squelch against the reference's bits", i)
        st = r.read()
        for name in QR.STATUS.names:
            assert same_bits(reads[0][name], st[name].astype(reads[0][name].dtype)), ("squelch status", name)


class AudioObj(Obj):
    """k_audio's tile is 256 OUTPUTS (tests/test_gpu_audio.py; there is no getter): the batches are the inputs that give
    at most 255 outputs, one input, and the inputs that give at least 2 x 256 + 5 outputs.  Audio has no set_rx: case B
    runs without changes."""
    id, L, M, P, T = "audio", 3072, 625, 128, 32

    def __init__(self):
        assert (self.L, self.M) in UR.RATIOS and (self.P, self.T) in UR.SHAPES
        self.g = UR.parity_prototype(self.L, self.M, self.P, self.T)

    def sizes(self, env):
        warm, before = [61, 7], 68
        b1 = max(n for n in range(1, 256) if UR.outputs(self.L, self.M, before, n) <= 255)
        b3 = min(n for n in range(1, 600) if UR.outputs(self.L, self.M, before + b1 + 1, n) >= 2 * 256 + 5)
        return warm, [b1, 1, b3]

    def inputs(self, env, n):
        return (np.random.default_rng(2032).uniform(-1.0, 1.0, (self.nrx, n)).astype(np.float32),)

    def make(self, env):
        return env.pkg.Audio(self.nrx, self.L, self.M, self.P, self.T, self.g)

    def out_specs(self, env, plan, b):
        import torch
        n = env.pkg.audio_outputs(self.L, self.M, plan.before, b)
        return [((self.nrx, n), torch.float32), ((self.nrx, n), torch.int16)]

    def process(self, env, obj, xs, bufs, st):
        return list(obj.process(xs[0], out_f32=bufs[0].t, out_i16=bufs[1].t, stream=st))

    def reference(self, env, xs, parts, reads):
        assert float(np.max(np.abs(xs[0]))) <= 1.0
        ref = UR.audio_ref(xs[0], self.L, self.M, self.P, self.T, self.g)
        out = cat(parts, 0, 1)
        assert out.shape == ref.shape
        e = float(np.max(np.abs(out.astype(np.float64) - ref)))
        print(f"stream order, audio: err {e:.2e} (TOL_AUDIO {UR.TOL_AUDIO:.2e})")
        assert e <= UR.TOL_AUDIO


class ScopeObj(Obj):
    """The kernel's blocks take scope_block_items(nfft) (slot, line) items side by side: the batches complete items - 1
    lines per slot, none (one sample), and 2 items + 5."""
    id, nfft, hop, avg, nsrc = "scope", 256, 128, 1, K

    def __init__(self):
        self.rows = [int(r) for r in SR.slot_rows(self.nrx, self.nsrc)]
        self.window = SR.hann(self.nfft)

    def sizes(self, env):
        items = int(env.pkg.scope_block_items(self.nfft))
        return [self.nfft + 2 * self.hop + 3, 7], [self.hop * (items - 1), 1, self.hop * (2 * items + 5)]

    def inputs(self, env, n):
        """scope_ref.gpu_series' recipe at this length: noise of sigma 0.1 per part, a tone of 0.7 and one 80 dB below"""
        rng = np.random.default_rng(77 + self.nfft + self.hop)
        z = 0.1 * (rng.standard_normal((self.nsrc, n)) + 1j * rng.standard_normal((self.nsrc, n)))
        t, r = np.arange(n), np.arange(self.nsrc)[:, None]
        z += 0.7 * np.exp(2j * np.pi * (((5 + 3 * r) % self.nfft + 0.3) / self.nfft) * t)
        z += 0.7e-4 * np.exp(-2j * np.pi * (((11 + 5 * r) % self.nfft + 0.45) / self.nfft) * t)
        return (z.astype(np.complex64),)

    def make(self, env):
        return env.pkg.Scope(self.nsrc, self.rows, self.nfft, self.hop, self.avg, self.window)

    def out_specs(self, env, plan, b):
        import torch
        return [((self.nrx, env.pkg.scope_lines(self.nfft, self.hop, self.avg, plan.before, b), self.nfft), torch.float32)]

    process = BlankerObj.process

    def change(self, obj, k):
        for j in rows_of(k, self.nrx):
            obj.set_slot(j, -1 if (j + k) % 5 == 0 else (self.rows[j] + k + 1) % self.nsrc)

    def reference(self, env, xs, parts, reads):
        want = SR.slot_lines(SR.scope_ref(xs[0], self.nfft, self.hop, self.avg, self.window), self.rows)
        got = cat(parts, 0, 1)
        assert got.shape == want.shape
        e = SR.err(got, want)
        print(f"stream order, scope: err {e:.2e} (TOL_SCOPE {SR.TOL_SCOPE:.1e})")
        assert e <= SR.TOL_SCOPE
        off = [j for j, r in enumerate(self.rows) if r < 0]
        assert off and not got[off].any()


class TunerObj(Obj):
    """Fed rows of its own (Gaussian, tuner_ref.gaussian_rows) on the range of 64 channels from `first`: (T, R) = (130, 7),
    one of tuner_ref.CASES_TR_SHAPES, in batches that all leave carried rows.  Change 1 also switches to list mode with a
    permuted list of the same channels (the rows are then read in that order)."""
    id, axis, nchan, hop, first, count, T, decim = "tuner", 0, 1024, 512, 0, 64, 130, 7

    def __init__(self):
        assert (self.T, self.decim) in TR.CASES_TR_SHAPES
        self.words = TR.receiver_set_in(self.nchan, self.first, self.count, self.nrx)
        self.unit = self.count

    def sizes(self, env):
        return [200, 13], [7 * 9 + 3, 1, 7 * 30 + 5]

    def inputs(self, env, n):
        return (np.ascontiguousarray(TR.gaussian_rows(n, self.count)).reshape(-1),)

    def make(self, env):
        g = types.SimpleNamespace(nchan=self.nchan, hop=self.hop, device=0, first=self.first, count=self.count)
        self.h = env.pkg.tuner_lowpass(self.T, self.decim)
        return env.pkg.Tuner(g, self.words, self.h, self.decim)

    def out_specs(self, env, plan, b):
        import torch
        return [((self.nrx, env.pkg.tuner_outputs(self.T, self.decim, plan.before, b)), torch.complex64)]

    def process(self, env, obj, xs, bufs, st):
        return [obj.process(xs[0], nrows=xs[0].numel() // self.count, out=bufs[0].t, stream=st)]

    def change(self, obj, k):
        if k == 1:
            obj.set_channels([(self.first + (5 * i + 3) % self.count) % self.nchan for i in range(self.count)])
        other = TR.receiver_set_in(self.nchan, self.first, self.count, self.nrx, seed=2025 + k)
        for j in rows_of(k, self.nrx):
            obj.set_freq(j, other[j])

    def reference(self, env, xs, parts, reads):
        rows = xs[0].reshape(-1, self.count)
        ref = TR.tuner_ref_range(rows, self.nchan, self.hop, self.first, self.words, self.h, self.decim)
        out = cat(parts, 0, 1)
        assert out.shape == ref.shape
        e = TR.err(out, ref)
        print(f"stream order, tuner: err {e:.2e} (TOL_TUNER_SHAPES {TR.TOL_TUNER_SHAPES:.2e})")
        assert e <= TR.TOL_TUNER_SHAPES


class PackedObj(Obj):
    """an object that reads the packed ADC stream: bytes, 6 per sample, batches of multiples of 8 samples"""
    axis, unit, seed = 0, 6, 4242

    def inputs(self, env, n):
        return (env.O.lcg_bytes(6 * n, self.seed),)


class ChannelizerObj(PackedObj):
    """M = 1024, hop 512, 4 taps per branch, all channels (the metric of channelizer_ref.TOL is over all of them); the
    changes are set_channels with lists of other lengths and orders (list mode)."""
    id, nchan, hop, first, count = "channelizer", 1024, 512, 0, 1024
    LISTS = ([100 + 2 * i for i in range(40)], [7, 1023, 0, 512, 100, 101, 102, 640, 3], [900 - 3 * i for i in range(37)])

    def plan(self):
        p = Plan()
        p.count = self.count
        return p

    def sizes(self, env):
        return [8192, 4104], [512 * 5 + 8, 8, 512 * 11 + 16]

    def make(self, env):
        self.proto = env.pkg.tuner_prototype(self.nchan, 4)
        return env.pkg.Channelizer(self.nchan, self.proto, self.hop, self.first, self.count)

    def out_specs(self, env, plan, b):
        import torch
        return [((env.pkg.channelizer_rows(self.nchan, self.hop, 4 * self.nchan, plan.before, b), plan.count), torch.complex64)]

    def process(self, env, obj, xs, bufs, st):
        return [obj.process(xs[0], out=bufs[0].t, stream=st)]

    def plan_change(self, plan, k):
        plan.count = len(self.LISTS[k])

    def change(self, obj, k):
        obj.set_channels(self.LISTS[k])

    def reference(self, env, xs, parts, reads):
        ref = HR.channelizer_ref(PR.to_complex(env.O, xs[0]), self.nchan, self.hop, self.proto)
        out = cat(parts, 0, 0)
        assert out.shape == ref.shape
        e = HR.err(out, ref)
        print(f"stream order, channelizer: err {e:.2e} (TOL {HR.TOL:.2e})")
        assert e <= HR.TOL


class SpectrumObj(PackedObj):
    """nfft 1024, the smallest the panorama takes, hop 512, with the peak.  A batch writes nothing the caller sees: the
    outputs are those of read(), issued behind the batches (the tail step) into tensors of the caller through the C ABI.
    There is no parameter to change: case B runs without changes."""
    id, nfft, hop = "spectrum", 1024, 512

    def sizes(self, env):
        return [8192, 520], [1024 * 3 + 8, 8, 512 * 7 + 24]

    def make(self, env):
        self.window = PR.hann(self.nfft)
        return env.pkg.Spectrum(self.nfft, self.hop, self.window, peak=True)

    def out_specs(self, env, plan, b):
        return []

    def process(self, env, obj, xs, bufs, st):
        obj.process(xs[0], stream=st)
        return []

    def tail_specs(self, env, plan):
        import torch
        return [((self.nfft,), torch.float32), ((self.nfft,), torch.float32)]

    def tail(self, env, obj, bufs, st):
        import ctypes as C
        import torch
        n = C.c_uint64()
        env.pkg.check(env.pkg.ddc_lib().pddc_spectrum_read(obj._h, bufs[0].t.data_ptr(), bufs[1].t.data_ptr(), C.byref(n), 0, st))
        self.nseg = int(n.value)
        return [bufs[0].t, bufs[1].t]

    def reference(self, env, xs, parts, reads):
        P, M, nseg = PR.spectrum_ref(PR.to_complex(env.O, xs[0]), self.nfft, self.hop, self.window)
        e1, e2 = PR.err(parts[-1][0], P), PR.err(parts[-1][1], M)
        print(f"stream order, spectrum: {nseg} segments, sum {e1:.2e} peak {e2:.2e} (TOL {SPECTRUM_TOL:.0e})")
        assert self.nseg == nseg and max(e1, e2) <= SPECTRUM_TOL


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def pipeline_plans(taps):
    """one plan per route family of the first launch (ddc_pipeline.cpp, choose_route), each tuned"""
    h1, h2, h3 = taps("c320_s1_d8_32"), taps("c320_s2_d8_64"), taps("c320_s3_d5_161")
    g = (np.random.default_rng(1225).standard_normal(40 * 12) / 40).astype(np.float32)
    return {
        "d8_127": [(8, taps("d8_127"))],                                     # the tuned decimate-by-8 alone
        "48-56": [(8, lowpass(48, 0.05)), (8, lowpass(56, 0.05))],           # the fused pair
        "8*8*5": [(8, h1), (8, h2), (5, h3)],                                # the pair and a tail behind it
        "d10_51": [(10, lowpass(51, 0.04))],                                 # the tuned decimate-by-10
        "rational": [(8, h1), (25, g, 12)],                                  # a 12/25 resampler behind: route Unpack
    }


class PipelineObj(PackedObj):
    """Batches of 2, 1 and 3 tiles of 8192 samples and a ragged one of 264, behind five warm-up batches (sizes()).  Case B retunes in front of each of seven
    batches: the word tables of the decimate-by-8 route go round their ring of four slots (the fifth upload waits for
    the first slot's event), those of the decimate-by-10 route change buffers three times, and the batch of 8 samples
    puts two words into the next batch's history window (route MixedHist), after which the route is the plan's again.
    overlap: the last stage rides along with the next batch, the tail step is the fence."""
    WORDS = (FREG, 123456789, 0x80000C35, 3000000000, 1 << 28, 0x7FFFF000, 987654321)
    seed = 5150

    def __init__(self, name, overlap=False):
        self.name, self.overlap, self.id = name, overlap, f"pipeline-{name}" + ("-overlap" if overlap else "")

    def stages(self, env):
        return pipeline_plans(env.taps)[self.name]

    def sizes(self, env):
        # The warm-up sizes every buffer the batches behind the gate use: the pipeline grows an inter-stage buffer, behind a
        # device synchronise, when a batch needs more of it than any before (ddc_pipeline.cpp, ensure_buf, and the second
        # half of overlap mode), and which buffers a batch needs depends on its route.  So: two batches of the largest
        # size on the plan's own route (a plan that pairs: the fused pair, both halves of overlap mode), a ragged one, after
        # which the second stage is off its 8-sample grid and whole tiles run unfused, the largest size on that route,
        # and 1784 samples, which put the second stage back on the grid (264 + 3 * 8192 + 1784 = 8 * 8 * 416).
        return [3 * TILE, 3 * TILE, 264, 3 * TILE, 1784], [2 * TILE, TILE, 3 * TILE, 264]

    def b_steps(self, env):
        sizes = [2 * TILE, TILE, 8, TILE, TILE, 2 * TILE, TILE]
        return [s for k, b in enumerate(sizes) for s in (("change", k), ("batch", b))]

    def make(self, env):
        p = env.pkg.Pipeline(self.stages(env), mix=True)
        p.set_freg(FREG)
        if self.overlap:
            p.set_overlap(True)
        return p

    def out_specs(self, env, plan, b):
        import torch
        n = b
        for st in self.stages(env):
            n = -(-n * (st[2] if len(st) > 2 else 1) // st[0]) + 1
        return [((n + 8, 2), torch.float32)]

    def process(self, env, obj, xs, bufs, st):
        n = obj.process_ptr(xs[0].data_ptr(), xs[0].numel() // 6, bufs[0].t.data_ptr(), bufs[0].shape[0], st)
        return [bufs[0].t[:n]]

    def tail(self, env, obj, bufs, st):
        obj.fence(st)
        return []

    def change(self, obj, k):
        obj.set_freg(self.WORDS[k])

    def reference(self, env, xs, parts, reads):
        ref = env.O.ddc_chain(xs[0], self.stages(env), freg=FREG, mix=True)
        y = np.concatenate([p[0].reshape(-1) for p in parts if p])
        assert y.size == ref.size
        e = env.O.rel_err(y, ref)
        print(f"stream order, {self.id}: rel err {e:.2e} (FIR_TOL {FIR_TOL:.0e})")
        assert e <= FIR_TOL


STAGES = [BlankerObj(), RxFilterObj(), CarrierObj(), DemodObj(), AdaptObj(), SquelchObj(), AudioObj(), ScopeObj()]
OBJECTS = STAGES + [CarrierObj(1), TunerObj(), ChannelizerObj(), SpectrumObj(), PipelineObj("d8_127"), PipelineObj("d10_51")]
# case D: every route family, in line and in overlap mode (the two plans above are among them: their case A runs there)
ROUTES = [PipelineObj(name, overlap) for name in ("d8_127", "48-56", "8*8*5", "d10_51", "rational") for overlap in (False, True)]
