"""Every stream object on a busy side stream with nothing synchronised (include/perseus_ddc.h: "Stream-ordered; one
stream per object, one thread at a time"): pddc_pipeline, pddc_bank, pddc_spectrum, pddc_channelizer, pddc_tuner and the
eight receiver stages.  The rest of the suite calls them on the null stream of an idle device, where a launch or a copy
that goes to stream 0 instead of the caller's stream, a host buffer rewritten under a pending upload, and a read, reset,
destroy or create that does not wait all behave as if they were right.

The harness (tests/stream_order.py), in four pieces:
 1. Side stream: a torch.cuda.Stream, which does not synchronise with the null stream (one that was tried and does not
    share the null stream's hardware queue either: stream_order.side_streams).  Every input, output and scratch
    tensor is allocated up front on the null stream, followed by a device synchronise; every library call gets the
    explicit stream and explicit output tensors (where a Python wrapper allocates inside the call -- Spectrum.read,
    Pipeline.process -- the C ABI or process_ptr is called with tensors of the test's).  torch's allocator plays no part.
 2. Filler and gate: before the calls under test the side stream is given elementwise kernels on a 256 MiB tensor that
    keep it busy for FILLER_MS and finish by themselves, then an event is recorded, the gate.
 3. Input behind the filler: the tensor the object reads holds the real series reversed in time; the real one is copied
    over it on the side stream behind the gate, so a launch that does not wait for the side stream reads other values.
 4. Canaries while the gate is closed: every output is prefilled with 0xA5 bytes.  With the whole sequence issued and
    nothing synchronised the gate must not have fired, every output downloaded on the null stream must still hold only
    the canary, and the gate must still not have fired (the download did not wait for the side stream).  Only then is
    the side stream synchronised and the results compared.  The two gate tests are conditions: a run in which the host
    did not stay ahead fails.

The clean run of every case is the same object type with the same batches and changes on the null stream with a device
synchronise after every call.  The busy run must have the clean run's bits (outputs and everything read() returns), and
once per object the clean run of case A is compared with the object's double reference at that reference's own
tolerance (stream_order.py, reference()).

Cases: A steady state (two warm-up batches, five for the pipeline, whose inter-stage buffers grow at first need, then three batches that straddle the tile, no parameter change: the host
must run ahead); B changes behind a busy stream (set_rx / set_freq / set_slot / set_channels / set_freg in front of every
batch, then read(), reset() and close() without an explicit synchronise; whether the host ran ahead is printed, not
asserted); C an object created while the device is busy; D the pipeline's route families in line and in overlap mode, and
a bank of four; E one chain over two streams.

Host times and filler lengths, measured on an MI355X (NOTEBOOK.md R22.1), Python and ctypes included.  Issuing the
sequence on the side stream: case A 0.03 .. 0.12 ms, case B 0.06 .. 0.27 ms (the pipeline's sequence waits for the
stream: its whole filler), case C with create 0.08 .. 0.48 ms, the bank's six rounds 0.15 ms, the chain 0.32 ms.  From the gate to
the second gate test, every output downloaded in between: 0.17 .. 2.6 ms, the decimate-by-10 pipeline 7.5 ms.  The filler
is 100 ms everywhere, more than 10 x the longest of these; one filler kernel takes 0.073 ms.
"""
import time
import types

import numpy as np
import pytest

import stream_order as S

pytestmark = pytest.mark.gpu

# the filler of every case in milliseconds: at least 10 x the longest host time from the gate to the second gate test
FILLER_MS = {"A": 100.0, "B": 100.0, "C": 100.0, "bank": 100.0, "chain": 100.0}

ids = lambda ad: ad.id


@pytest.fixture(scope="module")
def env(pkg, O, dev, taps):
    S.side_streams(dev, 2)
    return types.SimpleNamespace(pkg=pkg, O=O, dev=dev, taps=taps)


def results(views):
    return [[S.host(v) for v in vs] for vs in views]


def same_reads(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert S.same_bits(g, w), (what, "read", i)


def behind_the_gate(side, live, real):
    """the real series over the scrambled one, on the side stream"""
    import torch
    with torch.cuda.stream(side):
        for l, x in zip(live, real):
            l.copy_(x, non_blocking=True)


def gate_and_canaries(gate, bufs):
    """harness step 4, before anything is synchronised -> (gate closed, all canaries intact, gate still closed)"""
    closed1 = not gate.query()
    intact = all(b.untouched() for bl in bufs if bl for b in bl)
    return closed1, intact, not gate.query()


# ---- A, D: steady state ---------------------------------------------------------------------------------------------

_clean = {}


def a_steps(env, ad):
    warm, main = ad.sizes(env)
    return S.batches(warm), S.batches(main) + [("tail",)]


def clean_a(env, ad):
    """(the inputs, the clean run's results step by step, what read() returns behind it), once per object"""
    import torch
    if ad.id not in _clean:
        warm, main = a_steps(env, ad)
        xs = ad.inputs(env, sum(s[1] for s in warm + main if s[0] == "batch"))
        xd = S.upload(xs, env.dev)
        bufs = S.allocate(ad, env, warm + main)
        obj = ad.make(env)
        torch.cuda.synchronize()
        views = S.Runner(ad, env, obj, xd, 0, sync_each=True).go(warm + main, bufs)
        reads = ad.read(obj, 0)
        _clean[ad.id] = (xs, results(views), reads)
        obj.close()
    return _clean[ad.id]


def steady_state(env, ad):
    import torch
    dev = env.dev
    xs, clean, clean_reads = clean_a(env, ad)
    warm, main = a_steps(env, ad)
    keep = sum(s[1] for s in warm)
    real, live = S.upload(xs, dev), S.upload(S.scrambled(ad, xs, keep), dev)
    bufs = S.allocate(ad, env, warm + main)
    obj = ad.make(env)
    torch.cuda.synchronize()
    side = S.side_streams(dev)[0]
    st = side.cuda_stream
    r = S.Runner(ad, env, obj, live, st)
    vw = r.go(warm, bufs[:len(warm)])
    side.synchronize()                           # the create-time and `fresh`-mark uploads are through
    gate = S.occupy(side, dev, FILLER_MS["A"])
    behind_the_gate(side, live, real)
    t0 = time.perf_counter()
    vm = r.go(main, bufs[len(warm):])
    t1 = time.perf_counter()
    closed1, intact, closed2 = gate_and_canaries(gate, bufs[len(warm):])
    t2 = time.perf_counter()
    side.synchronize()
    reads = ad.read(obj, st)
    got = results(vw + vm)
    obj.close()
    print(f"stream order A {ad.id}: issued in {1e3 * (t1 - t0):.3f} ms, gate tested after {1e3 * (t2 - t0):.3f} ms")
    assert closed1, "the host did not run ahead of the side stream: a steady-state process() stalled it"
    assert intact, "an output was written while the side stream was still busy: a launch or copy on another stream"
    assert closed2, "the download on the null stream waited for the side stream"
    S.assert_same(got, clean, (ad.id, "busy against clean"))
    same_reads(reads, clean_reads, ad.id)


A_OBJECTS = [ad for ad in S.OBJECTS if not isinstance(ad, S.PipelineObj)]


@pytest.mark.parametrize("ad", A_OBJECTS, ids=ids)
def test_a_steady_state(env, ad):
    """Two warm-up batches on the side stream, a synchronise, then filler, gate, the input behind the gate and three
    batches without a parameter change (stages: tile - 1, 1, 2 tile + 5; the packed-stream objects: multiples of 8
    samples; the tuner: sizes that leave carried rows).  The host runs ahead, no output is touched while the gate is
    closed, and outputs and read() have the clean run's bits: a carry or tail kernel on another stream shows as a stale
    history in the next batch and as a touched canary."""
    steady_state(env, ad)


@pytest.mark.parametrize("ad", S.ROUTES, ids=ids)
def test_d_pipeline_routes(env, ad):
    """Case A for one plan per route family of the pipeline, each tuned: the decimate-by-8 first stage alone, the fused
    pair, the pair with a tail, the decimate-by-10 first stage and a rational plan (route Unpack), in batches of 2, 1 and
    3 tiles and a ragged one of 264 samples, in line and in overlap mode (the fence goes on the side stream)."""
    steady_state(env, ad)


@pytest.mark.parametrize("ad", A_OBJECTS + S.ROUTES, ids=ids)
def test_reference_of_the_clean_run(env, ad):
    """The clean run of case A, all batches in a row, against the object's double reference at the tolerance the
    reference's file carries (the bit-exact stages: the reference's bits)."""
    xs, clean, reads = clean_a(env, ad)
    nb = len([s for s in sum(a_steps(env, ad), []) if s[0] == "batch"])
    parts = clean[:nb] + ([clean[nb]] if clean[nb] else [])
    ad.reference(env, xs, parts, reads)


# ---- B: changes behind a busy stream --------------------------------------------------------------------------------

def b_steps(env, ad):
    steps = ad.b_steps(env) + [("tail",)]
    sizes = [s[1] for s in steps if s[0] == "batch"]
    return steps, [("reset",), ("batch", sizes[0]), ("batch", sizes[1]), ("tail",)], sum(sizes)


def clean_b(env, ad, xs):
    import torch
    steps, after, _ = b_steps(env, ad)
    xd = S.upload(xs, env.dev)
    bufs = S.allocate(ad, env, steps + after)
    obj = ad.make(env)
    torch.cuda.synchronize()
    r = S.Runner(ad, env, obj, xd, 0, sync_each=True)
    v1 = r.go(steps, bufs[:len(steps)])
    reads = ad.read(obj, 0)
    v2 = r.go(after, bufs[len(steps):])
    out = results(v1 + v2), reads
    obj.close()
    return out


# one stage once more with the largest receiver table there is, 1024 entries
B_OBJECTS = S.OBJECTS + [S.CarrierObj(1024)]


@pytest.mark.parametrize("ad", B_OBJECTS, ids=ids)
def test_b_changes_behind_a_busy_stream(env, ad):
    """Filler, gate, the input behind the gate, then a parameter change on several receivers in front of each batch (the
    second touches the same receivers and others; the pipeline: a new word in front of each of seven batches).  Every
    upload's staging is reused while the stream is still busy.  Then, with nothing synchronised by the test: read() on the
    side stream, reset() and the first batch again, one more batch and close() directly behind it.  All of it has the
    bits of the clean run that made the same changes at the same batch boundaries.  Whether the host was still ahead of
    the gate after the sequence -- the uploads did not stall it -- is printed (NOTEBOOK.md has the table), not asserted;
    where it was, the outputs must still hold their canaries."""
    import torch
    dev = env.dev
    steps, after, total = b_steps(env, ad)
    xs = ad.inputs(env, total)
    clean, clean_reads = clean_b(env, ad, xs)
    real, live = S.upload(xs, dev), S.upload(S.scrambled(ad, xs, 0), dev)
    bufs = S.allocate(ad, env, steps + after)
    obj = ad.make(env)
    torch.cuda.synchronize()
    side = S.side_streams(dev)[0]
    st = side.cuda_stream
    gate = S.occupy(side, dev, FILLER_MS["B"])
    behind_the_gate(side, live, real)
    r = S.Runner(ad, env, obj, live, st)
    t0 = time.perf_counter()
    v1 = r.go(steps, bufs[:len(steps)])
    t1 = time.perf_counter()
    ahead, intact, still = gate_and_canaries(gate, bufs[:len(steps)])
    reads = ad.read(obj, st)                     # waits for the side stream where the object has a read()
    v2 = r.go(after, bufs[len(steps):])          # reset() waits for the device; the two batches behind it do not
    obj.close()                                  # directly behind the last batch: destroy waits
    got = results(v1 + v2)
    side.synchronize()
    print(f"stream order B {ad.id}: issued in {1e3 * (t1 - t0):.3f} ms, host ran ahead: {'yes' if ahead else 'no'}")
    if still:
        assert intact, "an output was written while the side stream was still busy: a launch or copy on another stream"
    S.assert_same(got, clean, (ad.id, "busy against clean"))
    same_reads(reads, clean_reads, ad.id)


# ---- C: created while the device is busy ----------------------------------------------------------------------------

@pytest.mark.parametrize("ad", S.OBJECTS, ids=ids)
def test_c_created_while_busy(env, ad):
    """The filler is already running on the side stream when the object is created; its first batch follows at once on
    that stream.  The result has the bits of a clean first batch: the create-time clears and uploads, which go to the
    null stream, are through before a kernel on the side stream reads them.  Whether the device was still busy when
    create returned is printed: the pipeline's create waits for the device (its reset does), the other objects' do not."""
    import torch
    dev = env.dev
    steps = [("batch", ad.sizes(env)[1][-2 if isinstance(ad, S.PipelineObj) else -1]), ("tail",)]
    xs = ad.inputs(env, steps[0][1])
    xd = S.upload(xs, dev)
    bufs, cbufs = S.allocate(ad, env, steps), S.allocate(ad, env, steps)
    obj = ad.make(env)
    torch.cuda.synchronize()
    clean = results(S.Runner(ad, env, obj, xd, 0, sync_each=True).go(steps, cbufs))
    obj.close()
    torch.cuda.synchronize()
    side = S.side_streams(dev)[0]
    gate = S.occupy(side, dev, FILLER_MS["C"])
    t0 = time.perf_counter()
    obj = ad.make(env)
    busy = not gate.query()
    views = S.Runner(ad, env, obj, xd, side.cuda_stream).go(steps, bufs)
    t1 = time.perf_counter()
    side.synchronize()
    got = results(views)
    obj.close()
    print(f"stream order C {ad.id}: created and issued in {1e3 * (t1 - t0):.3f} ms, the device still busy behind create: "
          f"{'yes' if busy else 'no'}")
    S.assert_same(got, clean, (ad.id, "created while busy against clean"))


# ---- D: a bank of four ----------------------------------------------------------------------------------------------

BANK_FREGS = [0x7FFFF000, S.FREG, 3000000000, 123456789]


def bank_plans(taps):
    p = S.pipeline_plans(taps)
    return [p["8*8*5"], p["48-56"], [(8, taps("c320_s1_d8_32")), (8, taps("c320_s2_d8_64"))], [(8, S.lowpass(48, 0.05))]]


def bank_run(env, xd, sizes, bufs, st, clean, before=None):
    import torch
    pipes = []
    for stages, f in zip(bank_plans(env.taps), BANK_FREGS):
        p = env.pkg.Pipeline(stages, mix=True)
        p.set_freg(f)
        pipes.append(p)
    bank = env.pkg.Bank(pipes)
    torch.cuda.synchronize()
    views, off = [], 0
    for i, (ns, bl) in enumerate(zip(sizes, bufs)):
        if before:
            before(i)
        n, _ = bank.process_ptr(xd[6 * off:].data_ptr(), ns, [b.t.data_ptr() for b in bl], [b.shape[0] for b in bl], st)
        views.append([b.t[:k] for b, k in zip(bl, n)])
        off += ns
        if clean:
            torch.cuda.synchronize()
    return bank, pipes, views


def test_d_bank_round_on_a_side_stream(env):
    """Four members (the pair with a tail, the 48/56-tap pair, a pair, a first stage alone) through pddc_bank_process on
    the side stream: two warm-up rounds, then filler, gate, the input behind the gate and rounds of 2, 1 and 3 tiles and
    264 samples.  The host runs ahead, no member's output is touched while the gate is closed, every member has the bits
    of the same bank on the null stream, and the clean run is within FIR_TOL of the oracle's chain."""
    import torch
    dev = env.dev
    warm, main = 2, [3 * S.TILE, S.TILE, 2 * S.TILE, S.TILE, 3 * S.TILE, 264]      # (the first round sizes the members' buffers)
    xs = env.O.lcg_bytes(6 * sum(main), 4243)
    real = S.upload([xs], dev)[0]
    scr = np.array(xs, copy=True)
    scr[6 * 4 * S.TILE:] = xs[6 * 4 * S.TILE:][::-1]
    live = S.upload([scr], dev)[0]

    def alloc():
        return [[S.Buf((ns // 8 + 16, 2), torch.float32, dev) for _ in range(4)] for ns in main]

    cb, bb = alloc(), alloc()
    bank, pipes, views = bank_run(env, real, main, cb, 0, True)
    clean = results(views)
    bank.close()
    for p in pipes:
        p.close()
    side = S.side_streams(dev)[0]
    state = {}

    def before(i):
        if i == warm:
            side.synchronize()
            state["gate"] = S.occupy(side, dev, FILLER_MS["bank"])
            behind_the_gate(side, [live], [real])
            state["t0"] = time.perf_counter()

    bank, pipes, views = bank_run(env, live, main, bb, side.cuda_stream, False, before)
    t1 = time.perf_counter()
    closed1, intact, closed2 = gate_and_canaries(state["gate"], bb[warm:])
    t2 = time.perf_counter()
    side.synchronize()
    got = results(views)
    bank.close()
    for p in pipes:
        p.close()
    print(f"stream order bank: issued in {1e3 * (t1 - state['t0']):.3f} ms, gate tested after {1e3 * (t2 - state['t0']):.3f} ms")
    assert closed1 and intact and closed2, (closed1, intact, closed2)
    S.assert_same(got, clean, "bank, busy against clean")
    for i, (stages, f) in enumerate(zip(bank_plans(env.taps), BANK_FREGS)):
        y = np.concatenate([c[i].reshape(-1) for c in clean])
        ref = env.O.ddc_chain(xs, stages, freg=f, mix=True)
        assert y.size == ref.size and env.O.rel_err(y, ref) <= S.FIR_TOL, i


# ---- E: one chain over two streams ----------------------------------------------------------------------------------

def test_e_one_chain_over_two_streams(env):
    """Channelizer and Audio on stream A, Tuner and Demod on stream B, ordered by events, the filler on A: the audio has
    the bits of the same chain on one stream, and nothing is written while the gate is closed.  The objects share
    nothing that is bound to a stream."""
    import torch
    pkg, dev = env.pkg, env.dev
    M, hop, T, Rd, L, Ma, nrx = 1024, 512, 64, 4, 3072, 625, S.K
    sizes = [65536, 32776, 67072]
    proto, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, Rd)
    words, rx = S.TR.receiver_set(M, nrx), S.DR.interleaved_rx(nrx)
    xs = env.O.lcg_bytes(6 * sum(sizes), 2718)
    real, live = S.upload([xs], dev)[0], S.upload([np.ascontiguousarray(xs[::-1])], dev)[0]

    def alloc():
        out, s0, r0, n0 = [], 0, 0, 0
        for ns in sizes:
            r = pkg.channelizer_rows(M, hop, proto.size, s0, ns)
            n = pkg.tuner_outputs(T, Rd, r0, r)
            m = pkg.audio_outputs(L, Ma, n0, n)
            out.append([S.Buf((r, M), torch.complex64, dev), S.Buf((nrx, n), torch.complex64, dev),
                        S.Buf((nrx, n), torch.float32, dev), S.Buf((nrx, m), torch.float32, dev)])
            s0, r0, n0 = s0 + ns, r0 + r, n0 + n
        return out

    def chain(x, bufs, a, b, clean):
        ch = pkg.Channelizer(M, proto, hop)
        tu = pkg.Tuner(ch, words, h, Rd)
        de = pkg.Demod(rx, **S.DR.PARAMS)
        au = pkg.Audio(nrx, L, Ma)
        torch.cuda.synchronize()
        gate = None
        if not clean:
            gate = S.occupy(a, dev, FILLER_MS["chain"])
            behind_the_gate(a, [live], [real])
        sa, sb = (0, 0) if clean else (a.cuda_stream, b.cuda_stream)
        t0 = time.perf_counter()
        views, off = [], 0
        for ns, (rows, z, aud, out) in zip(sizes, bufs):
            rv = ch.process(x[6 * off:6 * (off + ns)], out=rows.t, stream=sa)
            if not clean:
                e = torch.cuda.Event()
                e.record(a)
                b.wait_event(e)
            zv = tu.process(rv, out=z.t, stream=sb)
            av = de.process(zv, out=aud.t, stream=sb)
            if not clean:
                e = torch.cuda.Event()
                e.record(b)
                a.wait_event(e)
            views.append([au.process(av, out_f32=out.t, stream=sa)])
            off += ns
            if clean:
                torch.cuda.synchronize()
        return (ch, tu, de, au), views, gate, time.perf_counter() - t0

    cb, bb = alloc(), alloc()
    objs, views, _, _ = chain(real, cb, None, None, True)
    clean = results(views)
    for o in objs:
        o.close()
    assert all(c[0].shape[1] > 0 for c in clean)
    a, b = S.side_streams(dev, 2)
    objs, views, gate, issue = chain(live, bb, a, b, False)
    closed1, intact, closed2 = gate_and_canaries(gate, bb)
    a.synchronize()
    b.synchronize()
    got = results(views)
    for o in objs:
        o.close()
    print(f"stream order chain: issued in {1e3 * issue:.3f} ms")
    assert closed1 and intact and closed2, (closed1, intact, closed2)
    S.assert_same(got, clean, "two streams against one")
