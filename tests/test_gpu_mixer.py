"""Mixer (pddc_mixer_*, k_mix, k_mix_bus) on the GPU against the numpy float32 reference (tests/mixer_ref.py) fed the
very float32 arrays uploaded.  Every comparison is by int32 / int16 views and exact equality: there are no tolerances.
The inputs' preconditions (the limiter acts in some blocks and not in others, a clamp is hit, a ramp is cut by a batch
boundary, a set_rx lands mid-ramp, the active count crosses a multiple of C) are asserted in tests/test_mixer_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import mixer_ref as MR
import squelch_ref as SR
import stream_order as S

pytestmark = pytest.mark.gpu
N0 = 3000
F32 = np.float32
LIMITS = [None] + [(Lb, MR.CEIL, MR.REL) for Lb in MR.BLOCKS]


@functools.lru_cache(maxsize=None)
def series(K):
    return SR.audio_series(K, N0, MR.SERIES_SEED)


_dev = {}


def on_device(K, dev):
    import torch
    if K not in _dev:
        _dev[K] = torch.from_numpy(series(K)).to(dev)
    return _dev[K]


@functools.lru_cache(maxsize=None)
def ref_y(K, Q, R):
    """the one-shot reference without the limiter: (y, its status), computed once"""
    g = MR.interleaved_gains(K, Q)
    y, _, st, _ = MR.mixer_ref(series(K), g, R, changes=MR.one_shot_changes(K, Q, g))
    y.setflags(write=False)
    return y, st


def ref_out(K, Q, R, limit):
    """-> (out [Q, count], pcm [count, Q], status) of the one-shot case"""
    y, st = ref_y(K, Q, R)
    if limit is None:
        return y, MR.pcm(y, 32767.0).T, st
    lim = MR.LimiterRef(Q, *limit)
    out = lim.process(y)
    st = st.copy()
    st["gain"], st["min_gain"] = lim.E, lim.min_gain
    return out, MR.pcm(out, 32767.0).T, st


def run(pkg, a, gains, R, limit=None, cuts=None, before=None, f32=True, i16=True, changes=()):
    """all of a (torch [K, n]) through a fresh Mixer in the given batches -> numpy (out [Q, count] or None, pcm
    [count, Q] or None, status); `changes` are set ahead of the first batch, before(i, m) is called ahead of batch i"""
    import torch
    m = pkg.Mixer(gains, R, limit=limit)
    for j, g in changes:
        m.set_rx(j, g)
    outs, off, Q = [], 0, m.nbus
    for i, b in enumerate(cuts or [a.shape[1]]):
        if before:
            before(i, m)
        due = m.next_outputs(b)
        o = m.process(a[:, off:off + b], f32=f32, i16=i16)
        o = o if isinstance(o, tuple) else (o,)
        fo = o[0] if f32 else None
        io = o[-1] if i16 else None
        assert fo is None or fo.shape == (Q, due)
        assert io is None or io.shape == (due, Q)
        outs.append((fo, io))
        off += b
    assert off == a.shape[1]
    status = m.read()
    m.close()
    fo = torch.cat([o[0] for o in outs], dim=1).cpu().numpy() if f32 else None
    io = torch.cat([o[1] for o in outs], dim=0).cpu().numpy() if i16 else None
    return fo, io, status


def same(got, want, what=""):
    fo, io, st = got
    wf, wi, wst = want
    if fo is not None:
        assert fo.shape == wf.shape and fo.dtype == F32, (what, "f32", fo.shape, wf.shape)
        assert np.array_equal(MR.bits(fo), MR.bits(wf)), (what, "f32", int((MR.bits(fo) != MR.bits(wf)).sum()))
    if io is not None:
        assert io.shape == wi.shape and io.dtype == np.int16, (what, "i16", io.shape, wi.shape)
        assert np.array_equal(io, wi), (what, "i16")
    if st is not None and wst is not None:
        for name in MR.STATUS.names:
            assert np.array_equal(st[name].view(np.uint32), wst[name].view(np.uint32)), (what, "status", name, st, wst)


def shapes(pkg):
    Cc = pkg.mixer_chunk()
    return {"1024x2": (1024, 2), "1024x8": (1024, 8), "1": (1, 2), "C-1": (Cc - 1, 2), "C": (Cc, 2), "C+1": (Cc + 1, 2),
            "37": (37, 2), "active C": (Cc + Cc // 2, 2), "active C+1": (Cc + Cc // 2 + 1, 2)}


@pytest.mark.parametrize("shape", ["1024x2", "1024x8", "1", "C-1", "C", "C+1", "37", "active C", "active C+1"])
def test_bits_against_the_reference(pkg, dev, shape):
    """n = 3000; K = 1024 with Q = 2 and 8, K = 1, C - 1, C, C + 1, 37 (and the two K around which the ACTIVE count is C)
    with Q = 2; gains interleaved receiver by receiver, a third of them silent, set_rx calls ahead of the batch so that
    ramps run and receivers go silent inside it; R in 1, 37, 4000; without the limiter and with Lb in 8, 48, 1000, 4096
    (the last writes nothing); float32 and int16 together for every combination, each alone for R = 37; read() too."""
    K, Q = shapes(pkg)[shape]
    assert pkg.mixer_status_dtype() == MR.STATUS
    a, g = on_device(K, dev), MR.interleaved_gains(K, Q)
    ch = MR.one_shot_changes(K, Q, g)
    for R in MR.RAMPS:
        for limit in LIMITS:
            want = ref_out(K, Q, R, limit)
            if limit and limit[0] > N0:
                assert want[0].shape == (Q, 0)
            same(run(pkg, a, g, R, limit, changes=ch), want, (shape, R, limit))
            if R == 37:
                same(run(pkg, a, g, R, limit, changes=ch, i16=False), want, (shape, R, limit, "f32 alone"))
                same(run(pkg, a, g, R, limit, changes=ch, f32=False), want, (shape, R, limit, "i16 alone"))


@pytest.mark.parametrize("K,Q", [(1024, 2), (37, 8)])
def test_bits_against_the_cut(pkg, dev, K, Q):
    """One batch against batches of 0, 1, 2, Lb - 1, Lb, tile - 1, tile, tile + 1, 3 tile + 5 and the rest, without the
    limiter and with Lb = 48, ramps under way (R = 37 and R = 4000, which no batch completes)."""
    TT, Lb = pkg.mixer_tile_outputs(), 48
    cuts = [0, 1, 2, Lb - 1, Lb, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(N0 - sum(cuts))
    assert cuts[-1] > 0
    a, g = on_device(K, dev), MR.interleaved_gains(K, Q)
    ch = MR.one_shot_changes(K, Q, g)
    for R in (37, 4000):
        for limit in (None, (Lb, MR.CEIL, MR.REL)):
            want = ref_out(K, Q, R, limit)
            same(run(pkg, a, g, R, limit, cuts, changes=ch), want, (K, Q, R, limit, "cut"))
            same(run(pkg, a, g, R, limit, cuts[::-1], changes=ch), want, (K, Q, R, limit, "cut, reversed"))


def test_a_bus_alone(pkg, dev):
    """Bus q among eight (every active receiver feeds every bus) against the same gains with the other buses' zero, and
    against a mixer of that one bus: the active set is the same, so are the bits; the zeroed buses are +0."""
    K, Q, R = 100, 8, 37
    a = on_device(K, dev)
    g = MR.interleaved_gains(K, Q)
    g[(g == 0) & (np.arange(K) % 3 != 2)[:, None]] = F32(0.0625)          # no hole in an active receiver
    for limit in (None, (48, MR.CEIL, MR.REL)):
        full = run(pkg, a, g, R, limit)
        for q in (0, 3, 7):
            only = np.zeros_like(g)
            only[:, q] = g[:, q]
            among = run(pkg, a, only, R, limit)
            alone = run(pkg, a, g[:, q:q + 1].copy(), R, limit)
            assert np.array_equal(MR.bits(among[0][q]), MR.bits(full[0][q])) and np.array_equal(among[1][:, q], full[1][:, q])
            assert np.array_equal(MR.bits(alone[0][0]), MR.bits(full[0][q])) and np.array_equal(alone[1][:, 0], full[1][:, q])
            rest = [p for p in range(Q) if p != q]
            assert not MR.bits(among[0][rest]).any() and not among[1][:, rest].any()
            for name in MR.STATUS.names:
                assert alone[2][name][0] == among[2][name][q] == full[2][name][q]


@pytest.mark.parametrize("limit", [None, (48, MR.CEIL, MR.REL)])
def test_set_rx_between_batches(pkg, dev, limit):
    """The scenario of mixer_ref.scenario_changes against the streaming reference, bit for bit: a change mid-ramp, two
    changes before one batch, receivers going silent inside a batch and coming back; a bad call is refused and changes
    nothing."""
    K, Q, R, cuts = MR.SCN_K, MR.SCN_Q, MR.SCN_R, list(MR.SCN_CUTS)
    a, g = on_device(K, dev), MR.interleaved_gains(K, Q)
    changes = MR.scenario_changes(g)
    nan, inf = float("nan"), float("inf")

    def before(i, m):
        for j, gg in changes.get(i, ()):
            m.set_rx(j, gg)
        for j, gg in ((K, [0.5, 0.5]), (-1, [0.5, 0.5]), (1, [nan, 0.5]), (1, [0.5, inf]), (1, [-inf, 0.0])):
            with pytest.raises(pkg.PddcError) as e:
                m.set_rx(j, gg)
            assert e.value.code == pkg.PDDC_EINVAL
        with pytest.raises(pkg.PddcError):
            m.set_rx(1, [0.5])

    got = run(pkg, a, g, R, limit, cuts, before)
    ref = MR.MixerRef(g, R, limit, chunk=pkg.mixer_chunk())
    wf, wi = MR.run_cuts(ref, series(K), cuts, lambda i, r: [r.set_rx(j, gg) for j, gg in changes.get(i, ())])
    same(got, (wf, wi, ref.read()), "set_rx")
    clean = run(pkg, a, g, R, limit, cuts)
    assert not np.array_equal(got[0], clean[0])


def test_layout_refusals_and_reset(pkg, dev):
    """a as the view Audio.process returns (row stride > n); outputs with padding, which keeps its fill value; process
    calls refused for each capacity, each alignment, a missing pointer and an output over a, between the batches: the
    next correct call's bits are those of an object that never saw them.  reset starts the series again."""
    import torch
    K, Q, R, limit = 37, 2, 37, (48, MR.CEIL, MR.REL)
    x = torch.from_numpy(series(K)).to(dev)
    au = pkg.Audio(K, 3, 2, phases=32, taps=8)
    cap = au.next_outputs(N0) + 29
    av = au.process(x, out_f32=torch.empty((K, cap), dtype=torch.float32, device=dev))
    n = av.shape[1]
    assert av.stride(0) == cap > n > 4000
    an = av.cpu().numpy()
    g = MR.interleaved_gains(K, Q)
    ch = MR.one_shot_changes(K, Q, g)
    cuts = [700, 1300, n - 2000]
    ref = MR.MixerRef(g, R, limit, chunk=pkg.mixer_chunk())
    for j, gg in ch:
        ref.set_rx(j, gg)
    wf, wi = MR.run_cuts(ref, an, cuts)
    want = (wf, wi, ref.read())
    count = wf.shape[1]
    # padded outputs
    m = pkg.Mixer(g, R, limit=limit)
    for j, gg in ch:
        m.set_rx(j, gg)
    fbuf = torch.full((Q, count + 7), 7.0, dtype=torch.float32, device=dev)
    ibuf = torch.full((count + 5, Q), 9, dtype=torch.int16, device=dev)
    fo, io = m.process(av, out_f32=fbuf, out_i16=ibuf)
    assert fo.data_ptr() == fbuf.data_ptr() and io.data_ptr() == ibuf.data_ptr()
    same((fo.cpu().numpy(), io.cpu().numpy(), m.read()), want, "strided")
    assert bool((fbuf[:, count:] == 7.0).all()) and bool((ibuf[count:] == 9).all())
    m.close()

    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY
    stream = torch.cuda.current_stream().cuda_stream

    def disturb(i, m):
        b = cuts[i]
        due = m.next_outputs(b)
        assert due >= 48
        f = torch.empty((Q, due), dtype=torch.float32, device=dev)
        p = torch.empty((due, Q), dtype=torch.int16, device=dev)
        for kw in (dict(out_f32=f[:, :due - 1]), dict(out_i16=p[:due - 1])):
            with pytest.raises(pkg.PddcError) as e:
                m.process(av[:, :b], **kw)
            assert e.value.code == ECAP, kw
        cnt = C.c_size_t(77)

        def call(ap=av.data_ptr(), nn=b, as_=cap, fp=f.data_ptr(), fs=due, ip=p.data_ptr(), ic=due):
            return L.pddc_mixer_process(m._h, ap, nn, as_, fp, fs, ip, ic, C.byref(cnt), stream)

        assert call(as_=b - 1) == ECAP and call(fs=due - 1) == ECAP and call(ic=due - 1) == ECAP
        assert call(ap=av.data_ptr() + 2) == EINVAL and call(fp=f.data_ptr() + 2) == EINVAL and call(ip=p.data_ptr() + 1) == EINVAL
        assert call(ap=None) == EINVAL and call(fp=None, ip=None) == EINVAL
        assert call(fp=av.data_ptr() + 4 * b, fs=cap) == EINVAL                  # f32 inside a's rows
        assert call(ip=av.data_ptr() + 4 * (cap * (K - 1) + b) - 2) == EINVAL    # i16 over a's last bytes
        assert cnt.value == 77
        assert call(ap=None, nn=0, as_=0, fp=None, fs=0, ip=None, ic=0) == pkg.PDDC_OK and cnt.value == 0

    same(run(pkg, av, g, R, limit, cuts, disturb, changes=ch), want, "refused")
    # reset: the series starts again, the targets stay
    m = pkg.Mixer(g, R, limit=limit)
    first = tuple(t.clone() for t in m.process(av, i16=True))
    st1 = m.read()
    m.reset()
    fresh = m.read()
    assert not fresh["peak"].any() and (fresh["gain"] == 1).all() and (fresh["min_gain"] == 1).all()
    second = m.process(av, i16=True)
    for u, v in zip(first, second):
        assert u.shape == v.shape and bool((u.view(torch.int32 if u.dtype == torch.float32 else torch.int16) ==
                                            v.view(torch.int32 if v.dtype == torch.float32 else torch.int16)).all())
    st2 = m.read()
    for name in MR.STATUS.names:
        assert np.array_equal(st1[name].view(np.uint32), st2[name].view(np.uint32))
    m.close()
    au.close()


@pytest.mark.parametrize("limit", [None, (48, MR.CEIL, MR.REL)])
def test_nan_stays_where_it_is(pkg, dev, limit):
    """One NaN in one active receiver changes only that index of each bus it feeds (to NaN; behind the limiter, whose
    block peaks drop it, to -ceil) and no gain of the limiter; in a silent receiver it changes nothing."""
    import torch
    K, Q, R = 37, 2, 37
    g = MR.interleaved_gains(K, Q)
    base = series(K)
    y, _ = ref_y(K, Q, R)
    # an index whose |y| is not its block's peak on either bus, so that the block peaks are the same without it
    Lb = 48
    at = next(i for i in range(1200, 1300) if all(abs(y[q, i]) < np.abs(y[q, i // Lb * Lb:(i // Lb + 1) * Lb]).max() for q in range(Q)))
    j_act = next(j for j in range(K) if g[j].all())
    j_sil = next(j for j in range(5, K) if not g[j].any() and not any(c[0] == j for c in MR.one_shot_changes(K, Q, g)))
    ch = MR.one_shot_changes(K, Q, g)
    clean = run(pkg, on_device(K, dev), g, R, limit, changes=ch)
    for j, silent in ((j_act, False), (j_sil, True)):
        x = base.copy()
        x[j, at] = np.nan
        got = run(pkg, torch.from_numpy(x).to(dev), g, R, limit, changes=ch)
        ref = MR.MixerRef(g, R, limit, chunk=pkg.mixer_chunk())
        for jj, gg in ch:
            ref.set_rx(jj, gg)
        wf, wi = ref.process(x)
        same(got, (wf, wi, ref.read()), ("nan", j))
        diff = np.flatnonzero((MR.bits(got[0]) != MR.bits(clean[0])).any(axis=0))
        if silent:
            assert diff.size == 0 and np.array_equal(got[1], clean[1])
        else:
            assert diff.tolist() == [at], diff
            if limit is None:
                assert np.isnan(got[0][:, at]).all() and not got[1][at].any()
            else:
                assert (got[0][:, at] == -F32(MR.CEIL)).all()
        for name in ("gain", "min_gain"):
            assert np.array_equal(got[2][name].view(np.uint32), clean[2][name].view(np.uint32))


def test_on_a_busy_side_stream(pkg, dev):
    """Batches with a set_rx between them on a side stream that is still busy with other work, nothing synchronised:
    the input arrives on that stream behind the filler, the outputs keep their canaries while it runs, and the bytes
    are those of the clean run on the null stream."""
    import torch
    K, Q, R, limit = 37, 2, 37, (48, MR.CEIL, MR.REL)
    TT = pkg.mixer_tile_outputs()
    cuts = [TT - 1, 1, 2 * TT + 5, 700]
    n = sum(cuts)
    g = MR.interleaved_gains(K, Q)
    changes = {1: MR.one_shot_changes(K, Q, g), 3: [(0, g[1]), (2, g[0])]}
    x = series(K)[:, :n]

    def go(m, a, st, bufs, sync):
        views, off = [], 0
        for i, b in enumerate(cuts):
            for j, gg in changes.get(i, ()):
                m.set_rx(j, gg)
            views.append(m.process(a[:, off:off + b], out_f32=bufs[i][0].t, out_i16=bufs[i][1].t, stream=st))
            off += b
            if sync:
                torch.cuda.synchronize()
        return views

    def allocate():
        bufs, before = [], 0
        for b in cuts:
            c = MR.outputs(limit[0], before, b)
            bufs.append((S.Buf((Q, c), torch.float32, dev), S.Buf((c, Q), torch.int16, dev)))
            before += b
        return bufs

    real = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    live = torch.from_numpy(np.ascontiguousarray(x[:, ::-1])).to(dev)
    cb, bb = allocate(), allocate()
    side = S.side_streams(dev)[0]
    mc, mb = pkg.Mixer(g, R, limit=limit), pkg.Mixer(g, R, limit=limit)
    torch.cuda.synchronize()
    clean = [[S.host(v) for v in vs] for vs in go(mc, real, 0, cb, True)]
    clean_read = mc.read()
    gate = S.occupy(side, dev, 100.0)
    with torch.cuda.stream(side):
        live.copy_(real, non_blocking=True)
    views = go(mb, live, side.cuda_stream, bb, False)
    closed = not gate.query()
    intact = all(b.untouched() for pair in bb for b in pair if b.raw.numel())
    still = not gate.query()
    read = mb.read(stream=side.cuda_stream)
    got = [[S.host(v) for v in vs] for vs in views]
    side.synchronize()
    print(f"mixer on a side stream: host ran ahead: {'yes' if closed else 'no'}")
    if still:
        assert intact, "an output was written while the side stream was still busy: a launch or copy on another stream"
    S.assert_same(got, clean, "mixer, busy against clean")
    for name in MR.STATUS.names:
        assert S.same_bits(read[name], clean_read[name])
    mc.close()
    mb.close()


def test_end_to_end(pkg, O, dev):
    """Two carriers keyed at different times through Channelizer -> Tuner -> Demod (AM) -> Squelch (GATE) -> Audio ->
    Mixer: stereo, one receiver per side, the limiter on.  The output equals the reference on the downloaded Audio
    output, and each side is +0 wherever its receiver's audio is +0 (squelch closed), the limiter's delay of one block
    taken off: the outputs are the first count samples."""
    import torch
    import demod_ref as DR
    c = DR.CHAIN
    ns, amp, noise = 1 << 19, 0.4, 0.003
    i = np.arange(ns, dtype=np.int64)
    words = [DR.CARRIER_WORD, (700 << 22) + 999]
    keyed = [(ns // 8, ns // 2), (ns // 2, 7 * ns // 8)]
    rng = np.random.default_rng(78)
    x = noise * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns))
    for w, (on, off) in zip(words, keyed):
        ph = 2.0 * np.pi * ((w * i) & DR.MASK).astype(np.float64) / 2.0 ** 32
        x = x + amp * ((i >= on) & (i < off)) * (1.0 + 0.5 * np.cos(2 * np.pi * i / 40000.0)) * np.exp(1j * ph)
    sig = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    packed = pkg.pack24_f32(torch.from_numpy(sig).to(dev))
    ch = pkg.Channelizer(c["nchan"], pkg.tuner_prototype(c["nchan"], c["proto_taps"]), c["hop"])
    t = pkg.Tuner(ch, words, pkg.tuner_lowpass(c["ntaps"], c["decim"]), c["decim"])
    d = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)] * 2)
    s = pkg.Squelch([(100.0, 30.0, pkg.PDDC_SQL_GATE | pkg.PDDC_SQL_RELATIVE)] * 2, 8, 2, 2, 16, up=SR.UP)
    au = pkg.Audio(2, 3, 1, phases=32, taps=8)
    z = t.process(ch.process(packed))
    gated = s.process(z, d.process(z))[0]
    aud = au.process(gated)
    an = aud.cpu().numpy()
    n = an.shape[1]
    # the ceiling at half of the loudest mixed sample, so that the limiter has to act
    Lb, gains = 16, [[1.5, 0.0], [0.0, 1.5]]
    ceil = float(F32(0.75) * np.abs(an).max())
    assert ceil > 0
    m = pkg.Mixer(gains, 8, limit=(Lb, ceil, 0.25))
    fo, io = m.process(aud, i16=True)
    assert fo.shape == (2, MR.outputs(Lb, 0, n)) and fo.shape[1] > 600
    ref = MR.MixerRef(gains, 8, (Lb, ceil, 0.25), chunk=pkg.mixer_chunk())
    wf, wi = ref.process(an)
    same((fo.cpu().numpy(), io.cpu().numpy(), m.read()), (wf, wi, ref.read()), "chain")
    got = fo.cpu().numpy()
    cnt = got.shape[1]
    for side in range(2):
        closed = MR.bits(an[side, :cnt]) == 0
        assert closed.sum() > 100 and (~closed).sum() > 100
        assert not MR.bits(got[side])[closed].any() and not io.cpu().numpy()[closed, side].any()
        assert np.count_nonzero(got[side][~closed]) > 0.9 * (~closed).sum()
    assert np.abs(got).max() <= ceil and ref.read()["min_gain"].max() < 1
    for obj in (m, au, s, d, t, ch):
        obj.close()
