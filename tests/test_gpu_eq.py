"""Eq (pddc_eq_*, k_eq) on the GPU against the numpy float64 reference (tests/eq_ref.py) fed the very float32 arrays
uploaded.  Every comparison is by int32 / int64 views and exact equality: there are no tolerances.  The inputs'
preconditions (every section count in every place of a wave's receivers, a row of zeros, a row that goes silent, a row of
denormals, finite outputs) are asserted in tests/test_eq_cpu.py."""
import types

import numpy as np
import pytest

import eq_ref as ER
import nonfinite as NF
import stream_order as SO

pytestmark = pytest.mark.gpu
K0, N0, FEW = ER.K0, ER.N0, ER.FEW


def run(pkg, x, rx, S, cuts=None, before=None):
    """all of x (torch [K, n]) through a fresh Eq in the given batches -> numpy (out, state); before(i, s) is called ahead
    of batch i"""
    import torch
    s = pkg.Eq(rx, S)
    outs, off = [], 0
    for i, b in enumerate(cuts or [x.shape[1]]):
        if before:
            before(i, s)
        o = s.process(x[:, off:off + b])
        assert o.shape == (len(rx), b)
        outs.append(o)
        off += b
    assert off == x.shape[1]
    st = s.read_state()
    s.close()
    return torch.cat(outs, dim=1).cpu().numpy(), st


def same(got, want, what=""):
    for name, g, w in zip(("out", "state"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(ER.bits(g), ER.bits(w)), (what, name, np.argwhere(ER.bits(g) != ER.bits(w))[:4].tolist())


def rows_of(r, sl):
    return tuple(v[sl] for v in r)


def ref_events(x, rx, S, cuts, changes):
    """the reference through the batches `cuts` with changes[i] = [(j, sections, flags), ..] ahead of batch i"""
    ref = ER.EqRef(rx, S)
    outs, off = [], 0
    for i, b in enumerate(cuts):
        for c in changes.get(i, ()):
            ref.set_rx(*c)
        outs.append(ref.process(x[:, off:off + b]))
        off += b
    return np.concatenate(outs, axis=1), ref.state.copy()


@pytest.fixture(scope="module")
def series(dev):
    """the input, its upload, and the reference at S = 8 for all K0 receivers: computed once, never changed"""
    import torch
    x, rx = ER.gpu_series(), ER.interleaved_rx(K0, 8)
    out, st, _ = ER.eq_ref(x, rx, 8)
    assert np.isfinite(out).all()
    return types.SimpleNamespace(x=x, rx=rx, xd=torch.from_numpy(x).to(dev), want=(out, st))


@pytest.mark.parametrize("S", (8, 1, 2, 4))
def test_bits_against_the_reference(pkg, dev, series, S):
    """K = 1024 at S = 8 and K = 37 at S = 1, 2, 4, n = 3000; section counts 0 .. S and the pool's designs interleaved
    receiver by receiver, a row of zeros, a row that goes silent after 1000 samples, a row of float32 denormals: out and
    read_state() equal eq_ref's."""
    if S == 8:
        same(run(pkg, series.xd, series.rx, 8), series.want, "S 8")
        return
    x, rx = series.x[:FEW], ER.interleaved_rx(FEW, S)
    got = run(pkg, series.xd[:FEW].contiguous(), rx, S)
    same(got, ER.eq_ref(x, rx, S)[:2], f"S {S}")
    assert not ER.bits(got[0][ER.ZERO_ROW]).any()


def test_bits_against_the_cut_and_the_company(pkg, dev, series):
    """One batch against batches of 0, 1, 2, S - 1, S, S + 1, TT - 1, TT, TT + 1, 3 TT + 5 and the rest for K = 1024 at
    S = 8; the receiver order reversed (with the cuts reversed); K = 7 and K = 1 slices against the same rows among the
    1024."""
    S, TT = 8, pkg.eq_tile_outputs()
    cuts = [0, 1, 2, S - 1, S, S + 1, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(N0 - sum(cuts))
    assert cuts[-1] > 0
    x, rx = series.xd, series.rx
    one = run(pkg, x, rx, S)
    same(one, series.want, "one batch")
    same(run(pkg, x, rx, S, cuts), one, "cut")
    rev = run(pkg, x.flip(0).contiguous(), rx[::-1], S, cuts[::-1])
    same(rev, rows_of(one, slice(None, None, -1)), "reversed")
    few = run(pkg, x[500:507].contiguous(), rx[500:507], S, cuts)
    same(few, rows_of(one, slice(500, 507)), "K 7")
    for j in (0, 1, 7, 8, ER.ZERO_ROW, ER.DENORMAL_ROW, 63, 64, 1023):
        alone = run(pkg, x[j:j + 1].contiguous(), rx[j:j + 1], S, cuts)
        same(alone, rows_of(one, slice(j, j + 1)), f"alone {j}")


def test_the_bits_do_not_depend_on_the_objects_sections(pkg, dev, series):
    """The same receivers (0 .. 2 sections each) through an S = 2, an S = 4 and an S = 8 object, K = 37 and K = 1024: the
    same outputs and the same states; the states of the sections an object has beyond a receiver's are 0."""
    for K in (FEW, K0):
        rx = ER.interleaved_rx(K, 2)
        x = series.xd[:K].contiguous()
        two = run(pkg, x, rx, 2)
        if K == FEW:
            same(two, ER.eq_ref(series.x[:K], rx, 2)[:2], "S 2 against the reference")
        for S in (4, 8):
            out, st = run(pkg, x, rx, S)
            same((out, np.ascontiguousarray(st[:, :2])), two, f"K {K}: S {S} against S 2")
            assert not ER.bits(st[:, 2:]).any()


@pytest.mark.parametrize("cuts", ([1], [3], [1, 3, 2, 7, 1, 1, 8, 5]))
def test_launches_shorter_than_the_cascade(pkg, dev, series, cuts):
    """Whole launches with n < S at S = 8: n = 1 and n = 3 alone, and a run of launches of 1 .. 8 samples -- the smallest
    shapes at which the fill and the drain of the skew can go wrong."""
    n = sum(cuts)
    x = series.xd[:, :n].contiguous()
    want = ER.eq_ref(series.x[:, :n], series.rx, 8)[:2]
    same(run(pkg, x, series.rx, 8, cuts), want, cuts)


def test_strides_and_in_place(pkg, dev, series):
    """The input is a view with row stride > n, out has capacity > n and its padding keeps its fill value; out is a gives
    the bits of out of place, and the padding of a keeps its fill."""
    import torch
    K, n = 13, 700
    rows = slice(64, 64 + K)
    for S in (1, 4, 8):
        rx = ER.interleaved_rx(K, S, first=64)
        xin = np.ascontiguousarray(series.x[rows, :n])
        want = ER.eq_ref(xin, rx, S)[:2]
        abuf = torch.full((K, n + 5), 3.0, dtype=torch.float32, device=dev)
        av = abuf[:, :n]
        av.copy_(series.xd[rows, :n])
        assert av.stride(0) == n + 5
        s = pkg.Eq(rx, S)
        obuf = torch.full((K, n + 11), 7.0, dtype=torch.float32, device=dev)
        out = s.process(av, out=obuf)
        assert out.data_ptr() == obuf.data_ptr() and out.shape == (K, n)
        same((out.cpu().numpy(), s.read_state()), want, f"strided, S {S}")
        assert bool((obuf[:, n:] == 7.0).all()) and bool((abuf[:, n:] == 3.0).all())
        assert np.array_equal(ER.bits(av.cpu().numpy()), ER.bits(xin))
        s.reset()
        assert not ER.bits(s.read_state()).any()
        out2 = s.process(av, out=av)                           # in place
        assert out2.data_ptr() == abuf.data_ptr()
        same((out2.cpu().numpy(), s.read_state()), want, f"in place, S {S}")
        assert bool((abuf[:, n:] == 3.0).all())
        s.close()


def test_set_rx_between_batches_keeps_the_states(pkg, dev, series):
    """A coefficient change, a cascade that shrinks 3 -> 1 and grows 1 -> 3 again (the regrown sections start from rest),
    a receiver switched off and on, and restarts, against the reference's same events, bit for bit; the receivers that
    were not touched have the bits of a run without the changes; a bad call is refused and changes nothing."""
    K, S = 12, 4
    cuts = [700, 1, 0, 999, 1300]
    rows = slice(100, 100 + K)
    rx = ER.interleaved_rx(K, S, first=100)
    p = ER.pool()
    rx[2], rx[6] = [p[0], p[1], p[2]], [p[4], p[5]]
    x = series.xd[rows].contiguous()
    R = ER.RESTART
    changes = {1: [(2, [p[0]], 0), (3, [p[6], p[7]], 0), (4, rx[4], R), (6, [], 0)],
               3: [(2, [p[0], p[1], p[2]], 0), (7, [p[3]], R), (7, [p[8]], 0), (6, [p[4], p[5]], 0)],     # 7: the restart stays asked for
               4: [(0, [p[9], p[10], p[1], p[2]], 0), (3, [p[6], p[7]], R), (9, [p[2]], 0)]}
    nan = float("nan")
    bad = ((1, [p[0]], 2), (1, [p[0]], 0x80000000), (1, [p[0]] * 5, 0), (1, [(1.0, 0.0, 0.0, 2.0, 0.5)], 0), (1, [(1.0, 0.0, 0.0, 0.0, 1.0)], 0),
           (1, [p[0], (nan, 0.0, 0.0, 0.0, 0.0)], 0), (1, [(1.0, 0.0, 0.0, 0.0, nan)], 0), (K, [p[0]], 0), (-1, [p[0]], 0))

    def before(i, s):
        for c in changes.get(i, ()):
            s.set_rx(*c)
        for b in bad:
            with pytest.raises(pkg.PddcError) as e:
                s.set_rx(*b)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, x, rx, S, cuts, before)
    clean = run(pkg, x, rx, S, cuts)
    touched = {c[0] for cs in changes.values() for c in cs}
    assert 1 not in touched
    for j in range(K):
        if j not in touched:
            same(rows_of(got, slice(j, j + 1)), rows_of(clean, slice(j, j + 1)), f"untouched {j}")
    same(got, ref_events(series.x[rows], rx, S, cuts, changes), "set_rx")
    assert all(not np.array_equal(got[0][j], clean[0][j]) for j in touched)


def test_a_refused_process_changes_nothing(pkg, dev, series):
    """process calls refused for capacity (each stride), for a misaligned or missing pointer and for a partial overlap of
    out with a, between the batches, a restart pending: the next correct call's bits are those of an object that never
    saw them.  reset starts the series again with the first run's bits."""
    import torch
    K, S = 9, 2
    cuts = [700, 300, 2000]
    rows = slice(300, 300 + K)
    rx = ER.interleaved_rx(K, S, first=300)
    x = series.xd[rows].contiguous()
    changes = {1: [(3, rx[3] or [ER.pool()[0]], ER.RESTART)]}
    want = ref_events(series.x[rows], rx, S, cuts, changes)
    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, s):
        for c in changes.get(i, ()):
            s.set_rx(*c)
        b = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            s.process(x[:, :b], out=torch.empty((K, b - 1), dtype=torch.float32, device=dev))
        assert e.value.code == ECAP
        o = torch.empty((K, b), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(ap=x.data_ptr(), n=b, as_=N0, op=o.data_ptr(), os_=b):
            return L.pddc_eq_process(s._h, ap, n, as_, op, os_, stream)

        assert call(as_=b - 1) == ECAP and call(os_=b - 1) == ECAP
        assert call(ap=x.data_ptr() + 2) == EINVAL and call(op=o.data_ptr() + 1) == EINVAL
        assert call(ap=None) == EINVAL and call(op=None) == EINVAL
        assert call(op=x.data_ptr() + 4, os_=N0) == EINVAL                                       # out over a, shifted
        assert call(op=x.data_ptr(), os_=N0 - 1) == EINVAL                                       # out is a, another stride
        assert call(op=x.data_ptr() + 4 * (N0 * (K - 1) + b - 1), os_=b) == EINVAL               # out's first value is a's last
        assert call(ap=None, n=0, as_=0, op=None, os_=0) == pkg.PDDC_OK
        assert L.pddc_eq_read_state(s._h, None, stream) == EINVAL

    got = run(pkg, x, rx, S, cuts, disturb)
    same(got, want, "refused")
    clean = ER.eq_ref(series.x[rows], rx, S)[:2]
    s = pkg.Eq(rx, S)                                           # reset starts the series again
    assert not ER.bits(s.read_state()).any()
    first = s.process(x).clone()
    st1 = s.read_state()
    s.reset()
    assert not ER.bits(s.read_state()).any()
    second = s.process(x)
    same((first.cpu().numpy(), st1), clean, "first")
    same((second.cpu().numpy(), s.read_state()), clean, "after reset")
    s.close()


def test_off_rows_are_their_input_words(pkg, dev, series):
    """Receivers without sections beside receivers with: -0.0, denormals, infinities and NaNs with payloads (a quiet and a
    signalling one, of either sign) come out word for word, at S = 1 and S = 8 and across a tile seam and a batch cut."""
    import torch
    K, n = 19, 600
    odd = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F812345, 0xFF800001, 0x7F800000, 0xFF800000, 0x7FFFFFFF],
                   np.uint32)
    x = np.ascontiguousarray(series.x[:K, :n]).copy()
    w = x.view(np.uint32)
    for j in range(K):
        for c in (0, 7, 255, 256, 300, n - 1):
            w[j, c] = odd[(j + c) % len(odd)]
        w[j, 100:100 + len(odd)] = odd
    for S in (1, 8):
        rx = [[] if j % 2 == 0 else ER.interleaved_rx(K, S)[j] for j in range(K)]
        off = [j for j in range(K) if not rx[j]]
        assert len(off) >= K // 2
        xd = torch.from_numpy(x).to(dev)
        for cuts in (None, [255, 2, n - 257]):
            out, st = run(pkg, xd, rx, S, cuts)
            assert np.array_equal(out.view(np.uint32)[off], w[off]), (S, cuts)
            assert not ER.bits(st[off]).any()


def nan_same64(got, want, what):
    """states: NaN exactly where the reference has NaN, every other value by its bits"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN places", np.argwhere(gn != wn)[:4].tolist())
    bad = (ER.bits(got) != ER.bits(want)) & ~wn
    assert not bad.any(), (what, "bits", np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("name", sorted(NF.POISON))
def test_non_finite_samples_stay_in_their_row(pkg, dev, series, name):
    """A NaN, +inf or -inf planted in four rows (the first and the last, and two that share a wave with clean ones) at each
    of nonfinite.placements' columns in turn, the batches cut by nonfinite.cuts_for: the poisoned rows equal the
    reference's (NaN where it has NaN, the same bits elsewhere), outputs and states; they are not finite from the sample
    on and stay so; every other row has the bits of the clean run.  After set_rx with RESTART the rows equal those of
    receivers restarted there."""
    import torch
    K, S, TT = 2 * ER.GROUP + 3, 4, pkg.eq_tile_outputs()
    n, n2 = 3 * TT + 40, 300
    bad_rows = NF.poisoned_rows(K, ER.GROUP)
    rx = ER.interleaved_rx(K, S, first=200)
    p = ER.pool()
    for j in bad_rows:
        if not rx[j]:
            rx[j] = [p[1], p[3]]
    x = np.ascontiguousarray(series.x[200:200 + K, :n + n2])
    assert np.isfinite(x).all()
    cuts = NF.cuts_for(TT, n) + [n2]
    clean = run(pkg, torch.from_numpy(x).to(dev), rx, S, cuts)
    same(clean, ER.eq_ref(x, rx, S)[:2], "clean")
    clean_rows = [j for j in range(K) if j not in bad_rows]
    changes = {len(cuts) - 1: [(j, rx[j], ER.RESTART) for j in bad_rows]}

    def before(i, s):
        for c in changes.get(i, ()):
            s.set_rx(*c)

    for col in NF.placements(TT, 1, n):
        xp = NF.plant(x, bad_rows, col, NF.POISON[name])
        got = run(pkg, torch.from_numpy(xp).to(dev), rx, S, cuts, before)
        what = (name, col)
        NF.clean_rows_identical(got[0], clean[0], clean_rows, what)
        assert np.array_equal(ER.bits(got[1][clean_rows]), ER.bits(clean[1][clean_rows])), what
        want = ref_events(xp, rx, S, cuts, changes)
        NF.same_or_both_nan(got[0][bad_rows], want[0][bad_rows], what)
        nan_same64(got[1][bad_rows], want[1][bad_rows], what)
        assert not np.isfinite(got[0][bad_rows][:, col:n]).any(), what          # sticky
        # restarted on the good samples: a fresh receiver's bits
        fresh = ER.eq_ref(x[bad_rows, n:], [rx[j] for j in bad_rows], S)[:2]
        same((np.ascontiguousarray(got[0][bad_rows][:, n:]), got[1][bad_rows]), fresh, (what, "restarted"))


class EqObj(SO.Obj):
    """the equaliser for tests/stream_order.py's harness: K = 37 receivers at S = 4, out with capacity > n"""
    id, tile, sections, pad = "eq", "eq_tile_outputs", 4, 6

    def __init__(self):
        self.rx = ER.interleaved_rx(self.nrx, self.sections)

    def inputs(self, env, n):
        x = ER.gpu_series()
        assert n <= x.shape[1]
        return (np.ascontiguousarray(x[:self.nrx, :n]),)

    def make(self, env):
        return env.pkg.Eq(self.rx, self.sections)

    def out_specs(self, env, plan, b):
        import torch
        return [((self.nrx, b + self.pad), torch.float32)]

    process = SO.BlankerObj.process

    def changed(self, j, k):
        p = ER.pool()
        return [p[(j + k + s) % len(p)] for s in range((j + k) % (self.sections + 1))]

    def change(self, obj, k):
        for j in SO.rows_of(k, self.nrx):
            obj.set_rx(j, self.changed(j, k), ER.RESTART if k == 1 else 0)

    def read(self, obj, st):
        return (obj.read_state(stream=st),)


def test_stream_order(pkg, dev):
    """On a side stream kept busy behind a gate (tests/stream_order.py), the input copied over a scrambled one behind the
    gate: three batches (TT - 1, 1, 2 TT + 5) with a set_rx on several receivers in front of each -- the second with
    RESTART -- and read_state(), nothing synchronised in between, give the bits of the run that synchronised after every
    call, which are the reference's.  While the gate is closed no output is touched, and the padding behind the outputs
    keeps its canary throughout."""
    import torch
    env = types.SimpleNamespace(pkg=pkg, dev=dev)
    ad = EqObj()
    sizes = ad.sizes(env)[1]
    steps = [s for k, b in enumerate(sizes) for s in (("change", k), ("batch", b))]
    xs = ad.inputs(env, sum(sizes))
    side = SO.side_streams(dev)[0]

    def go(st, live, sync_each):
        bufs = SO.allocate(ad, env, steps)
        obj = ad.make(env)
        torch.cuda.synchronize()
        return obj, bufs, SO.Runner(ad, env, obj, live, st, sync_each=sync_each)

    obj, cbufs, r = go(0, SO.upload(xs, dev), True)
    clean = [[SO.host(v) for v in vs] for vs in r.go(steps, cbufs)]
    clean_state = obj.read_state()
    obj.close()
    # the clean run is the reference's
    changes = {k: [(j, ad.changed(j, k), ER.RESTART if k == 1 else 0) for j in SO.rows_of(k, ad.nrx)] for k in range(len(sizes))}
    want = ref_events(xs[0], ad.rx, ad.sections, sizes, changes)
    same((np.concatenate([c[0] for c in clean if c], axis=1), clean_state), want, "clean against the reference")

    real, live = SO.upload(xs, dev), SO.upload(SO.scrambled(ad, xs, 0), dev)
    obj, bufs, r = go(side.cuda_stream, live, False)
    gate = SO.occupy(side, dev, 100.0)
    with torch.cuda.stream(side):
        for l, x in zip(live, real):
            l.copy_(x, non_blocking=True)
    views = r.go(steps, bufs)
    ahead = not gate.query()
    intact = all(b.untouched() for bl in bufs if bl for b in bl)
    still = not gate.query()
    state = obj.read_state(stream=side.cuda_stream)             # waits for the side stream
    got = [[SO.host(v) for v in vs] for vs in views]
    side.synchronize()
    print(f"stream order eq: host ran ahead: {'yes' if ahead else 'no'}")
    if still:
        assert intact, "an output was written while the side stream was still busy: a launch or copy on another stream"
    SO.assert_same(got, clean, "eq, busy against clean")
    assert np.array_equal(ER.bits(state), ER.bits(clean_state))
    for (kind, *_), bl in zip(steps, bufs):
        if kind == "batch":
            pad = bl[0].raw.view(torch.float32).view(bl[0].shape)[:, -ad.pad:].contiguous().view(torch.uint8)
            assert bool((pad == SO.CANARY).all()), "the padding behind an output was written"
    obj.close()
