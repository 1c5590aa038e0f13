"""The mixer without a GPU: the host arithmetic and the argument checks of the C ABI, the reference's own properties
(tests/mixer_ref.py), and the preconditions the GPU tests' inputs have to meet."""
import ctypes as C

import numpy as np
import pytest

import mixer_ref as MR
import squelch_ref as SR

F32 = np.float32


def test_outputs_is_host_arithmetic(pkg):
    L = pkg.ddc_lib()
    befores = [0, 1, 7, 8, 47, 48, 95, 96, 999, 4095, 4096, 8191, 8192, (1 << 40) - 1, 1 << 40, (1 << 40) + 12345]
    for Lb in (8, 9, 48, 256, 1000, 4095, 4096):
        for before in befores:
            for n in sorted({0, 1, Lb - 1, Lb, Lb + 1, 2 * Lb - 1, 2 * Lb, 3 * Lb + 5, 3000, 1 << 20}):
                assert pkg.mixer_outputs(Lb, before, n) == MR.outputs(Lb, before, n), (Lb, before, n)
        assert pkg.mixer_outputs(Lb, 0, Lb) == 0 and pkg.mixer_outputs(Lb, 0, 2 * Lb) == Lb
    for Lb in (0, -1, 7, 4097, 1 << 20, -(1 << 31)):
        assert pkg.mixer_outputs(Lb, 0, 1 << 20) == 0 and L.pddc_mixer_outputs(Lb, 5, 100000) == 0
    assert pkg.mixer_tile_outputs() >= 1
    Cc = pkg.mixer_chunk()
    assert Cc >= 1 and Cc & (Cc - 1) == 0
    assert pkg.PDDC_MIX_LIMIT == 1
    assert pkg.mixer_status_dtype() == MR.STATUS and MR.STATUS.itemsize == 12


def test_pan_is_constant_power(pkg):
    for db in (-12.0, 0.0, 6.0):
        g = 10.0 ** (db / 20.0)
        for pan in (-1.0, -0.5, 0.0, 0.25, 1.0):
            l, r = pkg.mixer_pan(db, pan)
            assert abs(l * l + r * r - g * g) <= 1e-6 * g * g and l >= 0 and r >= 0
    assert pkg.mixer_pan(0.0, -1.0)[0] == 1.0 and abs(pkg.mixer_pan(0.0, -1.0)[1]) < 1e-7
    l, r = pkg.mixer_pan(0.0, 0.0)
    assert l == r == float(F32(np.sqrt(0.5)))
    with pytest.raises(pkg.PddcError):
        pkg.mixer_pan(0.0, 1.5)


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    nan, inf = float("nan"), float("inf")

    def create(gains=((1.0, 0.5), (0.0, -0.0), (-2.0, 1e-3)), nrx=None, params=(2, 37, 1, 48, 1.0, 0.5, 32767.0),
               null_gains=False, null_params=False):
        flat = [v for row in gains for v in row]
        arr = (C.c_float * max(len(flat), 1))(*flat)
        par = pkg.MixerParams(*params)
        h = C.c_void_p()
        rc = L.pddc_mixer_create(C.byref(h), 0, len(gains) if nrx is None else nrx, None if null_params else C.byref(par),
                                 None if null_gains else arr)
        if rc == 0:
            L.pddc_mixer_destroy(h)
        return rc

    ok = (2, 37, 1, 48, 1.0, 0.5, 32767.0)
    par = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("nbus", "ramp", "flags", "block", "ceil", "rel", "scale"), ok))
    bad = [dict(nrx=0), dict(nrx=-1), dict(gains=[(1.0, 0.5)] * 1025), dict(null_gains=True), dict(null_params=True),
           dict(params=par(nbus=0)), dict(params=par(nbus=9)), dict(params=par(nbus=-2)),
           dict(params=par(ramp=0)), dict(params=par(ramp=65537)), dict(params=par(ramp=-37)),
           dict(params=par(flags=2)), dict(params=par(flags=0x80000001)),
           dict(params=par(block=7)), dict(params=par(block=4097)), dict(params=par(block=0)), dict(params=par(block=-48)),
           dict(params=par(ceil=0.0)), dict(params=par(ceil=-1.0)), dict(params=par(ceil=nan)), dict(params=par(ceil=inf)),
           dict(params=par(rel=0.0)), dict(params=par(rel=1.0000001)), dict(params=par(rel=-0.5)), dict(params=par(rel=nan)),
           dict(params=par(rel=inf)),
           dict(params=par(scale=0.0)), dict(params=par(scale=nan)), dict(params=par(scale=inf)), dict(params=par(scale=-1.0)),
           dict(gains=[(1.0, nan)]), dict(gains=[(1.0, 0.5), (inf, 0.5)]), dict(gains=[(1.0, 0.5), (0.5, -inf)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    one = (C.c_float * 2)(1.0, 0.5)
    p = pkg.MixerParams(*ok)
    assert L.pddc_mixer_create(None, 0, 1, C.byref(p), one) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        # without the flag the limiter's parameters are not looked at
        assert create(params=par(flags=0, block=0, ceil=nan, rel=nan)) == pkg.PDDC_ENODEV
        assert create(gains=[(3.0e38,) * 8] * 1024, params=(8, 65536, 1, 4096, 3.0e38, 1.0, 3.0e38)) == pkg.PDDC_ENODEV
        assert create(gains=[(-0.0,)], params=(1, 1, 1, 8, 1e-30, 1e-30, 1.0)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Mixer([[1.0, 0.0], [0.0, 1.0]], 37, limit=(48, 1.0, 0.5))
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(gains=[[1.0, nan]], ramp=37), dict(gains=[[1.0, 0.5]], ramp=1 << 40),
               dict(gains=[[1.0, 0.5]], ramp=37, limit=(1 << 40, 1.0, 0.5)), dict(gains=[[1.0] * 9], ramp=37),
               dict(gains=[1.0, 0.5], ramp=37)):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Mixer(**kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    n = C.c_size_t()
    assert L.pddc_mixer_process(None, None, 8, 8, None, 8, None, 8, C.byref(n), None) == pkg.PDDC_EINVAL
    assert L.pddc_mixer_set_rx(None, 0, one) == pkg.PDDC_EINVAL
    assert L.pddc_mixer_next_outputs(None, 8, C.byref(n)) == pkg.PDDC_EINVAL
    assert L.pddc_mixer_read(None, None, 0, None) == pkg.PDDC_EINVAL
    assert L.pddc_mixer_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_mixer_destroy(None) == 0


def test_reference_fma_is_one_rounding():
    """The case the double sum gets wrong: a b + c lies just below the middle of two float32 values, the double sum
    exactly on it, and the tie goes to the even neighbour, the wrong one."""
    a = F32(2.0 ** -14) * (F32(1) + F32(2.0 ** -23))
    b = F32(1) - F32(2.0 ** -23)
    c = F32(2.0 ** 10 + 2.0 ** -13)
    assert (np.float64(a) * np.float64(b) + np.float64(c)).astype(F32) != c           # what a double sum gives
    assert MR.fma(a, b, c) == c and MR.fma(-a, b, -c) == -c
    assert MR.fma(a, F32(1) + F32(2.0 ** -23), c) == np.nextafter(c, F32(np.inf))      # just above the middle
    rng = np.random.default_rng(1)
    x, y, z = (rng.standard_normal(100000).astype(F32) for _ in range(3))
    from fractions import Fraction
    got = MR.fma(x[:300], y[:300], z[:300])
    for i in range(300):                                                              # against exact rationals
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo, hi = sorted((float(got[i]), float(np.nextafter(got[i], F32(np.inf) if exact > Fraction(float(got[i])) else F32(-np.inf)))))
        assert abs(exact - Fraction(float(got[i]))) <= (Fraction(hi) - Fraction(lo)) / 2
    assert np.isnan(MR.fma(F32(np.nan), F32(1), F32(1))) and MR.fma(F32(np.inf), F32(1), F32(1)) == np.inf
    assert np.isnan(MR.fma(F32(0), F32(np.inf), F32(1)))


def same(a, b):
    return all(np.array_equal(MR.bits(x), MR.bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def small():
    K, Q = 70, 3
    g = MR.interleaved_gains(K, Q)
    return K, Q, g, SR.audio_series(K, 1500, 3), MR.one_shot_changes(K, Q, g)


def test_reference_streaming_equals_one_shot(small):
    """arbitrary cuts, batches of 0 and of fewer than Lb samples included, ramps and receivers going silent under way;
    the status too"""
    K, Q, g, a, ch = small
    for R, limit in ((1, None), (37, (8, MR.CEIL, MR.REL)), (400, (48, MR.CEIL, MR.REL)), (4000, (1000, MR.CEIL, MR.REL))):
        out, p, st, one = MR.mixer_ref(a, g, R, limit, changes=ch)
        assert out.shape == (Q, MR.outputs(limit[0], 0, 1500) if limit else 1500) and p.shape == out.shape[::-1]
        cuts = [0, 1, 2, 0, 47, 48, 63, 65, 1, 300, 0]
        cuts.append(1500 - sum(cuts))
        r = MR.MixerRef(g, R, limit)
        for j, gg in ch:
            r.set_rx(j, gg)
        assert same(MR.run_cuts(r, a, cuts), (out, p))
        got = r.read()
        for name in MR.STATUS.names:
            assert np.array_equal(got[name].view(np.uint32), st[name].view(np.uint32)), name


def test_reference_limiter_properties(small):
    """|out| <= ceil exactly, the outputs come one block late, the gain never rises by more than rel of what is missing
    and is 1 again after a quiet stretch; +-Inf in y gives gain 0 and the sample -ceil, NaN changes no gain."""
    K, Q, g, a, ch = small
    y = MR.mixer_ref(a, g, 37)[0]
    ceil, rel = F32(MR.CEIL), F32(MR.REL)
    for Lb in (8, 48):
        lim = MR.LimiterRef(Q, Lb, ceil, rel)
        out = lim.process(y)
        assert out.shape == (Q, Lb * (1500 // Lb - 1)) and np.abs(out).max() <= ceil
        G = np.array(lim.gains)
        assert (G < 1).any() and (G == 1).any() and (G > 0).all()
        up = G[1:] - G[:-1]
        assert (up <= rel * (1 - G[:-1]) + 1e-6).all()
    quiet = np.concatenate([y[:, :480], np.zeros((Q, 48 * 40), F32)], axis=1)
    lim = MR.LimiterRef(Q, 48, ceil, rel)
    lim.process(quiet)
    assert (lim.E == 1).all() and (lim.min_gain < 1).all()
    for bad, val in ((np.inf, -ceil), (-np.inf, -ceil), (np.nan, -ceil)):
        z = y.copy()
        z[1, 700] = bad
        a_, b_ = MR.LimiterRef(Q, 48, ceil, rel), MR.LimiterRef(Q, 48, ceil, rel)
        o1, o0 = a_.process(z), b_.process(y)
        assert o1[1, 700] == val
        if np.isnan(bad):
            peak_there = abs(y[1, 700]) == np.abs(y[1, 672:720]).max()
            diff = np.flatnonzero(MR.bits(o1[1]) != MR.bits(o0[1]))
            assert peak_there or diff.tolist() == [700]
        else:
            k = 700 // 48
            assert np.array(a_.gains)[k - 1, 1] == 0 and np.array(a_.gains)[k, 1] == 0 and np.array(a_.gains)[k + 1, 1] == rel
            assert np.array_equal(MR.bits(o1[[0, 2]]), MR.bits(o0[[0, 2]])) and (a_.E == b_.E)[[0, 2]].all()


def test_reference_ramp_and_silence():
    """A ramp's first gain is fmaf(to - from, 1 / R, from) and its R-th is `to` itself; two set_rx before a batch count
    as one; a change mid-ramp starts from the gain of the last sample; a silent receiver with NaN changes nothing, and
    it is not in the tree: the receivers behind it move up."""
    R, n = 8, 40
    a = SR.audio_series(3, n, 9)
    a[:, 0] = 1.0
    a[1] = 1.0
    g = np.array([[0.0], [0.5], [0.0]], F32)
    r = MR.MixerRef(g, R)
    r.set_rx(1, [4.0])
    r.set_rx(1, [2.0])                                        # the later wins, from stays 0.5
    y = r.process(a)[0][0]
    invR = F32(1) / F32(R)
    want = [MR.fma(F32(1.5), F32(c) * invR, F32(0.5)) for c in range(1, R)] + [F32(2.0)] * (n - R + 1)
    assert np.array_equal(MR.bits(y), MR.bits(np.array(want, F32)))
    assert y[0] == F32(0.5) + F32(1.5) / 8 and y[R - 1] == 2
    r = MR.MixerRef(g, R)
    r.set_rx(1, [2.0])
    y1 = r.process(a[:, :3])[0][0]
    r.set_rx(1, [0.0])                                        # mid-ramp, c = 3: from = the third gain
    y2 = r.process(a[:, 3:])[0][0]
    assert y1[2] == r.frm[1, 0] == F32(0.5) + F32(1.5) * F32(3) * invR and r.midramp_sets == 1
    assert y2[R - 2] != 0 and not MR.bits(y2[R - 1:]).any()   # silent from the sample where c == R: +0
    # NaN in silent receivers: nothing changes; and the tree skips them
    K, Q = 70, 2
    gg = MR.interleaved_gains(K, Q)
    x = SR.audio_series(K, 200, 4)
    base = MR.mixer_ref(x, gg, 37)[0]
    z = x.copy()
    z[2::3, 50] = np.nan
    z[5, :] = np.inf
    assert np.array_equal(MR.bits(MR.mixer_ref(z, gg, 37)[0]), MR.bits(base))
    act = np.flatnonzero(gg.any(axis=1))
    assert np.array_equal(MR.bits(MR.mixer_ref(x[act], gg[act], 37)[0]), MR.bits(base))
    with pytest.raises(ValueError):
        r.set_rx(3, [1.0])
    with pytest.raises(ValueError):
        r.set_rx(0, [np.nan])


def test_gpu_inputs_meet_their_preconditions():
    """Preconditions of tests/test_gpu_mixer.py, on the reference alone: with the chosen series and ceiling the limiter
    reduces the gain in some blocks and not in others (Lb = 8 and 48), at least one clamp is hit, a third of the receivers
    is silent, ramps run and receivers go silent inside the one-shot batch (the active count crosses a multiple of C);
    in the set_rx scenario a ramp is cut by a batch boundary, a set_rx lands mid-ramp and the active count crosses a
    multiple of C inside a batch."""
    K, Q = 1024, 8
    g = MR.interleaved_gains(K, Q)
    assert abs((~g.any(axis=1)).sum() - K / 3) <= 1 and (g < 0).any() and (g > 0).any()
    a = SR.audio_series(K, 3000, MR.SERIES_SEED)
    y, _, st, ref = MR.mixer_ref(a, g, 37, changes=MR.one_shot_changes(K, Q, g))
    assert any(len(c) > 1 and c[0] // 1 != c[-1] for c in ref.chunk_counts), ref.chunk_counts
    clamped = 0
    for Lb in (8, 48):
        lim = MR.LimiterRef(Q, Lb, MR.CEIL, MR.REL)
        out = lim.process(y)
        G = np.array(lim.gains)
        print(f"Lb {Lb}: {(G < 1).sum()} of {G.size} block gains below 1, {lim.clamped} outputs clamped")
        assert (G < 1).sum() >= 10 and (G == 1).sum() >= 10 and np.abs(out).max() <= F32(MR.CEIL)
        clamped += lim.clamped
    assert clamped >= 1
    assert MR.mixer_ref(a, g, 4000, changes=MR.one_shot_changes(K, Q, g))[3].ramps_cut > 0      # R = 4000 > n: cut
    K, Q, R, cuts = MR.SCN_K, MR.SCN_Q, MR.SCN_R, list(MR.SCN_CUTS)
    g = MR.interleaved_gains(K, Q)
    ch = MR.scenario_changes(g)
    r = MR.MixerRef(g, R)
    MR.run_cuts(r, SR.audio_series(K, sum(cuts), MR.SERIES_SEED), cuts, lambda i, m: [m.set_rx(j, gg) for j, gg in ch.get(i, ())])
    assert r.ramps_cut >= 1 and r.midramp_sets >= 1 and any(len(c) > 1 for c in r.chunk_counts), (r.ramps_cut, r.midramp_sets)
    assert sum(cuts) == 3000 and len([j for j, _ in ch[2]]) > len({j for j, _ in ch[2]})          # two changes before one batch
