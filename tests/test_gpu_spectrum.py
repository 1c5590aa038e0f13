"""Panorama (pddc_spectrum_*, Spectrum) on the GPU against the numpy reference in double (tests/spectrum_ref.py)."""
import time

import numpy as np
import pytest

import spectrum_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
SIZES = (1024, 2048, 4096, 8192)


@pytest.fixture(scope="module")
def lcg19(O):
    packed = O.lcg_bytes(6 << 19, 12345)
    return packed, R.to_complex(O, packed)


def windows(nfft):
    rng = np.random.default_rng(nfft)
    return {"rect": np.ones(nfft, np.float32), "hann": R.hann(nfft),
            "random": rng.uniform(0.05, 1.0, nfft).astype(np.float32)}


def run(pkg, dev, packed, nfft, hop, w, cuts=None, peak=True):
    import torch
    d = torch.from_numpy(packed).to(dev)
    sp = pkg.Spectrum(nfft, hop, w, peak=peak)
    n, off = 0, 0
    for b in cuts or [packed.size // 6]:
        n += sp.process(d[6 * off:6 * (off + b)].data_ptr(), b)
        off += b
    s, p, nseg = sp.read()
    torch.cuda.synchronize()
    assert n == nseg
    sp.close()
    return s.cpu().numpy(), p.cpu().numpy() if peak else None, nseg


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nfft", SIZES)
def test_parity(pkg, O, dev, lcg19, nfft, half):
    """max_k |P - Pref| / max_k Pref (and the same for the peak hold) <= 1e-5, one batch and ragged batches down to 8
    samples, for rectangular, Hann and a seeded random positive window.
    Where 1e-5 comes from: an independent float32 model (scipy.fft on complex64, float32 sums, the same 2^19 LCG samples,
    seed 12345, up to 1023 segments) is 0.3e-6 .. 1.4e-6 away from the double reference in this metric, worst at N = 1024
    with hop 512 (re-measured by tests/test_spectrum_cpu.py::test_float32_model_against_double); 1e-5 is 7 x that worst
    case, the room for another factorisation and summation order.  k_spectrum measured 1.2e-7 .. 3.0e-7."""
    packed, x = lcg19
    hop = nfft // 2 if half else nfft
    for name, w in windows(nfft).items():
        Pref, Mref, nref = R.spectrum_ref(x, nfft, hop, w)
        s1, p1, n1 = run(pkg, dev, packed, nfft, hop, w)
        s2, p2, n2 = run(pkg, dev, packed, nfft, hop, w, cuts=R.ragged_cuts(packed.size // 6, nfft, 7 + nfft))
        figs = dict(one_sum=R.err(s1, Pref), one_peak=R.err(p1, Mref), ragged_sum=R.err(s2, Pref),
                    ragged_peak=R.err(p2, Mref), one_vs_ragged=R.err(s2, s1.astype(np.float64)))
        print(f"N {nfft} hop {hop} {name}: " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert n1 == nref and n2 == nref
        assert max(figs.values()) <= TOL, (name, figs)


def test_short_batches_and_streams_shorter_than_a_segment(pkg, O, dev, lcg19):
    import torch
    packed, x = lcg19
    nfft = 2048
    w = R.hann(nfft)
    sp = pkg.Spectrum(nfft, nfft // 2, w)
    d = torch.from_numpy(packed).to(dev)
    assert sp.process(d.data_ptr(), nfft - 8) == 0
    s, p, n = sp.read()
    assert n == 0 and p is None and float(s.abs().max()) == 0.0
    assert sp.process(d[6 * (nfft - 8):].data_ptr(), 8) == 1
    s, _, n = sp.read()
    Pref, _, _ = R.spectrum_ref(x[:nfft], nfft, nfft // 2, w)
    assert n == 1 and R.err(s.cpu().numpy(), Pref) <= TOL
    sp.close()


def test_repeatability(pkg, dev):
    """The same batches twice, on a fresh object and after reset(): bit-identical sum and peak, 20 repetitions at 2^22
    samples (one batch plus a ragged remainder)."""
    import torch
    ns = 1 << 22
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 777, 0, torch.cuda.current_stream().cuda_stream))
    cuts = [ns - 40 * 4096 - 8 * 5, 8 * 5, 4096 * 39, 4096]
    assert sum(cuts) == ns

    def once(sp):
        off = 0
        for b in cuts:
            sp.process(d[6 * off:].data_ptr(), b)
            off += b
        s, p, n = sp.read()
        torch.cuda.synchronize()
        return s.clone(), p.clone(), n

    for nfft, hop in ((4096, 2048), (1024, 1024)):
        sp = pkg.Spectrum(nfft, hop, None, peak=True)
        s0, p0, n0 = once(sp)
        for _ in range(20):
            sp.reset()
            s, p, n = once(sp)
            assert n == n0 and torch.equal(s.view(torch.int32), s0.view(torch.int32))
            assert torch.equal(p.view(torch.int32), p0.view(torch.int32))
        sp.close()
        fresh = pkg.Spectrum(nfft, hop, None, peak=True)
        s, p, n = once(fresh)
        assert n == n0 and torch.equal(s.view(torch.int32), s0.view(torch.int32))
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32))
        fresh.close()


def test_read_with_clear_adds_up(pkg, O, dev, lcg19):
    import torch
    packed, x = lcg19
    nfft, hop = 4096, 2048
    w = R.hann(nfft)
    d = torch.from_numpy(packed).to(dev)
    sp = pkg.Spectrum(nfft, hop, w)
    tot, nt, off = np.zeros(nfft), 0, 0
    for b in R.ragged_cuts(packed.size // 6, nfft, 99):
        sp.process(d[6 * off:].data_ptr(), b)
        off += b
        if off % 3 == 0:
            s, _, n = sp.read(clear=True)
            tot += s.cpu().numpy().astype(np.float64)
            nt += n
    s, _, n = sp.read(clear=True)
    tot += s.cpu().numpy().astype(np.float64)
    nt += n
    s, _, n = sp.read()
    assert n == 0 and float(s.abs().max()) == 0.0
    Pref, _, nref = R.spectrum_ref(x, nfft, hop, w)
    assert nt == nref and R.err(tot, Pref) <= TOL
    sp.close()


@pytest.mark.parametrize("nfft", SIZES)
def test_levels_and_floor(pkg, O, dev, nfft):
    """0.9 of full scale at bin floor(0.23 N) and a tone 100 dB below it at N - floor(0.11 N), then seven seeded pairs of
    bins (spectrum_ref.level_pairs: other butterflies in every pass), 24-bit, Hann, 64 segments: the strong bin reads
    20 log10(0.9) dBFS within 0.001 dB, the weak one its level within 0.1 dB, and no bin further than 3 from either is
    above -135 dBFS.  (The float32 model puts that floor at -144 .. -158 dBFS over these placements;
    tests/test_spectrum_cpu.py::test_levels_and_floor_model holds the model to the same three bounds.)"""
    w = R.hann(nfft)
    for k1, k2 in R.level_pairs(nfft):
        packed = R.tone_packed(O, 64 * nfft, nfft, [(0.9, k1), (0.9 * 1e-5, k2)])
        s, _, n = run(pkg, dev, packed, nfft, nfft, w, peak=False)
        strong, weak, floor = R.levels(pkg.spectrum_dbfs(s, n, w), k1, k2)
        print(f"N {nfft} bins {k1} / {k2}: strong {strong:+.5f} dB, weak {weak:+.4f} dB, floor {floor:.1f} dBFS")
        assert n == 64 and abs(strong) <= 0.001 and abs(weak) <= 0.1 and floor <= -135.0, (k1, k2)


def test_full_size(pkg, O, dev):
    """One 2^28-sample batch of the LCG stream, N = 4096, hop = N, Hann: 65 536 segments, every bin against the double
    reference (computed in chunks).  Tolerance: the kernel adds 128 segments per float32 partial row (512 rows) and the
    rows in double; the float32 model with 128 segments per float32 row is 1.61e-7 away from double
    (tests/test_spectrum_cpu.py::test_float32_model_with_the_kernels_partial_sums); 8 x that = 1.3e-6."""
    import torch
    ns = 1 << 28
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, torch.cuda.current_stream().cuda_stream))
    w = R.hann(4096)
    sp = pkg.Spectrum(4096, 4096, w)
    assert sp.process(d) == 65536
    s, _, n = sp.read()
    torch.cuda.synchronize()
    s = s.cpu().numpy()
    sp.close()
    t0 = time.time()
    P = np.zeros(4096)
    step = 1 << 23
    for a in range(0, ns, step):
        chunk = d[6 * a:6 * (a + step)].cpu().numpy()
        P += R.spectrum_ref(R.to_complex(O, chunk), 4096, 4096, w)[0]
    del d
    e = R.err(s, P)
    print(f"full size: err {e:.2e}, reference took {time.time() - t0:.0f} s")
    assert n == 65536 and e <= 1.3e-6


def test_bank_and_panorama_on_one_batch(pkg, dev, taps):
    """One d_packed, a Bank of four 48-tap members and a Spectrum on the same stream: the bank's outputs are bit-identical
    to the run without the spectrum and the spectrum to the run without the bank."""
    import torch
    ns = 1 << 22
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 4242, 0, st))
    t48 = taps("d8_127")[:48].copy()
    fregs = [0x12345678, 0x3456789A, 0x9ABCDEF0, 0xDEADBEEF]

    def bank_round(with_spec, with_bank=True):
        pipes = [pkg.Pipeline([(8, t48)], device=0, mix=True) for _ in fregs]
        for p, f in zip(pipes, fregs):
            p.set_freg(f)
        bank = pkg.Bank(pipes)
        sp = pkg.Spectrum(4096, 2048, None, peak=True) if with_spec else None
        outs = [torch.zeros((ns // 8 + 16, 2), dtype=torch.float32, device=dev) for _ in fregs]
        res = []
        for rnd in range(2):
            if with_bank:
                n, nb = bank.process_ptr(d.data_ptr(), ns, [o.data_ptr() for o in outs], [o.shape[0] for o in outs], st)
                assert nb == 4
                res += [o[:k].clone() for o, k in zip(outs, n)]
            if sp:
                sp.process(d)
        spec = sp.read() if sp else None
        torch.cuda.synchronize()
        bank.close()
        for p in pipes:
            p.close()
        if sp:
            sp.close()
        return res, spec

    both, spec_both = bank_round(True)
    alone, _ = bank_round(False)
    _, spec_alone = bank_round(True, with_bank=False)
    assert len(both) == len(alone) == 8
    for a, b in zip(both, alone):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert spec_both[2] == spec_alone[2] > 0
    assert torch.equal(spec_both[0].view(torch.int32), spec_alone[0].view(torch.int32))
    assert torch.equal(spec_both[1].view(torch.int32), spec_alone[1].view(torch.int32))


@pytest.mark.perf
@pytest.mark.parametrize("lg", [24, 28])
def test_spectrum_time_against_the_host_path(pkg, dev, perf_record, lg):
    """k_spectrum against what a host had before it: pddc_unpack24_f32 into a float buffer, window multiply,
    torch.fft.fft over (nseg, N), abs^2 and a sum over segments -- same box, same process, hop = N, median of 15.
    The kernel must be faster at every point."""
    import torch
    ns = 1 << lg
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, torch.cuda.current_stream().cuda_stream))

    def timed(fn, reps=15):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    for nfft in (1024, 4096, 8192):
        w = torch.from_numpy(R.hann(nfft)).to(dev)
        sp = pkg.Spectrum(nfft, nfft, None)

        def host_path():
            x = torch.view_as_complex(pkg.unpack24_f32(d)).view(-1, nfft)
            X = torch.fft.fft(x * w, dim=1)
            return (X.real * X.real + X.imag * X.imag).sum(dim=0)

        host_path()
        sp.process(d)
        torch.cuda.synchronize()
        time.sleep(1.0)                      # freshly allocated buffers are slow at first
        t_host = timed(host_path)
        t_new = timed(lambda: sp.process(d))
        sp.close()
        torch.cuda.empty_cache()
        perf_record(f"spectrum_2p{lg}_n{nfft}_ms", round(t_new, 4), unit="ms", host_path_ms=round(t_host, 4),
                    ratio=round(t_host / t_new, 2))
        assert t_new < t_host, (lg, nfft, t_new, t_host)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nfft", SIZES)
def test_parity_in_the_walk(pkg, O, dev, nfft, half):
    """2^24 LCG samples: 2048 .. 32767 segments, several (up to 16) per block, so the prefetch of the next segment, the
    barrier before the next loaders and the float32 sums and peak hold across a block's segments are compared with the
    double reference -- for every size, both hops, with the peak hold.  Same metric and bar as test_parity."""
    import torch
    ns = 1 << 24
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, torch.cuda.current_stream().cuda_stream))
    hop = nfft // 2 if half else nfft
    w = windows(nfft)["random"]
    sp = pkg.Spectrum(nfft, hop, w, peak=True)
    n = sp.process(d)
    s, p, nseg = sp.read()
    torch.cuda.synchronize()
    sp.close()
    x = R.to_complex(O, d.cpu().numpy())
    Pref, Mref, nref = R.spectrum_ref(x, nfft, hop, w)
    e1, e2 = R.err(s.cpu().numpy(), Pref), R.err(p.cpu().numpy(), Mref)
    print(f"walk N {nfft} hop {hop}: nseg {nseg} sum {e1:.2e} peak {e2:.2e}")
    assert n == nseg == nref and nseg >= 2048 and max(e1, e2) <= TOL


# ------------------------------------------------------------------ the drop-in API
import ctypes as C


@pytest.fixture()
def L(pkg, dev, monkeypatch):
    for k in ("PERSEUS_AMD_MODE", "PERSEUS_AMD_SOURCE", "PERSEUS_AMD_DEVICES", "PERSEUS_AMD_FAULTS",
              "PERSEUS_AMD_DROP", "PERSEUS_AMD_BATCH", "PERSEUS_AMD_CPU_SOURCE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PERSEUS_AMD_PACE", "0")
    lib = pkg.sdr_lib()
    lib.perseus_set_debug(0)
    yield lib
    lib.perseus_exit()


def api_open(L, pkg, i, seed, nbuf, batch, spectrum):
    d = L.perseus_open(i)
    assert d and L.perseus_firmware_download(d, None) == 0 and L.perseus_set_sampling_rate(d, 125000) == 0
    assert L.perseus_set_ddc_center_freq(d, C.c_double(7.1e6), 1) == 0
    cfg = pkg.AmdConfig()
    L.perseus_amd_get_config(d, C.byref(cfg))
    cfg.pace, cfg.mode, cfg.batch_samples, cfg.max_buffers, cfg.lcg_seed = 0, 1, batch, nbuf, seed
    assert L.perseus_amd_set_config(d, C.byref(cfg)) == 0, L.perseus_errorstr()
    if spectrum:
        assert L.perseus_amd_spectrum_enable(d, 4096, 4096, None, 0) == 0, L.perseus_errorstr()
    return d


def api_run(L, pkg, ds, on_buffer=None, bufsize=12288):
    outs, cbs = [[] for _ in ds], []
    for i in range(len(ds)):
        def cb(b, n, x, i=i):
            outs[i].append(C.string_at(b, n))
            if on_buffer:
                on_buffer(i, len(outs[i]))
            return 0
        cbs.append(pkg.PERSEUS_CALLBACK(cb))
    t0 = time.time()
    for i, d in enumerate(ds):
        assert L.perseus_start_async_input(d, bufsize, cbs[i], None) == 0, L.perseus_errorstr()
    while any(L.perseus_amd_source_running(d) for d in ds) and time.time() - t0 < 120:
        time.sleep(0.002)
    stats = []
    for d in ds:
        st = pkg.AmdStats()
        L.perseus_amd_get_stats(d, C.byref(st))
        stats.append((int(st.adc_samples), int(st.ganged_batches)))
        assert L.perseus_stop_async_input(d) == 0
    return [b"".join(o) for o in outs], stats


def api_read(L, d, clear=0):
    s = np.zeros(4096, np.float32)
    n = C.c_uint64()
    assert L.perseus_amd_spectrum_read(d, s.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(n), clear) == 0, \
        L.perseus_errorstr()
    return s.astype(np.float64), int(n.value)


def api_ref(O, seed, adc):
    x = R.to_complex(O, O.lcg_bytes(6 * adc, seed))
    return R.spectrum_ref(x, 4096, 4096, R.hann(4096))


def test_api_receiver_spectrum(L, pkg, O):
    """A DDC-mode receiver with perseus_amd_spectrum_enable(4096, 4096, NULL, 0) on a bounded LCG source: read gives the
    reference's spectrum of exactly the stats.adc_samples samples the GPU was handed (1e-5, exact segment count), and
    the callback bytes equal those of a run with the feature off."""
    nbuf, batch = 300, 1 << 20
    assert L.perseus_init() == 1
    d = api_open(L, pkg, 0, 12345, nbuf, batch, True)
    (on,), ((adc, _),) = api_run(L, pkg, [d])
    s, n = api_read(L, d)
    Pref, _, nref = api_ref(O, 12345, adc)
    e = R.err(s, Pref)
    print(f"api: adc_samples {adc} segments {n} err {e:.2e}")
    assert adc > 0 and n == nref and e <= TOL
    L.perseus_exit()
    assert L.perseus_init() == 1
    d = api_open(L, pkg, 0, 12345, nbuf, batch, False)
    (off,), _ = api_run(L, pkg, [d])
    assert len(on) > 0 and on == off
    assert L.perseus_amd_spectrum_read(d, None, None, None, 0) == -9          # PERSEUS_FNNOTAVAIL: not enabled


def test_api_gang_of_two_each_its_own_spectrum(L, pkg, O, monkeypatch):
    nbuf, batch = 300, 1 << 20
    monkeypatch.setenv("PERSEUS_AMD_DEVICES", "2")
    assert L.perseus_init() == 2
    ds = [api_open(L, pkg, i, 12345 + 7 * i, nbuf, batch, True) for i in range(2)]
    _, stats = api_run(L, pkg, ds)
    print(f"gang: (adc_samples, ganged_batches) per receiver {stats}")
    for i, d in enumerate(ds):
        s, n = api_read(L, d)
        Pref, _, nref = api_ref(O, 12345 + 7 * i, stats[i][0])
        assert n == nref and R.err(s, Pref) <= TOL, i
    assert max(g for _, g in stats) > 0, "no round of the two receivers was ganged"


def test_api_clearing_reads_add_up(L, pkg, O):
    """clear = 1 read-outs from the callback thread's side while streaming add up to the one read-out of an identical
    run: segment counts exactly, sums at 1e-5."""
    nbuf, batch = 300, 1 << 20
    assert L.perseus_init() == 1
    d = api_open(L, pkg, 0, 999, nbuf, batch, True)
    tot, cnt, reads = np.zeros(4096), [0], [0]

    def on_buffer(i, k):
        if k % 40 == 0:
            s, n = api_read(L, d, clear=1)
            tot[:] += s
            cnt[0] += n
            reads[0] += 1

    _, ((adc, _),) = api_run(L, pkg, [d], on_buffer=on_buffer)
    s, n = api_read(L, d, clear=1)
    tot += s
    cnt[0] += n
    L.perseus_exit()
    assert L.perseus_init() == 1
    d = api_open(L, pkg, 0, 999, nbuf, batch, True)
    _, ((adc2, _),) = api_run(L, pkg, [d])
    s1, n1 = api_read(L, d)
    print(f"clearing reads: {reads[0]} during the stream, segments {cnt[0]} / {n1}, err {R.err(tot, s1):.2e}")
    assert adc == adc2 and reads[0] >= 3 and cnt[0] == n1 > 0 and R.err(tot, s1) <= TOL
