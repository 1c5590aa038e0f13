"""Panorama (pddc_spectrum_*), what can be checked without a GPU: the numpy reference against closed forms, the
segment arithmetic, argument checks, and the source-level rules of the new files."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libperseus-sdr_amd", "csrc")
SIZES = (1024, 2048, 4096, 8192)


@pytest.mark.parametrize("nfft", [1024, 4096])
def test_reference_against_closed_forms(O, nfft):
    """A e^{+2 pi i k0 n / N}, quantised to 24 bits: P[k0] = nseg (A sum w)^2 within 1e-6, argmax k0; a negative frequency
    lands in N - k; I and Q swapped mirror the spectrum; a full-scale tone reads 0 dBFS through the Hann helper."""
    k0, a, nseg = nfft // 5 + 3, 0.7, 6
    for w in (np.ones(nfft, np.float32), R.hann(nfft)):
        for hop in (nfft, nfft // 2):
            n = nfft + (nseg - 1) * hop
            packed = R.tone_packed(O, n, nfft, [(a, k0)])
            P, M, ns = R.spectrum_ref(R.to_complex(O, packed), nfft, hop, w)
            assert ns == nseg and int(np.argmax(P)) == k0
            want = nseg * (a * float(np.sum(w.astype(np.float64)))) ** 2
            assert abs(P[k0] - want) / want < 1e-6
            assert abs(M[k0] - want / nseg) / (want / nseg) < 1e-6
    w = R.hann(nfft)
    neg = R.tone_packed(O, 4 * nfft, nfft, [(a, -k0)])
    P, _, _ = R.spectrum_ref(R.to_complex(O, neg), nfft, nfft, w)
    assert int(np.argmax(P)) == nfft - k0
    pos = R.tone_packed(O, 4 * nfft, nfft, [(a, k0), (0.01, 17)])
    Pp, _, _ = R.spectrum_ref(R.to_complex(O, pos), nfft, nfft, w)
    sw = pos.reshape(-1, 2, 3)[:, ::-1, :].reshape(-1).copy()          # I <-> Q
    Ps, _, _ = R.spectrum_ref(R.to_complex(O, sw), nfft, nfft, w)
    assert np.allclose(Ps, Pp[(-np.arange(nfft)) % nfft], rtol=1e-9, atol=1e-12 * Pp.max())
    full = R.tone_packed(O, 4 * nfft, nfft, [(1.0, k0)])
    Pf, _, ns = R.spectrum_ref(R.to_complex(O, full), nfft, nfft, w)
    assert abs(R.dbfs(Pf, ns, w)[k0]) < 1e-5


def test_dbfs_helper_of_the_package(pkg, O):
    nfft, k0 = 1024, 100
    w = pkg.hann_window(nfft)
    assert np.array_equal(w, R.hann(nfft))
    full = R.tone_packed(O, 4 * nfft, nfft, [(1.0, k0)])
    P, _, ns = R.spectrum_ref(R.to_complex(O, full), nfft, nfft, w)
    d = pkg.spectrum_dbfs(P, ns, w)
    assert abs(d[k0]) < 1e-5 and int(np.argmax(d)) == k0


@pytest.mark.parametrize("nfft", SIZES)
@pytest.mark.parametrize("half", [0, 1])
def test_segment_grid_is_cut_invariant(pkg, nfft, half):
    """pddc_spectrum_segments, summed over ragged batches of 8 .. 3 N samples, is the whole stream's
    max(0, (len - N) // hop + 1)"""
    hop = nfft // 2 if half else nfft
    L = pkg.ddc_lib()
    for seed, total in ((1, 40 * nfft + 8), (2, nfft - 8), (3, nfft), (4, 17 * nfft + 5 * 8)):
        done = before = 0
        for b in R.ragged_cuts(total, nfft, seed):
            done += L.pddc_spectrum_segments(nfft, hop, before, b)
            before += b
        assert before == total and done == R.nseg_of(total, nfft, hop), (nfft, hop, total)
        assert L.pddc_spectrum_segments(nfft, hop, 0, total) == done
    assert L.pddc_spectrum_segments(1000, 1000, 0, 1 << 20) == 0
    assert L.pddc_spectrum_segments(nfft, nfft // 4, 0, 1 << 20) == 0


def test_argument_checks_come_before_the_device(pkg):
    L = pkg.ddc_lib()
    h = C.c_void_p()
    w = (C.c_float * 8192)(*([1.0] * 8192))
    EINVAL, ENODEV = -1, -2
    for nfft, hop in ((1000, 1000), (512, 512), (16384 * 2, 16384), (4096, 1024), (4096, 0), (0, 0)):
        assert L.pddc_spectrum_create(C.byref(h), 0, nfft, hop, w, 0) == EINVAL
    assert L.pddc_spectrum_create(C.byref(h), 0, 4096, 4096, None, 0) == EINVAL
    assert L.pddc_spectrum_create(C.byref(h), 0, 4096, 4096, w, 0x10) == EINVAL
    assert L.pddc_spectrum_create(None, 0, 4096, 4096, w, 0) == EINVAL
    assert L.pddc_spectrum_process(None, None, 8, None) == EINVAL
    assert L.pddc_spectrum_read(None, None, None, None, 0, None) == EINVAL
    assert L.pddc_spectrum_reset(None) == EINVAL
    assert L.pddc_spectrum_destroy(None) == 0
    if L.pddc_device_count() == 0:
        assert L.pddc_spectrum_create(C.byref(h), 0, 4096, 4096, w, 0) == ENODEV
        assert b"no CPU fallback" in L.pddc_last_error()
        with pytest.raises(pkg.PddcError):
            pkg.Spectrum(4096)
    else:
        sp = pkg.Spectrum(1024)
        assert L.pddc_spectrum_process(sp._h, None, 64, None) == EINVAL
        assert L.pddc_spectrum_process(sp._h, 16, 12, None) == EINVAL
        assert L.pddc_spectrum_process(sp._h, 24, 64, None) == EINVAL          # misaligned
        sp.close()
    with pytest.raises(pkg.PddcError):
        pkg.Spectrum(4096, window=np.ones(100, np.float32))


def test_new_sources_hold_no_getenv_and_do_not_name_the_checker():
    for name in ("ddc_spectrum.hip", "ddc_spectrum.cpp", "ddc_spectrum.h", "ddc_packed.h", "ddc_host.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert "getenv" not in src, name
        assert "oracle" not in src.lower(), name
        assert not re.search(r"__sinf|__cosf|sincosf|atomicAdd|atomic_add|__hip_atomic", src), name
    py = open(os.path.join(ROOT, "libperseus-sdr_amd", "__init__.py")).read()
    cls = py[py.index("class _StreamObject"):py.index("class PinnedBuffer")]     # the classes' shared base comes first
    assert cls.index("class Spectrum") > 0
    assert "oracle" not in cls.lower() and "environ" not in cls


def test_float32_model_against_double(O):
    """The independent float32 model the GPU tolerance rests on (scipy.fft on complex64, float32 sums; 2^19 LCG samples,
    seed 12345), re-measured here: 0.3e-6 .. 1.4e-6 against the double reference, worst at N = 1024 with hop 512.  The GPU
    tests use 1e-5 = 7 x that worst case."""
    x = R.to_complex(O, O.lcg_bytes(6 << 19, 12345))
    worst = 0.0
    for nfft, hop in ((1024, 512), (1024, 1024), (4096, 2048), (8192, 8192)):
        w = R.hann(nfft)
        Pref, _, _ = R.spectrum_ref(x, nfft, hop, w)
        e = R.err(R.spectrum_model_f32(x, nfft, hop, w), Pref)
        print(f"float32 model N {nfft} hop {hop}: {e:.2e}")
        worst = max(worst, e)
    assert 1e-8 < worst < 1e-5 / 5


@pytest.mark.parametrize("nfft", SIZES)
def test_levels_and_floor_model(O, nfft):
    """The inputs of tests/test_gpu_spectrum.py::test_levels_and_floor, every placement, through the independent float32
    model: the three bounds of that test hold -- strong bin within 0.001 dB, weak bin within 0.1 dB, floor below
    -135 dBFS -- so the inputs alone meet them."""
    w = R.hann(nfft)
    pairs = R.level_pairs(nfft)
    assert len(pairs) == R.LEVEL_CASES and pairs[0] == (int(0.23 * nfft), nfft - int(0.11 * nfft))
    for k1, k2 in pairs:
        assert min((k1 - k2) % nfft, (k2 - k1) % nfft) >= 8
        x = R.to_complex(O, R.tone_packed(O, 64 * nfft, nfft, [(0.9, k1), (0.9 * 1e-5, k2)]))
        P = R.spectrum_model_f32(x, nfft, nfft, w)
        strong, weak, floor = R.levels(R.dbfs(P, 64, w), k1, k2)
        print(f"float32 model N {nfft} bins {k1} / {k2}: strong {strong:+.5f} dB, weak {weak:+.4f} dB, floor {floor:.1f} dBFS")
        assert abs(strong) <= 0.001 and abs(weak) <= 0.1 and floor <= -135.0, (k1, k2)


def test_float32_model_with_the_kernels_partial_sums(O):
    """Full-size structure (tests/test_gpu_spectrum.py::test_full_size): 65 536 segments of 4096 go to 512 float32 partial
    rows of 128 segments each (row = segment mod 512), added in double.  Measured on 2^24 samples of the LCG stream cut
    into 4096 segments over 32 rows (the same 128 per row): the printed figure, 1.61e-7 (more rows added in double
    do not raise a relative error); the full-size tolerance is 8 x that = 1.3e-6."""
    x = R.to_complex(O, O.lcg_bytes(6 << 24, 12345))
    w = R.hann(4096)
    Pref, _, n = R.spectrum_ref(x, 4096, 4096, w)
    e = R.err(R.spectrum_model_f32(x, 4096, 4096, w, rows=32), Pref)
    print(f"float32 model, 128 segments per float32 partial row: {e:.2e}")
    assert n == 4096 and 1.2e-7 < e < 2.0e-7           # the figure the GPU tolerance quotes


def test_api_enable_answers(pkg, monkeypatch):
    """perseus_amd_spectrum_enable: wire mode PERSEUS_FNNOTAVAIL, bad sizes PERSEUS_ERRPARAM, while streaming
    PERSEUS_ASYNCSTARTED; read without a stream that had it PERSEUS_FNNOTAVAIL."""
    import time
    FNNOTAVAIL, ASYNCSTARTED, ERRPARAM, NULLDESCR = -9, -19, -22, -2
    monkeypatch.setenv("PERSEUS_AMD_PACE", "0")
    for k in ("PERSEUS_AMD_MODE", "PERSEUS_AMD_SOURCE", "PERSEUS_AMD_DEVICES"):
        monkeypatch.delenv(k, raising=False)
    L = pkg.sdr_lib()
    L.perseus_set_debug(0)
    try:
        assert L.perseus_init() == 1
        d = L.perseus_open(0)
        assert L.perseus_firmware_download(d, None) == 0 and L.perseus_set_sampling_rate(d, 95000) == 0
        assert L.perseus_amd_spectrum_enable(None, 4096, 4096, None, 0) == NULLDESCR
        assert L.perseus_amd_spectrum_enable(d, 4096, 4096, None, 0) == FNNOTAVAIL          # wire mode (the default)
        n = C.c_uint64()
        assert L.perseus_amd_spectrum_read(d, None, None, C.byref(n), 0) == FNNOTAVAIL
        cfg = pkg.AmdConfig()
        L.perseus_amd_get_config(d, C.byref(cfg))
        cfg.mode, cfg.pace = 1, 0
        assert L.perseus_amd_set_config(d, C.byref(cfg)) == 0
        for nfft, hop in ((1000, 1000), (512, 512), (16384, 16384), (4096, 1024), (4096, 0)):
            assert L.perseus_amd_spectrum_enable(d, nfft, hop, None, 0) == ERRPARAM, (nfft, hop)
        assert L.perseus_amd_spectrum_enable(d, 4096, 4096, None, 0x10) == ERRPARAM
        w = (C.c_float * 4096)(*([1.0] * 4096))
        assert L.perseus_amd_spectrum_enable(d, 4096, 2048, w, 1) == 0
        assert L.perseus_amd_spectrum_enable(d, 0, 0, None, 0) == 0                         # off again
        cfg.mode = 0
        assert L.perseus_amd_set_config(d, C.byref(cfg)) == 0
        cb = pkg.PERSEUS_CALLBACK(lambda b, k, x: 0)
        assert L.perseus_start_async_input(d, 6144, cb, None) == 0
        assert L.perseus_amd_spectrum_enable(d, 4096, 4096, None, 0) == ASYNCSTARTED
        time.sleep(0.01)
        assert L.perseus_stop_async_input(d) == 0
    finally:
        L.perseus_exit()
