"""Demod (pddc_demod_*, k_demod) on the GPU against the numpy reference in double (tests/demod_ref.py).  Tolerances:
demod_ref.TOL_DEMOD / TOL_DEMOD_CHAIN, 7 x the float32 models' worst cases (tests/test_demod_cpu.py), never taken from
k_demod."""
import types

import numpy as np
import pytest

import channelizer_ref as CR
import demod_ref as DR
import spectrum_ref as R
import tuner_ref as TR

pytestmark = pytest.mark.gpu
P = DR.PARAMS


def make(pkg, rx):
    return pkg.Demod(rx, rho=P["rho"], lam=P["lam"], target=P["target"], gmax=P["gmax"])


def run(pkg, z, rx, cuts=None, before=None):
    """all of z (torch complex64 [K, n]) through a fresh Demod in the given batches -> float32 [K, n]; before(i, d) is
    called ahead of batch i"""
    import torch
    d = make(pkg, rx)
    outs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, d)
        o = d.process(z[:, off:off + b])
        assert o.shape == (len(rx), b)
        outs.append(o)
        off += b
    assert off == z.shape[1]
    torch.cuda.synchronize()
    d.close()
    return torch.cat(outs, dim=1)


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def random_series(dev, K, n, seed=99):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.view_as_complex(torch.randn((K, n, 2), generator=gen, dtype=torch.float32)).to(dev)


@pytest.fixture(scope="module")
def tuner_outputs(O):
    """the tuner reference's outputs on the 2^19-sample LCG stream, rounded to complex64 (as in test_demod_cpu.py)"""
    x = R.to_complex(O, O.lcg_bytes(6 << 19, 12345))
    M, hop, T, Rd = 1024, 512, 64, 4
    y = CR.channelizer_ref(x, M, hop, TR.kaiser_prototype_wide(M, 4))
    return TR.tuner_ref(y, M, hop, TR.receiver_set(M, 1024), TR.kaiser_lowpass(T, Rd), Rd).astype(np.complex64)


def test_parity_demod_alone(pkg, dev, tuner_outputs):
    """The same complex64 series uploaded; the double reference from those very values.  K = 1024 with modes and flag
    sets interleaved receiver by receiver (mode j mod 3, flag set (j // 3) mod 4: every mode with and without DCBLOCK /
    AGC), then K = 1 and K = 7 for every mode and flag set; 239 outputs per receiver.  err <= TOL_DEMOD[mode] per mode.
    k_demod measured 4.6e-8 .. 1.5e-6 here (profiles/r14/demod_tests_figures.txt)."""
    import torch
    z64 = tuner_outputs
    zd = torch.from_numpy(z64).to(dev)
    done = 0

    def case(name, rows, rx):
        nonlocal done
        out = run(pkg, zd[rows].contiguous(), rx).cpu().numpy()
        ref = DR.demod_ref(z64[rows], rx, **P)
        assert out.shape == ref.shape
        for mode, e in DR.err_by_mode(out, ref, rx).items():
            print(f"{name} {DR.MODE_NAMES[mode]}: err {e:.2e} (bar {DR.TOL_DEMOD[mode]:.2e})")
            assert e <= DR.TOL_DEMOD[mode], (name, mode, e)
        done += 1

    case("K 1024 interleaved", np.arange(1024), DR.interleaved_rx(1024))
    for mode in DR.MODES:
        for flags in DR.FLAG_SETS:
            case(f"K 1 flags {flags}", np.array([30 + mode + 3 * flags]), [(mode, 0x1234567 * (flags + 1), flags)])
        case("K 7 one mode", np.arange(100, 107), [(mode, 77777 * (j + 1), DR.FLAG_SETS[j % 4]) for j in range(7)])
    case("K 7 interleaved", np.arange(200, 207), DR.interleaved_rx(7))
    assert done >= 12


def test_bits_against_the_cut_and_the_company(pkg, dev):
    """3000 seeded random complex64 values per receiver.  One batch against batches of 0, 1, 2, TT - 1, TT, TT + 1,
    3 TT + 5 and the rest (TT = demod_tile_outputs()): equal int32 views for K = 1024, 7 and 1; with the receiver order
    reversed receiver j's bits are the same; and a receiver alone, or among plain receivers (the walk without a post
    stage), gives the bits it has among the 1024."""
    import torch
    TT, n = pkg.demod_tile_outputs(), 3000
    cuts = [0, 1, 2, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > TT
    rx = DR.interleaved_rx(1024)
    z = random_series(dev, 1024, n)
    one = run(pkg, z, rx)
    assert torch.isfinite(one).all()
    assert torch.equal(bits(run(pkg, z, rx, cuts)), bits(one))
    rev = run(pkg, z.flip(0).contiguous(), rx[::-1], cuts[::-1])
    assert torch.equal(bits(rev), bits(one.flip(0)))
    few = run(pkg, z[500:507].contiguous(), rx[500:507], cuts)
    assert torch.equal(bits(few), bits(one[500:507]))
    for j in (0, 1, 2, 4, 5, 9, 10, 11, 1023):               # every mode, plain and with a post stage
        alone = run(pkg, z[j:j + 1].contiguous(), rx[j:j + 1], cuts)
        assert torch.equal(bits(alone[0]), bits(one[j])), j
    plain = [j for j in range(1024) if rx[j][2] == 0][:10]   # a group of plain receivers takes the other walk
    got = run(pkg, z[plain].contiguous(), [rx[j] for j in plain], cuts)
    assert torch.equal(bits(got), bits(one[plain]))
    big = run(pkg, z[plain].contiguous(), [rx[j] for j in plain])
    assert torch.equal(bits(big), bits(one[plain]))


def test_strides(pkg, dev):
    """Input as the view Tuner.process returns (row stride = capacity > n) and `out` with capacity > n: the bits of the
    contiguous call."""
    import torch
    M, hop, T, Rd, K, S = 1024, 512, 64, 4, 13, 1200
    rows = random_series(dev, S, M, seed=5)
    words = TR.receiver_set(M, K)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, words, pkg.tuner_lowpass(T, Rd), Rd)
    cap = t.next_outputs(S) + 37
    zv = t.process(rows, out=torch.empty((K, cap), dtype=torch.complex64, device=dev))
    n = zv.shape[1]
    assert zv.stride(0) == cap > n > 256
    rx = DR.interleaved_rx(K)
    want = run(pkg, zv.contiguous(), rx)
    d = make(pkg, rx)
    buf = torch.full((K, n + 11), 7.0, dtype=torch.float32, device=dev)
    got = d.process(zv, out=buf)
    torch.cuda.synchronize()
    assert got.shape == (K, n) and got.data_ptr() == buf.data_ptr()
    assert torch.equal(bits(got), bits(want)) and bool((buf[:, n:] == 7.0).all())
    d.close()
    t.close()


def test_set_rx_between_batches(pkg, dev):
    """Against the streaming reference with the same history: a BFO change goes on phase-continuously, a mode or flag
    change starts that receiver afresh, <= TOL_DEMOD per mode; the receivers that were not touched have the bits of a
    run without the changes; an unknown mode or flag is refused and changes nothing."""
    import torch
    K, n = 12, 900
    cuts = [300, 1, 299, 300]
    rx = DR.interleaved_rx(K)
    z = random_series(dev, K, n, seed=21)
    changes = {1: [(2, DR.SSB, 0x0BADF00D, rx[2][2]), (3, DR.FM, 0, DR.DC | DR.AGC)],          # word alone; mode + flags
               2: [(2, DR.SSB, 0x01000000, rx[2][2]), (7, rx[7][0], rx[7][1], DR.DC)],          # word again; flags alone
               3: [(0, DR.SSB, 0x22222222, DR.DC)]}                                             # mode

    def before(i, d):
        for c in changes.get(i, ()):
            d.set_rx(*c)
        for bad in ((1, 3, 0, 0), (1, DR.AM, 0, 4), (K, DR.AM, 0, 0)):
            with pytest.raises(pkg.PddcError) as e:
                d.set_rx(*bad)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, z, rx, cuts, before)
    clean = run(pkg, z, rx, cuts)
    touched = {c[0] for cs in changes.values() for c in cs}
    for j in range(K):
        if j not in touched:
            assert torch.equal(bits(got[j]), bits(clean[j])), j
    assert torch.equal(bits(got[:, :300]), bits(clean[:, :300]))
    ref = DR.DemodRef(rx, **P)
    zn = z.cpu().numpy()
    outs, off = [], 0
    for i, b in enumerate(cuts):
        for c in changes.get(i, ()):
            ref.set_rx(*c)
        outs.append(ref.process(zn[:, off:off + b]))
        off += b
    want = np.concatenate(outs, axis=1)
    o = got.cpu().numpy()
    for j in sorted(touched):
        for a, b, mode in ((0, 300, rx[j][0]), (600, 900, int(ref.mode[j]))):
            e = DR.err(o[j:j + 1, a:b], want[j:j + 1, a:b], wrap=(mode == DR.FM))
            print(f"receiver {j} outputs {a}..{b} {DR.MODE_NAMES[mode]}: err {e:.2e}")
            assert e <= DR.TOL_DEMOD[mode], (j, a, e)
    e = DR.err(o[2:3], want[2:3])                          # the retuned SSB receiver over all four batches
    assert e <= DR.TOL_DEMOD[DR.SSB]


@pytest.mark.parametrize("mode", DR.MODES)
def test_end_to_end(pkg, O, dev, mode):
    """chain_signal(mode), 2^19 samples with a strong modulated carrier in channel 300, packed by the package's pack24
    (the oracle's bytes), through Channelizer (M = 1024, hop 512, tuner_prototype) -> Tuner (T = 64, R = 4) -> Demod on
    one stream, against channelizer_ref -> tuner_ref -> demod_ref in double: <= TOL_DEMOD_CHAIN[mode], 7 x the float32
    model chain's worst case on this very input.  The reference's min |z| / max |z| >= 0.1.
    k_demod behind k_channelize and k_tune measured 2.8e-7 .. 1.1e-6 (profiles/r14/demod_tests_figures.txt)."""
    import torch
    c = DR.CHAIN
    sig = DR.chain_signal(mode)
    packed = pkg.pack24_f32(torch.from_numpy(sig).to(dev))
    pb = packed.cpu().numpy()
    assert np.array_equal(pb, O.pack24_f32(sig))
    words, rx = DR.chain_receivers(mode)
    w, h = pkg.tuner_prototype(c["nchan"], c["proto_taps"]), pkg.tuner_lowpass(c["ntaps"], c["decim"])
    ch = pkg.Channelizer(c["nchan"], w, c["hop"])
    t = pkg.Tuner(ch, words, h, c["decim"])
    d = make(pkg, rx)
    out = d.process(t.process(ch.process(packed.clone())))
    torch.cuda.synchronize()
    y = CR.channelizer_ref(R.to_complex(O, pb), c["nchan"], c["hop"], w)
    z = TR.tuner_ref(y, c["nchan"], c["hop"], words, h, c["decim"])
    assert float(np.min(np.abs(z)) / np.max(np.abs(z))) >= 0.1
    ref = DR.demod_ref(z, rx, **P)
    o = out.cpu().numpy()
    assert o.shape == ref.shape == (3, 239)
    for j, r in enumerate(rx):
        e = DR.err(o[j:j + 1], ref[j:j + 1], wrap=(mode == DR.FM))
        print(f"chain {DR.MODE_NAMES[mode]} flags {r[2]}: err {e:.2e} (bar {DR.TOL_DEMOD_CHAIN[mode]:.2e})")
        assert e <= DR.TOL_DEMOD_CHAIN[mode], (mode, r, e)
    for obj in (d, t, ch):
        obj.close()


def test_a_refused_process_changes_nothing(pkg, dev):
    """process calls refused for capacity (out too small, a z stride below n) and for a misaligned or missing pointer,
    between the batches: the next correct call's bits are those of an object that never saw them."""
    import torch
    K, n = 9, 700
    cuts = [300, 150, 250]
    rx = DR.interleaved_rx(K)
    z = random_series(dev, K, n, seed=4)
    clean = run(pkg, z, rx, cuts)
    L = pkg.ddc_lib()

    def disturb(i, d):
        b = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            d.process(z[:, :b], out=torch.empty((K, b - 1), dtype=torch.float32, device=dev))
        assert e.value.code == pkg.PDDC_ECAPACITY
        o = torch.empty((K, b), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        assert L.pddc_demod_process(d._h, z.data_ptr(), b, b - 1, o.data_ptr(), b, st) == pkg.PDDC_ECAPACITY
        assert L.pddc_demod_process(d._h, z.data_ptr() + 4, b, n, o.data_ptr(), b, st) == pkg.PDDC_EINVAL
        assert L.pddc_demod_process(d._h, z.data_ptr(), b, n, o.data_ptr() + 2, b, st) == pkg.PDDC_EINVAL
        assert L.pddc_demod_process(d._h, None, b, n, o.data_ptr(), b, st) == pkg.PDDC_EINVAL
        assert L.pddc_demod_process(d._h, z.data_ptr(), b, n, None, b, st) == pkg.PDDC_EINVAL
        assert L.pddc_demod_process(d._h, None, 0, 0, None, 0, st) == pkg.PDDC_OK

    got = run(pkg, z, rx, cuts, disturb)
    assert torch.equal(bits(got), bits(clean))
    d = make(pkg, rx)                                          # reset starts the series again
    a = d.process(z)
    d.reset()
    b = d.process(z)
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(clean))
    d.close()
