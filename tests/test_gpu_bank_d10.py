"""GPU tests (-m gpu) of the channel bank's decimate-by-10 pairs (pddc_bank_*, include/perseus_ddc.h): the 1, 1.6 and
2 MS/s plans start with the tuned decimate-by-10 stage (route I8xD10), and two such members whose batch starts on the same
decimation phase share one k_fir_i8x_bank<64, 2, 10> launch -- one read of the batch.  Every banked member's outputs must
be the bits of the same pipeline processed alone (its I8xD10 route, layout 0), and within 1e-6 of full scale of the CPU
oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIR_TOL = 1e-6
FREGS = [381178347, 0x7FFFF000, 123456789, 0x80000C35, 3000000000, 1 << 28]
# rounds of multiples of 8 but not of 10: the first-output phase walks (offsets 0, 2, 4, 8, 4, 0, 2, 2, 6, 8, 0 from a
# fresh stream), with 8-sample rounds that have one stage-0 output and one that has none, and a 64-sample round
RAGGED = [10240 * 3 + 8, 8, 10240 * 260 + 16, 64, 10240 * 2 + 24, 8, 10240 * 5, 1016, 10240 * 300 + 8, 8, 10240 * 7 + 32]


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def plan(pkg, name):
    if name == "8*8*5":                    # decimate-by-8 first stage of 32 taps (hist 32)
        from conftest import load_taps
        return [(8, load_taps("c320_s1_d8_32")), (8, load_taps("c320_s2_d8_64")), (5, load_taps("c320_s3_d5_161"))]
    if name == "8*8*10":                   # 48 taps (hist 64)
        return [(8, lowpass(48, 0.05)), (8, lowpass(51, 0.05)), (10, lowpass(287, 0.04))]
    return pkg.api_plan({"1M": 1000000, "1.6M": 1600000, "2M": 2000000}[name])   # 10*8 (49 taps), 10*5 (51), 10*4 (54)


class Members:
    """pipelines of the named plans at FREGS[i] and their output tensors; bank rounds or solo rounds on the same inputs"""

    def __init__(self, pkg, dev, names, nmax, opts=None, fregs=None):
        import torch
        self.names = names
        self.stages = [plan(pkg, n) for n in names]
        self.fregs = fregs or [FREGS[i % len(FREGS)] for i in range(len(names))]
        self.pipes = []
        for st, f, nm in zip(self.stages, self.fregs, names):
            p = pkg.Pipeline(st, mix=True)
            p.set_freg(f)
            for k, v in ((opts or {}).get(nm) or {}).items():
                p.set_option(k, v)
            self.pipes.append(p)
        self.outs = [torch.empty((p.max_output(nmax) + 8, 2), dtype=torch.float32, device=dev) for p in self.pipes]
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def bank_round(self, bank, d_in, ns):
        import torch
        n, nb = bank.process_ptr(d_in.data_ptr(), ns, [o.data_ptr() for o in self.outs], [o.shape[0] for o in self.outs],
                                 self.stream)
        torch.cuda.synchronize()
        return [o[:k].cpu().numpy().copy() for o, k in zip(self.outs, n)], nb

    def solo_round(self, i, d_in, ns):
        import torch
        k = self.pipes[i].process_ptr(d_in.data_ptr(), ns, self.outs[i].data_ptr(), self.outs[i].shape[0], self.stream)
        torch.cuda.synchronize()
        return self.outs[i][:k].cpu().numpy().copy()

    def close(self):
        for p in self.pipes:
            p.close()


NO_FUSE2 = {"8*8*5": {"no_fuse2": 1}, "8*8*10": {"no_fuse2": 1}}     # the decimate-by-8 members' solo twins


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_round(O, packed, first_in, ns, stages, freg, got):
    r = O.chain_check(packed, first_in, ns, stages, got, freg=freg, mix=True, tol=FIR_TOL)
    assert r["n"] == got.shape[0] and r["ok"] and r["worst_chunk_rel_err"] <= FIR_TOL, r


def popcount(x):
    return bin(x).count("1")


@pytest.mark.parametrize("log2", [20, 24])
def test_two_2msps_members_share_one_launch(pkg, O, dev, log2):
    """two fresh 2 MS/s members: one bank launch for both, twice over the same batch; the second round's every output
    against the oracle"""
    ns = 1 << log2
    d_in = pkg.synth_lcg(6 * ns, 1010 + log2, 0, dev)
    m = Members(pkg, dev, ["2M", "2M"], ns)
    assert m.pipes[0].on_i8(ns) == 2                       # (the I8xD10 route alone)
    bank = pkg.Bank(m.pipes)
    assert bank.schedule(ns) == (0b11, 1)
    outs, nb = m.bank_round(bank, d_in, ns)
    assert nb == 2
    assert bank.schedule(ns) == (0b11, 1)
    outs, nb = m.bank_round(bank, d_in, ns)
    assert nb == 2
    packed = d_in.cpu().numpy()
    for i in range(2):
        check_round(O, packed, ns, ns, m.stages[i], m.fregs[i], outs[i])
    bank.close()
    m.close()


def test_histories_48_and_56_pair_up_through_ragged_rounds(pkg, dev):
    """1 M + 1.6 M + 2 M + 2 M (hist 48 / 56 / 56 / 56): two pairs, each channel 0 the longer history.  Ragged rounds walk
    the phase; a round without a stage-0 output leaves everybody unbanked.  Every output is the bits of a twin processed
    alone, and the save_state blobs agree at the end."""
    names = ["1M", "1.6M", "2M", "2M"]
    nmax = max(RAGGED)
    m = Members(pkg, dev, names, nmax)
    solo = Members(pkg, dev, names, nmax, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    assert bank.schedule(RAGGED[0]) == (0xF, 2)
    masks = []
    for r, ns in enumerate(RAGGED):
        d_in = pkg.synth_lcg(6 * ns, 300 + r, 0, dev)
        has_out = [p.on_i8(ns) == 2 for p in m.pipes]
        mask, launches = bank.schedule(ns)
        assert (mask, launches) == ((0xF, 2) if all(has_out) else (0, 0)), (r, ns, has_out)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == popcount(mask), (r, nb)
        masks.append(mask)
        for i in range(4):
            assert same_bits(outs[i], solo.solo_round(i, d_in, ns)), (r, ns, names[i])
    assert 0 in masks and masks.count(0xF) >= len(RAGGED) - 2, masks   # (the 8-sample round without an output went alone)
    for i in range(4):
        assert m.pipes[i].save_state() == solo.pipes[i].save_state(), names[i]
    bank.close()
    m.close()
    solo.close()


def test_mixed_bank_of_decimate_by_8_groups_and_decimate_by_10_pairs(pkg, dev):
    """hist 32 / 64 decimate-by-8 members and decimate-by-10 members in one bank: the 8s grouped by history, the 10s
    paired (the odd one alone); each member the bits of its solo twin (no_fuse2 = 1 for the 8s)"""
    names = ["8*8*5", "2M", "8*8*10", "1.6M", "8*8*5", "1M"]
    nmax = 1 << 20
    m = Members(pkg, dev, names, nmax)
    solo = Members(pkg, dev, names, nmax, opts=NO_FUSE2, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    # hist 32: members 0, 4 (a pair); hist 64: member 2 (alone, a launch of the solo kernel); /10: 1 and 3 (hist 56) a
    # pair, 5 (hist 48) without a partner
    for r, ns in enumerate([1 << 20, 8 * 100003, 1 << 20]):
        assert bank.schedule(ns) == (0b011111, 3), r
        d_in = pkg.synth_lcg(6 * ns, 40 + r, 0, dev)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == 5
        for i in range(len(names)):
            assert same_bits(outs[i], solo.solo_round(i, d_in, ns)), (r, names[i])
    for i in range(len(names)):
        assert m.pipes[i].save_state() == solo.pipes[i].save_state(), names[i]
    bank.close()
    m.close()
    solo.close()


def test_members_of_different_phases_are_never_paired(pkg, O, dev):
    """member 0 processes a lone 8-sample batch outside the bank: unaligned for one round, and from then on its first
    outputs sit on another phase than its partner's -- never paired again; both correct and the bits of their twins"""
    ns = 8 * 123457
    names = ["2M", "2M"]
    m = Members(pkg, dev, names, ns)
    solo = Members(pkg, dev, names, ns, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    ins = [pkg.synth_lcg(6 * ns, 500 + r, 0, dev) for r in range(4)]
    extra = pkg.synth_lcg(6 * 8, 9, 0, dev)
    streams, got = [[], []], [[], []]
    for r, d_in in enumerate(ins):
        if r == 1:
            y = m.solo_round(0, extra, 8)
            assert same_bits(y, solo.solo_round(0, extra, 8))
            streams[0].append(extra.cpu().numpy())
            got[0].append(y)
        assert bank.schedule(ns) == ((0b11, 1) if r == 0 else (0, 0)), r
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == (2 if r == 0 else 0), r
        for i in range(2):
            assert same_bits(outs[i], solo.solo_round(i, d_in, ns)), (r, i)
            streams[i].append(d_in.cpu().numpy())
            got[i].append(outs[i])
    for i in range(2):
        y = np.concatenate(got[i]).reshape(-1)
        ref = O.ddc_chain(np.concatenate(streams[i]), m.stages[i], freg=m.fregs[i], mix=True)
        assert y.size == ref.size and O.rel_err(y, ref) <= FIR_TOL, i
        assert m.pipes[i].save_state() == solo.pipes[i].save_state(), i
    bank.close()
    m.close()
    solo.close()


def test_retune_in_the_history_window_goes_alone_for_one_round(pkg, O, dev):
    """member 0 retuned between rounds: two words in its next history window, so that round goes alone (its partner then
    has none); the round after pairs them again.  Member 0 follows the retuned oracle, member 1 is the bits of its twin."""
    ns = 1 << 20
    names = ["2M", "2M"]
    m = Members(pkg, dev, names, ns)
    solo = Members(pkg, dev, names[1:], ns, fregs=m.fregs[1:])
    bank = pkg.Bank(m.pipes)
    d_in = pkg.synth_lcg(6 * ns, 4711, 0, dev)
    new_word = 987654321
    got = []
    for r, want in enumerate([(0b11, 1), (0, 0), (0b11, 1)]):
        if r == 1:
            m.pipes[0].set_freg(new_word)                     # at sample ns: inside the next batch's history window
        assert bank.schedule(ns) == want, r
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == popcount(want[0]), r
        assert same_bits(outs[1], solo.solo_round(0, d_in, ns)), r
        got.append(outs[0])
    packed = d_in.cpu().numpy()
    ref = O.ddc_chain_retuned(np.concatenate([packed] * 3), m.stages[0], [(0, m.fregs[0]), (ns, new_word)])
    y = np.concatenate(got).reshape(-1)
    assert y.size == ref.size and O.rel_err(y, ref) <= FIR_TOL
    bank.close()
    m.close()
    solo.close()


@pytest.mark.parametrize("names,mask", [(["2M"], 0), (["1M", "2M", "2M"], 0b110), (["2M", "1M", "1.6M"], 0b101)])
def test_a_member_without_a_partner_goes_alone(pkg, O, dev, names, mask):
    """a lone decimate-by-10 member, or the third of one phase (the shortest history is left out), runs alone; all
    correct against the oracle"""
    ns = 1 << 20
    m = Members(pkg, dev, names, ns)
    bank = pkg.Bank(m.pipes)
    d_in = pkg.synth_lcg(6 * ns, 77, 0, dev)
    for _ in range(2):
        assert bank.schedule(ns) == (mask, 1 if mask else 0)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == popcount(mask)
    packed = d_in.cpu().numpy()
    for i in range(len(names)):
        check_round(O, packed, ns, ns, m.stages[i], m.fregs[i], outs[i])
    bank.close()
    m.close()


def test_repeated_rounds_give_identical_bits(pkg, dev):
    """five pair rounds at 2^24 from the same input and state (fresh members each time): identical bits"""
    ns = 1 << 24
    d_in = pkg.synth_lcg(6 * ns, 2025, 0, dev)
    first = None
    for _ in range(5):
        m = Members(pkg, dev, ["2M", "1.6M"], ns)
        bank = pkg.Bank(m.pipes)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == 2
        digest = [o.tobytes() for o in outs]
        bank.close()
        m.close()
        if first is None:
            first = digest
        assert digest == first


def test_full_size_pair_against_the_oracle(pkg, O, dev):
    """2^27 samples, two 2 MS/s members (the second round: the batch's own tail as history): every output"""
    ns = 1 << 27
    d_in = pkg.synth_lcg(6 * ns, 27, 0, dev)
    m = Members(pkg, dev, ["2M", "2M"], ns)
    bank = pkg.Bank(m.pipes)
    for _ in range(2):
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == 2
    packed = d_in.cpu().numpy()
    for i in range(2):
        check_round(O, packed, ns, ns, m.stages[i], m.fregs[i], outs[i])
    bank.close()
    m.close()


@pytest.mark.perf
@pytest.mark.parametrize("log2", [24, 28])
def test_pair_round_against_two_solo_rounds(pkg, dev, perf_record, log2):
    """record: a round of two 2 MS/s members through the bank (one k_fir_i8x_bank<64, 2, 10> launch) against the same two
    members each processed alone (two reads); fails only on gross breakage (the bank 25 % slower)"""
    import torch
    ns = 1 << log2
    d_in = pkg.synth_lcg(6 * ns, 6, 0, dev)
    m = Members(pkg, dev, ["2M", "2M"], ns)
    solo = Members(pkg, dev, ["2M", "2M"], ns, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    st = torch.cuda.current_stream(dev)
    outs = [o.data_ptr() for o in m.outs]
    caps = [o.shape[0] for o in m.outs]
    assert bank.schedule(ns) == (0b11, 1)

    def timed(fn, reps=15):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    t_bank = timed(lambda: bank.process_ptr(d_in.data_ptr(), ns, outs, caps, m.stream))
    t_two = timed(lambda: [p.process_ptr(d_in.data_ptr(), ns, o.data_ptr(), o.shape[0], solo.stream)
                           for p, o in zip(solo.pipes, solo.outs)])
    perf_record("d10_pair_bank_round_ms", t_bank, unit="ms", k=2, nsamples=ns)
    perf_record("d10_two_solo_rounds_ms", t_two, unit="ms", k=2, nsamples=ns)
    bank.close()
    m.close()
    solo.close()
    assert t_bank < 1.25 * t_two, (t_bank, t_two)
