"""GPU tests (-m gpu) of the channel bank (pddc_bank_*, include/perseus_ddc.h): several tuned receivers fed the SAME
batch, whose first stages -- the tuned decimate-by-8 on the matrix cores, <= 64 taps -- come from one read of it
(k_fir_i8x_bank, up to four per launch).  Every member's outputs must be the bits of the same pipeline processed alone
with no_fuse2 = 1 (k_fir_i8x alone, then the per-stage kernels), and within 1e-6 of full scale of the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_taps

pytestmark = pytest.mark.gpu
FIR_TOL = 1e-6
# 0 Hz, both band edges (just below +fs/2, just above -fs/2), and words in between
FREGS = [0, 0x7FFFF000, 0x80000C35, 381178347, 1 << 28, 3000000000, 123456789, 0xFFFFF3CB]


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def plans():
    h1, h2, h3 = load_taps("c320_s1_d8_32"), load_taps("c320_s2_d8_64"), load_taps("c320_s3_d5_161")
    return {
        "8*8*5": [(8, h1), (8, h2), (5, h3)],                                                  # 32 taps, hist 32
        "8*8*10": [(8, lowpass(48, 0.05)), (8, lowpass(51, 0.05)), (10, lowpass(287, 0.04))],  # 48 taps, hist 64
        "8*8": [(8, h1), (8, h2)],
        "8*7": [(8, h1), (7, lowpass(57, 0.06))],                                              # generic decimator behind
        "10*5m": [(10, lowpass(51, 0.04)), (5, lowpass(117, 0.08))],                           # /10: never banked
        "8/48": [(8, lowpass(48, 0.05))],                                                      # the first stage alone
    }


PLAN_CYCLE = ["8*8*5", "8*8*10", "8*8", "8*7"]


def member_plans(k):
    return [PLAN_CYCLE[i % len(PLAN_CYCLE)] for i in range(k)]


class Members:
    """k pipelines at FREGS[i], their output tensors; run bank rounds or solo rounds on the same inputs"""

    def __init__(self, pkg, dev, names, nmax, opts=None, fregs=None):
        import torch
        self.names = names
        self.stages = [plans()[n] for n in names]
        self.fregs = fregs or [FREGS[i % len(FREGS)] for i in range(len(names))]
        self.pipes = []
        for st, f in zip(self.stages, self.fregs):
            p = pkg.Pipeline(st, mix=True)
            p.set_freg(f)
            for k, v in (opts or {}).items():
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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_round(O, packed, first_in, ns, stages, freg, got):
    r = O.chain_check(packed, first_in, ns, stages, got, freg=freg, mix=True, tol=FIR_TOL)
    assert r["n"] == got.shape[0] and r["ok"] and r["worst_chunk_rel_err"] <= FIR_TOL, r


@pytest.mark.parametrize("k,log2", [(1, 24), (2, 24), (3, 24), (4, 24), (6, 24), (8, 24), (4, 26)])
def test_every_member_matches_the_oracle(pkg, O, dev, k, log2):
    """two rounds of the same batch (zero history, then the batch's own tail as history); the second round's every output
    of every member against the double oracle, per chunk"""
    ns = 1 << log2
    d_in = pkg.synth_lcg(6 * ns, 4242 + k, 0, dev)
    m = Members(pkg, dev, member_plans(k), ns)
    bank = pkg.Bank(m.pipes)
    assert bank.schedule(ns)[0] == (1 << k) - 1
    outs, nb = m.bank_round(bank, d_in, ns)
    assert nb == k
    outs, nb = m.bank_round(bank, d_in, ns)
    assert nb == k
    packed = d_in.cpu().numpy()
    for i in range(k):
        check_round(O, packed, ns, ns, m.stages[i], m.fregs[i], outs[i])
    bank.close()
    m.close()


RAGGED = [8 * 12345, 1 << 20, 8 * 100003, 8 * 8191 + 8 * 8192, 3 << 18, 8 * 77777]


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_members_are_bit_identical_to_solo_no_fuse2(pkg, dev, k):
    """several rounds of ragged sizes (8 k samples, not whole tiles), a new batch each round: every member's every output
    is the bits of the same pipeline processed alone with no_fuse2 = 1"""
    nmax = max(RAGGED)
    names = member_plans(k)
    m = Members(pkg, dev, names, nmax)
    solo = Members(pkg, dev, names, nmax, opts={"no_fuse2": 1}, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    for r, ns in enumerate(RAGGED):
        d_in = pkg.synth_lcg(6 * ns, 99 + r, 0, dev)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == k, (r, nb)
        for i in range(k):
            ref = solo.solo_round(i, d_in, ns)
            assert same_bits(outs[i], ref), (k, r, i, names[i])
    for i in range(k):
        assert m.pipes[i].save_state() == solo.pipes[i].save_state()
    bank.close()
    m.close()
    solo.close()


@pytest.mark.parametrize("k,mask,launches", [(4, 0xF, 1), (6, 0x3F, 2), (8, 0xFF, 2), (3, 0x7, 2)])
def test_schedule_groups_by_four_two_one(pkg, dev, k, mask, launches):
    # all members of one history length (hist 32): groups of 4, 2, 1
    m = Members(pkg, dev, ["8*8*5"] * k, 1 << 20)
    bank = pkg.Bank(m.pipes)
    assert bank.schedule(1 << 20) == (mask, launches)
    d_in = pkg.synth_lcg(6 << 20, 5, 0, dev)
    assert m.bank_round(bank, d_in, 1 << 20)[1] == k
    bank.close()
    m.close()


def test_unbanked_members_go_alone_and_stay_correct(pkg, O, dev):
    """a /10 member and a member retuned inside its history window are reported unbanked, run on their own in the same
    round, and are correct; the retuned one is banked again in the round after"""
    ns = 1 << 20
    names = ["8*8*5", "8*8*10", "10*5m", "8*8"]
    m = Members(pkg, dev, names, ns)
    bank = pkg.Bank(m.pipes)
    d_in = pkg.synth_lcg(6 * ns, 31337, 0, dev)
    assert bank.schedule(ns) == (0b1011, 2)                   # hist 32: members 0, 3 (one launch of 2); hist 64: member 1
    outs0, nb = m.bank_round(bank, d_in, ns)
    assert nb == 3
    new_word = 987654321
    m.pipes[3].set_freg(new_word)                             # at sample ns: inside the next batch's history window
    assert bank.schedule(ns) == (0b0011, 2)
    outs1, nb = m.bank_round(bank, d_in, ns)
    assert nb == 2
    assert bank.schedule(ns) == (0b1011, 2)
    outs2, nb = m.bank_round(bank, d_in, ns)
    assert nb == 3
    packed = d_in.cpu().numpy()
    for i in range(3):
        check_round(O, packed, ns, ns, m.stages[i], m.fregs[i], outs1[i])
    got = np.concatenate([outs0[3], outs1[3], outs2[3]])
    ref = O.ddc_chain_retuned(np.concatenate([packed] * 3), m.stages[3], [(0, m.fregs[3]), (ns, new_word)])
    assert O.rel_err(got.reshape(-1), ref) <= FIR_TOL
    bank.close()
    m.close()


def test_retune_between_rounds(pkg, O, dev):
    """one member retuned between rounds follows ddc_chain_retuned; the others are the bits of a bank without the retune"""
    ns = 1 << 20
    names = member_plans(4)
    a = Members(pkg, dev, names, ns)
    b = Members(pkg, dev, names, ns, fregs=a.fregs)
    ba, bb = pkg.Bank(a.pipes), pkg.Bank(b.pipes)
    ins = [pkg.synth_lcg(6 * ns, 700 + r, 0, dev) for r in range(3)]
    new_word = 2222222222
    got_a, got_b = [], []
    for r, d_in in enumerate(ins):
        if r == 1:
            a.pipes[1].set_freg(new_word)
        got_a.append(a.bank_round(ba, d_in, ns)[0])
        got_b.append(b.bank_round(bb, d_in, ns)[0])
    for r in range(3):
        for i in (0, 2, 3):
            assert same_bits(got_a[r][i], got_b[r][i]), (r, i)
    packed = np.concatenate([d.cpu().numpy() for d in ins])
    y = np.concatenate([got_a[r][1] for r in range(3)]).reshape(-1)
    ref = O.ddc_chain_retuned(packed, a.stages[1], [(0, a.fregs[1]), (ns, new_word)])
    assert O.rel_err(y, ref) <= FIR_TOL
    ba.close()
    bb.close()
    a.close()
    b.close()


def test_a_member_pushed_alone_is_unaligned_for_one_round(pkg, dev):
    """member 2 processes a different batch outside the bank: the next round takes it alone (n_banked = K - 1), correct,
    and the round after banks it again; its outputs are the bits of a solo no_fuse2 pipeline given the same sequence"""
    ns = 1 << 20
    names = member_plans(4)
    m = Members(pkg, dev, names, ns)
    solo = Members(pkg, dev, names, ns, opts={"no_fuse2": 1}, fregs=m.fregs)
    bank = pkg.Bank(m.pipes)
    ins = [pkg.synth_lcg(6 * ns, 50 + r, 0, dev) for r in range(3)]
    other = pkg.synth_lcg(6 * ns, 12345, 0, dev)
    outs, nb = m.bank_round(bank, ins[0], ns)
    assert nb == 4
    for i in range(4):
        assert same_bits(outs[i], solo.solo_round(i, ins[0], ns)), i
    m.pipes[2].set_option("no_fuse2", 1)                  # (its batch alone takes the solo pipeline's route)
    assert same_bits(m.solo_round(2, other, ns), solo.solo_round(2, other, ns))
    assert bank.schedule(ns) == (0b1011, 2)
    for r, want in ((1, 3), (2, 4)):
        outs, nb = m.bank_round(bank, ins[r], ns)
        assert nb == want, (r, nb)
        for i in range(4):
            assert same_bits(outs[i], solo.solo_round(i, ins[r], ns)), (r, i)
    bank.close()
    m.close()
    solo.close()


def test_leave_and_continue_alone(pkg, dev):
    """member 1 is retuned between bank rounds (its next round goes alone: two words in its history window, then it is
    banked again), and after five rounds it continues alone: bit-identical to a pipeline that ran alone throughout with
    no_fuse2 = 1 and got the same retune, and the two save_state blobs are equal -- in the bank and after it"""
    ns = 8 * 98765
    names = member_plans(4)
    m = Members(pkg, dev, names, ns, opts={"no_fuse2": 1})   # (the retuned round goes alone: the solo twin's route then)
    solo = Members(pkg, dev, [names[1]], ns, opts={"no_fuse2": 1}, fregs=[m.fregs[1]])
    bank = pkg.Bank(m.pipes)
    new_word = 2718281828
    for r in range(5):
        if r == 2:
            m.pipes[1].set_freg(new_word)
            solo.pipes[0].set_freg(new_word)
        d_in = pkg.synth_lcg(6 * ns, 1000 + r, 0, dev)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == (3 if r == 2 else 4), (r, nb)
        assert same_bits(outs[1], solo.solo_round(0, d_in, ns)), r
    assert m.pipes[1].save_state() == solo.pipes[0].save_state()
    for r in range(5, 7):
        d_in = pkg.synth_lcg(6 * ns, 1000 + r, 0, dev)
        assert same_bits(m.solo_round(1, d_in, ns), solo.solo_round(0, d_in, ns)), r
    assert m.pipes[1].save_state() == solo.pipes[0].save_state()
    bank.close()
    m.close()
    solo.close()


def test_refused_rounds_move_nothing_and_early_destroy_detaches(pkg, dev):
    import torch
    L = pkg.ddc_lib()
    ns = 1 << 18
    m = Members(pkg, dev, member_plans(3), ns)
    bank = pkg.Bank(m.pipes)
    d_in = pkg.synth_lcg(6 * ns, 77, 0, dev)
    m.bank_round(bank, d_in, ns)
    before = [p.save_state() for p in m.pipes]
    outs = [o.data_ptr() for o in m.outs]
    caps = [o.shape[0] for o in m.outs]
    with pytest.raises(pkg.PddcError) as e:
        bank.process_ptr(d_in.data_ptr(), ns + 4, outs, caps)           # not a multiple of 8
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        bank.process_ptr(d_in.data_ptr(), ns, outs[:2] + [0], caps)     # a null output
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        bank.process_ptr(d_in.data_ptr(), ns, outs, caps[:2] + [10])    # capacity
    assert e.value.code == pkg.PDDC_ECAPACITY
    n = (C.c_size_t * 3)()
    nb = C.c_int()
    assert L.pddc_bank_process(bank._h, d_in.data_ptr(), ns, None, None, n, C.byref(nb), None) == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        pkg.Bank([m.pipes[0]])                                            # a member in two banks
    assert e.value.code == pkg.PDDC_ESTATE
    assert [p.save_state() for p in m.pipes] == before                   # refused: nobody moved
    # overlap mode with a tail held back (k_fir8's pair carries the 8*8*5 plan's last stage into its next launch)
    p0 = m.pipes[0]
    p0.set_option("i8x", 0)
    p0.set_overlap(True)
    p0.process_ptr(d_in.data_ptr(), ns, outs[0], caps[0], m.stream)
    with pytest.raises(pkg.PddcError) as e:
        bank.process_ptr(d_in.data_ptr(), ns, outs, caps, m.stream)
    assert e.value.code == pkg.PDDC_ESTATE and b"overlap" in L.pddc_last_error()
    p0.fence(m.stream)
    torch.cuda.synchronize()
    assert [p.save_state() for p in m.pipes[1:]] == before[1:]
    # a member destroyed before its bank: detached, further rounds refused, the bank still closes
    m.pipes[2].close()
    with pytest.raises(pkg.PddcError) as e:
        bank.process_ptr(d_in.data_ptr(), ns, outs, caps)
    assert e.value.code == pkg.PDDC_ESTATE
    assert bank.schedule(ns) == (0, 0)
    bank.close()
    m.close()


def test_repeated_rounds_give_identical_bits(pkg, dev):
    """ten K = 4 rounds at 2^24 from the same input and state (fresh members each time): identical bits"""
    ns = 1 << 24
    d_in = pkg.synth_lcg(6 * ns, 2024, 0, dev)
    first = None
    for _ in range(10):
        m = Members(pkg, dev, member_plans(4), ns)
        bank = pkg.Bank(m.pipes)
        outs, nb = m.bank_round(bank, d_in, ns)
        assert nb == 4
        digest = [o.tobytes() for o in outs]
        bank.close()
        m.close()
        if first is None:
            first = digest
        assert digest == first


@pytest.mark.perf
def test_bank_round_beats_four_reads(pkg, dev, perf_record):
    """record-only bound against gross breakage: a K = 4 bank round at 2^26 (four tuned 48-tap first stages, one launch)
    takes less than 0.8x the same four members reading the batch four times, each processed alone.  (This deviates from
    the gang round of the issue on purpose: a gang round cannot be timed from here -- it runs on the gang's own stream with
    its generator and copies; K solo reads are the traffic of its k_fir_i8x_many launch.  The gang's kernel itself is
    timed against the bank from a kernel trace: tools/bank_time.py --legs / --summarize, profiles/r07.)  Measured on
    MI355X: 0.235 against 0.371 ms (profiles/r07/bank_time.txt)"""
    import torch
    ns = 1 << 26
    d_in = pkg.synth_lcg(6 * ns, 6, 0, dev)
    names = ["8/48"] * 4
    m = Members(pkg, dev, names, ns)
    solo = Members(pkg, dev, names, ns, opts={"no_fuse2": 1}, fregs=m.fregs)
    assert m.pipes[0].on_i8(ns) == 2
    bank = pkg.Bank(m.pipes)
    st = torch.cuda.current_stream(dev)

    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        return best

    outs = [o.data_ptr() for o in m.outs]
    caps = [o.shape[0] for o in m.outs]
    t_bank = timed(lambda: bank.process_ptr(d_in.data_ptr(), ns, outs, caps, m.stream))
    t_four = timed(lambda: [p.process_ptr(d_in.data_ptr(), ns, o.data_ptr(), o.shape[0], solo.stream)
                            for p, o in zip(solo.pipes, solo.outs)])
    perf_record("bank_round_ms", t_bank, unit="ms", k=4, nsamples=ns)
    perf_record("four_solo_ms", t_four, unit="ms", k=4, nsamples=ns)
    bank.close()
    m.close()
    solo.close()
    assert t_bank < 0.8 * t_four, (t_bank, t_four)
