"""GPU tests (-m gpu) of the front end at stream positions past 2^31 and 2^32 samples (27 s and 54 s of the 80 MS/s ADC
stream; 125 * 2^32 is two hours, 125 * 2^41 forty days).  The pipeline carries a 64-bit sample counter and every kernel
narrows it to 32 bits in its own way -- (n0lo + K (t 1024 + o)) freg + phase_off in k_fir_i8x, (uint32_t)nabs * freg in
k_fir8's mixer, phase_off + (uint32_t)n0 (freg - freg_hist) behind a retune, n0 + in_off of the decimate-by-10 form, the
word segments' n_begin against n0 - hist, the resampler's (m0 + q) M and t / L - consumed -- and every other test starts
its stream at sample 0.  pddc_pipeline_seek places a stream anywhere at no cost, so every route of the front end runs
here across each edge, through retunes at and around it, and a whole number of phase periods away from a stream that
began at 0 (bit for bit).  Reference: tests/deep_ref.py (the oracle's mixer from an absolute start, checked on the CPU
in test_deep_ref_cpu.py); bar: max|y - ref| / max|ref| <= 1e-6, the bar of every front-end test, or equal bits.  The
stages behind the tuner have no seek and are not covered."""
import importlib

import numpy as np
import pytest

import deep_ref as D
from deep_ref import FIR_TOL

pytestmark = pytest.mark.gpu
EDGE_IDS = {2**31: "2p31", 2**32: "2p32", 125 * 2**32: "125x2p32", 125 * 2**41: "125x2p41"}

# the queries that put a row of the route table on its route, for a batch of n samples
QUERIES = {
    "i8x":       lambda p, n: p.on_i8(n) == 2 and p.fused_pair(n) == 0,
    "i8x_48":    lambda p, n: p.on_i8(n) == 2 and p.fused_pair(n) == 0,
    "i8x_255":   lambda p, n: p.on_i8(n) == 2 and p.fused_pair(n) == 0,
    "fir8":      lambda p, n: p.fused and p.on_i8(n) == 0,
    "i8x_pair":  lambda p, n: p.fused_pair(n) == 2,
    "fir8_pair": lambda p, n: p.fused_pair(n) == 1 and not p.fused_cascade(n),
    "fused3":    lambda p, n: p.fused_cascade(n),
    "i8x_d10":   lambda p, n: not p.fused and p.on_i8(n) == 2,
    "firp":      lambda p, n: p.stage0_reads_packed and not p.fused and p.on_i8(n) == 0,
    "generic7":  lambda p, n: p.stage0_reads_packed and not p.fused and p.on_i8(n) == 0,
    "unpack":    lambda p, n: not p.stage0_reads_packed,
    "rational":  lambda p, n: p.on_i8(n) == 2,
}
assert sorted(QUERIES) == sorted(D.ROUTE_NAMES)


@pytest.fixture(scope="module")
def R():
    return D.routes()


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_pipe(pkg, row):
    p = pkg.Pipeline(row["stages"], mix=True, no_fast=row["no_fast"])
    for k, v in row["opts"].items():
        p.set_option(k, v)
    return p


def place(p, case):
    """seek, then the stream's first word (a stream from 0 is a fresh pipeline: no seek at all)"""
    if case["start"]:
        p.seek(case["start"])
    p.set_freg(case["segments"][0][1])
    assert p.phase_offset == 0


def run_case(pkg, dev, O, route, row, case, on_route=True, rec=None):
    """One stream of a case on a pipeline of its own: every batch on its route where asked (the batch behind a retune takes
    the kernel that re-mixes the history, so it is not asked), the phase offset behind every retune against exact
    integers.  -> float32 outputs, flat."""
    cuts = D.check_case(case)
    packed = D.stream_bytes(O, cuts[-1] - cuts[0])
    p = make_pipe(pkg, row)
    place(p, case)
    parts = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        n = b - a
        if k in case["retune_at"]:
            p.set_freg(case["retune_at"][k])
            assert p.phase_offset == D.exact_phase_offset(case["segments"], a), (route, k, a)
        elif on_route:
            assert QUERIES[route](p, n), (route, k, n)
        if rec is not None:
            rec.append(p.on_i8(n))
        parts.append(p.process(to_dev(packed[6 * (a - cuts[0]):6 * (b - cuts[0])], dev)).cpu().numpy().reshape(-1))
    p.check()
    p.close()
    return np.concatenate(parts)


def against_reference(O, key, stages, case, y, what):
    ref = D.reference(O, key, stages, case)
    err = O.rel_err(y, ref)
    print(f"deep stream: {what}: rel err {err:.3e} over {ref.size // 2} outputs")
    assert y.size == ref.size, (what, y.size, ref.size)
    assert err <= FIR_TOL, (what, err)
    return err


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("E", D.EDGES, ids=[EDGE_IDS[E] for E in D.EDGES])
@pytest.mark.parametrize("route", D.ROUTE_NAMES)
def test_every_route_across_every_edge(pkg, dev, O, R, route, E):
    """seek(start_for(E, u)), the word, four batches [u, 2u, u, last] with E strictly inside the second: every output
    against deep_chain from the same absolute sample"""
    row = R[route]
    case = D.edge_case(route, row, E)
    y = run_case(pkg, dev, O, route, row, case)
    against_reference(O, f"edge/{route}/{E}", row["stages"], case, y,
                      f"{route} across {EDGE_IDS[E]}, word {case['segments'][0][1]:#x}")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("form", ["boundaries", "storm32"])
@pytest.mark.parametrize("E", [2**32, 125 * 2**32], ids=["2p32", "125x2p32"])
@pytest.mark.parametrize("route", D.RETUNE_ROUTES)
def test_retunes_at_and_around_the_edge(pkg, dev, O, R, route, E, form):
    """boundaries: a new word before the batch that starts at E - 8, at E and at E + 8 (at E = 2^32 the host multiplies by
    (uint32_t)n0 == 0).  Each of the three alone, between two long batches: the batch behind it mixes its packed history
    with the old word and its own samples with the new one -- k_fir_i8x's row reads 2, 0, 2 (k_fir8's re-mix ran at
    depth), as in test_retune_between_batches_goes_through_the_vector_kernel_once; then all three in one stream, 8 samples
    apart.  storm32: batches of 32 samples, a new word before each of three consecutive ones, the first at E: three words
    in one history window, the mixed-history route at depth (test_packed_first_stage_through_retunes, nb = 32).  The phase
    offset behind every retune equals sum n (w_old - w_new) mod 2^32 in exact integers (run_case)."""
    row = R[route]
    if form == "storm32":
        case = D.storm_case(row, E)
        y = run_case(pkg, dev, O, route, row, case, on_route=False)
        against_reference(O, f"storm/{route}/{E}", row["stages"], case, y, f"{route} retune storm at {EDGE_IDS[E]}")
        return
    for b in (E - 8, E, E + 8):
        case = D.boundary_case(row, E, b)
        rec = []
        y = run_case(pkg, dev, O, route, row, case, rec=rec)
        print(f"deep stream: {route} retune at {EDGE_IDS[E]}{b - E:+d}: on_i8 per batch {rec}")
        if route == "i8x":
            assert rec == [2, 0, 2], rec
        against_reference(O, f"boundary/{route}/{E}/{b - E}", row["stages"], case, y, f"{route} retune at {EDGE_IDS[E]}{b - E:+d}")
    case = D.three_boundaries_case(row, E)
    y = run_case(pkg, dev, O, route, row, case, on_route=False)
    against_reference(O, f"three/{route}/{E}", row["stages"], case, y, f"{route} retunes at {EDGE_IDS[E]} -8, +0, +8")


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("route", D.ROUTE_NAMES)
def test_a_shift_by_a_whole_number_of_phase_periods_changes_no_bit(pkg, dev, O, R, route):
    """delta = lcm(u, 2^32) leaves every 32-bit phase alone and stays on the grid.  (i) a stream at seek(k delta), k = 1 and
    2^9, is the bits of a fresh stream from 0 over the same bytes, words and cuts; (ii) a stream at seek(delta - 2u), which
    crosses delta in its second batch, is the bits of one at seek(2^9 delta - 2u); one retune behind the crossing in each.
    No tolerance to hide behind.  (The stream from 0 also gives the route's error at position 0, next to which the errors
    at depth are read.)"""
    row = R[route]
    cases = D.shift_cases(route, row)
    ys = {key: run_case(pkg, dev, O, route, row, case) for key, case in cases.items()}
    e0 = against_reference(O, f"shift/{route}/0", row["stages"], cases["0"], ys["0"], f"{route} from position 0")
    e1 = against_reference(O, f"shift/{route}/d-2u", row["stages"], cases["d-2u"], ys["d-2u"], f"{route} across delta")
    print(f"deep stream: {route}: rel err at position 0 {e0:.3e}, across lcm(u, 2^32) {e1:.3e}")
    assert same_bits(ys["d"], ys["0"]), route
    assert same_bits(ys["512d"], ys["0"]), route
    assert same_bits(ys["512d-2u"], ys["d-2u"]), route
    assert not same_bits(ys["d-2u"], ys["0"])               # (another phase: the comparison can tell streams apart)


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("route", ["i8x_pair", "rational"])
def test_checkpoint_taken_past_the_edge_resumes_bit_identically(pkg, dev, O, R, route):
    """seek(start_for(2^32, u)), two batches (the stream is across 2^32), save_state; restored into a new pipeline, the
    rest is bit-identical on both, the whole stream within the bar of deep_chain, and so is one more batch behind a retune
    of both: StateHeader's n0 and the stages' `consumed` are 64 bits wide all the way."""
    row = R[route]
    case = D.checkpoint_case(row)
    cuts = D.check_case(case)
    packed = D.stream_bytes(O, cuts[-1] - cuts[0])
    batch = [to_dev(packed[6 * (a - cuts[0]):6 * (b - cuts[0])], dev) for a, b in zip(cuts[:-1], cuts[1:])]
    a = make_pipe(pkg, row)
    place(a, case)
    ya = []
    for k in (0, 1):
        assert QUERIES[route](a, case["sizes"][k])
        ya.append(a.process(batch[k]).cpu().numpy())
    assert cuts[2] > 2**32
    blob = a.save_state()
    b = make_pipe(pkg, row)
    b.restore_state(blob)
    assert b.freg == a.freg and b.phase_offset == a.phase_offset == 0
    for k in (2, 3, 4):
        if k in case["retune_at"]:
            for p in (a, b):
                p.set_freg(case["retune_at"][k])
                assert p.phase_offset == D.exact_phase_offset(case["segments"], cuts[k])
        else:
            assert QUERIES[route](a, case["sizes"][k]) and QUERIES[route](b, case["sizes"][k])
        ya.append(a.process(batch[k]).cpu().numpy())
        yb = b.process(batch[k]).cpu().numpy()
        assert same_bits(ya[-1], yb), (route, k)
    assert a.save_state() == b.save_state()
    for p in (a, b):
        p.check()
        p.close()
    against_reference(O, f"checkpoint/{route}", row["stages"], case, np.concatenate(ya).reshape(-1),
                      f"{route} through a checkpoint past 2p32")


# ------------------------------------------------------------------------------------------------ 5
def test_bank_and_gang_members_at_depth(pkg, dev, O, R):
    """Bank: two tuned d8_127 members with different words, both at start_for(2^32, 8192) -- and, because the bank's shared
    launch takes first stages of up to 64 taps only (a 127-tap member runs its own launch inside the round), two 48-tap
    members beside them, which bank.schedule reports sharing a launch from the first round: FirI8xBankCh::n0 at depth.
    Every member's every output is the bits of a solo pipeline at the same position, and within the bar of deep_chain.
    Gang: the two d8_127 members, host-fed, through Gang.push_async against solo pushes, bit for bit."""
    import torch
    names = ["i8x", "i8x", "i8x_48", "i8x_48"]
    words = [D.WORDS[0], D.WORDS[1], D.WORDS[1], D.WORDS[0]]
    cases = [D.member_case(w) for w in words]
    cuts = D.check_case(cases[0])
    sizes = cases[0]["sizes"]
    packed = D.stream_bytes(O, cuts[-1] - cuts[0])
    st = torch.cuda.current_stream(dev).cuda_stream

    def members():
        ps = [make_pipe(pkg, R[n]) for n in names]
        for p, c in zip(ps, cases):
            place(p, c)
        return ps

    banked, solo = members(), members()
    outs = [torch.empty((p.max_output(max(sizes)) + 8, 2), dtype=torch.float32, device=dev) for p in banked]
    bank = pkg.Bank(banked)
    got = [[] for _ in names]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        n = b - a
        d_in = to_dev(packed[6 * (a - cuts[0]):6 * (b - cuts[0])], dev)
        mask, launches = bank.schedule(n)
        print(f"deep stream: bank round {k}: {n} samples, mask {mask:#06b}, {launches} shared launches")
        assert mask & 0b1100 == 0b1100 and launches >= 1, (k, mask)        # the two 48-tap members share a launch
        n_out, nb = bank.process_ptr(d_in.data_ptr(), n, [o.data_ptr() for o in outs], [o.shape[0] for o in outs], st)
        torch.cuda.synchronize()
        assert nb == bin(mask).count("1")
        for i, p in enumerate(solo):
            y = outs[i][:n_out[i]].cpu().numpy().copy()
            assert same_bits(y, p.process(d_in).cpu().numpy()), (k, i)
            got[i].append(y.reshape(-1))
    for i in range(len(names)):
        assert banked[i].save_state() == solo[i].save_state()
        against_reference(O, f"member/{names[i]}/{words[i]}", R[names[i]]["stages"], cases[i], np.concatenate(got[i]),
                          f"bank member {i} ({names[i]}, word {words[i]:#x}) past 2p32")
    bank.close()
    for p in banked + solo:
        p.close()

    # the gang: host-fed members (test_gang_host_fed_members_and_change_between_gang_and_solo), one round per batch
    ganged, solo = members()[:2], members()[:2]
    cap = ganged[0].max_output(max(sizes)) + 8
    hin = pkg.PinnedBuffer(6 * max(sizes))
    hout = [pkg.PinnedBuffer(8 * cap) for _ in range(4)]
    gang = pkg.Gang(0)
    got = [[], []]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        n = b - a
        hin.array[:6 * n] = packed[6 * (a - cuts[0]):6 * (b - cuts[0])]
        items = [{"pipe": p, "h_packed": hin.ptr, "h_out": hout[i].ptr, "out_cap": cap} for i, p in enumerate(ganged)]
        res, ng = gang.push_async(items, n)
        assert ng == 2, (k, ng)
        for i, (p, (n_out, t)) in enumerate(zip(ganged, res)):
            p.wait_ticket(t)
            y = hout[i].array[:8 * n_out].view(np.float32).copy()
            m_out, t2 = solo[i].push_host_async(hin.ptr, n, hout[2 + i].ptr, cap)
            solo[i].wait_ticket(t2)
            assert m_out == n_out and same_bits(y, hout[2 + i].array[:8 * m_out].view(np.float32)), (k, i)
            got[i].append(y)
    for i in range(2):
        against_reference(O, f"member/i8x/{words[i]}", R["i8x"]["stages"], cases[i], np.concatenate(got[i]),
                          f"gang member {i} (word {words[i]:#x}) past 2p32")
    gang.close()
    for p in ganged + solo[:2]:
        p.close()
    for h in [hin] + hout:
        h.free()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", ["d8_127", "c320"])
def test_time_chunks_cut_from_a_deep_stream(pkg, dev, O, R, name):
    """test_time_chunk_sharding_on_one_gpu with the stream's first sample at start_for(2^32, u): four chunks of a 14-unit
    stream, each a seek(chunk start - halo) and a process of halo + chunk; the first chunk has nothing in front of it.
    Stitched, that is deep_chain from the stream's first sample."""
    shard = importlib.import_module("libperseus-sdr_amd.shard")
    stages, unit = (R["i8x"]["stages"], 8192) if name == "d8_127" else (D.c320(), 4096 * 5)
    case = D.time_chunk_case(unit)
    base, total, word = case["start"], case["sizes"][0], case["segments"][0][1]
    stream = D.stream_bytes(O, total)
    dtot = int(np.prod([st[0] for st in stages]))
    halo = shard.cascade_halo(stages, align=unit)                 # whole tiles: stays on the fused kernels
    parts = []
    for start, length in shard.time_chunks(total, 4, unit):
        h = min(halo, start)                                      # (what lies in front of the chunk inside this stream)
        pipe = pkg.Pipeline(stages, mix=True)
        pipe.set_freg(word)
        y = shard.process_time_chunk(pipe, to_dev(stream[6 * (start - h):6 * (start + length)], dev), base + start, h, dtot)
        parts.append(y.cpu().numpy().reshape(-1))
        pipe.close()
    assert base < 2**32 < base + total
    against_reference(O, f"chunks/{name}", stages, case, np.concatenate(parts), f"time chunks of {name} across 2p32")
