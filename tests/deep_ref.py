"""Helpers of the deep-stream tests (test_deep_ref_cpu.py, test_gpu_deep_stream.py): the front end at absolute stream
positions past 2^31 and 2^32 samples.  At the ADC rate of 80 MS/s a receiver passes sample 2^31 after 27 s and 2^32 after
54 s; 125 * 2^32 (about 2^39) after two hours, 125 * 2^41 (about 2^48) after forty days.  pddc_pipeline_seek places a
stream at any such sample with zero history and the absolute NCO phase, so no test streams its way there.

No GPU work here: the reference (the oracle's mixer from an absolute start, then its FIR stages), the positions, the
route table and the cases both test files walk through.  A stream *means* what one that began at sample 0 with the first
tuning word would be: `segments` are [(0, w0), (abs_sample, w1), ...] in absolute sample numbers, which is the contract
pddc_pipeline_seek documents (include/perseus_ddc.h)."""
import math

import numpy as np

from conftest import load_taps

FIR_TOL = 1e-6
EDGES = [2**31, 2**32, 125 * 2**32, 125 * 2**41]
WORDS = [381178347, 0xC0000000 | 1]                 # 7.1 MHz (odd), and a word past 2^31 (odd)
RETUNE_WORDS = [123456789, 0x9E3779B1, 0x7FFFFFF1]  # the words the retune tests switch to
GRANULE = 8                                         # PDDC_INPUT_GRANULE
RAGGED = 8 * 37                                     # what the last batch adds where the route takes ragged batches
SEED = 2032
MAX_STREAM = 5 * 57344 + RAGGED                     # the longest stream any case cuts from the shared bytes


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def _noise_taps(D, nt):
    """the taps of test_packed_first_stage_through_retunes (test_gpu_parity.py)"""
    rng = np.random.default_rng(D * 1000 + nt)
    return (rng.standard_normal(nt) / np.sqrt(nt)).astype(np.float32)


def c320():
    return [(8, load_taps("c320_s1_d8_32")), (8, load_taps("c320_s2_d8_64")), (5, load_taps("c320_s3_d5_161"))]


def rational_plan():
    """the rational plan of test_random_chunking_is_equivalent_to_one_batch (test_gpu_parity.py), seed 1"""
    g = (np.random.default_rng(1).standard_normal(12 * 20) / 20).astype(np.float32)
    return [(8, load_taps("c320_s1_d8_32")), (5, load_taps("c320_s3_d5_161")[:41]), (25, g, 12)]


# ------------------------------------------------------------------------------------------------ the route table
# name -> stages, pipeline options, no_fast, the seek unit u, the tile the route needs, ragged last batch or not.
# The queries that prove a row is on its route are in test_gpu_deep_stream.py (they need a pipeline).
def routes():
    d8_127, d8_255 = load_taps("d8_127"), load_taps("d8_255")
    r = {
        "i8x":       dict(stages=[(8, d8_127)], u=8192, tile=8192, ragged=True),
        "i8x_48":    dict(stages=[(8, lowpass(48, 0.05))], u=8192, tile=8192, ragged=True),
        "i8x_255":   dict(stages=[(8, d8_255)], u=8192, tile=8192, ragged=True),
        "fir8":      dict(stages=[(8, d8_127)], opts={"no_i8": 1}, u=8192, tile=4096, ragged=True),
        "i8x_pair":  dict(stages=c320(), u=40960, tile=8192, ragged=False),
        "fir8_pair": dict(stages=c320(), opts={"no_i8": 1}, u=40960, tile=4096, ragged=False),
        "fused3":    dict(stages=c320(), opts={"no_i8": 1, "fuse3": 1}, u=40960, tile=4096, ragged=False),
        "i8x_d10":   dict(stages=[(10, lowpass(51, 0.04))], u=40960, tile=10240, ragged=True),
        "firp":      dict(stages=[(10, _noise_taps(10, 69))], u=40960, tile=8, ragged=True),
        "generic7":  dict(stages=[(7, _noise_taps(7, 99))], u=57344, tile=8, ragged=True),
        "unpack":    dict(stages=[(8, d8_127)], no_fast=True, u=8192, tile=8, ragged=True),
        "rational":  dict(stages=rational_plan(), u=1000, tile=8, ragged=False),
    }
    for name, row in r.items():
        row.setdefault("opts", {})
        row.setdefault("no_fast", False)
        check_unit(row["stages"], row["u"], row["tile"])
    return r


ROUTE_NAMES = ["i8x", "i8x_48", "i8x_255", "fir8", "i8x_pair", "fir8_pair", "fused3", "i8x_d10", "firp", "generic7",
               "unpack", "rational"]
RETUNE_ROUTES = ["i8x", "i8x_d10", "firp", "generic7"]


# ------------------------------------------------------------------------------------------------ positions
def seek_accepts(stages, pos):
    """pddc_pipeline_seek's grid rule (ddc_pipeline.cpp), restated: every stage lands on an output boundary -- a rational
    stage on a phase-0 one --, and the position is a multiple of the input granule."""
    at = int(pos)
    for st in stages:
        D = int(st[0])
        L = int(st[2]) if len(st) > 2 and st[2] and int(st[2]) > 1 else 1
        if at % D:
            return False
        at = at // D * L
    return pos >= 0 and pos % GRANULE == 0


def check_unit(stages, u, tile=1):
    """A seek unit is a multiple of every stage's output grid, of 8 and of the tile the route needs: every multiple of it is
    then a position seek accepts (each stage's position scales with the multiple)."""
    assert u > 0 and u % GRANULE == 0 and u % tile == 0, (u, tile)
    assert seek_accepts(stages, u) and seek_accepts(stages, 3 * u), u


def start_for(E, u):
    """(ceil(E / u) - 2) u: with batches [u, 2u, u, last] the edge E lies strictly inside the second batch, whether or not
    u divides E."""
    s = (-(-E // u) - 2) * u
    assert s + u < E < s + 3 * u
    return s


def delta_for(u):
    """lcm(u, 2^32): a shift by it leaves every 32-bit phase unchanged, for every tuning word, and stays on the grid"""
    return math.lcm(u, 2**32)


def batches(u, ragged):
    return [u, 2 * u, u, u + RAGGED if ragged else u]


def cuts_of(start, sizes):
    c = [start]
    for n in sizes:
        c.append(c[-1] + n)
    return c


def word_for(route, E):
    """both words over the (route, edge) grid, each route seeing both"""
    return WORDS[(ROUTE_NAMES.index(route) + EDGES.index(E)) % 2]


def shifted(segments, by):
    """the same stream `by` samples later: the first word still begins at sample 0"""
    return [(a if a == 0 else a + by, w) for a, w in segments]


# ------------------------------------------------------------------------------------------------ the cases
def edge_case(route, row, E):
    """test 1: four batches from start_for(E, u), the edge inside the second, one word"""
    start = start_for(E, row["u"])
    return dict(start=start, sizes=batches(row["u"], row["ragged"]), segments=[(0, word_for(route, E))], retune_at={})


def boundary_case(row, E, b):
    """test 2, one retune between two long batches, at absolute sample b (E - 8, E or E + 8): the batch behind it mixes its
    packed history with the old word"""
    u = row["u"]
    start = start_for(E, u)
    w1 = RETUNE_WORDS[(b - E) // 8 + 1]
    return dict(start=start, sizes=[b - start, u, u + RAGGED], segments=[(0, WORDS[0]), (b, w1)], retune_at={1: w1})


def three_boundaries_case(row, E):
    """test 2, a new word before the batches that start at E - 8, E and E + 8 (two of them 8 samples long)"""
    u = row["u"]
    start = start_for(E, u)
    sizes = [E - 8 - start, 8, 8, u, u + RAGGED]
    segs = [(0, WORDS[1]), (E - 8, RETUNE_WORDS[0]), (E, RETUNE_WORDS[1]), (E + 8, RETUNE_WORDS[2])]
    return dict(start=start, sizes=sizes, segments=segs, retune_at={1: RETUNE_WORDS[0], 2: RETUNE_WORDS[1], 3: RETUNE_WORDS[2]})


def storm_case(row, E):
    """test 2, second form (test_packed_first_stage_through_retunes with nb = 32): one batch up to E - 128, then twelve of 32
    samples with a new word before the fifth, sixth and seventh -- at E, E + 32 and E + 64: three words in one history
    window"""
    start = start_for(E, row["u"])
    sizes = [E - 128 - start] + [32] * 12
    segs = [(0, 0x9E3779B1), (E, 381178347), (E + 32, 0x7FFFFFF1), (E + 64, 3000000000)]
    return dict(start=start, sizes=sizes, segments=segs, retune_at={5: 381178347, 6: 0x7FFFFFF1, 7: 3000000000})


def shift_cases(route, row):
    """test 3: (i) a fresh stream from 0 against the same at k delta, k = 1 and 2^9; (ii) streams that cross a multiple of
    delta in their second batch, at delta - 2u and 2^9 delta - 2u.  One retune before the third batch in each."""
    u, d = row["u"], delta_for(row["u"])
    w0, w1 = word_for(route, EDGES[1]), RETUNE_WORDS[0]
    sizes = batches(u, row["ragged"])
    out = {}
    for key, start in (("0", 0), ("d", d), ("512d", 2**9 * d), ("d-2u", d - 2 * u), ("512d-2u", 2**9 * d - 2 * u)):
        out[key] = dict(start=start, sizes=sizes, segments=[(0, w0), (start + 3 * u, w1)], retune_at={2: w1})
    return out


def checkpoint_case(row):
    """test 4: two batches across 2^32, the checkpoint, two more, a retune and a fifth"""
    u = row["u"]
    start = start_for(2**32, u)
    sizes = batches(u, row["ragged"]) + [u]
    return dict(start=start, sizes=sizes, segments=[(0, WORDS[0]), (start + sum(sizes[:4]), RETUNE_WORDS[1])],
                retune_at={4: RETUNE_WORDS[1]})


def member_case(word):
    """test 5: a member of the bank or the gang at start_for(2^32, 8192)"""
    return dict(start=start_for(2**32, 8192), sizes=batches(8192, True), segments=[(0, word)], retune_at={})


def time_chunk_case(u):
    """test 6: a 14-unit stream whose first sample is at start_for(2^32, u)"""
    return dict(start=start_for(2**32, u), sizes=[14 * u], segments=[(0, WORDS[0])], retune_at={})


def all_cases():
    """every (plan, case) the GPU file runs: [(name, stages, case)]"""
    R = routes()
    out = []
    for name in ROUTE_NAMES:
        row = R[name]
        for E in EDGES:
            out.append((f"edge/{name}/{E}", row["stages"], edge_case(name, row, E)))
        for key, case in shift_cases(name, row).items():
            out.append((f"shift/{name}/{key}", row["stages"], case))
    for name in RETUNE_ROUTES:
        row = R[name]
        for E in (2**32, 125 * 2**32):
            for b in (E - 8, E, E + 8):
                out.append((f"boundary/{name}/{E}/{b - E}", row["stages"], boundary_case(row, E, b)))
            out.append((f"three/{name}/{E}", row["stages"], three_boundaries_case(row, E)))
            out.append((f"storm/{name}/{E}", row["stages"], storm_case(row, E)))
    for name in ("i8x_pair", "rational"):
        out.append((f"checkpoint/{name}", R[name]["stages"], checkpoint_case(R[name])))
    for name in ("i8x", "i8x_48"):
        for w in WORDS:
            out.append((f"member/{name}/{w}", R[name]["stages"], member_case(w)))
    for name, u in (("i8x", 8192), ("i8x_pair", 20480)):
        out.append((f"chunks/{name}", R[name]["stages"], time_chunk_case(u)))
    return out


def check_case(case):
    """a case is consistent with itself: the retunes are where the segments say, at batch boundaries"""
    c = cuts_of(case["start"], case["sizes"])
    assert all(n > 0 and n % GRANULE == 0 for n in case["sizes"]), case["sizes"]
    assert case["segments"][0][0] == 0
    assert [(c[k], w) for k, w in sorted(case["retune_at"].items())] == list(case["segments"][1:])
    assert c[-1] - c[0] <= MAX_STREAM
    return c


# ------------------------------------------------------------------------------------------------ the reference
_bytes = {}


def stream_bytes(O, nsamples, seed=SEED):
    """the first nsamples samples of the one byte stream every case reads (O.lcg_bytes, made once per seed)"""
    if seed not in _bytes:
        _bytes[seed] = O.lcg_bytes(6 * MAX_STREAM, seed)
    assert nsamples <= MAX_STREAM
    return _bytes[seed][:6 * nsamples]


def deep_mix(O, packed, n0, segments):
    """unpack -> the retuned NCO from absolute sample n0; float64 pairs"""
    return O.nco_mix_retuned(O.unpack24_f32(packed), segments, int(n0))


def deep_chain(O, packed, stages, n0, segments, dtype=np.float32):
    """oracle.ddc_chain_retuned with an absolute start: unpack -> retuned NCO from sample n0 -> FIR chain (plain decimators
    or rational stages) in double, from zero history -- what a pipeline placed at n0 by seek computes.  n0 must be a
    position seek accepts (the stages' decimation phases are then 0, as the oracle's are)."""
    assert seek_accepts(stages, n0), n0
    x = deep_mix(O, packed, n0, segments)
    for st in stages:
        L = int(st[2]) if len(st) > 2 and st[2] and int(st[2]) > 1 else 1
        x = O.resample(x, st[1], L, int(st[0])) if L > 1 else O.fir_decim(x, st[1], int(st[0]))
    return np.asarray(x, dtype=dtype)


_refs = {}


def reference(O, key, stages, case, seed=SEED):
    """deep_chain of a case, computed once per key and left unchanged (read-only)"""
    k = (key, seed)
    if k not in _refs:
        ns = sum(case["sizes"])
        y = deep_chain(O, stream_bytes(O, ns, seed), stages, case["start"], case["segments"])
        y.setflags(write=False)
        _refs[k] = y
    return _refs[k]


# ------------------------------------------------------------------------------------------------ exact integers
def exact_phase(n, segments):
    """the accumulator's phase at absolute sample n, in Python integers: sum of the words of all samples before n"""
    acc = 0
    for i, (a, w) in enumerate(segments):
        b = segments[i + 1][0] if i + 1 < len(segments) else None
        if b is not None and n >= b:
            acc += (b - a) * w
        else:
            acc += (n - a) * w
            break
    return acc % 2**32


def exact_phases(n0, ns, segments):
    """phases of samples n0 .. n0 + ns - 1 (uint64 array of values below 2^32): everything that depends on the absolute
    position is a Python integer; inside a stretch of one word the ramp k * w, k < ns < 2^20, is exact in uint64"""
    out = np.empty(ns, dtype=np.uint64)
    marks = sorted({n0, n0 + ns} | {a for a, _ in segments if n0 < a < n0 + ns})
    for a, b in zip(marks[:-1], marks[1:]):
        w = [wd for s, wd in segments if s <= a][-1]
        assert (b - a) * w < 2**63
        out[a - n0:b - n0] = (np.uint64(exact_phase(a, segments)) + np.arange(b - a, dtype=np.uint64) * np.uint64(w)) \
            & np.uint64(0xFFFFFFFF)
    return out


def exact_mix(x_iq, n0, segments):
    """x e^{-j 2 pi phase / 2^32} with exact_phases; float64 pairs"""
    x = np.asarray(x_iq, dtype=np.float64).reshape(-1, 2)
    a = exact_phases(n0, x.shape[0], segments).astype(np.float64) * (2.0 * np.pi / 4294967296.0)
    z = (x[:, 0] + 1j * x[:, 1]) * np.exp(-1j * a)
    return np.stack([z.real, z.imag], axis=1).reshape(-1)


def exact_phase_offset(segments, upto):
    """pddc_pipeline_get_phase_offset after the retunes at or before sample `upto`: sum of n (w_old - w_new) mod 2^32"""
    off = 0
    for (_, w_old), (n, w_new) in zip(segments[:-1], segments[1:]):
        if n <= upto:
            off += n * (w_old - w_new)
    return off % 2**32
