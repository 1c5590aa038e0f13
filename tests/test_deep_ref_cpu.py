"""CPU tests of tests/deep_ref.py: the reference the deep-stream GPU tests (test_gpu_deep_stream.py) rest on is sound at
every position they use.  The oracle's retuned mixer from an absolute start against its numpy twin and against phases
made of Python integers; a shift by a whole number of phase periods changes no bit of the reference; every start position
lies on the grid pddc_pipeline_seek accepts for its plan."""
import numpy as np
import pytest

import deep_ref as D


@pytest.fixture(scope="module")
def cases():
    out = D.all_cases()
    assert len({name for name, _, _ in out}) == len(out)
    return out


def _windows(case, half=384):
    """the stretches of a case's stream where the mixer can go wrong: its first and last samples, every retune, every edge
    and every multiple of 2^32 it crosses; [(first sample, length)]"""
    c = D.cuts_of(case["start"], case["sizes"])
    lo, hi = c[0], c[-1]
    pts = {lo + half, hi - half} | {a for a, _ in case["segments"] if lo < a < hi} | {E for E in D.EDGES if lo < E < hi}
    pts |= {m * 2**32 for m in range(lo // 2**32 + 1, hi // 2**32 + 1)}
    return sorted({(max(lo, p - half), min(hi, p + half) - max(lo, p - half)) for p in pts})


def test_the_mixer_at_every_start_position_against_its_twin_and_exact_integers(O, cases):
    worst, nwin = 0.0, 0
    for name, stages, case in cases:
        D.check_case(case)
        lo = case["start"]
        total = sum(case["sizes"])
        packed = D.stream_bytes(O, total)
        for a, n in _windows(case):
            b = packed[6 * (a - lo):6 * (a - lo + n)]
            got = D.deep_mix(O, b, a, case["segments"])
            x = O.unpack24_f32(b)
            with np.errstate(over="ignore"):          # (the twin's uint64 products wrap, which is what it means them to do)
                twin = O.nco_mix_retuned_numpy(x, case["segments"], a)
            exact = D.exact_mix(x, a, case["segments"])
            top = float(np.max(np.abs(exact)))
            err = max(float(np.max(np.abs(got - twin))), float(np.max(np.abs(got - exact)))) / top
            worst = max(worst, err)
            nwin += 1
            assert got.size == 2 * n and err <= 1e-12, (name, a, n, err)
    print(f"mixer at depth: {len(cases)} cases, {nwin} windows, worst difference {worst:.3e} of the largest value")


def test_exact_phases_are_the_sum_of_the_words_sample_by_sample():
    """the vectorised statement against the plainest one: phase(n) = sum of the word of every sample before n, from a
    phase that Python integers give at the window's first sample"""
    segs = [(0, D.WORDS[1]), (2**32 - 8, D.RETUNE_WORDS[0]), (2**32, D.RETUNE_WORDS[1]), (2**32 + 8, D.RETUNE_WORDS[2])]
    n0 = 2**32 - 40
    want, acc = [], (n0 * D.WORDS[1]) % 2**32
    for n in range(n0, n0 + 80):
        want.append(acc)
        acc = (acc + [w for a, w in segs if a <= n][-1]) % 2**32
    assert [int(v) for v in D.exact_phases(n0, 80, segs)] == want
    assert [D.exact_phase(n0 + k, segs) for k in range(80)] == want
    # the offset the library reports: phase(n) = n * word + offset behind every retune
    for k in range(1, len(segs)):
        n = segs[k][0] + 5
        assert (n * segs[k][1] + D.exact_phase_offset(segs, segs[k][0])) % 2**32 == D.exact_phase(n, segs)


@pytest.mark.parametrize("route", D.ROUTE_NAMES)
def test_a_shift_by_whole_phase_periods_changes_no_bit_of_the_reference(O, route):
    row = D.routes()[route]
    u, d = row["u"], D.delta_for(row["u"])
    assert d % u == 0 and d % 2**32 == 0
    ns = 6000
    packed = D.stream_bytes(O, ns)
    for n0 in (0, D.start_for(2**32, u)):
        segs = [(0, D.WORDS[1]), (n0 + 2504, D.RETUNE_WORDS[0])]
        base = D.deep_chain(O, packed, row["stages"], n0, segs, dtype=np.float64)
        assert base.size > 0 and np.all(np.isfinite(base))
        for k in (1, 2**9):
            moved = D.deep_chain(O, packed, row["stages"], n0 + k * d, D.shifted(segs, k * d), dtype=np.float64)
            assert np.array_equal(base.view(np.uint64), moved.view(np.uint64)), (route, n0, k)
        # ... and the reference does notice a shift that is no period (the comparison is not vacuous)
        other = D.deep_chain(O, packed, row["stages"], n0 + u, D.shifted(segs, u), dtype=np.float64)
        assert not np.array_equal(base, other)


def test_deep_chain_from_sample_zero_is_the_oracles_own_chain(O):
    for route in ("i8x", "i8x_pair", "rational"):
        row = D.routes()[route]
        packed = D.stream_bytes(O, 8000)
        segs = [(0, D.WORDS[0]), (4000, D.RETUNE_WORDS[1])]
        assert np.array_equal(D.deep_chain(O, packed, row["stages"], 0, segs), O.ddc_chain_retuned(packed, row["stages"], segs))


def test_every_start_position_is_on_the_grid_seek_accepts(cases):
    R = D.routes()
    for name, row in R.items():
        u = row["u"]
        assert D.seek_accepts(row["stages"], u) and not D.seek_accepts(row["stages"], u + 4)
        for E in D.EDGES:
            s = D.start_for(E, u)
            assert D.seek_accepts(row["stages"], s) and s + u < E < s + 3 * u
            if name != "generic7" and E >= 125 * 2**32:
                assert E % u == 0                     # 125 * 2^32 = 2^32 * 5^3: every unit but decimate-by-7's divides it
        for k in (1, 2**9):
            assert D.seek_accepts(row["stages"], k * D.delta_for(u)) and D.seek_accepts(row["stages"], k * D.delta_for(u) - 2 * u)
            assert k * D.delta_for(u) < 2**63
    for name, stages, case in cases:
        assert D.seek_accepts(stages, case["start"]), name
    # the rule itself, on the rational plan: 40 input samples per third-stage input, 25 of those per phase-0 boundary
    rat = R["rational"]["stages"]
    assert [p for p in range(0, 2001, 8) if D.seek_accepts(rat, p)] == [0, 1000, 2000]
    assert D.seek_accepts(D.c320(), 320) and not D.seek_accepts(D.c320(), 64) and not D.seek_accepts(D.c320(), 324)
