"""CPU tests of the wideband blanker: the two references of tests/wblank_ref.py agree byte for byte on every input the GPU
tests use, those inputs hold what the GPU tests rely on, the band scenario of the contract reproduces, and
pddc_wblank_create refuses what it must without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import wblank_ref as R

TILE = 2048                      # pddc_wblank_tile_samples(), asserted below where the library is at hand


@functools.lru_cache(maxsize=None)
def small():
    return R.small_stream()


def same(a, b):
    assert np.array_equal(a["out"], b["out"])
    assert np.array_equal(a["t"], b["t"])
    assert np.array_equal(a["num"], b["num"])
    assert (a["triggers"], a["blanked"], a["mean"]) == (b["triggers"], b["blanked"], b["mean"])


@pytest.mark.parametrize("params", R.PARAM_SETS[:4])
@pytest.mark.parametrize("thr", R.THRS)
def test_references_agree_on_the_small_stream(params, thr):
    packed, _ = small()
    sched = ((0, int(thr * 16), True),)
    same(R.wblank_fast(packed, *params, sched), R.wblank_plain(packed, *params, sched))


def test_references_agree_off_short_and_with_a_schedule():
    packed, _ = small()
    off = ((0, 256, False),)
    for params in R.PARAM_SETS[:4]:
        a = R.wblank_fast(packed, *params, off)
        D = R.delay_of(params[2], params[3])
        assert a["triggers"] == 0 and a["blanked"] == 0
        assert np.array_equal(a["out"][6 * D:], packed[:packed.size - 6 * D]) and not a["out"][:6 * D].any()
    same(R.wblank_fast(packed, *R.PARAM_SETS[2], off), R.wblank_plain(packed, *R.PARAM_SETS[2], off))
    short = packed[:6 * R.N_SHORT]
    B, H, W, r = R.PARAM_SETS[4]
    assert B > R.N_SHORT
    a = R.wblank_fast(short, B, H, W, r)
    same(a, R.wblank_plain(short, B, H, W, r))
    D = R.delay_of(W, r)
    assert a["triggers"] == 0 and np.array_equal(a["out"][6 * D:], short[:short.size - 6 * D])
    sched = ((0, 256, True), (10008, 16 * 4096, True), (20480, 64, False), (30000, 64, True))
    same(R.wblank_fast(packed, *R.PARAM_SETS[2], sched), R.wblank_plain(packed, *R.PARAM_SETS[2], sched))


def test_references_agree_on_the_extremes():
    B, H, W, r = R.PARAM_SETS[2]
    n = 16 * B
    zeros = np.zeros(6 * n, dtype=np.uint8)
    a = R.wblank_fast(zeros, B, H, W, r)
    same(a, R.wblank_plain(zeros, B, H, W, r))
    assert a["triggers"] == 0 and not a["out"].any() and a["mean"] == 0
    full = R.full_scale_stream(n, B)
    for thr16 in (16, 65536):
        a = R.wblank_fast(full, B, H, W, r, ((0, thr16, True),))
        same(a, R.wblank_plain(full, B, H, W, r, ((0, thr16, True),)))
        assert a["triggers"] == 0
    assert R.wblank_fast(full[:6 * 3 * B], B, H, W, r)["mean"] == 1 << 47
    near = R.near_full_scale_stream(n, B)
    a = R.wblank_fast(near, B, H, W, r, ((0, 16, True),))
    same(a, R.wblank_plain(near, B, H, W, r, ((0, 16, True),)))
    assert a["triggers"] == (n - B) - (n - B) // B and a["mean"] == (1 << 47) - (1 << 47) // B
    a = R.wblank_fast(near, B, H, W, r, ((0, 17, True),))
    same(a, R.wblank_plain(near, B, H, W, r, ((0, 17, True),)))
    assert a["triggers"] == 0


def test_references_agree_on_the_large_stream():
    packed, _ = R.large_stream()
    params = R.PARAM_SETS[2]
    a = R.wblank_fast(packed, *params)
    same(a, R.wblank_plain(packed, *params))
    assert a["triggers"] > 600


def test_the_small_stream_holds_what_the_gpu_tests_rely_on():
    packed, pos = small()
    n = R.N_SMALL
    for params in R.PARAM_SETS[:4]:
        B, H, W, r = params
        D = R.delay_of(W, r)
        ref = R.wblank_fast(packed, *params)
        trig = np.flatnonzero(ref["t"])
        # (with a short history an impulse lifts the reference of the blocks behind it: not every impulse is a trigger)
        assert set(trig) <= set(pos) and trig.size >= pos.size // 2
        # in the stream's first block there is no reference: the impulses there do not trigger
        assert {3, 10} <= set(pos) and trig.min() >= B
        # on the last sample in front of a tile seam and on the first behind one (the run seams of one, two and three
        # tiles are among them), and within D of seams on either side
        seams = range(TILE, n, TILE)
        assert any(ref["t"][s - 1] for s in seams) and any(ref["t"][s] for s in seams)
        if H >= 2:
            assert any(ref["t"][s - 1] and ref["t"][s] for s in seams)
        if D >= 5:
            assert any(ref["t"][s - 3] and ref["t"][s + 5] for s in seams)
        # within D of a batch cut, and in the last D samples of a batch: cut_stream() puts impulses on the cuts (the test
        # below); here: the list is well formed and its edges are multiples of 8
        cuts = R.cut_list(n, D, B, TILE)
        assert sum(cuts) == n and all(c % 8 == 0 and c >= 0 for c in cuts) and cuts.count(0) >= 2
        # the last samples of the stream
        assert ref["t"][n - 1] and ref["t"][n - 2]
        # overlapping neighbourhoods
        if D >= 2:
            assert np.any(np.diff(trig) <= D)
        # every numerator of the ramp, and the guard's zero
        seen = set(np.unique(ref["num"]))
        assert set(range(0, (1 << r))) <= seen and -1 in seen
    ref = R.wblank_fast(packed, *R.PARAM_SETS[2], ((0, 16, True),))
    assert 0.25 < ref["triggers"] / n < 0.45                # thr = 1: about a third of the samples


def test_the_cut_stream_has_triggers_on_every_cut():
    for params in R.PARAM_SETS[:4]:
        B, H, W, r = params
        packed, cuts, edges = R.cut_stream(params)
        ref = R.wblank_fast(packed, *params)
        same(ref, R.wblank_plain(packed, *params))
        t = ref["t"]
        # the last sample of a batch and the third of the next are triggers (with a history of one block an impulse
        # keeps the block behind it from triggering: there, some of the cuts)
        hits = [e for e in edges if t[e - 1] and t[e + 2]]
        assert len(edges) >= 8 and len(hits) >= (len(edges) if H >= 2 else 3), (params, edges, hits)


def test_a_delay_longer_than_a_block_counts_only_outputs_made_from_an_input():
    """D = 255 > B = 64: triggers at samples 70 and 200 lie within D of outputs 0 .. 254, which are made from no input
    (c = n - D < 0): six zero bytes, and not counted as blanked, by either reference"""
    packed, pos = small()
    B, H, W, r = R.PARAM_DEEP
    D = R.delay_of(W, r)
    assert D > B and {70, 200} <= set(pos)
    a, b = R.wblank_fast(packed, B, H, W, r), R.wblank_plain(packed, B, H, W, r)
    same(a, b)
    assert a["t"][70] and a["t"][200] and not a["out"][:6 * D].any()
    n = R.N_SMALL
    gated = a["num"] >= 0
    assert a["blanked"] == int(gated[:n - D].sum()) and gated[:D].all()
    # what a count over every output index within D of a trigger's delayed place would give: more, by the outputs
    # n < D that have a trigger at an input u <= n
    u = np.flatnonzero(a["t"])
    extra = sum(1 for k in range(D) if np.any(u <= k))
    assert extra == D - 70
    packed, cuts, edges = R.cut_stream(R.PARAM_DEEP)
    same(R.wblank_fast(packed, B, H, W, r), R.wblank_plain(packed, B, H, W, r))


def test_the_band_scenario():
    """the figures of the contract's motivation, on the reference: B = 256, H = 8, W = 4, r = 3, thr = 16"""
    clean, dirty = R.band_streams()
    ref = R.wblank_fast(dirty, 256, 8, 4, 3)
    D = R.delay_of(4, 3)
    blanked = np.concatenate([ref["out"][6 * D:], np.zeros(6 * D, dtype=np.uint8)])
    (fc, tc), (fd, td), (fb, tb) = R.floor_db(clean), R.floor_db(dirty), R.floor_db(blanked)
    print(f"floor clean {fc:.3f} dB, dirty {fd:.3f} dB, blanked {fb:.3f} dB; tone over floor {td - fd:.2f} -> {tb - fb:.2f} dB; "
          f"{ref['triggers']} triggers, {ref['blanked']} samples touched")
    assert abs(fb - fc) <= 0.1
    assert fd - fc >= 20.0
    assert tb - fb >= 10.0
    at = np.concatenate([np.arange(s, s + 3) for s in range(20011, (1 << 20) - 3, 20011)])
    hits = int(ref["t"][at].sum())
    assert hits >= 0.95 * at.size and ref["triggers"] - hits <= 8


def test_create_refuses_bad_parameters_before_it_looks_for_a_device(pkg):
    L = pkg.ddc_lib()
    assert L.pddc_wblank_tile_samples() == TILE and L.pddc_wblank_run_samples() == TILE
    h = C.c_void_p()
    good = dict(block=256, history=8, guard=4, ramp_log2=3)

    def create(thr16=256, flags=pkg.PDDC_WB_ON, params=True, **kw):
        p = pkg.WBlankParams(**{**good, **kw})
        return L.pddc_wblank_create(C.byref(h), 0, C.byref(p) if params else None, thr16, flags)

    bad = [dict(block=32), dict(block=8192), dict(block=96), dict(block=0), dict(block=-64), dict(history=0), dict(history=17),
           dict(guard=-1), dict(guard=129), dict(ramp_log2=-1), dict(ramp_log2=8), dict(guard=129, ramp_log2=7)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
        assert not h.value
    for thr16 in (0, 15, 65537, 0xFFFFFFFF):
        assert create(thr16=thr16) == pkg.PDDC_EINVAL
    assert create(flags=2) == pkg.PDDC_EINVAL
    assert create(params=False) == pkg.PDDC_EINVAL
    assert L.pddc_wblank_create(None, 0, None, 256, 1) == pkg.PDDC_EINVAL
    assert L.pddc_wblank_set(None, 256, 1) == pkg.PDDC_EINVAL
    assert L.pddc_wblank_delay(None) == 0
    with pytest.raises(pkg.PddcError) as e:
        pkg.WBlank(256, 8, 4, 3, thr=0.5)
    assert e.value.code == pkg.PDDC_EINVAL
    if L.pddc_device_count() == 0:
        assert create() == pkg.PDDC_ENODEV
        assert create(guard=128, ramp_log2=7, block=4096, history=16) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.WBlank(256, 8, 4, 3)
        assert e.value.code == pkg.PDDC_ENODEV


def test_the_run_tunable_is_in_the_table(pkg):
    assert pkg.get_tunable("wblank_run") == 0
    pkg.set_tunable("wblank_run", 3 * TILE - 5)
    try:
        assert pkg.wblank_run_samples() == 3 * TILE
    finally:
        pkg.set_tunable("wblank_run", 0)
    assert pkg.wblank_run_samples() == TILE
