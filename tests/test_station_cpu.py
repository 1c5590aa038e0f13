"""The station without a GPU: the scene of tests/station_ref.py through the stages' double references, chained in the
device's topology with the device's hand-over types.  The radio facts that tests/test_gpu_station.py asserts of the
device hold on the reference chain alone, every recorded figure and every MODEL_WORST_STATION entry is what the
references give today, the decoders' margins hold for every receiver, and the stage-by-stage harness passes on the
reference chain itself and reports exactly the stage whose input was tampered with."""
import time

import numpy as np
import pytest

import station_ref as S

_CACHE = {}


def chain(O):
    """(x, R): the unpacked stream and the reference chain's arrays, built once for the file"""
    if "R" not in _CACHE:
        t0 = time.time()
        packed = O.pack24_f32(S.scene())
        x = O.unpack24_f32(packed).reshape(-1, 2)
        x = x[:, 0].astype(np.float64) + 1j * x[:, 1]
        t1 = time.time()
        R = S.reference_chain(x)
        print(f"station: scene and packing {t1 - t0:.1f} s, reference chain {R['seconds']:.1f} s")
        _CACHE["x"], _CACHE["R"] = x, R
    return _CACHE["x"], _CACHE["R"]


def test_the_station_is_what_the_issue_asks_for():
    """21 receivers (16 + 5), every one on a channel centre plus a residue that is not zero, two of the occupied ones in
    channel 0 from below (words near 2^32), f and g on one word, the counts the closed forms give."""
    assert S.K == 21 and len(S.WORDS) == S.K and len(set(S.WORDS)) == S.K - 1 and S.WORDS[S.RX["f"]] == S.WORDS[S.RX["g"]]
    kr = [S.TR.channel_of(S.M, f) for f in S.WORDS]
    assert all(r != 0 for _, r in kr)
    wrapped = [S.NAMES[j] for j, (k, r) in enumerate(kr) if k == 0 and S.WORDS[j] >= 1 << 31]
    assert len(wrapped) >= 2 and all(name not in S.SILENT for name in wrapped), wrapped
    assert S.CHANNELS == sorted(set(k for k, _ in kr)) and len(S.CHANNELS) < S.K
    assert S.NS <= 1 << 23 and S.NROWS == 16377 and S.NRX == 4079
    assert S.FILTER_TAPS <= 63 and S.BLANKER_DELAY == 8 and len(set(S.SEL)) >= 3
    assert len({S.SEL[S.RX[n]] for n in ("a", "c", "j")}) == 3
    sc = S.scene()
    assert sc.shape == (S.NS, 2) and sc.dtype == np.float32 and np.abs(sc).max() < 1.0


def test_every_stage_input_is_within_the_qualified_levels(O):
    x, R = chain(O)
    for name in ("rows", "tun", "blk", "flt", "car", "dem", "sql", "adp", "dns", "eq", "aud", "mix"):
        assert np.isfinite(R[name]).all() and np.abs(R[name]).max() <= 1.0, (name, np.abs(R[name]).max())
    assert R["aud"].shape == (S.K, S.UR.outputs(S.AUDIO["L"], S.AUDIO["M"], 0, S.NRX))
    assert R["mix"].shape == (2, S.MR.outputs(S.MIX_BLOCK, 0, R["aud"].shape[1]))


@pytest.mark.parametrize("fact", list(S.FACTS))
def test_radio_fact(O, fact):
    """every radio fact of section 3 on the reference chain"""
    x, R = chain(O)
    print(fact, S.FACTS[fact](R))


def test_decision_margins_hold_for_every_receiver(O):
    """no receiver is left out of the exact comparison of characters, counts and status: the modules' own margins"""
    x, R = chain(O)
    print("fsk", R["fsk_margin"][[S.RX["j"], S.RX["k"]]], "morse", R["morse_margin"][[S.RX["l"], S.RX["m"]]])
    assert (R["fsk_margin"] >= S.FR.MARGIN).all(), R["fsk_margin"]
    assert (R["morse_margin"] >= S.KR.MARGIN).all(), R["morse_margin"]


def test_recorded_figures(O):
    """X, Y, the SINAD gain and the carrier-offset bound are what the reference chain gives"""
    x, R = chain(O)
    got = dict(mirror=S.mirror_db(R), notch=S.notch_db(R)[0], sinad=S.sinad_gain_db(R), offset=S.carrier_offset_bound(R))
    print(got)
    assert abs(got["mirror"] - S.REF_MIRROR_DB) < 0.05 and abs(got["notch"] - S.REF_NOTCH_DB) < 0.05
    assert abs(got["sinad"] - S.REF_SINAD_GAIN_DB) < 0.05
    assert got["offset"] <= S.CARRIER_OFFSET_BOUND_HZ <= 1.02 * got["offset"]
    # the loop's own error dwarfs what float32 does to freq (carrier_ref: 4.9e-9 half-turns, 2.4e-5 Hz)
    assert S.CARRIER_OFFSET_BOUND_HZ > 100 * 4.9e-9 * S.RATE / 2


def test_model_worst_station(O):
    """MODEL_WORST_STATION is what the float32 models give on the reference chain's arrays today, rounded up by a tenth at
    the most; TOL_STATION is 7 x that"""
    x, R = chain(O)
    got = S.model_worst(R, x)
    for k in sorted(got):
        print(f"{k:12s} model {got[k]:.3e}  recorded {S.MODEL_WORST_STATION[k]:.3e}  TOL {S.TOL_STATION[k]:.3e}")
    assert set(got) == set(S.MODEL_WORST_STATION)
    for k, v in got.items():
        assert v <= S.MODEL_WORST_STATION[k] <= 1.1 * v, (k, v, S.MODEL_WORST_STATION[k])
        assert S.TOL_STATION[k] == 7 * S.MODEL_WORST_STATION[k]


def test_the_harness_on_the_reference_chain(O):
    """check_stages on the reference chain's own (rounded) arrays passes every stage; with two receivers' rows swapped
    between RxFilter and Demod it reports the Demod comparison and no other, with the squelch's a one sample late
    against z the Squelch comparison and no other"""
    x, R = chain(O)
    figures, failures = S.check_stages(R, x)
    print(figures)
    assert failures == [], failures
    for stage, inputs in S.controls(R).items():
        _, failures = S.check_stages(R, only=(stage,), inputs={stage: inputs})
        assert [f[0] for f in failures] == [stage], (stage, failures)
