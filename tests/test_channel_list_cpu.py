"""The channel list's host side (pddc_channelizer_set_channels, pddc_tuner_set_channels, pddc_tuner_channel_list): what
can be checked without a device.  The list arithmetic is compared with a numpy restatement on tests/tuner_ref.py's
channel rule, never with the code under test."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tuner_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pddc_channelizer_set_channels", "pddc_tuner_set_channels", "pddc_tuner_channel_list")


def ref_list(nchan, words):
    return np.array(sorted({TR.channel_of(nchan, f)[0] for f in words}), dtype=np.int32)


def c_list(pkg, nchan, words):
    f = np.asarray(words, dtype=np.uint64).astype(np.uint32)
    out = np.full(f.size + 1, -7, dtype=np.int32)
    n = pkg.ddc_lib().pddc_tuner_channel_list(nchan, f.ctypes.data_as(C.POINTER(C.c_uint32)), f.size,
                                              out.ctypes.data_as(C.POINTER(C.c_int)))
    assert 0 < n <= f.size and out[f.size] == -7 and np.all(out[n:] == -7)     # nothing behind the n entries is written
    return out[:n]


def test_the_new_symbols_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "perseus_ddc.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.DDC_LIB], text=True)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\bT\s+" + name + r"$", exported, re.M), name
        assert hasattr(pkg.ddc_lib(), name)
    for name in ("set_channels",):
        assert hasattr(pkg.Channelizer, name) and hasattr(pkg.Tuner, name)
    assert callable(pkg.tuner_channel_list)


@pytest.mark.parametrize("nchan", [1024, 4096])
def test_channel_list_against_the_restatement(pkg, nchan):
    b = nchan.bit_length() - 1
    sh, half = 32 - b, 1 << (31 - b)
    rng = np.random.default_rng(5 + nchan)
    ks = [0, 1, 17, nchan // 2, nchan - 2, nchan - 1]
    cases = {
        "centres": [k << sh for k in ks[::-1]],
        "midway": [((k << sh) + half) & TR.MASK for k in ks] + [((k << sh) - half) & TR.MASK for k in ks],
        "wrap": [TR.MASK, TR.MASK - half + 1, TR.MASK - half, 0, half - 1, ((nchan - 1) << sh) + half - 1],
        "random": [int(v) for v in rng.integers(0, 1 << 32, 1024, dtype=np.uint64)],
        "one": [0x12345678],
        "twice": [0x12345678, 0x12345678, 0x12345679],
    }
    for name, words in cases.items():
        want = ref_list(nchan, words)
        got = c_list(pkg, nchan, words)
        assert np.array_equal(got, want), (nchan, name)
        assert np.all(np.diff(got) > 0)
        py = pkg.tuner_channel_list(nchan, words)
        assert py.dtype == np.int32 and np.array_equal(py, want), (nchan, name)
    # what the cases are there for
    assert ref_list(nchan, cases["midway"]).tolist() == sorted({(k + 1) % nchan for k in ks} | set(ks))   # a tie goes up
    assert 0 in ref_list(nchan, cases["wrap"][:2]) and nchan - 1 in ref_list(nchan, cases["wrap"][2:3])
    assert ref_list(nchan, cases["random"]).size < 1024                      # duplicates collapse
    assert ref_list(nchan, cases["twice"]).size == 1


def test_bad_arguments_are_refused_without_a_device(pkg):
    L = pkg.ddc_lib()
    f = np.array([1, 2, 3], dtype=np.uint32)
    out = np.full(4, -7, dtype=np.int32)
    pf, po = f.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_int))
    assert L.pddc_tuner_channel_list(1024, None, 3, po) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_channel_list(1024, pf, 3, None) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_channel_list(1024, pf, 0, po) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_channel_list(1024, pf, -1, po) == pkg.PDDC_EINVAL
    for nchan in (0, 512, 1000, 8192):
        assert L.pddc_tuner_channel_list(nchan, pf, 3, po) == pkg.PDDC_EINVAL
    assert np.all(out == -7)
    with pytest.raises(pkg.PddcError) as e:
        pkg.tuner_channel_list(512, [1, 2])
    assert e.value.code == pkg.PDDC_EINVAL
    ch = np.array([1, 2], dtype=np.int32)
    pc = ch.ctypes.data_as(C.POINTER(C.c_int))
    assert L.pddc_channelizer_set_channels(None, pc, 2) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_set_channels(None, pc, 2) == pkg.PDDC_EINVAL
