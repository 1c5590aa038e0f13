"""Denoise on the GPU, row by row and stream by stream.

Non-finite samples (include/perseus_ddc.h, the denoise section): a NaN, an infinity or a value whose square overflows
in some rows leaves every other row's bits as they are -- outputs and noise estimates, whichever block the rows share --
and the documented recovery (nfft good samples, then set_rx with PDDC_DENOISE_RESTART) gives, once the overlap has
drained, the bits of a receiver restarted at the same place on the good series.

Side stream: the object on a busy side stream with nothing synchronised has the bits of the quiet run, in the harness
of tests/test_gpu_stream_order.py (steady state, and set_rx / read_noise / reset / close behind a busy stream)."""
import types

import numpy as np
import pytest

import denoise_ref as R
import nonfinite as NF
import stream_order as S
import test_gpu_stream_order as G

pytestmark = pytest.mark.gpu

K, N = S.K, R.N_GPU
BAD = {k: NF.POISON_EXACT[k] for k in ("nan", "+inf", "-inf", "huge")}
SIZES = [(256, 64), (512, 128), (1024, 512)]


def run(pkg, dev, x, rx, nfft, hop, sizes, events=()):
    import torch
    s = pkg.Denoise(rx, nfft, hop, window=R.window(nfft, hop))
    xd = torch.from_numpy(x).to(dev)
    pending = sorted(events, key=lambda e: e[0])
    outs, at = [], 0
    for b in sizes:
        while pending and pending[0][0] == at:
            s.set_rx(*pending.pop(0)[1:])
        outs.append(s.process(xd[:, at:at + b]).clone())
        at += b
    assert at == x.shape[1] and not pending
    got = torch.cat(outs, dim=1).cpu().numpy(), s.read_noise()
    s.close()
    return got


@pytest.mark.parametrize("nfft,hop", SIZES)
def test_a_bad_sample_stays_in_its_row(pkg, dev, nfft, hop):
    x, rx = R.rows(K), R.receivers(K)
    rows = NF.poisoned_rows(K)
    others = [j for j in range(K) if j not in rows]
    sizes = [hop - 1, 1, nfft + 3, N - nfft - hop - 3]
    clean = run(pkg, dev, x, rx, nfft, hop, sizes)
    cols = [0, hop - 1, hop, nfft + hop + 2, N - 1]            # a batch's first and last sample, a batch of 1, the last sample
    for name, v in BAD.items():
        got = run(pkg, dev, NF.plant(x, rows, cols, v), rx, nfft, hop, sizes)
        for g, c, what in zip(got, clean, ("out", "noise")):
            NF.clean_rows_identical(g, c, others, f"{name} {what}")
        hit = [j for j in rows if j not in (R.ZERO_ROW,) and rx[j][0] != R.OFF]
        assert hit and all(not np.isfinite(got[1][j]).all() for j in hit), name     # N of a poisoned row is not finite


@pytest.mark.parametrize("nfft,hop", SIZES[:2])
def test_recovery_is_a_receiver_restarted_on_the_good_series(pkg, dev, nfft, hop):
    x, rx = R.rows(K), R.receivers(K)
    rows = NF.poisoned_rows(K)
    p, at = 700, 1500                                           # at least nfft good samples between them
    assert at - p > nfft and at % hop
    sizes = [at, N - at]
    ev = [(at, j, rx[j][0], rx[j][1], rx[j][2], rx[j][3], R.RESTART | (rx[j][4] if len(rx[j]) > 4 else 0)) for j in rows]
    want = run(pkg, dev, x, rx, nfft, hop, sizes, ev)
    q = at // hop                                               # the first frame the restart governs
    for name, v in BAD.items():
        got = run(pkg, dev, NF.plant(x, rows, [p], v), rx, nfft, hop, sizes, ev)
        NF.clean_rows_identical(got[0][:, q * hop + nfft:], want[0][:, q * hop + nfft:], np.arange(K), f"{name} out")
        NF.clean_rows_identical(got[1], want[1], np.arange(K), f"{name} noise")
        assert not all(np.array_equal(got[0][j, p:q * hop + nfft], want[0][j, p:q * hop + nfft]) for j in rows)


class DenoiseObj(S.Obj):
    """the adapter of tests/stream_order.py's harness: batches in samples around the hop and the frame"""
    id, nfft, hop = "denoise", 256, 64

    def __init__(self):
        self.rx = R.receivers(self.nrx)

    def sizes(self, env):
        return [self.nfft + 3, 7], [self.hop - 1, 1, 2 * self.nfft + 5]

    def inputs(self, env, n):
        return (R.rows(self.nrx, n),)

    def make(self, env):
        return env.pkg.Denoise(self.rx, self.nfft, self.hop, window=R.window(self.nfft, self.hop))

    out_specs = S.DemodObj.out_specs
    process = S.BlankerObj.process

    def change(self, obj, k):
        for j in S.rows_of(k, self.nrx):
            mode, beta, gmin, alpha = R.receivers(self.nrx)[(j + k + 1) % self.nrx][:4]
            obj.set_rx(j, mode, beta, gmin, alpha, (R.RESTART, R.HOLD, 0)[k % 3])

    def read(self, obj, st):
        return (obj.read_noise(stream=st),)


@pytest.fixture(scope="module")
def env(pkg, dev):
    S.side_streams(dev, 1)
    return types.SimpleNamespace(pkg=pkg, dev=dev)


def test_steady_state_on_a_busy_side_stream(env):
    G.steady_state(env, DenoiseObj())


def test_changes_behind_a_busy_stream(env):
    G.test_b_changes_behind_a_busy_stream(env, DenoiseObj())
