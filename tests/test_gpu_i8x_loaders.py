"""GPU tests (-m gpu) of k_fir_i8x's loaders (ddc_fir_i8.hip): the main groups of a tile come through a buffer descriptor of
that tile -- no branch, no zero fill: a group that is not wholly inside the batch is zeros by the hardware's range check --,
the front groups of the tiles behind the first through one of their own, and the bytes are de-interleaved in two stages.
None of it may move a bit: integer accumulation is exact and the float recombination is what it was, so every output of
every loader instantiation must be the bits the kernel gave BEFORE that change (tests/golden/i8x_loaders_<case>.f32,
recorded by tools/i8x_loader_golden.py from the parent build), and within 1e-6 of the oracle per chunk (orc_chain_check),
as everywhere.

The cases (tests/i8x_loader_cases.py) are the smallest shapes at which the loads can go wrong: batches of one group, a tile
less one group, a tile, a tile and one group, three tiles less one group -- consecutive on one stream, so that every batch
starts on the history a ragged one left --; with two blocks, batches that give a block 0 .. 5 tiles (the prologue alone,
both halves of the unrolled loop, the drain), the last tile ragged; for the decimate-by-10 form every decimation phase a
stream of whole groups can reach (first outputs on samples 0, 2, 4, 6, 8: both values of in_off, tap delays 0, 2, 4, 6)."""
import numpy as np
import pytest

import i8x_loader_cases as K

pytestmark = pytest.mark.gpu
FIR_TOL = 1e-6


@pytest.mark.parametrize("name", K.CASES)
def test_loader_case_gives_the_recorded_bits_and_the_oracles_values(pkg, dev, O, name):
    recs, shared = K.run_case(pkg, dev, O, name)
    if name.startswith("bank") or name.startswith("gang"):
        # the shared kernels really ran: every batch of at least a tile went out as ONE launch for all members
        members = len(recs) // len(shared)
        sizes = [r["n_in"] for r in recs[::members]]
        assert all(s == members for s, n in zip(shared, sizes) if n >= K.TILE), (shared, sizes)
    for r in recs:
        if r["out"].size == 0:
            continue                                    # (a decimate-by-10 batch of one group can have no output)
        c = O.chain_check(r["packed"], r["first_in"], r["n_in"], r["stages"], r["out"], freg=r["freg"], mix=r["mix"], tol=FIR_TOL)
        assert c["n"] == r["out"].size // 2 and c["ok"] and c["worst_chunk_rel_err"] <= FIR_TOL, (name, r["first_in"], r["n_in"], c)
    y = K.flat(recs, name)
    g = np.fromfile(K.golden_path(name), dtype=np.float32)
    assert y.size == g.size, (name, y.size, g.size)
    diff = np.flatnonzero(y.view(np.uint32) != g.view(np.uint32))
    assert diff.size == 0, (name, diff.size, diff[:8])


def test_the_cases_reach_every_kernel_form(pkg, dev):
    """what the pipeline chooses for the cases' batches: the matrix-core first stage for every batch of at least the history
    (8-sample batches take the vector kernel on the same stream state), the fused pair for whole tiles"""
    for name, (stages, mix, opts, sizes) in K.solo_cases().items():
        pipe = pkg.Pipeline(stages, mix=mix)
        for k, v in opts.items():
            pipe.set_option(k, v)
        if mix:
            pipe.set_freg(K.FREG)
        for ns in sizes:
            assert pipe.on_i8(ns) == (2 if stages[0][0] == 10 or ns >= 256 else 0), (name, ns, pipe.on_i8(ns))
            if len(stages) == 2:
                assert pipe.fused_pair(ns) == (2 if ns % K.TILE == 0 else 0), (name, ns)
        pipe.close()
