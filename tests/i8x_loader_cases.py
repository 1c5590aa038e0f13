"""The cases of tests/test_gpu_i8x_loaders.py: every loader instantiation of k_fir_i8x (ddc_fir_i8.hip) at the smallest
shapes at which its input loads can go wrong.  tools/i8x_loader_golden.py runs the same cases to record the fixtures
tests/golden/i8x_loaders_<case>.f32 (recorded from the build BEFORE the loaders took their main groups through per-tile
buffer descriptors; integer accumulation is exact and the float recombination did not change, so every later build must
give the same bits).

A case is a stream cut into consecutive batches on ONE pipeline (bank: one set of members, gang: one set of receivers),
so every batch but the first starts on the history the batch before left -- ragged batches included.  run_case returns
one record per (batch, member): what the oracle needs to check it, and the outputs."""
import os

import numpy as np

FREG = 381178347
TILE = 8192
TILE10 = 10240
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def load_taps(name):
    return np.fromfile(os.path.join(GOLD, f"taps_{name}.f32"), dtype=np.float32)


# one group; a tile less one group, a tile, a tile and one group; three tiles less one group
LENS = [8, TILE - 8, TILE, TILE + 8, 3 * TILE - 8]
# with two blocks (option i8x_blocks = 2, tile-interleaved): batches of k tiles, the last one ragged, give the blocks
# (1, 0), (1, 1), (2, 1), (3, 2), (4, 3), (5, 4) tiles -- each count 0 .. 5: the prologue alone, both halves of the unrolled
# loop, the drain, the ragged tile as a block's last in either half
KS = [1, 2, 3, 5, 7, 9]
# decimate by 10: a batch of a tile and one group moves the stream's decimation phase by 8, so five of them start on every
# phase a stream of whole groups can reach (first outputs on samples 0, 2, 4, 6, 8 of the batch: tap delays 0, 6, 4, 2, 0,
# in_off 0 and 8 -- odd phases need a batch that is no multiple of 8 samples, which no route accepts); then the lengths
# around a tile
LENS10 = [TILE10 + 8] * 5 + [8, TILE10 - 8, TILE10, 3 * TILE10 - 8]


def solo_cases():
    """name -> (stages, mix, options, batch sizes)"""
    t127, t255, h48, h56, h51 = load_taps("d8_127"), load_taps("d8_255"), lowpass(48, 0.05), lowpass(56, 0.05), lowpass(51, 0.04)
    return {
        "plain127": ([(8, t127)], False, {"i8x_plain": 1}, LENS),
        "tuned48": ([(8, h48)], True, {}, LENS),                       # paired rows, two k-steps
        "tuned127": ([(8, t127)], True, {}, LENS),                     # paired rows, three k-steps
        "tuned255": ([(8, t255)], True, {}, LENS),                     # tap sets split over the waves; the loaders finish
        # the fused pair runs on whole tiles (the ragged batches between them take the unfused kernel on the same state)
        "pair48_56": ([(8, h48), (8, h56)], True, {}, [TILE, 8, TILE - 8, 3 * TILE, TILE + 8, 3 * TILE - 8, 2 * TILE]),
        "d10_51": ([(10, h51)], True, {}, LENS10),
        "plain127_b2": ([(8, t127)], False, {"i8x_plain": 1, "i8x_blocks": 2}, [k * TILE - 8 for k in KS]),
        "tuned255_b2": ([(8, t255)], True, {"i8x_blocks": 2}, [k * TILE - 8 for k in (1, 2, 3, 5)]),
        "pair48_56_b2": ([(8, h48), (8, h56)], True, {"i8x_blocks": 2}, [k * TILE for k in KS + [10]]),
        "d10_51_b2": ([(10, h51)], True, {"i8x_blocks": 2}, [k * TILE10 - 8 for k in KS]),
    }


def bank_cases(pkg):
    """name -> ([(stages, freg)], batch sizes)"""
    h32, h48 = load_taps("c320_s1_d8_32"), lowpass(48, 0.05)
    m2 = pkg.api_plan(2000000)
    return {
        "bank2": ([([(8, h48)], FREG), ([(8, h48)], 123456789)], LENS),
        "bank4": ([([(8, h32)], f) for f in (FREG, 0x7FFFF000, 123456789, 3000000000)], LENS),
        "bank10": ([(m2, FREG), (m2, 123456789)], [TILE10 + 8, TILE10 + 8, 3 * TILE10 - 8]),
    }


GANG_SIZES = [3 * TILE - 8, TILE + 8, TILE]
GANG_SEEDS = [777, 790]
CASES = ["plain127", "tuned48", "tuned127", "tuned255", "pair48_56", "d10_51", "plain127_b2", "tuned255_b2", "pair48_56_b2",
         "d10_51_b2", "bank2", "bank4", "bank10", "gang2"]
SEED = 2026


PAD = TILE          # zero samples behind a case's stream: the oracle checks batches of the PERIODIC stream, and a pipeline
                    # starts on a history of zeros -- with the pad the stream's first batch has the same past in both


def stream_len(pkg, name):
    if name == "gang2":
        return sum(GANG_SIZES)
    solo = solo_cases()
    return sum(solo[name][3] if name in solo else bank_cases(pkg)[name][1])


def stream_bytes(pkg, O, name, seed=SEED):
    """the packed stream of a case: lcg bytes, then the zero pad (never processed)"""
    return np.concatenate([O.lcg_bytes(6 * stream_len(pkg, name), seed), np.zeros(6 * PAD, np.uint8)])


def run_case(pkg, dev, O, name):
    """-> (list of dicts: packed (the member's whole stream), first_in, n_in, stages, freg, mix, out (float32, interleaved);
    bank / gang: per round, the number of members that shared the launch)"""
    import torch
    recs, shared = [], []
    solo = solo_cases()
    if name in solo:
        stages, mix, opts, sizes = solo[name]
        packed = stream_bytes(pkg, O, name)
        d_in = torch.from_numpy(packed).to(dev)
        pipe = pkg.Pipeline(stages, mix=mix)
        for k, v in opts.items():
            pipe.set_option(k, v)
        if mix:
            pipe.set_freg(FREG)
        pos = 0
        for ns in sizes:
            y = pipe.process(d_in[6 * pos:6 * (pos + ns)]).cpu().numpy().reshape(-1).copy()
            recs.append(dict(packed=packed, first_in=pos, n_in=ns, stages=stages, freg=FREG if mix else 0, mix=mix, out=y))
            pos += ns
        pipe.close()
        return recs, shared
    if name == "gang2":
        stages = [(8, load_taps("d8_127"))]
        packs = [stream_bytes(pkg, O, name, sd) for sd in GANG_SEEDS]
        gang = pkg.Gang(0)
        pipes, bufs = [], []
        for s in GANG_SEEDS:
            p = pkg.Pipeline(stages, mix=True)
            p.set_freg(FREG)
            pipes.append(p)
            bufs.append(pkg.PinnedBuffer((p.max_output(max(GANG_SIZES)) + 8) * 8))
        pos = 0
        for ns in GANG_SIZES:
            items = [dict(pipe=p, h_out=b.ptr, out_cap=p.max_output(max(GANG_SIZES)) + 8, seed=s, byte_offset=6 * pos)
                     for p, b, s in zip(pipes, bufs, GANG_SEEDS)]
            res, ng = gang.push_async(items, ns)
            shared.append(ng)
            for p, b, (n_out, t), pk in zip(pipes, bufs, res, packs):
                p.wait_ticket(t)
                y = b.array[:8 * n_out].view(np.float32).copy()
                recs.append(dict(packed=pk, first_in=pos, n_in=ns, stages=stages, freg=FREG, mix=True, out=y))
            pos += ns
        gang.close()
        for p, b in zip(pipes, bufs):
            p.close()
            b.free()
        return recs, shared
    members, sizes = bank_cases(pkg)[name]
    packed = stream_bytes(pkg, O, name)
    d_in = torch.from_numpy(packed).to(dev)
    pipes = []
    for stages, freg in members:
        p = pkg.Pipeline(stages, mix=True)
        p.set_freg(freg)
        pipes.append(p)
    outs = [torch.empty((p.max_output(max(sizes)) + 8, 2), dtype=torch.float32, device=dev) for p in pipes]
    bank = pkg.Bank(pipes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pos = 0
    for ns in sizes:
        n, nb = bank.process_ptr(d_in[6 * pos:].data_ptr(), ns, [o.data_ptr() for o in outs], [o.shape[0] for o in outs], stream)
        torch.cuda.synchronize()
        shared.append(nb)
        for (stages, freg), o, k in zip(members, outs, n):
            recs.append(dict(packed=packed, first_in=pos, n_in=ns, stages=stages, freg=freg, mix=True,
                             out=o[:k].cpu().numpy().reshape(-1).copy()))
        pos += ns
    bank.close()
    for p in pipes:
        p.close()
    return recs, shared


def golden_path(name):
    return os.path.join(GOLD, f"i8x_loaders_{name}.f32")


# The fixtures of these cases hold only the outputs whose windows touch something the loaders decide: 32 outputs either side
# of every tile boundary (1024 outputs), 16 either side of the boundaries between the loader threads' rounds of groups (512
# groups: output 512 of a tile, decimate by 10: 409.6 and 819.2), and the batch's last 32.  Everything else of a large batch is
# the middle of a round of whole groups; the oracle still sees every output.  (The other cases keep every output.)
EDGES_ONLY = {"plain127_b2", "tuned255_b2", "d10_51", "d10_51_b2", "bank2", "bank4", "gang2"}


def kept(name, rec):
    """indices (complex outputs) of a record that go into the case's fixture"""
    n = rec["out"].size // 2
    i = np.arange(n)
    if name not in EDGES_ONLY or len(rec["stages"]) != 1:
        return i
    r = i % 1024
    mids = (409.6, 819.2) if rec["stages"][0][0] == 10 else (512.0,)
    m = (r < 32) | (r >= 992) | (i >= n - 32)
    for c in mids:
        m |= np.abs(r - c) < 16
    return i[m]


def flat(recs, name):
    """the fixture's content: the kept outputs of every record, in order (float32, interleaved)"""
    parts = [r["out"].reshape(-1, 2)[kept(name, r)].reshape(-1) for r in recs]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)
