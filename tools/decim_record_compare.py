#!/usr/bin/env python3
"""Results of the main pipeline, one build of the kernel library against another, bit for bit.

    python tools/decim_record_compare.py A.so B.so        (on a machine with the GPU; build them with tools/ab.sh build)

One fresh process per library (PDDC_DDC_LIB, as tools/ab.sh selects a build); every process runs the same plans over
the seed-12345 LCG stream generated on the device, cut into unequal batches that are multiples of 8, and takes the
sha256 of the raw output bytes of every batch.  The plans are the ones that go through the plain-decimator launcher
and the NCO record: packed first stages on k_firp and on k_fir_generic through a retune, carried and fenced tails of
both kinds, the fused cascade, the mixed-history route (a history window of three tuning words) and a gang round.
The parent prints one line per plan and exits 1 if any batch differs.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
NS = 1 << 22
WORDS = [381178347, 123456789, 0x9E3779B1, 3000000000, 0x7FFFFFF1]
# unequal, multiples of 8; the first two and the last are whole tiles of every first-stage kernel (tails are carried), the
# others are not (tails run in line, or are fenced)
CUTS = [0, 1 << 20, 3 << 19, (3 << 19) + 98760, (3 << 20) + 24, NS]


def lowpass(ntaps, cutoff):
    import numpy as np
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def digests(buf, where):
    """sha256 of every batch's outputs: buf is the host copy of the float32 pairs, where = [(first pair, pairs)]"""
    return [hashlib.sha256(buf[2 * at:2 * (at + n)].tobytes()).hexdigest() for at, n in where]


def run_stream(pkg, torch, dev, stages, cuts, retune, overlap=False, opts=None):
    """retune: {batch index: word} (0: the first word).  Outputs are read only behind the fence, after the last batch."""
    d_in = pkg.synth_lcg(6 * cuts[-1], SEED, 0, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    pipe = pkg.Pipeline(stages, mix=True)
    for k, v in (opts or {}).items():
        pipe.set_option(k, v)
    if overlap:
        pipe.set_overlap(True)
    sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    out = torch.zeros((sum(pipe.max_output(n) + 2 for n in sizes), 2), dtype=torch.float32, device=dev)
    where, at = [], 0
    for k, (a, n) in enumerate(zip(cuts[:-1], sizes)):
        if k in retune:
            pipe.set_freg(retune[k])
        m = pipe.process_ptr(d_in[6 * a:].data_ptr(), n, out[at:].data_ptr(), out.shape[0] - at, st)
        where.append((at, m))
        at += m + (m & 1)                         # every batch's outputs start 16-byte aligned
    pipe.fence(st)
    torch.cuda.synchronize()
    pipe.close()
    return digests(out[:at].cpu().numpy().reshape(-1), where)


def run_gang(pkg, stages, nrx, sizes):
    import numpy as np
    gang = pkg.Gang(0)
    pipes, bufs, cap = [], [], 0
    for i in range(nrx):
        p = pkg.Pipeline(stages, mix=True)
        p.set_freg(WORDS[i % len(WORDS)])
        cap = p.max_output(max(sizes)) + 8
        pipes.append(p)
        bufs.append(pkg.PinnedBuffer(cap * 8))
    out, pos = [], 0
    for k, ns in enumerate(sizes):
        if k == 2:
            pipes[1].set_freg(WORDS[4])
        items = [{"pipe": p, "h_out": b.ptr, "out_cap": cap, "seed": SEED, "byte_offset": 6 * pos} for p, b in zip(pipes, bufs)]
        res, shared = gang.push_async(items, ns)
        for p, b, (n_out, t) in zip(pipes, bufs, res):
            p.wait_ticket(t)
            out.append(hashlib.sha256(np.array(b.array[:8 * n_out], copy=True).tobytes()).hexdigest() + ":%d" % shared)
        pos += ns
    for p, b in zip(pipes, bufs):
        p.close()
        b.free()
    gang.close()
    return out


def child():
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    pkg = importlib.import_module("libperseus-sdr_amd")
    dev = torch.device("cuda:0")
    two = {0: WORDS[0], 2: WORDS[1]}
    res = {}
    res["10*5 nco, retune (packed k_firp)"] = run_stream(
        pkg, torch, dev, [(10, lowpass(97, 0.04)), (5, lowpass(81, 0.08))], CUTS, two)
    res["7*4 nco, retune (packed k_fir_generic)"] = run_stream(
        pkg, torch, dev, [(7, lowpass(99, 0.06)), (4, lowpass(33, 0.1))], CUTS, two)
    for name, tail in (("8*10", (10, lowpass(287, 0.04))), ("8*7", (7, lowpass(99, 0.06)))):
        for ov in (False, True):
            res["%s vector kernels, overlap %s" % (name, "on" if ov else "off")] = run_stream(
                pkg, torch, dev, [(8, lowpass(56, 0.05)), tail], CUTS, two, overlap=ov, opts={"i8x": 0})
    res["8*8*5 nco"] = run_stream(pkg, torch, dev, [(8, lowpass(32, 0.05)), (8, lowpass(64, 0.05)), (5, lowpass(161, 0.08))],
                                  CUTS, two)
    # decimate by 8, 127 taps (history 128): 32-sample batches, a new word before each of batches 8..13, 40..42 and every
    # fourth one of 100..200 -- history windows of one, two, three and four words -- then the rest of the stream at once
    small = 256
    cuts = [32 * k for k in range(small + 1)] + [NS]
    retune = {0: WORDS[0]}
    for j, k in enumerate(list(range(8, 14)) + [40, 41, 42] + list(range(100, 200, 4)) + [small]):
        retune[k] = WORDS[(j + 1) % len(WORDS)] + 977 * j
    res["8 nco, 32-sample batches with retunes (mixed history)"] = run_stream(pkg, torch, dev, [(8, lowpass(127, 0.05))], cuts, retune)
    res["gang of four 8*10"] = run_gang(pkg, [(8, lowpass(64, 0.05)), (10, lowpass(161, 0.04))], 4,
                                        [1 << 18, 3 << 16, 1 << 20, 4096, 5 << 14])
    print("RESULT " + json.dumps(res))


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        return child()
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    got = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, PDDC_DDC_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                           timeout=300)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
            sys.exit("%s: the run failed (exit %d); nothing more is started" % (lib, p.returncode))
        got.append(json.loads(line[0][7:]))
    bad = 0
    for name in got[0]:
        a, b = got[0][name], got[1].get(name)
        same = a == b
        bad += not same
        whole = hashlib.sha256("".join(a).encode()).hexdigest()[:16]
        print("  %-58s batches %4d: %s  (%s)" % (name, len(a), "identical" if same else "DIFFERENT", whole))
        if not same:
            print("     first differing batch:", next((i for i, (x, y) in enumerate(zip(a, b or [])) if x != y), None))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
