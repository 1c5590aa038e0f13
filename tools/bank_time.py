"""Timing of the channel bank (pddc_bank_process, k_fir_i8x_bank) on the GPU box: K tuned receivers (48-tap decimate-by-8
first stage alone, hist 64, K different tuning words) fed the same batch, as ONE bank round against the same K pipelines
processed one after another (K solo process() calls: K reads of the batch, the traffic of a gang round).  Same on-device
LCG input, first-come buffers, HIP events on the launch stream, median of `steps` rounds after warm-up.  A 32-tap (hist 32)
row at 2^28 as well.  Usage: python tools/bank_time.py [--steps N] [--max-log2 28] [--only-k 4] [--rounds-only]
--rounds-only: K = 4 at 2^28, bank rounds only (for a rocprofv3 --kernel-trace --stats listing).
The GANG leg: a gang round (pddc_gang_push_async) brings its own generator launch and copies, so its first-stage kernel
is timed from a kernel trace instead -- `--legs K LOG2` runs `steps` gang rounds (on-device source, pageable outputs:
the kernel writes device memory) and `steps` bank rounds of the same K members, under
`rocprofv3 --kernel-trace -d DIR -o NAME -- ...`; `--summarize DB...` then prints per trace the gang's k_fir_i8x_many
(one launch, the member as the grid's second dimension: K reads of the batch) against the bank's k_fir_i8x_bank launches
of a round (median kernel time per round).
--d10: the decimate-by-10 pairs instead -- K = 2, 4, 8 members of the drop-in API's 2, 1.6, 2, 1 MS/s plans (a 54 / 51 / 54 /
49-tap tuned /10 first stage, hist 56 / 56 / 56 / 48, then /4, /5, /4, /8), one k_fir_i8x_bank<64, 2, 10> launch per pair,
against K solo process() calls (the I8xD10 route: k_fir_i8x<64, 2, false, 0, 10> and the second stage, per member);
with --rounds-only: bank rounds of K = 2 (--only-k) at 2^28 for a kernel trace."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("libperseus-sdr_amd")
dev = torch.device("cuda:0")
FREGS = [381178347, 0x7FFFF000, 123456789, 3000000000, 0x80000C35, 1 << 28, 0x0ABCDEF0, 0xFFFFF3CB]


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def members(k, ns, ntaps):
    pipes = []
    for i in range(k):
        p = pkg.Pipeline([(8, lowpass(ntaps, 0.05))], mix=True)
        p.set_freg(FREGS[i])
        pipes.append(p)
    outs = [torch.empty((p.max_output(ns) + 8, 2), dtype=torch.float32, device=dev) for p in pipes]
    return pipes, outs


D10_CYCLE = [2000000, 1600000, 2000000, 1000000]


def members_d10(k, ns):
    pipes = []
    for i in range(k):
        p = pkg.Pipeline([(d, t) for d, t, _ in pkg.api_plan(D10_CYCLE[i % len(D10_CYCLE)])], mix=True)
        p.set_freg(FREGS[i])
        pipes.append(p)
    outs = [torch.empty((p.max_output(ns) + 8, 2), dtype=torch.float32, device=dev) for p in pipes]
    return pipes, outs


def median_ms(fn, steps, st):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def row(k, log2, steps, ntaps=48):
    """ntaps 0: the decimate-by-10 members (members_d10)"""
    ns = 1 << log2
    st = torch.cuda.current_stream(dev)
    d_in = pkg.synth_lcg(6 * ns, 12345, 0, dev)
    make = (lambda k, ns: members_d10(k, ns)) if ntaps == 0 else (lambda k, ns: members(k, ns, ntaps))
    bp, bo = make(k, ns)
    bank = pkg.Bank(bp)
    ptrs, caps = [o.data_ptr() for o in bo], [o.shape[0] for o in bo]

    def bank_round():
        _, nb = bank.process_ptr(d_in.data_ptr(), ns, ptrs, caps, st.cuda_stream)
        assert nb == k

    t_bank = median_ms(bank_round, steps, st)
    mask, launches = bank.schedule(ns)
    bank.close()
    for p in bp:
        p.close()
    del bo
    sp, so = make(k, ns)

    def solo_round():
        for p, o in zip(sp, so):
            p.process_ptr(d_in.data_ptr(), ns, o.data_ptr(), o.shape[0], st.cuda_stream)

    t_solo = median_ms(solo_round, steps, st)
    for p in sp:
        p.close()
    del so, d_in
    torch.cuda.empty_cache()
    return dict(k=k, log2=log2, ntaps=ntaps, launches=launches, bank_ms=t_bank, solo_ms=t_solo)


def legs(k, log2, steps):
    """gang rounds, then bank rounds, of the same K members (for the kernel trace)"""
    ns = 1 << log2
    pipes, outs = members(k, ns, 48)
    gang = pkg.Gang(0)
    cap = pipes[0].max_output(ns) + 8
    h_out = [np.empty(2 * cap, np.float32) for _ in range(k)]      # pageable: the gang's kernel writes device memory
    for r in range(steps):
        items = [dict(pipe=p, h_out=h.ctypes.data, out_cap=cap, seed=12345, byte_offset=6 * ns * r) for p, h in zip(pipes, h_out)]
        res, ng = gang.push_async(items, ns)
        assert ng == k, ng
        for p, (_, t) in zip(pipes, res):
            p.wait_ticket(t)
    gang.close()
    for p in pipes:
        p.close()
    bp, bo = members(k, ns, 48)
    bank = pkg.Bank(bp)
    d_in = pkg.synth_lcg(6 * ns, 12345, 0, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(steps):
        _, nb = bank.process_ptr(d_in.data_ptr(), ns, [o.data_ptr() for o in bo], [o.shape[0] for o in bo], st)
        assert nb == k
    torch.cuda.synchronize()
    bank.close()
    for p in bp:
        p.close()
    print(f"legs: K {k} 2^{log2}: {steps} gang rounds, {steps} bank rounds")


def summarize(dbs):
    import re
    import sqlite3
    print("first-stage kernel time per round from a kernel trace (median over rounds, ms): the gang's k_fir_i8x_many "
          "(K reads) against the bank's k_fir_i8x_bank launches (one read per group of 4 / 2)")
    print(f"{'trace':>24} {'K':>2} {'gang':>9} {'bank':>9} {'gang/bank':>9}")
    for db in dbs:
        c = sqlite3.connect(db)
        rows = c.execute("select name, grid_y, end - start from kernels order by start").fetchall()
        gang = [d for n, gy, d in rows if "k_fir_i8x_many" in n]
        bank = [(int(re.search(r"k_fir_i8x_bank<\d+, (\d)(?:, \d+)?>", n).group(1)), d) for n, gy, d in rows if "k_fir_i8x_bank" in n]
        ks = {gy for n, gy, d in rows if "k_fir_i8x_many" in n}
        k = max(ks) if ks else 0
        per_round = []
        acc, members_done = 0, 0
        for nch, d in bank:                       # a round's launches cover K members
            acc += d
            members_done += nch
            if members_done >= k:
                per_round.append(acc)
                acc, members_done = 0, 0
        g = float(np.median(gang)) / 1e6 if gang else float("nan")
        b = float(np.median(per_round)) / 1e6 if per_round else float("nan")
        print(f"{os.path.basename(db)[:24]:>24} {k:>2} {g:>9.4f} {b:>9.4f} {g / b:>9.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, nargs=2, metavar=("K", "LOG2"))
    ap.add_argument("--summarize", nargs="+", metavar="DB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-log2", type=int, default=28)
    ap.add_argument("--only-k", type=int, default=0)
    ap.add_argument("--rounds-only", action="store_true")
    ap.add_argument("--d10", action="store_true", help="the decimate-by-10 pairs (see the module's text)")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    if a.legs:
        legs(a.legs[0], a.legs[1], a.steps)
        return
    if a.d10 and a.rounds_only:
        ns, k = 1 << 28, a.only_k or 2
        bp, bo = members_d10(k, ns)
        bank = pkg.Bank(bp)
        d_in = pkg.synth_lcg(6 * ns, 12345, 0, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        mask, launches = bank.schedule(ns)
        for _ in range(a.steps):
            _, nb = bank.process_ptr(d_in.data_ptr(), ns, [o.data_ptr() for o in bo], [o.shape[0] for o in bo], st)
            assert nb == k, nb
        torch.cuda.synchronize()
        bank.close()
        print(f"{a.steps} bank rounds, K = {k} decimate-by-10 members, 2^28 samples, {launches} bank launches per round")
        return
    if a.d10:
        print(f"bank round vs K solo process() calls, decimate-by-10 members (2 / 1.6 / 2 / 1 MS/s plans), median of {a.steps}, ms")
        print(f"{'K':>2} {'log2':>4} {'launches':>8} {'bank':>9} {'K solo':>9} {'ratio':>6} {'bank/K':>8}")
        for k in [a.only_k] if a.only_k else [2, 4, 8]:
            for log2 in (22, 24, 26, 28):
                if log2 > a.max_log2:
                    continue
                r = row(k, log2, a.steps, ntaps=0)
                print(f"{k:>2} {log2:>4} {r['launches']:>8} {r['bank_ms']:>9.4f} {r['solo_ms']:>9.4f} "
                      f"{r['solo_ms'] / r['bank_ms']:>6.2f} {r['bank_ms'] / k:>8.4f}", flush=True)
        return
    if a.rounds_only:
        ns = 1 << 28
        bp, bo = members(4, ns, 48)
        bank = pkg.Bank(bp)
        d_in = pkg.synth_lcg(6 * ns, 12345, 0, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for _ in range(a.steps):
            bank.process_ptr(d_in.data_ptr(), ns, [o.data_ptr() for o in bo], [o.shape[0] for o in bo], st)
        torch.cuda.synchronize()
        bank.close()
        print(f"{a.steps} bank rounds, K = 4, 2^28 samples")
        return
    print(f"bank round vs K solo process() calls, 48-tap tuned /8 first stage (hist 64), median of {a.steps}, ms")
    print(f"{'K':>2} {'log2':>4} {'launches':>8} {'bank':>9} {'K solo':>9} {'ratio':>6} {'bank/K':>8}")
    ks = [a.only_k] if a.only_k else [1, 2, 4, 8]
    for k in ks:
        for log2 in (22, 24, 26, 28):
            if log2 > a.max_log2:
                continue
            r = row(k, log2, a.steps)
            print(f"{k:>2} {log2:>4} {r['launches']:>8} {r['bank_ms']:>9.4f} {r['solo_ms']:>9.4f} "
                  f"{r['solo_ms'] / r['bank_ms']:>6.2f} {r['bank_ms'] / k:>8.4f}", flush=True)
    if a.max_log2 >= 28 and not a.only_k:
        for k in (2, 4):
            r = row(k, 28, a.steps, ntaps=32)
            print(f"32 taps (hist 32): K {k} 2^28 bank {r['bank_ms']:.4f} K solo {r['solo_ms']:.4f} "
                  f"ratio {r['solo_ms'] / r['bank_ms']:.2f}", flush=True)


if __name__ == "__main__":
    main()
