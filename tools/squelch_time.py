"""Timing of the squelch (pddc_squelch_process, k_squelch) on the GPU box: K receivers behind Channelizer (M = 4096, hop
2048) -> Tuner (T = 64, R = 4) -> Demod (AM), B = 48, attack 2, hang 3, ramp 37, GATE | RELATIVE on every other receiver.
Per point: (a) Squelch.process -- 16 bytes per value: 8 of z and 4 of a read, 4 of out written --, (b) Demod.process,
the detectors alone (12 bytes per value), and (c) the detectors with DCBLOCK + AGC on the same z: the yardsticks for a
12-to-16-byte-per-value pass.  Same on-device LCG input, same process, HIP events on the launch stream, median of
`steps` after a settle second.
Usage: python tools/squelch_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--block 48] [--only-kernel]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("libperseus-sdr_amd")
dev = torch.device("cuda:0")


def timed(fn, steps):
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--logs", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--rx", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--block", type=int, default=48)
    ap.add_argument("--only-kernel", action="store_true", help="k_squelch only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    M, hop, T, R = 4096, 2048, 64, 4
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    both = pkg.PDDC_DEMOD_DCBLOCK | pkg.PDDC_DEMOD_AGC
    print("samples   outputs      K   squelch ms   GB/s   us/output   detect ms   GB/s   +DC+AGC ms   open at the end")
    for lg in a.logs:
        ns = 1 << lg
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        ch = pkg.Channelizer(M, w, hop)
        rows = ch.process(d)
        S = rows.shape[0]
        rng = np.random.default_rng(2024)
        for K in a.rx:
            words = [int(v) for v in rng.integers(0, 1 << 32, K, dtype=np.uint64)]
            tun = pkg.Tuner(ch, words, h, R)
            zbuf = torch.empty((K, (S - T) // R + 1 + T), dtype=torch.complex64, device=dev)
            z = tun.process(rows, out=zbuf)
            n = z.shape[1]
            au = torch.empty((K, n), dtype=torch.float32, device=dev)
            out = torch.empty((K, n), dtype=torch.float32, device=dev)
            plain = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)] * K)
            post = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, both)] * K)
            # full-scale noise in every channel: relative thresholds around 1 keep the gates moving
            sq = pkg.Squelch([(1.3, 1.1, (pkg.PDDC_SQL_GATE | pkg.PDDC_SQL_RELATIVE) if j % 2 else 0) for j in range(K)],
                             a.block, 2, 3, 37, up=1.03125)
            blocks = n // a.block + 1
            lv = torch.empty((K, blocks), dtype=torch.float32, device=dev)
            ss = torch.empty((K, blocks), dtype=torch.uint8, device=dev)
            post.process(z, out=out)
            plain.process(z, out=au)
            sq.process(z, au, out=out, levels=lv, states=ss)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_sq = timed(lambda: sq.process(z, au, out=out, levels=lv, states=ss), a.steps)
            t_plain = t_post = float("nan")
            if not a.only_kernel:
                t_plain = timed(lambda: plain.process(z, out=au), a.steps)
                t_post = timed(lambda: post.process(z, out=out), a.steps)
            nopen = int(sq.read()["open"].sum())
            print(f"2^{lg:<2}     {n:7d}   {K:4d}   {t_sq:10.4f}   {16e-6 * K * n / t_sq:4.0f}   {1e3 * t_sq / n:9.4f}   "
                  f"{t_plain:9.4f}   {12e-6 * K * n / t_plain:4.0f}   {t_post:10.4f}   {nopen:4d} of {K}", flush=True)
            for o in (sq, plain, post, tun):
                o.close()
            del out, au, lv, ss, zbuf, z
            torch.cuda.empty_cache()
        ch.close()
        del d, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
