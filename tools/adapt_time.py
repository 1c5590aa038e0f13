"""Timing of the adaptive filter (pddc_adapt_process, k_adapt) on the GPU box: K receivers behind Channelizer (M = 4096,
hop 2048) -> Tuner (T = 64, R = 4) -> Demod (AM), every third receiver in NR, NOTCH and OFF, mu 0.25, leak 2^-10, delay 1.
Per point: (a) Adapt.process at 32, 64 and 128 taps on the demodulator's audio -- 8 bytes per value, 4 read and 4 written;
what bounds it is the dependent chain per sample, so the figure beside the time is ns per sample of one receiver's
series -- and (b) Demod.process with DCBLOCK + AGC on the same shape: the existing per-sample recursion, the yardstick.
Same on-device LCG input, same process, HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/adapt_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--taps 32 64 128] [--only-kernel]"""
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
    ap.add_argument("--taps", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--delay", type=int, default=1)
    ap.add_argument("--only-kernel", action="store_true", help="k_adapt only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    M, hop, T, R = 4096, 2048, 64, 4
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    both = pkg.PDDC_DEMOD_DCBLOCK | pkg.PDDC_DEMOD_AGC
    modes = (pkg.PDDC_ADAPT_NR, pkg.PDDC_ADAPT_NOTCH, pkg.PDDC_ADAPT_OFF)
    print("samples   values      K   taps   adapt ms   ns/sample   +DC+AGC ms   adapt / +DC+AGC")
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
            plain.process(z, out=au)
            post.process(z, out=out)
            torch.cuda.synchronize()
            t_post = float("nan")
            if not a.only_kernel:
                time.sleep(1.0)
                t_post = timed(lambda: post.process(z, out=out), a.steps)
            for taps in a.taps:
                ad = pkg.Adapt([(modes[j % 3], 0.25, 2.0 ** -10) for j in range(K)], taps, a.delay)
                ad.process(au, out=out)
                torch.cuda.synchronize()
                time.sleep(1.0)
                t_ad = timed(lambda: ad.process(au, out=out), a.steps)
                print(f"2^{lg:<2}     {n:7d}   {K:4d}   {taps:4d}   {t_ad:8.4f}   {1e6 * t_ad / n:9.1f}   {t_post:10.4f}   "
                      f"{t_ad / t_post:8.1f}", flush=True)
                ad.close()
            for o in (plain, post, tun):
                o.close()
            del out, au, zbuf, z
            torch.cuda.empty_cache()
        ch.close()
        del d, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
