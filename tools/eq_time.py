"""Timing of the equaliser (pddc_eq_process, k_eq) on the GPU box: 1024 receivers x 32 768 samples, and the 0.1 s batch of
1024 x 977 samples at 9765.625 Hz.  Per shape: (a) Eq.process at S = 1, 2, 4 and 8 with every receiver at nsec = S (the
pool of tests/eq_ref.py's designs in turn), and at S = 8 with nsec = 2 -- 8 bytes per value, 4 read and 4 written; what
bounds it is the dependent binary64 chain per step, so the figure beside the time is ns per sample of one receiver's
series; (b) a device copy of the same bytes, the floor of the traffic; (c) Demod.process with DCBLOCK + AGC on the same
shape: the existing per-sample recursion, the yardstick.  Same process, HIP events on the launch stream, median of
`steps` after a settle second.
Usage: python tools/eq_time.py [--steps 15] [--rx 1024] [--samples 32768 977] [--only-kernel]"""
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
RATE = 9765.625


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


def pool():
    """stable sections of every kind: the receivers take them in turn"""
    P = pkg
    return [P.eq_section(P.PDDC_EQ_NOTCH, RATE, 20.0, 30.0), P.eq_section(P.PDDC_EQ_PEAK, RATE, 700.0, 20.0, 18.0),
            P.eq_deemphasis(RATE, 750e-6), P.eq_section(P.PDDC_EQ_HIGHPASS, RATE, 300.0), P.eq_section(P.PDDC_EQ_NOTCH, RATE, 50.0, 30.0),
            P.eq_section(P.PDDC_EQ_LOWSHELF, RATE, 400.0, 0.7071, -6.0), P.eq_section(P.PDDC_EQ_LOWPASS, RATE, 2700.0),
            P.eq_section(P.PDDC_EQ_HIGHSHELF, RATE, 2000.0, 0.7071, 4.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rx", type=int, default=1024)
    ap.add_argument("--samples", type=int, nargs="+", default=[32768, 977])
    ap.add_argument("--only-kernel", action="store_true", help="k_eq only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    K, p = a.rx, pool()
    both = pkg.PDDC_DEMOD_DCBLOCK | pkg.PDDC_DEMOD_AGC
    cases = [(1, 1), (2, 2), (4, 4), (8, 8), (8, 2)]
    print("samples      K    S  nsec      eq ms   ns/sample    copy ms   +DC+AGC ms   eq / +DC+AGC   eq / eq(S=1)")
    for n in a.samples:
        gen = torch.Generator(device="cpu").manual_seed(7)
        z = torch.view_as_complex(torch.randn((K, n, 2), generator=gen, dtype=torch.float32)).to(dev)
        au = (0.1 * torch.randn((K, n), generator=gen, dtype=torch.float32)).to(dev)
        out = torch.empty((K, n), dtype=torch.float32, device=dev)
        t_copy = t_post = float("nan")
        if not a.only_kernel:
            post = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, both)] * K)
            post.process(z, out=out)
            out.copy_(au)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_post = timed(lambda: post.process(z, out=out), a.steps)
            t_copy = timed(lambda: out.copy_(au), a.steps)
            post.close()
        t_one = None
        for S, nsec in cases:
            eq = pkg.Eq([[p[(j + s) % len(p)] for s in range(nsec)] for j in range(K)], S)
            eq.process(au, out=out)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all())
            time.sleep(1.0)
            t = timed(lambda: eq.process(au, out=out), a.steps)
            t_one = t if t_one is None else t_one
            print(f"{n:7d}   {K:4d}   {S:2d}    {nsec:2d}   {t:8.4f}   {1e6 * t / n:9.1f}   {t_copy:8.4f}   {t_post:10.4f}   "
                  f"{t / t_post:12.2f}   {t / t_one:12.2f}", flush=True)
            eq.close()
        del z, au, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
