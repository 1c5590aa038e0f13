"""Timing of the carrier stage (pddc_carrier_process, k_carrier) on the GPU box: K receivers of AM carriers (the test
signal of tests/carrier_ref.py, 30 Hz loops), n outputs each, for DSB and for USB at L = 127 and L = 255; beside it
Demod.process with DCBLOCK + AGC on the same K and n -- the chain's other serial walk, here only the comparator.
A launch walks every receiver's n outputs in sequence, so its time is close to n times the latency of one loop step
whatever K is: per point the time, the implied clock cycles per step (at --mhz, a nominal engine clock: the
clock itself is not read) and the input GB/s (8 bytes per value read, 8 written).
Same on-device input, same process, HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/carrier_time.py [--steps 15] [--rx 1024] [--n 32768] [--mhz 2400] [--only-kernel]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # the signal maker is the tests' (carrier_ref.am_carriers): one definition
pkg = importlib.import_module("libperseus-sdr_amd")
import carrier_ref as CR  # noqa: E402  (the signal maker)

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
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--only-kernel", action="store_true", help="k_carrier only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    n = a.n
    kp, ki = pkg.carrier_loop(30.0, CR.RATE)
    both = pkg.PDDC_DEMOD_DCBLOCK | pkg.PDDC_DEMOD_AGC
    print("      n      K   mode   L    carrier ms   cycles/step   GB/s in   locked at the end   demod +DC+AGC ms   cycles/step")
    for K in a.rx:
        # 64 distinct carriers, repeated: the walk's time does not depend on the values.  Every timed call feeds the same z
        # again to loops that go on, so each call begins with a phase jump and a pull-in; that changes values, not time
        base, _ = CR.am_carriers(min(K, 64), n)
        z = torch.from_numpy(base).to(dev).repeat((K + base.shape[0] - 1) // base.shape[0], 1)[:K].contiguous()
        u = torch.empty_like(z)
        au = torch.empty((K, n), dtype=torch.float32, device=dev)
        post = pkg.Demod([(pkg.PDDC_DEMOD_SSB, 0, both)] * K)
        t_post = float("nan")
        if not a.only_kernel:
            post.process(z, out=au)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_post = timed(lambda: post.process(z, out=au), a.steps)
        for mode, name, L in ((pkg.PDDC_CARRIER_DSB, "DSB", 127), (pkg.PDDC_CARRIER_USB, "USB", 127), (pkg.PDDC_CARRIER_USB, "USB", 255)):
            c = pkg.Carrier([(mode, kp, ki)] * K, pkg.carrier_hilbert(L))
            c.process(z, out=u)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t = timed(lambda: c.process(z, out=u), a.steps)
            locked = int(c.read()["locked"].sum())
            cyc = lambda ms: ms * 1e-3 * a.mhz * 1e6 / n
            print(f"{n:7d}   {K:4d}   {name}   {L:3d}   {t:10.4f}   {cyc(t):11.0f}   {8e-6 * K * n / t:7.1f}   {locked:6d} of {K:4d}     "
                  f"{t_post:14.4f}   {cyc(t_post):11.0f}", flush=True)
            c.close()
        post.close()
        del z, u, au
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
