"""Timing of the scope (pddc_scope_process, k_scope) on the GPU box: K display slots, each on a row of its own, nfft 256 /
1024 / 2048 / 4096 with hop nfft/2 and avg 4, n samples per row in one batch (K = 1: 32 n, so that the one slot has lines
to spread).  Per point: (a) Scope.process, with its time per segment; (b) a device copy of the same input bytes
(pddc_measure_copy: what reading z once costs at least); (c) for 1024, 2048 and 4096 the panorama's time per segment
(Spectrum.process over 2^24 packed samples at hop nfft/2, existing code, the same process).  The scope reads 8 bytes per
sample where the panorama reads 6, and writes a line per avg segments.  Gaussian input made on the device, HIP events on
the launch stream, median of `steps` batches of one running series after a settle second.
Usage: python tools/scope_time.py [--steps 15] [--n 32768] [--slots 1024 64 1] [--sizes 256 1024 2048 4096] [--avg 4]
                                  [--only-kernel]"""
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
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--slots", type=int, nargs="+", default=[1024, 64, 1])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 2048, 4096])
    ap.add_argument("--avg", type=int, default=4)
    ap.add_argument("--only-kernel", action="store_true", help="k_scope only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    pano = {}
    if not a.only_kernel:
        ns = 1 << 24
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        for nfft in (s for s in a.sizes if s >= 1024):
            sp = pkg.Spectrum(nfft, nfft // 2, None)
            sp.process(d)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t = timed(lambda: sp.process(d), a.steps)
            pano[nfft] = 1e6 * t / (ns // (nfft // 2))
            sp.close()
        del d
        torch.cuda.empty_cache()
    print(f"avg {a.avg}, hop nfft/2")
    print("    K    nfft   samples/row   segments   scope ms   GB/s(8 B)   ns/segment   copy ms   scope/copy   panorama ns/segment   ratio")
    for K in a.slots:
        n = a.n * (32 if K == 1 else 1)
        gen = torch.Generator(device=dev).manual_seed(7)
        z = torch.view_as_complex(torch.randn((K, n, 2), generator=gen, dtype=torch.float32, device=dev))
        zc = torch.empty_like(z)
        t_copy = float("nan") if a.only_kernel else pkg.measure_copy(zc.data_ptr(), z.data_ptr(), 8 * K * n, a.steps, st)
        for nfft in a.sizes:
            sc = pkg.Scope(K, range(K), nfft, nfft // 2, a.avg)
            out = torch.empty((K, sc.next_lines(n) + 1, nfft), dtype=torch.float32, device=dev)
            nseg = K * (n // (nfft // 2))          # per batch of the running series
            sc.process(z, out=out)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t = timed(lambda: sc.process(z, out=out), a.steps)
            per = 1e6 * t / nseg
            p = pano.get(nfft, float("nan"))
            print(f"{K:5d}   {nfft:5d}   {n:11d}   {nseg:8d}   {t:8.4f}   {8e-6 * K * n / t:9.0f}   {per:10.1f}   {t_copy:7.4f}   "
                  f"{t / t_copy:10.2f}   {p:19.1f}   {per / p:5.2f}", flush=True)
            sc.close()
            del out
        del z, zc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
