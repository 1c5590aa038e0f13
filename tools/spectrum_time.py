"""Timing of the panorama (pddc_spectrum_process, k_spectrum) on the GPU box against the path a host had before it:
pddc_unpack24_f32 into a float buffer, window multiply, torch.fft.fft over (nseg, N), abs^2 and a sum over segments.
Same on-device LCG input, same process, hop = N, HIP events on the launch stream, median of `steps` after a settle second
(freshly allocated buffers are slow at first).  Also: a bank round of four 48-tap members and the panorama on the same
d_packed back to back at the largest size.  Usage: python tools/spectrum_time.py [--steps 15] [--logs 24 28] [--no-host]"""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096, 8192])
    ap.add_argument("--no-host", action="store_true", help="k_spectrum only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("samples     N   k_spectrum ms   GB/s(6 B)   host path ms   ratio")
    for lg in a.logs:
        ns = 1 << lg
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        for nfft in a.sizes:
            w = torch.from_numpy(pkg.hann_window(nfft)).to(dev)
            sp = pkg.Spectrum(nfft, nfft, None)

            def host_path():
                x = torch.view_as_complex(pkg.unpack24_f32(d)).view(-1, nfft)
                X = torch.fft.fft(x * w, dim=1)
                return (X.real * X.real + X.imag * X.imag).sum(dim=0)

            sp.process(d)
            if not a.no_host:
                host_path()
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_new = timed(lambda: sp.process(d), a.steps)
            t_host = float("nan") if a.no_host else timed(host_path, a.steps)
            print(f"2^{lg:<2}   {nfft:5d}   {t_new:13.4f}   {6e-6 * ns / t_new:9.0f}   {t_host:12.4f}   {t_host / t_new:5.2f}",
                  flush=True)
            sp.close()
            torch.cuda.empty_cache()
        if lg == max(a.logs) and not a.no_host:
            t48 = np.hamming(48).astype(np.float32)
            t48 /= t48.sum()
            pipes = [pkg.Pipeline([(8, t48)], mix=True) for _ in range(4)]
            for p, f in zip(pipes, (381178347, 0x7FFFF000, 123456789, 3000000000)):
                p.set_freg(f)
            bank = pkg.Bank(pipes)
            outs = [torch.empty((ns // 8 + 16, 2), dtype=torch.float32, device=dev) for _ in pipes]
            sp = pkg.Spectrum(4096, 4096, None)
            ptrs, caps = [o.data_ptr() for o in outs], [o.shape[0] for o in outs]

            def both():
                bank.process_ptr(d.data_ptr(), ns, ptrs, caps, st)
                sp.process(d)

            both()
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_bank = timed(lambda: bank.process_ptr(d.data_ptr(), ns, ptrs, caps, st), a.steps)
            t_both = timed(both, a.steps)
            print(f"2^{lg}: bank round of 4 alone {t_bank:.4f} ms; bank round + panorama (N 4096) back to back {t_both:.4f} ms")
            bank.close()
            sp.close()
            for p in pipes:
                p.close()
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
