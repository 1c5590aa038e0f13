"""Timing of the spectral noise reduction (pddc_denoise_process, k_denoise) on the GPU box: K receivers x n samples in one
batch of a running series, at (nfft, hop) = (256, 128) and (1024, 256) with n = 32768, and a 0.1 s batch of 977 samples.
Per point: (a) Denoise.process, with its time per frame of the walk (all receivers side by side); (b) a device copy of the same in + out bytes
(pddc_measure_copy over 8 bytes per sample: what reading x and writing out once costs at least); (c) Scope.process on
the same rows (as complex64 with a zero imaginary part) with the same nfft and hop and avg 1 -- the forward half of the
same frames, existing code, the same process.  Gaussian input made on the device, HIP events on the launch stream, median
of `steps` batches after a settle second.
Usage: python tools/denoise_time.py [--steps 15] [--rx 1024] [--only-kernel]"""
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

POINTS = [(256, 128, 32768), (1024, 256, 32768), (256, 128, 977), (1024, 256, 977)]


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
    ap.add_argument("--rx", type=int, default=1024)
    ap.add_argument("--only-kernel", action="store_true", help="k_denoise only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    K = a.rx
    st = torch.cuda.current_stream().cuda_stream
    print("    K    nfft    hop   samples/row   frames   denoise ms   us/frame   copy ms   denoise/copy   scope ms   denoise/scope")
    for nfft, hop, n in POINTS:
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn((K, n), generator=gen, dtype=torch.float32, device=dev)
        out = torch.empty_like(x)
        dn = pkg.Denoise(K, nfft, hop)
        dn.process(x, out=out)
        torch.cuda.synchronize()
        time.sleep(1.0)
        t = timed(lambda: dn.process(x, out=out), a.steps)
        dn.close()
        t_copy = t_scope = float("nan")
        if not a.only_kernel:
            t_copy = pkg.measure_copy(out.data_ptr(), x.data_ptr(), 4 * K * n, a.steps, st)
            z = torch.complex(x, torch.zeros_like(x))
            sc = pkg.Scope(K, range(K), nfft, hop, 1)
            lines = torch.empty((K, n // hop + 1, nfft), dtype=torch.float32, device=dev)     # a batch of the running series completes at most that many
            sc.process(z, out=lines)
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_scope = timed(lambda: sc.process(z, out=lines), a.steps)
            sc.close()
            del z, lines
        frames = n // hop
        print(f"{K:5d}   {nfft:5d}   {hop:4d}   {n:11d}   {frames:6d}   {t:10.4f}   {1e3 * t / max(frames, 1):8.3f}   {t_copy:7.4f}   "
              f"{t / t_copy:12.2f}   {t_scope:8.4f}   {t / t_scope:13.2f}", flush=True)
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
