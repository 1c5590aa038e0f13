"""Timing of the Morse decoder (pddc_morse_process, k_morse) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, windows of W = 64 and 256 taps; every receiver is a carrier keyed at random, a dot of 16 samples down or up
with equal chance (noise 20 dB below the carrier), so that the meter, the key and the element timing are busy.  Beside
every point, in the same run, on the same tensor:
  (a) the FSK decoder (Fsk.process, k_fsk) with as many taps: its two complex matched filters do 8 fmaf per tap and
      output where the real envelope filter does 2;
  (b) the receiver filter (RxFilter.process, k_rxfilter) with as many taps: 2 fmaf per tap and output, like the envelope;
  (c) a plain device copy (pddc_measure_copy) of the input bytes.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/morse_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--only-kernel]"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("libperseus-sdr_amd")
dev = torch.device("cuda:0")

SPD = 16


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


def keyed(K, n, seed):
    """[K, n] complex64 on the device: a carrier of unit amplitude and a random phase per receiver, down or up for every
    dot of 16 samples with equal chance, noise 20 dB below"""
    g = torch.Generator(device=dev).manual_seed(seed)
    dots = torch.randint(0, 2, (K, n // SPD + 1), generator=g, device=dev, dtype=torch.int32).to(torch.float32)
    line = dots.repeat_interleave(SPD, dim=1)[:, :n]
    ph = 2.0 * math.pi * torch.rand((K, 1), generator=g, device=dev, dtype=torch.float32)
    sigma = 10.0 ** (-20.0 / 20.0) / math.sqrt(2.0)
    noise = torch.randn((K, n, 2), generator=g, device=dev, dtype=torch.float32) * sigma
    return (torch.polar(line, ph.expand(K, n).contiguous()) + torch.view_as_complex(noise)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--values", type=int, nargs="+", default=[32768, 977], help="samples per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--window", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_morse only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    W   k_morse ms   with p ms   ps/(tap out)   chars/batch    k_fsk ms   morse/fsk   k_rxfilter ms   morse/rxf   copy ms")
    for K in a.rx:
        for n in a.values:
            z = keyed(K, n, 7 * n + K)
            for W in a.window:
                # the Hann window of half a dot in front, small taps behind it: every tap works
                h, two0, two_min, two_max, shift = pkg.morse_keyer(SPD * 20.0 / 1.2, 20.0, W)
                h[SPD // 2:] = 1e-4
                f = pkg.Morse([(h, two0, two_min, two_max, shift)], [(0, pkg.PDDC_MORSE_ON)] * K, W)
                chars = torch.empty((K, f.max_chars(n), 4), dtype=torch.int32, device=dev)
                counts = torch.empty((K,), dtype=torch.int32, device=dev)
                p = torch.empty((K, n), dtype=torch.float32, device=dev)

                def kernel():
                    f.process(z, chars=chars, counts=counts)

                def kernel_p():
                    f.process(z, chars=chars, counts=counts, p=p)

                kernel_p()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                t_p = t if a.only_kernel else timed(kernel_p, a.steps)
                nchars = int(counts.sum())
                f.close()
                del chars, counts, p
                t_fsk = t_rx = t_copy = float("nan")
                if not a.only_kernel:
                    k = pkg.Fsk([pkg.fsk_modem(16.0, 1.0, 1.5, -1.5, W)], [(0, pkg.PDDC_FSK_ON)] * K, W)
                    fc = torch.empty((K, k.max_chars(n), 4), dtype=torch.int32, device=dev)
                    fk = torch.empty((K,), dtype=torch.int32, device=dev)
                    k.process(z, chars=fc, counts=fk)
                    torch.cuda.synchronize()
                    t_fsk = timed(lambda: k.process(z, chars=fc, counts=fk), a.steps)
                    k.close()
                    del fc, fk
                    rf = pkg.RxFilter(pkg.rxfilter_bank(1.0, [0.05], W), [0] * K)
                    out = torch.empty((K, n), dtype=torch.complex64, device=dev)
                    rf.process(z, out=out)
                    torch.cuda.synchronize()
                    t_rx = timed(lambda: rf.process(z, out=out), a.steps)
                    rf.close()
                    del out
                    src = torch.empty(K * n * 8, dtype=torch.uint8, device=dev)
                    dst = torch.empty(K * n * 8, dtype=torch.uint8, device=dev)
                    t_copy = pkg.measure_copy(dst.data_ptr(), src.data_ptr(), K * n * 8, a.steps, st)
                    del src, dst
                per = 1e9 / (K * n * W)                                  # ms -> ps per tap and output
                print(f"{K:4d}  {n:8d}  {W:3d}   {t:10.4f}   {t_p:9.4f}   {t * per:12.3f}   {nchars:11d}   {t_fsk:9.4f}   {t / t_fsk:9.3f}"
                      f"   {t_rx:13.4f}   {t / t_rx:9.2f}   {t_copy:7.4f}", flush=True)
                torch.cuda.empty_cache()
            del z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
