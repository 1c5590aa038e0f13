"""Timing of the FSK decoder (pddc_fsk_process, k_fsk) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, windows of W = 64 and 256 taps; every receiver keys random 5-bit start-stop characters at 16 samples per bit
(tones at +-3/32 cycles per sample, noise 16 dB below the tone), so that the start-stop receivers are busy.  Beside
every point, on the same tensor:
  (a) the receiver filter (RxFilter.process) with as many taps: its time per tap and output is the yardstick -- the two
      complex matched filters do 8 fmaf per tap and output where it does 2;
  (b) a plain device copy (pddc_measure_copy) of the input bytes.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/fsk_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--only-kernel]"""
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

SPS, MARK, SPACE = 16, 3.0 / 32.0, -3.0 / 32.0


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
    """[K, n] complex64 on the device: random 5-bit characters (a start element, five data elements, a stop element of
    1.5 bits: 120 samples), continuous phase, unit amplitude, noise 16 dB below"""
    g = torch.Generator(device=dev).manual_seed(seed)
    nchar = n // (15 * SPS // 2) + 2
    data = torch.randint(0, 2, (K, nchar, 5), generator=g, device=dev, dtype=torch.int32).bool()      # True: mark
    frame = torch.cat([torch.zeros((K, nchar, 1), dtype=torch.bool, device=dev), data], dim=2)         # start: space
    line = torch.cat([frame.repeat_interleave(SPS, dim=2), torch.ones((K, nchar, 3 * SPS // 2), dtype=torch.bool, device=dev)],
                     dim=2).reshape(K, -1)[:, :n]
    f = torch.where(line, torch.tensor(MARK, dtype=torch.float64, device=dev), torch.tensor(SPACE, dtype=torch.float64, device=dev))
    ph = 2.0 * math.pi * torch.cumsum(f, dim=1)
    sigma = 10.0 ** (-16.0 / 20.0) / math.sqrt(2.0)
    noise = torch.randn((K, n, 2), generator=g, device=dev, dtype=torch.float32) * sigma
    return (torch.polar(torch.ones_like(ph), ph).to(torch.complex64) + torch.view_as_complex(noise)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--values", type=int, nargs="+", default=[32768, 977], help="samples per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--window", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_fsk only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    W    k_fsk ms   with d ms   ps/(tap out)   chars/batch   k_rxfilter ms   ps/(tap out)   ratio   copy ms")
    for K in a.rx:
        for n in a.values:
            z = keyed(K, n, 7 * n + K)
            for W in a.window:
                f = pkg.Fsk([pkg.fsk_modem(float(SPS), 1.0, MARK * SPS, SPACE * SPS, W)], [(0, pkg.PDDC_FSK_ON)] * K, W)
                chars = torch.empty((K, f.max_chars(n), 4), dtype=torch.int32, device=dev)
                counts = torch.empty((K,), dtype=torch.int32, device=dev)
                d = torch.empty((K, n), dtype=torch.float32, device=dev)

                def kernel():
                    f.process(z, chars=chars, counts=counts)

                def kernel_d():
                    f.process(z, chars=chars, counts=counts, d=d)

                kernel_d()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                t_d = t if a.only_kernel else timed(kernel_d, a.steps)
                nchars = int(counts.sum())
                f.close()
                t_rx = t_copy = float("nan")
                if not a.only_kernel:
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
                print(f"{K:4d}  {n:8d}  {W:3d}   {t:9.4f}   {t_d:9.4f}   {t * per:12.3f}   {nchars:11d}   {t_rx:13.4f}"
                      f"   {t_rx * per:12.3f}   {t / t_rx:5.2f}   {t_copy:7.4f}", flush=True)
                del chars, counts, d
                torch.cuda.empty_cache()
            del z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
