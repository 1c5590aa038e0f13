"""Timing of the SITOR decoder (pddc_sitor_process, k_sitor) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, windows of W = 64 and 256 taps; every receiver is a two-tone signal that keys random mode-B text (every
character twice, five slots apart, behind 16 phasing pairs) at 16 samples per bit, noise 20 dB below the tone, so that the
clock, the framing and the records are busy.
Beside every point, in the same run, on the same tensor:
  (a) the FSK decoder (Fsk.process, k_fsk) with as many taps: the same two complex filter passes, 8 fmaf per tap and
      output, behind them a walk with one event per bit where this one has about 1.5 (a strobe per bit, a transition
      on every other one): the yardstick;
  (b) the receiver filter (RxFilter.process, k_rxfilter) with as many taps: 2 fmaf per tap and output;
  (c) a plain device copy (pddc_measure_copy) of the input bytes;
  (d) the run with `soft` asked for.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/sitor_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--only-kernel]"""
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

SPS = 16
TONE = 1.5 / SPS                                                      # +-1.5 bauds: the boxcars of a bit are blind to the other tone
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ 0123456789"


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
    """[K, n] complex64 on the device: per receiver the bits of random text in mode B behind 16 phasing pairs (repeated to
    fill the batch), a continuous-phase two-tone signal at +-TONE cycles per sample, a lead of up to a bit, noise 20 dB
    below the tone"""
    rng = np.random.default_rng(seed)
    nbit = n // SPS + 3
    bits = np.empty((K, nbit), np.uint8)
    for j in range(K):
        row = []
        while len(row) < nbit:
            text = "".join(LETTERS[int(i)] for i in rng.integers(0, len(LETTERS), 40))
            row += list(pkg.sitor_encode(text, 16)[1])
        bits[j] = row[:nbit]
    g = torch.Generator(device=dev).manual_seed(seed)
    b = torch.from_numpy(bits).to(dev)
    freq = torch.where(b > 0, TONE, -TONE).to(torch.float32).repeat_interleave(SPS, dim=1)
    shift = int(rng.integers(0, SPS))
    freq = freq[:, shift:shift + n].contiguous()
    ph = 2.0 * math.pi * (torch.rand((K, 1), generator=g, device=dev, dtype=torch.float32) + torch.cumsum(freq.double(), 1).float())
    sigma = 10.0 ** (-20.0 / 20.0) / math.sqrt(2.0)
    noise = torch.randn((K, n, 2), generator=g, device=dev, dtype=torch.float32) * sigma
    return (torch.polar(torch.ones_like(ph), ph) + torch.view_as_complex(noise)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--values", type=int, nargs="+", default=[32768, 977], help="samples per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--window", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_sitor only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    W   k_sitor ms   with soft ms   ps/(tap out)   chars/batch   syms/batch   valid %   locked    k_fsk ms   sitor/fsk"
          "   k_rxfilter ms   sitor/rxf   copy ms")
    for K in a.rx:
        for n in a.values:
            z = keyed(K, n, 7 * n + K)
            for W in a.window:
                # the boxcar pair of a bit in front, small taps behind it: every tap works
                hm, hs, inc, step, lock, unlock = pkg.sitor_modem(W, SPS, shift=2.0 * TONE * SPS)
                hm[SPS:] = 1e-4
                hs[SPS:] = 1e-4
                f = pkg.Sitor([(hm, hs, inc, step, lock, unlock)], [(0, pkg.PDDC_SITOR_ON)] * K, W)
                chars = torch.empty((K, f.max_chars(n), 4), dtype=torch.int32, device=dev)
                counts = torch.empty((K,), dtype=torch.int32, device=dev)
                soft = torch.empty((K, f.max_syms(n)), dtype=torch.float32, device=dev)
                nsoft = torch.empty((K,), dtype=torch.int32, device=dev)

                def kernel():
                    f.process(z, chars=chars, counts=counts)

                def kernel_s():
                    f.process(z, chars=chars, counts=counts, soft=soft, nsoft=nsoft)

                kernel_s()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                t_s = t if a.only_kernel else timed(kernel_s, a.steps)
                nchars, nsyms = int(counts.sum()), int(nsoft.sum())
                rec = chars.cpu().numpy().view(pkg.sitor_char_dtype())[..., 0]
                k = counts.cpu().numpy()
                valid = sum(int((rec[j, :k[j]]["flags"] & pkg.PDDC_SITOR_VALID).sum()) for j in range(K))
                locked = int(f.read()["locked"].sum())
                f.close()
                del chars, counts, soft, nsoft
                t_fsk = t_rx = t_copy = float("nan")
                if not a.only_kernel:
                    fm = pkg.fsk_modem(float(SPS), 1.0, TONE * SPS, -TONE * SPS, W)
                    fm[0][SPS:] = 1e-4
                    fm[1][SPS:] = 1e-4
                    fk = pkg.Fsk([fm], [(0, pkg.PDDC_FSK_ON)] * K, W)
                    fc = torch.empty((K, fk.max_chars(n), 4), dtype=torch.int32, device=dev)
                    fn = torch.empty((K,), dtype=torch.int32, device=dev)
                    fk.process(z, chars=fc, counts=fn)
                    torch.cuda.synchronize()
                    t_fsk = timed(lambda: fk.process(z, chars=fc, counts=fn), a.steps)
                    fk.close()
                    del fc, fn
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
                print(f"{K:4d}  {n:8d}  {W:3d}   {t:10.4f}   {t_s:12.4f}   {t * per:12.3f}   {nchars:11d}   {nsyms:10d}   {100.0 * valid / max(nchars, 1):7.1f}"
                      f"   {locked:6d}   {t_fsk:9.4f}   {t / t_fsk:9.3f}   {t_rx:13.4f}   {t / t_rx:9.2f}   {t_copy:7.4f}", flush=True)
                torch.cuda.empty_cache()
            del z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
