"""Timing of the PSK decoder (pddc_psk_process, k_psk) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, windows of W = 64 and 256 taps; every receiver is a carrier that keys random Varicode at 16 samples per symbol
with raised-cosine reversals (noise 20 dB below the carrier), so that the clock, the decision and the framing are busy.
Beside every point, in the same run, on the same tensor:
  (a) the Morse decoder (Morse.process, k_morse) with as many taps: its real envelope filter does the same 2 fmaf per tap
      and output as the matched filter here, so it is the yardstick;
  (b) the FSK decoder (Fsk.process, k_fsk) with as many taps: 8 fmaf per tap and output;
  (c) the receiver filter (RxFilter.process, k_rxfilter) with as many taps: 2 fmaf per tap and output;
  (d) a plain device copy (pddc_measure_copy) of the input bytes.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/psk_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--only-kernel]"""
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
    """[K, n] complex64 on the device: per receiver the bits of random printable text in Varicode, keyed as PSK31 keys
    them (the amplitude turns its sign with every 0 through a cosine of one symbol, 16 samples), a random carrier phase
    and starting phase of the symbol clock, noise 20 dB below"""
    rng = np.random.default_rng(seed)
    nsym = n // SPS + 3
    amp = np.empty((K, nsym), np.float32)
    for j in range(K):
        bits = []
        while len(bits) < nsym:
            bits += pkg.psk_varicode_bits(chr(int(rng.integers(32, 127))))
        amp[j] = np.cumprod(np.where(np.array(bits[:nsym]) > 0, 1.0, -1.0))
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.from_numpy(amp).to(dev)
    t = torch.arange(SPS, device=dev, dtype=torch.float32) / SPS
    w = 0.5 * (1.0 + torch.cos(math.pi * t))                          # the old symbol's share across one symbol
    base = (a[:, :-1, None] * w + a[:, 1:, None] * (1.0 - w)).reshape(K, -1)
    shift = torch.randint(0, SPS, (1,), generator=g, device=dev).item()
    base = base[:, shift:shift + n].contiguous()
    ph = 2.0 * math.pi * torch.rand((K, 1), generator=g, device=dev, dtype=torch.float32)
    sigma = 10.0 ** (-20.0 / 20.0) / math.sqrt(2.0)
    noise = torch.randn((K, n, 2), generator=g, device=dev, dtype=torch.float32) * sigma
    return (torch.polar(base.abs(), ph.expand(K, n) + math.pi * (base < 0)) + torch.view_as_complex(noise)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--values", type=int, nargs="+", default=[32768, 977], help="samples per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--window", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_psk only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    W   k_psk ms   with sym ms   ps/(tap out)   chars/batch   syms/batch   k_morse ms   psk/morse    k_fsk ms   psk/fsk"
          "   k_rxfilter ms   psk/rxf   copy ms")
    for K in a.rx:
        for n in a.values:
            z = keyed(K, n, 7 * n + K)
            for W in a.window:
                # the raised cosine of two symbols in front, small taps behind it: every tap works
                h, inc, q, step = pkg.psk_modem(W, SPS)
                h[2 * SPS:] = 1e-4
                f = pkg.Psk([(h, inc, q, step)], [(0, pkg.PDDC_PSK_ON)] * K, W)
                chars = torch.empty((K, f.max_chars(n), 4), dtype=torch.int32, device=dev)
                counts = torch.empty((K,), dtype=torch.int32, device=dev)
                sym = torch.empty((K, f.max_syms(n), 2), dtype=torch.float32, device=dev)
                nsym = torch.empty((K,), dtype=torch.int32, device=dev)

                def kernel():
                    f.process(z, chars=chars, counts=counts)

                def kernel_s():
                    f.process(z, chars=chars, counts=counts, sym=sym, nsym=nsym)

                kernel_s()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                t_s = t if a.only_kernel else timed(kernel_s, a.steps)
                nchars, nsyms = int(counts.sum()), int(nsym.sum())
                f.close()
                del chars, counts, sym, nsym
                t_mo = t_fsk = t_rx = t_copy = float("nan")
                if not a.only_kernel:
                    mh, two0, two_min, two_max, shift = pkg.morse_keyer(SPS * 20.0 / 1.2, 20.0, W)
                    mh[SPS // 2:] = 1e-4
                    mo = pkg.Morse([(mh, two0, two_min, two_max, shift)], [(0, pkg.PDDC_MORSE_ON)] * K, W)
                    mc = torch.empty((K, mo.max_chars(n), 4), dtype=torch.int32, device=dev)
                    mk = torch.empty((K,), dtype=torch.int32, device=dev)
                    mo.process(z, chars=mc, counts=mk)
                    torch.cuda.synchronize()
                    t_mo = timed(lambda: mo.process(z, chars=mc, counts=mk), a.steps)
                    mo.close()
                    del mc, mk
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
                print(f"{K:4d}  {n:8d}  {W:3d}   {t:8.4f}   {t_s:11.4f}   {t * per:12.3f}   {nchars:11d}   {nsyms:10d}   {t_mo:10.4f}   {t / t_mo:9.3f}"
                      f"   {t_fsk:9.4f}   {t / t_fsk:7.3f}   {t_rx:13.4f}   {t / t_rx:7.2f}   {t_copy:7.4f}", flush=True)
                torch.cuda.empty_cache()
            del z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
