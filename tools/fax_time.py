"""Timing of the radiofax decoder (pddc_fax_process, k_fax) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, windows of W = 64 and 256 taps; every receiver is a frequency-modulated picture (start tone, phasing, grey wedges
and bars, stop tone, over and over) at 120 lines a minute, IOC 576 and 9765.625 Hz, 2.7 samples per pixel, noise 20 dB
below the carrier, so that the pixel path, the masks and the line records are busy.
Beside every point, in the same run, on the same tensor:
  (a) the run with `disc` asked for: 4 more bytes written per sample;
  (b) the PSK decoder (Psk.process, k_psk) with as many taps: the same real filter pass, 2 fmaf per tap and output, and
      behind it one lane that walks a strobe every 16 samples: the yardstick.  The ratio says what the discriminator, the
      arctangent and the pixel path cost against that walk;
  (c) the receiver filter (RxFilter.process, k_rxfilter) with as many taps: 2 fmaf per tap and output, samples out;
  (d) a plain device copy (pddc_measure_copy) of the input bytes.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/fax_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--only-kernel]"""
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


def pictures(K, n, modem, seed):
    """[K, n] complex64 on the device: one transmission (fax_encode: 4 start-tone lines, 3 phasing lines, 6 lines of a grey
    wedge and bars, 4 stop-tone lines) repeated to fill the batch, every receiver from another sample of it, noise 20 dB
    below the carrier"""
    width = int(modem[2])
    col = np.arange(width)
    img = np.stack([(col * 255 // (width - 1)).astype(np.uint8), ((col * 8 // width) * 255 // 7).astype(np.uint8)] * 3)
    one = pkg.fax_encode(img, modem, RATE, start_lines=4, phasing_lines=3, stop_lines=4, trail_lines=1)
    f = np.angle(one[1:] * np.conj(one[:-1])).astype(np.float32)      # the frequency, so that the repeats join in phase
    rng = np.random.default_rng(seed)
    reps = -(-(n + f.size) // f.size)
    freq = torch.from_numpy(np.tile(f, reps)).to(dev)
    starts = rng.integers(0, f.size, K)
    rows = torch.stack([freq[int(s):int(s) + n] for s in starts])
    ph = torch.cumsum(rows.double(), 1).float()
    g = torch.Generator(device=dev).manual_seed(seed)
    sigma = 10.0 ** (-20.0 / 20.0) / math.sqrt(2.0)
    noise = torch.randn((K, n, 2), generator=g, device=dev, dtype=torch.float32) * sigma
    return (torch.polar(torch.ones_like(ph), ph) + torch.view_as_complex(noise)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--values", type=int, nargs="+", default=[32768, 977], help="samples per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--window", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_fax only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    W    k_fax ms   with disc ms   ps/(tap out)   pixels/batch   lines/batch   start+stop lines    k_psk ms   fax/psk"
          "   k_rxfilter ms   fax/rxf   copy ms")
    for K in a.rx:
        for n in a.values:
            z = None
            for W in a.window:
                modem = pkg.fax_modem(RATE, W)
                if z is None:
                    z = pictures(K, n, modem, 7 * n + K)
                f = pkg.Fax([modem], [(0, pkg.PDDC_FAX_ON)] * K, W)
                pix = torch.empty((K, f.max_pixels(n)), dtype=torch.uint8, device=dev)
                npix = torch.empty((K,), dtype=torch.int32, device=dev)
                lines = torch.empty((K, f.max_lines(n), 4), dtype=torch.int32, device=dev)
                counts = torch.empty((K,), dtype=torch.int32, device=dev)
                disc = torch.empty((K, n), dtype=torch.float32, device=dev)

                def kernel():
                    f.process(z, pix=pix, npix=npix, lines=lines, counts=counts)

                def kernel_d():
                    f.process(z, pix=pix, npix=npix, lines=lines, counts=counts, disc=disc)

                kernel_d()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                t_d = t if a.only_kernel else timed(kernel_d, a.steps)
                npx, nln = int(npix.sum()), int(counts.sum())
                rec = lines.cpu().numpy().view(pkg.fax_line_dtype())[..., 0]
                k = counts.cpu().numpy()
                tones = sum(int((rec[j, :k[j]]["flags"] & (pkg.PDDC_FAX_START | pkg.PDDC_FAX_STOP) != 0).sum()) for j in range(K))
                f.close()
                del pix, npix, lines, counts, disc
                t_psk = t_rx = t_copy = float("nan")
                if not a.only_kernel:
                    pm = pkg.psk_modem(W, 16.0)
                    pm[0][32:] = 1e-4                                    # small taps behind the pulse: every tap works
                    pk = pkg.Psk([pm], [(0, pkg.PDDC_PSK_ON)] * K, W)
                    pc = torch.empty((K, pk.max_chars(n), 4), dtype=torch.int32, device=dev)
                    pn = torch.empty((K,), dtype=torch.int32, device=dev)
                    pk.process(z, chars=pc, counts=pn)
                    torch.cuda.synchronize()
                    t_psk = timed(lambda: pk.process(z, chars=pc, counts=pn), a.steps)
                    pk.close()
                    del pc, pn
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
                print(f"{K:4d}  {n:8d}  {W:3d}   {t:9.4f}   {t_d:12.4f}   {t * per:12.3f}   {npx:12d}   {nln:11d}   {tones:16d}   {t_psk:9.4f}   {t / t_psk:7.3f}"
                      f"   {t_rx:13.4f}   {t / t_rx:7.2f}   {t_copy:7.4f}", flush=True)
                torch.cuda.empty_cache()
            del z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
