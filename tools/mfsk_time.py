"""Timing of the MFSK decoder (pddc_mfsk_process, k_mfsk) on the GPU box: K = 1024 receivers, batches of 32 768 and 977
samples, M = 8 and 32 tones, windows of W = 64 and 256 taps; every receiver hears seeded random tones of its modem at 16
samples per symbol (continuous phase; the tones a baud apart, or 1 / M of the rate where M bauds do not fit), noise
20 dB below, so that the maximum, the clock and the records are busy.
Beside every point, in the same run, on the same tensor:
  (a) the FSK decoder (Fsk.process, k_fsk) with as many taps: one complex pair pass, 8 fmaf per tap and output -- k_mfsk
      runs ceil(M / 2) of them per tile: the expectation to test is ceil(M / 2) x k_fsk's filter part and one walk;
  (b) the PSK decoder (Psk.process, k_psk) with as many taps: 2 fmaf per tap and output and a strobe walk of the same
      kind, the nearest thing to this one's walk;
  (c) a plain device copy (pddc_measure_copy) of the input bytes;
  (d) the run with `best` asked for.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/mfsk_time.py [--steps 15] [--values 32768 977] [--rx 1024] [--window 64 256] [--tones 8 32] [--only-kernel]"""
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


def spacing(M):
    """cycles per sample between two tones: a baud, or 1 / M where M bauds are more than the rate holds"""
    return 1.0 / max(SPS, M)


def keyed(K, n, M, seed):
    """[K, n] complex64 on the device: per receiver random tones of M, centred, SPS samples each, continuous phase, a lead
    of up to a symbol, noise 20 dB below the tone"""
    g = torch.Generator(device=dev).manual_seed(seed)
    nsym = n // SPS + 3
    tones = torch.randint(0, M, (K, nsym), generator=g, device=dev)
    freq = ((tones.to(torch.float32) - (M - 1) / 2.0) * spacing(M)).repeat_interleave(SPS, dim=1)
    shift = seed % SPS
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
    ap.add_argument("--tones", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--only-kernel", action="store_true", help="k_mfsk only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("   K    values    M    W   k_mfsk ms   with best ms   ps/(tone tap out)   syms/batch   mean quality    k_fsk ms   mfsk/fsk   pairs"
          "   (mfsk - psk)/(pairs fsk)    k_psk ms   copy ms")
    for K in a.rx:
        for n in a.values:
            for M in a.tones:
                z = keyed(K, n, M, 7 * n + K + M)
                for W in a.window:
                    # the boxcar of a symbol in front, small taps behind it: every tap works
                    m = pkg.mfsk_modem(float(SPS), 1.0, -(M - 1) / 2.0 * spacing(M) * SPS, spacing(M) * SPS, M, W, step=(1 << 28) // 4)
                    m[0][:, SPS:] = 1e-4
                    f = pkg.Mfsk([m], [(0, pkg.PDDC_MFSK_ON)] * K, W)
                    syms = torch.empty((K, f.max_syms(n), 4), dtype=torch.int32, device=dev)
                    counts = torch.empty((K,), dtype=torch.int32, device=dev)
                    best = torch.empty((K, n), dtype=torch.float32, device=dev)

                    def kernel():
                        f.process(z, syms=syms, counts=counts)

                    def kernel_b():
                        f.process(z, syms=syms, counts=counts, best=best)

                    kernel_b()
                    torch.cuda.synchronize()
                    time.sleep(1.0)
                    t = timed(kernel, a.steps)
                    t_b = t if a.only_kernel else timed(kernel_b, a.steps)
                    nsyms = int(counts.sum())
                    rec = syms.cpu().numpy().view(pkg.mfsk_sym_dtype())[..., 0]
                    k = counts.cpu().numpy()
                    quality = float(np.mean([rec[j, :k[j]]["quality"].mean() for j in range(K) if k[j]]))
                    f.close()
                    del syms, counts, best
                    t_fsk = t_psk = t_copy = float("nan")
                    if not a.only_kernel:
                        fm = pkg.fsk_modem(float(SPS), 1.0, 0.5, -0.5, W)
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
                        pm = pkg.psk_modem(W, SPS)
                        pm[0][2 * SPS:] = 1e-4
                        pk = pkg.Psk([pm], [(0, pkg.PDDC_PSK_ON)] * K, W)
                        pc = torch.empty((K, pk.max_chars(n), 4), dtype=torch.int32, device=dev)
                        pn = torch.empty((K,), dtype=torch.int32, device=dev)
                        pk.process(z, chars=pc, counts=pn)
                        torch.cuda.synchronize()
                        t_psk = timed(lambda: pk.process(z, chars=pc, counts=pn), a.steps)
                        pk.close()
                        del pc, pn
                        src = torch.empty(K * n * 8, dtype=torch.uint8, device=dev)
                        dst = torch.empty(K * n * 8, dtype=torch.uint8, device=dev)
                        t_copy = pkg.measure_copy(dst.data_ptr(), src.data_ptr(), K * n * 8, a.steps, st)
                        del src, dst
                    pairs = (M + 1) // 2
                    per = 1e9 / (K * n * W * 2 * pairs)                  # ms -> ps per tone (the padded one counted), tap and output
                    print(f"{K:4d}  {n:8d}  {M:3d}  {W:3d}   {t:9.4f}   {t_b:12.4f}   {t * per:17.3f}   {nsyms:10d}   {quality:12.3f}   {t_fsk:9.4f}"
                          f"   {t / t_fsk:8.3f}   {pairs:5d}   {(t - t_psk) / (pairs * t_fsk):24.3f}   {t_psk:9.4f}   {t_copy:7.4f}", flush=True)
                    torch.cuda.empty_cache()
                del z
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
