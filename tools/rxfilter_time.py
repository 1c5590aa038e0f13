"""Timing of the receiver filter (pddc_rxfilter_process, k_rxfilter) on the GPU box: K = 256 / 1024 receivers at the
tuner's output sizes for 2^24 and 2^28 samples (M = 1024, hop 512, T = 64, R = 16: 2031 and 32 751 values per receiver),
banks of 8 filters of T = 64 and 256 taps, receiver j on filter j mod 8.  Beside every point, on the same tensors:
  (a) the torch expression: grouped conv1d on the re / im planes, the weights gathered per receiver outside the timed
      region (the input padded with T - 1 zeros per row, which is what a first batch sees);
  (b) a plain device copy (pddc_measure_copy) of the same bytes, input plus output;
  (c) Tuner.process and Demod.process (AM) of the same batch.
HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/rxfilter_time.py [--steps 15] [--values 2031 32751] [--rx 256 1024] [--taps 64 256] [--only-kernel]"""
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

NCHAN, HOP, T_TUNER, DECIM = 1024, 512, 64, 16


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
    ap.add_argument("--values", type=int, nargs="+", default=[2031, 32751], help="values per receiver and batch")
    ap.add_argument("--rx", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--taps", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only-kernel", action="store_true", help="k_rxfilter only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    B = 8
    print("   K    values    T   k_rxfilter ms   G fmaf pairs/s   MB moved   torch conv1d ms   copy ms   tuner ms   demod ms")
    for K in a.rx:
        for n in a.values:
            z = torch.view_as_complex(torch.rand((K, n, 2), dtype=torch.float32, device=dev) * 2.0 - 1.0)
            out = torch.empty((K, n), dtype=torch.complex64, device=dev)
            t_tuner = t_demod = float("nan")
            if not a.only_kernel:
                # (c) the neighbours: the tuner on the rows that give n outputs, the demodulator on z
                nrows = (n - 1) * DECIM + T_TUNER
                words = [((300 + (j % 400)) << 22) + 12345 * j for j in range(K)]
                grid = type("G", (), dict(nchan=NCHAN, hop=HOP, device=0, first=0, count=NCHAN))()
                tu = pkg.Tuner(grid, words, pkg.tuner_lowpass(T_TUNER, DECIM), DECIM)
                rows = torch.view_as_complex(torch.rand((nrows, NCHAN, 2), dtype=torch.float32, device=dev) - 0.5)
                zt = torch.empty((K, n + DECIM), dtype=torch.complex64, device=dev)

                def tuner():
                    tu.reset()
                    tu.process(rows, out=zt)

                tuner()
                torch.cuda.synchronize()
                t_tuner = timed(tuner, a.steps)
                tu.close()
                del rows, zt
                de = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)] * K)
                au = torch.empty((K, n), dtype=torch.float32, device=dev)
                de.process(z, out=au)
                torch.cuda.synchronize()
                t_demod = timed(lambda: de.process(z, out=au), a.steps)
                de.close()
                del au
                torch.cuda.empty_cache()
            for T in a.taps:
                bank = pkg.rxfilter_bank(1.0, [0.03 + 0.05 * f for f in range(B)], T)
                sel = [j % B for j in range(K)]
                rf = pkg.RxFilter(bank, sel)

                def kernel():
                    rf.process(z, out=out)

                kernel()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t = timed(kernel, a.steps)
                rf.close()
                nbytes = 2 * K * n * 8
                t_conv = t_copy = float("nan")
                if not a.only_kernel:
                    # (a) conv1d is a correlation: the taps reversed, one group per receiver and plane
                    w = torch.from_numpy(np.ascontiguousarray(bank[sel][:, ::-1])).to(dev)
                    w2 = torch.cat([w, w], dim=0).unsqueeze(1)                           # [2 K, 1, T]
                    planes = torch.cat([z.real, z.imag], dim=0)                          # [2 K, n]
                    x = torch.nn.functional.pad(planes, (T - 1, 0)).unsqueeze(0).contiguous()   # [1, 2 K, n + T - 1]

                    def conv():
                        return torch.nn.functional.conv1d(x, w2, groups=2 * K)

                    try:
                        y = conv()
                        torch.cuda.synchronize()
                        ref = torch.complex(y[0, :K], y[0, K:])
                        # (out is a later batch of the stream: its first T - 1 values saw the batch before, not zeros)
                        e = float((ref[:, T - 1:] - out[:, T - 1:]).abs().max())
                        assert e < 1e-4, e                                                # the same filter, to rounding
                        t_conv = timed(conv, a.steps)
                        del y, ref
                    except RuntimeError as ex:                                            # torch has no kernel for the shape
                        print(f"# conv1d K {K} n {n} T {T}: {str(ex).splitlines()[0]}", flush=True)
                    del x, w, w2, planes
                    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)         # a copy reads and writes
                    dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
                    t_copy = pkg.measure_copy(dst.data_ptr(), src.data_ptr(), nbytes // 2, a.steps, st)
                    del src, dst
                print(f"{K:4d}  {n:8d}  {T:3d}   {t:13.4f}   {K * n * T / 1e6 / t:14.1f}   {nbytes / 1e6:8.1f}   {t_conv:15.4f}"
                      f"   {t_copy:7.4f}   {t_tuner:8.4f}   {t_demod:8.4f}", flush=True)
                torch.cuda.empty_cache()
            del z, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
