"""Timing of the audio resampler (pddc_audio_process, k_audio) on the GPU box: 1024 receivers' real series, seeded
random, at 9765.625 Hz -> 48 kHz (3072/625, P = 128, T = 32) and 39062.5 Hz -> 8 kHz (128/625, P = 128, T = 64), each to
float32, to int16, and to both.  Beside every point a plain device copy (pddc_measure_copy) of the same bytes, input plus
output(s).  HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/audio_time.py [--steps 15] [--inputs 2048 32768] [--rx 1024] [--only-kernel]"""
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

POINTS = (("9765.625 -> 48000", 3072, 625, 128, 32), ("39062.5 -> 8000", 128, 625, 128, 64))


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
    ap.add_argument("--inputs", type=int, nargs="+", default=[2048, 32768], help="inputs per receiver and batch")
    ap.add_argument("--rx", type=int, default=1024)
    ap.add_argument("--only-kernel", action="store_true", help="k_audio only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    K = a.rx
    st = torch.cuda.current_stream().cuda_stream
    print("ratio                inputs   outputs     K   out     k_audio ms   MB moved   GB/s   copy of the same bytes ms")
    for name, L, M, P, T in POINTS:
        g = pkg.audio_prototype(P, T, 0.45 * min(1.0, L / M))
        for n in a.inputs:
            x = torch.rand((K, n), dtype=torch.float32, device=dev) * 2.0 - 1.0
            au = pkg.Audio(K, L, M, P, T, g)
            c = au.next_outputs(n)
            f = torch.empty((K, c), dtype=torch.float32, device=dev)
            p = torch.empty((K, c), dtype=torch.int16, device=dev)
            for what, kw, obytes in (("f32", dict(out_f32=f, f32=True), 4), ("i16", dict(out_i16=p, f32=False), 2),
                                     ("both", dict(out_f32=f, out_i16=p), 6)):
                nbytes = K * (4 * n + obytes * c)

                def kernel():
                    au.process(x, **kw)

                kernel()
                torch.cuda.synchronize()
                time.sleep(1.0)
                # later batches start at other remainders r; their work is the same to within one output per tile
                t = timed(kernel, a.steps)
                t_copy = float("nan")
                if not a.only_kernel:
                    half = (nbytes // 2 + 15) // 16 * 16                  # a copy reads and writes: half the bytes, the same traffic
                    src = torch.empty(half, dtype=torch.uint8, device=dev)
                    dst = torch.empty(half, dtype=torch.uint8, device=dev)
                    t_copy = pkg.measure_copy(dst.data_ptr(), src.data_ptr(), half, a.steps, st)
                    del src, dst
                print(f"{name:18s} {n:8d}  {c:8d}  {K:4d}   {what:4s}   {t:10.4f}   {nbytes / 1e6:8.1f}   {nbytes / 1e6 / t:5.0f}"
                      f"   {t_copy:10.4f}", flush=True)
            au.close()
            del x, f, p
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
