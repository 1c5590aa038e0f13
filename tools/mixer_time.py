"""Timing of the mixer (pddc_mixer_process: k_mix and k_mix_bus) on the GPU box: K receivers' float32 audio summed into
Q buses, all receivers active or 1 in 16, the limiter off or on (Lb = 48, every block above the ceiling), float32 and
int16 outputs both.  Per point the milliseconds of Mixer.process and the GB/s of input read (4 bytes per active
receiver and sample), beside pddc_measure_copy of the same byte count on the same box: a device-to-device copy reads
and writes that many bytes.  Unit-normal input on the device, HIP events on the launch stream, median of `steps` after
a settle second.
Usage: python tools/mixer_time.py [--steps 15] [--n 4800 32768] [--rx 1024] [--bus 2 8] [--block 48]"""
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
    ap.add_argument("--n", type=int, nargs="+", default=[4800, 32768])
    ap.add_argument("--rx", type=int, nargs="+", default=[1024])
    ap.add_argument("--bus", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--block", type=int, default=48)
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print(f"chunk {pkg.mixer_chunk()}, tile {pkg.mixer_tile_outputs()}")
    print("   K       n   Q   active   limiter   mixer ms   GB/s read   copy ms   copy GB/s   ratio")
    rng = np.random.default_rng(2025)
    for K in a.rx:
        for n in a.n:
            x = torch.randn((K, n), dtype=torch.float32, device=dev)
            y = torch.empty_like(x)
            for Q in a.bus:
                for every in (1, 16):
                    g = (rng.uniform(0.25, 1.0, (K, Q)) / np.sqrt(K / every)).astype(np.float32)
                    g[np.arange(K) % every != 0] = 0.0
                    nact = int(g.any(axis=1).sum())
                    nbytes = 4 * nact * n
                    t_copy = pkg.measure_copy(y.data_ptr(), x.data_ptr(), nbytes, a.steps, st)
                    for limit in (None, (a.block, 0.25, 0.5)):
                        m = pkg.Mixer(g, 480, limit=limit)
                        # (the limiter writes whole blocks: a batch can give up to block - 1 outputs more than n)
                        of = torch.empty((Q, n + a.block), dtype=torch.float32, device=dev)
                        oi = torch.empty((n + a.block, Q), dtype=torch.int16, device=dev)
                        m.process(x, out_f32=of, out_i16=oi)
                        torch.cuda.synchronize()
                        time.sleep(1.0)
                        t = timed(lambda: m.process(x, out_f32=of, out_i16=oi), a.steps)
                        print(f"{K:4d}  {n:6d}   {Q}   {nact:6d}   {'on ' if limit else 'off'}       {t:8.4f}   {1e-6 * nbytes / t:9.0f}   "
                              f"{t_copy:7.4f}   {1e-6 * nbytes / t_copy:9.0f}   {t / t_copy:5.2f}", flush=True)
                        m.close()
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
