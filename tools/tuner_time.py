"""Timing of the tuner (pddc_tuner_process, k_tune) on the GPU box: K receivers behind a Channelizer of M = 4096, hop
2048, against the path a host had before it on the same rows (rows[:, idx] times a phasor table built outside the timed
region, then a strided conv1d with h), and beside Channelizer.process for the same batch.  Same on-device LCG input,
same process, HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/tuner_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--taps 64] [--decim 4] [--no-host]"""
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
    ap.add_argument("--logs", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--rx", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--taps", type=int, default=64)
    ap.add_argument("--decim", type=int, default=4)
    ap.add_argument("--no-host", action="store_true", help="k_tune only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    M, hop, T, R = 4096, 2048, a.taps, a.decim
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    print("samples    rows      K   k_tune ms   GB/s(rows)   torch path ms   ratio   k_channelize ms")
    for lg in a.logs:
        ns = 1 << lg
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        ch = pkg.Channelizer(M, w, hop)
        S = ch.next_rows(ns)
        buf = torch.empty((S + 16, M), dtype=torch.complex64, device=dev)
        rows = ch.process(d, out=buf)
        t_chan = timed(lambda: ch.process(d, out=buf), a.steps)
        rng = np.random.default_rng(2024)
        for K in a.rx:
            words = [int(v) for v in rng.integers(0, 1 << 32, K, dtype=np.uint64)]
            kr = [pkg.tuner_channel(M, f) for f in words]
            tun = pkg.Tuner(ch, words, h, R)
            out = torch.empty((K, (S - T) // R + 1 + T), dtype=torch.complex64, device=dev)
            tun.process(rows, out=out)
            t_host = float("nan")
            if not a.no_host:
                idx = torch.tensor([k for k, _ in kr], device=dev)
                sd = (np.arange(S, dtype=np.uint64) * np.uint64(hop)) & np.uint64(0xFFFFFFFF)
                res = np.array([r for _, r in kr], dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
                th = (sd[:, None] * res[None, :]) & np.uint64(0xFFFFFFFF)
                ph = torch.from_numpy(np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32).astype(np.complex64)).to(dev)
                wt = torch.from_numpy(h[::-1].copy()).to(dev).view(1, 1, T).repeat(2, 1, 1)

                def host_path():
                    z = rows[:, idx] * ph
                    return torch.nn.functional.conv1d(torch.view_as_real(z).permute(1, 2, 0), wt, stride=R, groups=2)

                host_path()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t_host = timed(host_path, a.steps)
                del ph
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_new = timed(lambda: tun.process(rows, out=out), a.steps)
            print(f"2^{lg:<2}   {S:7d}   {K:4d}   {t_new:9.4f}   {8e-6 * S * M / t_new:10.0f}   {t_host:13.4f}   "
                  f"{t_host / t_new:5.2f}   {t_chan:15.4f}", flush=True)
            tun.close()
            del out
            torch.cuda.empty_cache()
        ch.close()
        del d, buf, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
