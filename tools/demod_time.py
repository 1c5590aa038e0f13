"""Timing of the demodulator (pddc_demod_process, k_demod) on the GPU box: K receivers behind Channelizer (M = 4096, hop
2048) -> Tuner (T = 64, R = 4), modes interleaved receiver by receiver (AM, FM, SSB).  Per point: (a) the detectors
alone, (b) the detectors with DCBLOCK + AGC, (c) Tuner.process for the same batch, (d) the torch expressions for the
three detectors on the same tensor (abs, angle of the lagged product, real part of a phasor product with the phasor
table built outside the timed region) -- torch has no form for the recursive part.  Same on-device LCG input, same
process, HIP events on the launch stream, median of `steps` after a settle second.
Usage: python tools/demod_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--only-kernel]"""
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
    ap.add_argument("--only-kernel", action="store_true", help="k_demod only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    M, hop, T, R = 4096, 2048, 64, 4
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    both = pkg.PDDC_DEMOD_DCBLOCK | pkg.PDDC_DEMOD_AGC
    print("samples   outputs      K   detect ms   GB/s   +DC+AGC ms   us/output   k_tune ms   torch detect ms")
    for lg in a.logs:
        ns = 1 << lg
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        ch = pkg.Channelizer(M, w, hop)
        rows = ch.process(d)
        S = rows.shape[0]
        rng = np.random.default_rng(2024)
        for K in a.rx:
            words = [int(v) for v in rng.integers(0, 1 << 32, K, dtype=np.uint64)]
            bfo = [int(v) for v in rng.integers(0, 1 << 32, K, dtype=np.uint64)]
            tun = pkg.Tuner(ch, words, h, R)
            zbuf = torch.empty((K, (S - T) // R + 1 + T), dtype=torch.complex64, device=dev)
            z = tun.process(rows, out=zbuf)
            n = z.shape[1]
            out = torch.empty((K, n), dtype=torch.float32, device=dev)
            plain = pkg.Demod([(j % 3, bfo[j], 0) for j in range(K)])
            post = pkg.Demod([(j % 3, bfo[j], both) for j in range(K)])
            plain.process(z, out=out)
            post.process(z, out=out)
            t_tune = t_torch = float("nan")
            if not a.only_kernel:
                m = (np.arange(n, dtype=np.uint64)[None, :] * np.array(bfo[2::3], dtype=np.uint64)[:, None]) & np.uint64(0xFFFFFFFF)
                ph = torch.from_numpy(np.exp(-2j * np.pi * m.astype(np.float64) / 2.0 ** 32).astype(np.complex64)).to(dev)

                def torch_path():
                    zf = z[1::3]
                    return (z[0::3].abs(), torch.angle(zf[:, 1:] * zf[:, :-1].conj()) * (1.0 / np.pi), (z[2::3] * ph).real)

                torch_path()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t_torch = timed(torch_path, a.steps)
                t_tune = timed(lambda: tun.process(rows, out=zbuf), a.steps)
                del ph
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_plain = timed(lambda: plain.process(z, out=out), a.steps)
            t_post = timed(lambda: post.process(z, out=out), a.steps)
            print(f"2^{lg:<2}     {n:7d}   {K:4d}   {t_plain:9.4f}   {12e-6 * K * n / t_plain:4.0f}   {t_post:10.4f}   "
                  f"{1e3 * t_post / n:9.4f}   {t_tune:9.4f}   {t_torch:15.4f}", flush=True)
            for o in (plain, post, tun):
                o.close()
            del out, zbuf, z
            torch.cuda.empty_cache()
        ch.close()
        del d, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
