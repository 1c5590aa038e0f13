"""Timing of the noise blanker (pddc_blanker_process, k_blanker) on the GPU box: K receivers behind Channelizer (M = 4096,
hop 2048) -> Tuner (T = 64, R = 4), B = 48, guard 3, ramp 5 (D = 8), every receiver ON with thr 16 (full-scale noise in
every channel: a trigger every few million samples, the common case of a quiet band; --thr 3 makes about one sample in
twenty a trigger).  Per point: (a) Blanker.process -- 16 bytes per value: 8 of z read, 8 of out written --, (b) the
yardstick, Squelch.process on the same z in the same process (B = 48, attack 2, hang 3, ramp 37), which moves the same
16 bytes per value: 8 of z and 4 of a read, 4 of out written.  Same on-device LCG input, HIP events on the launch
stream, median of `steps` after a settle second.
Usage: python tools/blanker_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--block 48] [--guard 3] [--ramp 5]
                                    [--thr 16] [--only-kernel]"""
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
    ap.add_argument("--block", type=int, default=48)
    ap.add_argument("--guard", type=int, default=3)
    ap.add_argument("--ramp", type=int, default=5)
    ap.add_argument("--thr", type=float, default=16.0)
    ap.add_argument("--only-kernel", action="store_true", help="k_blanker only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    M, hop, T, R = 4096, 2048, 64, 4
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    print(f"B {a.block} W {a.guard} R {a.ramp} thr {a.thr}")
    print("samples   outputs      K   blanker ms   GB/s   us/output   squelch ms   GB/s   ratio   triggers   blanked per batch")
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
            tun = pkg.Tuner(ch, words, h, R)
            zbuf = torch.empty((K, (S - T) // R + 1 + T), dtype=torch.complex64, device=dev)
            z = tun.process(rows, out=zbuf)
            n = z.shape[1]
            out = torch.empty((K, n), dtype=torch.complex64, device=dev)
            nb = pkg.Blanker([(a.thr, pkg.PDDC_NB_ON)] * K, a.block, a.guard, a.ramp)
            nb.process(z, out=out)
            before = nb.read()
            torch.cuda.synchronize()
            time.sleep(1.0)
            t_nb = timed(lambda: nb.process(z, out=out), a.steps)
            after = nb.read()
            per = lambda name: (int(after[name].astype(np.int64).sum()) - int(before[name].astype(np.int64).sum())) // a.steps
            t_sq = float("nan")
            if not a.only_kernel:
                au = torch.empty((K, n), dtype=torch.float32, device=dev)
                gated = torch.empty((K, n), dtype=torch.float32, device=dev)
                plain = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)] * K)
                plain.process(z, out=au)
                sq = pkg.Squelch([(1.3, 1.1, (pkg.PDDC_SQL_GATE | pkg.PDDC_SQL_RELATIVE) if j % 2 else 0) for j in range(K)],
                                 a.block, 2, 3, 37, up=1.03125)
                lv = torch.empty((K, n // a.block + 1), dtype=torch.float32, device=dev)
                ss = torch.empty((K, n // a.block + 1), dtype=torch.uint8, device=dev)
                sq.process(z, au, out=gated, levels=lv, states=ss)
                torch.cuda.synchronize()
                t_sq = timed(lambda: sq.process(z, au, out=gated, levels=lv, states=ss), a.steps)
                for o in (sq, plain):
                    o.close()
                del au, gated, lv, ss
            print(f"2^{lg:<2}     {n:7d}   {K:4d}   {t_nb:10.4f}   {16e-6 * K * n / t_nb:4.0f}   {1e3 * t_nb / n:9.4f}   "
                  f"{t_sq:10.4f}   {16e-6 * K * n / t_sq:4.0f}   {t_nb / t_sq:5.2f}   {per('triggers'):8d}   {per('blanked'):8d}",
                  flush=True)
            for o in (nb, tun):
                o.close()
            del out, zbuf, z
            torch.cuda.empty_cache()
        ch.close()
        del d, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
