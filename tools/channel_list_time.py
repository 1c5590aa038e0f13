"""Timing of the channel list on the GPU box: Channelizer.process, Tuner.process and their sum, in range mode with the full
matrix (rows of M values, the tuner gathers its columns) and in list mode (rows of the receivers' n distinct channels,
tuner_channel_list), in the same process on the same input.  M = 4096, hop 2048, P = 4; the receivers are placed as in
tools/tuner_time.py (seeded random words).  On-device LCG input, HIP events on the launch stream, median of `steps`
after a settle second.  The tuner's outputs of the two modes are compared bit for bit before anything is timed.  With
tools/ubench/chan_list_staged.patch applied, --stores 1 2 3 times list mode once per store pattern of k_channelize_list
(tunable chan_list_store: 1 direct 8-byte stores, 2 the row staged in LDS, 3 staged in buf).  (The timed calls feed the same batch again, so the
stream goes on and a call gives ns / hop rows, at most 7 more than the S of the first call and of the buffer column:
the buffers have 16 rows of slack.)
Usage: python tools/channel_list_time.py [--steps 15] [--logs 24 28] [--rx 256 1024] [--taps 64] [--decim 4] [--stores ...]"""
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
    ap.add_argument("--stores", type=int, nargs="+", default=[], help="chan_list_store values (the staged-store patch)")
    a = ap.parse_args()
    lists = [f"list{v}" for v in a.stores] or ["list"]
    M, hop, T, R = 4096, 2048, a.taps, a.decim
    st = torch.cuda.current_stream().cuda_stream
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, R)
    print(f"M {M} hop {hop} P 4 T {T} R {R}, median of {a.steps}; ms")
    print("samples    rows      K      n   mode     rows buffer B   channelizer      tuner        sum")
    for lg in a.logs:
        ns = 1 << lg
        d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
        pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, 12345, 0, st))
        rng = np.random.default_rng(2024)
        for K in a.rx:
            words = [int(v) for v in rng.integers(0, 1 << 32, K, dtype=np.uint64)]
            chans = pkg.tuner_channel_list(M, words)
            res, outs = {}, {}
            for mode in ["range"] + lists:
                if a.stores:
                    pkg.set_tunable("chan_list_store", int(mode[4:]) if mode != "range" else 0)
                ch = pkg.Channelizer(M, w, hop)
                if mode != "range":
                    ch.set_channels(chans)
                S = ch.next_rows(ns)
                buf = torch.empty((S + 16, ch.count), dtype=torch.complex64, device=dev)
                tun = pkg.Tuner(ch, words, h, R)
                out = torch.empty((K, (S - T) // R + 1 + T), dtype=torch.complex64, device=dev)
                rows = ch.process(d, out=buf)
                outs[mode] = tun.process(rows, out=out).clone()
                torch.cuda.synchronize()
                time.sleep(1.0)
                t_ch = timed(lambda: ch.process(d, out=buf), a.steps)
                t_tu = timed(lambda: tun.process(rows, out=out), a.steps)
                res[mode] = (t_ch, t_tu)
                print(f"2^{lg:<2}   {S:7d}   {K:4d}   {ch.count:4d}   {mode:6s}   {8 * S * ch.count:13d}   {t_ch:11.4f}   "
                      f"{t_tu:8.4f}   {t_ch + t_tu:8.4f}", flush=True)
                tun.close()
                ch.close()
                del buf, rows, out
                torch.cuda.empty_cache()
            rc, rt = res["range"]
            for mode in lists:
                same = torch.equal(torch.view_as_real(outs["range"]).view(torch.int32),
                                   torch.view_as_real(outs[mode]).view(torch.int32))
                lc, lt = res[mode]
                print(f"        {mode} / range: channelizer {lc / rc:.3f}, tuner {lt / rt:.3f}, sum {(lc + lt) / (rc + rt):.3f}; "
                      f"tuner outputs bit-identical: {same}", flush=True)
            if a.stores:
                pkg.set_tunable("chan_list_store", 0)
            del outs
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
