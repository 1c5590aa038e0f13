"""Timing of the wideband blanker (pddc_wblank_process: k_wblank_sums, k_wblank_means, k_wblank_gate) on the GPU box.
Input: uniform noise of +-2000 codes made on the device, packed; `quiet` has no trigger at thr 16, `impulses` has one
full-size sample every 20000.  Per point: (a) WBlank.process of the batch -- the stream is read twice and written once,
18 bytes per sample, 12 of them (6 in, 6 out) the floor a single pass would move --, (b) the yardstick, measure_copy of
the same bytes (6 n from the input to the output buffer) in the same process.  GB/s counts 12 bytes per sample for both.
`chunk` is the "wblank_chunk" tunable: the samples one round of launches takes (0: 2^26); a round of 2^21 is 12 MiB in and
12 MiB out, short enough for the second read to be served from the memory-side cache if it were to help.  HIP events on
the launch stream, median of `steps` after a settle second.  `run` is the "wblank_run" tunable: the samples one workgroup of
k_wblank_gate walks (0: one tile of 2048).  The first line printed is the command line.
Usage: python tools/wblank_time.py [--steps 15] [--logs 20 24 28] [--chunks 0 8388608 2097152] [--runs 0] [--only-kernel]"""
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


def make_stream(n, every):
    """packed uniform noise of +-2000 codes, a full-size sample every `every` (0: none), made on the device in slices"""
    out = torch.empty((n, 6), dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev).manual_seed(2025)
    step = min(n, 1 << 24)
    for s in range(0, n, step):
        iq = torch.randint(-2000, 2001, (step, 2), dtype=torch.int32, device=dev, generator=gen)
        if every:
            hit = (torch.arange(s, s + step, device=dev) % every) == every - 1
            iq[hit] = torch.tensor([4000000, -4000000], dtype=torch.int32, device=dev)
        for k in range(3):
            out[s:s + step, k] = ((iq[:, 0] >> (8 * k)) & 0xFF).to(torch.uint8)
            out[s:s + step, 3 + k] = ((iq[:, 1] >> (8 * k)) & 0xFF).to(torch.uint8)
    return out.view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--logs", type=int, nargs="+", default=[20, 24, 28])
    ap.add_argument("--chunks", type=int, nargs="+", default=[0, 1 << 23, 1 << 21])
    ap.add_argument("--runs", type=int, nargs="+", default=[0])
    ap.add_argument("--guard", type=int, default=4)
    ap.add_argument("--ramp-log2", type=int, default=3)
    ap.add_argument("--thr", type=float, default=16.0)
    ap.add_argument("--only-kernel", action="store_true", help="WBlank.process only (for a kernel trace or a counter run)")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    print("python tools/wblank_time.py " + " ".join(sys.argv[1:]))
    print(f"W {a.guard} r {a.ramp_log2} thr {a.thr}; design (a): sums pass + gate pass, 18 bytes per sample moved, GB/s over 12")
    print("samples   input        B    H      chunk      run   wblank ms   GB/s    copy ms   GB/s   ratio   triggers    blanked per batch")
    for lg in a.logs:
        n = 1 << lg
        out = torch.empty(6 * n, dtype=torch.uint8, device=dev)
        for name, every in (("quiet", 0), ("impulses", 20000)):
            d = make_stream(n, every)
            torch.cuda.synchronize()
            t_cp = float("nan")
            if not a.only_kernel:
                pkg.measure_copy(out.data_ptr(), d.data_ptr(), 6 * n, 3, st)
                t_cp = pkg.measure_copy(out.data_ptr(), d.data_ptr(), 6 * n, a.steps, st)
            for B, H in ((256, 8), (4096, 16)):
                for chunk, run in ((c, r) for c in a.chunks for r in a.runs):
                    pkg.set_tunable("wblank_chunk", chunk)
                    pkg.set_tunable("wblank_run", run)
                    wb = pkg.WBlank(B, H, a.guard, a.ramp_log2, thr=a.thr)
                    wb.process(d, out=out)
                    before = wb.read()
                    torch.cuda.synchronize()
                    time.sleep(1.0)
                    t = timed(lambda: wb.process(d, out=out), a.steps)
                    after = wb.read()
                    per = lambda k: (int(after[k]) - int(before[k])) // a.steps
                    print(f"2^{lg:<2}      {name:9s} {B:5d}   {H:2d}   {chunk or (1 << 26):8d}   {pkg.wblank_run_samples():6d}   {t:9.4f}   {12e-6 * n / t:4.0f}   "
                          f"{t_cp:8.4f}   {12e-6 * n / t_cp:4.0f}   {t / t_cp:5.2f}   {per('triggers'):8d}   {per('blanked'):8d}",
                          flush=True)
                    wb.close()
            pkg.set_tunable("wblank_chunk", 0)
            pkg.set_tunable("wblank_run", 0)
            del d
            torch.cuda.empty_cache()
        del out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
