#!/usr/bin/env python3
"""The fixtures of tests/test_gpu_i8x_loaders.py (tests/golden/i8x_loaders_<case>.f32): every case of
tests/i8x_loader_cases.py run on the GPU, the batches' outputs in order as float32 (the large cases: the outputs
round tile, loader-round and batch boundaries only, i8x_loader_cases.kept).

  python tools/i8x_loader_golden.py record [case ...]    write the fixtures (from the build whose bits are the reference:
                                                         select it with PDDC_DDC_LIB, tools/ab.sh)
  python tools/i8x_loader_golden.py check [case ...]     compare the loaded build with them, bit for bit

Both print, per case, the outputs' size, the kernels the pipeline chose per batch where that can be asked, the members that
shared a bank / gang launch per round, and the worst per-chunk error against the oracle (oracle.chain_check)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import i8x_loader_cases as K
from oracle import oracle as O

pkg = importlib.import_module("libperseus-sdr_amd")


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "check"
    names = sys.argv[2:] or K.CASES
    if mode not in ("record", "check"):
        sys.exit(__doc__)
    O.build()
    dev = torch.device("cuda:0")
    print("library:", os.environ.get("PDDC_DDC_LIB", pkg.DDC_LIB))
    bad = 0
    for name in names:
        recs, shared = K.run_case(pkg, dev, O, name)
        y = K.flat(recs, name)
        worst = 0.0
        for r in recs:
            if r["out"].size:
                c = O.chain_check(r["packed"], r["first_in"], r["n_in"], r["stages"], r["out"], freg=r["freg"], mix=r["mix"], tol=1e-6)
                worst = max(worst, c["worst_chunk_rel_err"])
                if not c["ok"] or c["n"] != r["out"].size // 2:
                    print(f"   {name}: batch at {r['first_in']} (+{r['n_in']}): oracle says {c}")
                    bad += 1
        line = f"{name:14s} {y.size * 4:8d} bytes, {len(recs):3d} batches, oracle worst chunk {worst:.2e}, shared {shared}"
        if mode == "record":
            y.tofile(K.golden_path(name))
            print(line, "-> recorded", flush=True)
        else:
            g = np.fromfile(K.golden_path(name), dtype=np.float32)
            same = g.size == y.size and np.array_equal(g.view(np.uint32), y.view(np.uint32))
            nd = int(np.count_nonzero(g.view(np.uint32) != y.view(np.uint32))) if g.size == y.size else -1
            print(line, "-> same bits" if same else f"-> DIFFERS ({nd} words; sizes {g.size} / {y.size})", flush=True)
            bad += 0 if same else 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
