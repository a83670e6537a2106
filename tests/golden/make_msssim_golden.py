#!/usr/bin/env python3
"""Writes tests/golden/msssim_ref.npz: what the REFERENCE's own ssim_down / msssim (wildgaussians/method.py:126-187, with _ssim_parts and
ssim) return on the cases of tests/msssim_lib.py, on the CPU.

    python tests/golden/make_msssim_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies.  As tests/test_ssim.py does for ssim, the four function bodies are executed out of
method.py (the module itself needs packages a test machine may lack).  The fixture holds recorded data only: per case its seed, shape, kind
and arguments, the reference's float32 output, its output on the same inputs in float64 (its window is still built from float32 taps:
`torch.Tensor([...])`), and ref32_dev = max |float32 - float64|.  Inputs are regenerated from the seed by tests/msssim_lib.make_inputs.
"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import msssim_lib as L  # noqa: E402


def reference_functions(checkout):
    src = open(os.path.join(checkout, "wildgaussians", "method.py")).read()
    ns = {"torch": torch, "F": F, "math": math}
    for head in ("def ssim(img1, img2, window_size=11, size_average=True):", "def ssim_down(x, y, max_size=None):",
                 "def _ssim_parts(img1, img2, window_size=11):", "def msssim(x, y, max_size=None, min_size=200):"):
        a = src.index(head)
        exec(src[a:src.index("\n\n\n", a)], ns)  # one function body
    return {"msssim": ns["msssim"], "ssim_down": ns["ssim_down"]}


def main():
    checkout = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    fns = reference_functions(checkout)
    torch.set_num_threads(1)
    arrays, devs, cases = {}, [], []
    for i, c in enumerate(L.CASES):
        o32 = L.run_case(c, fns, torch.float32)
        o64 = L.run_case(c, fns, torch.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and o32.shape == o64.shape
        arrays[f"out32_{i}"], arrays[f"out64_{i}"] = o32, o64
        devs.append(float(np.abs(o32.astype(np.float64) - o64).max()))
        cases.append(dict(c, shape=list(c["shape"])))
        print(f"{L.case_id(c):55s} out {o32.shape}  ref32_dev {devs[-1]:.3e}  range [{o64.min():.4f}, {o64.max():.4f}]")
    np.savez_compressed(L.GOLDEN, cases=np.array(json.dumps(cases)), ref32_dev=np.array(devs, dtype=np.float64), **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
