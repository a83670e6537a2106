#!/usr/bin/env python3
"""Writes tests/golden/image_metrics_ref.npz: what the REFERENCE's own mse / mae / ssim / psnr / dmpix_ssim (wildgaussians/evaluation.py) and
convert_image_dtype (wildgaussians/utils.py:108) return on the cases of tests/image_metrics_lib.py, on the CPU.

    python tests/golden/make_image_metrics_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies.  The function bodies are executed out of the reference's files at run time (the modules
themselves need packages a test machine may lack), with the argument order of compute_metrics (evaluation.py:339-347).  The fixture holds
recorded numbers only: the case table, per case psnr / ssim / mae / mse as float64 (and the dtype the reference returned them in), dmpix_ssim on
float64 copies of the same inputs, and the bytes convert_image_dtype gives for tests/image_metrics_lib.edge_floats() after render()'s
torch.clamp(x, 0, 1).nan_to_num_(0).  Inputs are regenerated from the seeds by image_metrics_lib.make_inputs.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_metrics_lib as L  # noqa: E402


def main():
    checkout = sys.argv[1]
    ns = L.reference_functions(checkout)
    arrays, dtypes = {}, {}
    for c in L.CASES:
        pred, gt = L.make_inputs(c)
        v = L.reference_values(ns, c, pred, gt)
        dtypes[c["name"]] = {k: str(np.asarray(x).dtype) for k, x in v.items()}
        for k, x in v.items():
            arrays[f"{c['name']}__{k}"] = np.asarray(x, dtype=np.float64)
        print(f"{c['name']:24s}", {k: np.asarray(x).tolist() for k, x in v.items()})
    edge = L.edge_floats()
    clamped = torch.clamp(torch.from_numpy(edge.copy()), 0, 1).nan_to_num_(0).numpy()
    arrays["edge_bytes"] = ns["convert_image_dtype"](clamped, np.uint8)
    assert arrays["edge_bytes"].dtype == np.uint8
    cases = [dict(c, shape=list(c["shape"]), roi=list(c["roi"]) if c["roi"] else None) for c in L.CASES]
    np.savez_compressed(L.GOLDEN, cases=np.array(json.dumps(cases)), dtypes=np.array(json.dumps(dtypes)), edge_count=np.array(edge.size), **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
