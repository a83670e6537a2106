#!/usr/bin/env python3
"""Records tests/golden/step_loss_ref.npz from the reference's own statements, on the CPU of the build machine.

    python tests/golden/make_step_loss_golden.py /path/to/reference/checkout

From wildgaussians/method.py it takes, as text, the functions `scale_grads` and `ssim` and the statements of `train_iteration` from
"# Apply mask" to "# Densification" (method.py:1920-1992), and executes them as they stand -- method.py itself needs packages the build
machine lacks -- once in float32 and once in float64 per case of tests/step_loss_lib.py: `self`, the uncertainty model and the config are
stand-ins that hold only what those statements read.  Recorded per case: the inputs, every logged value, the loss and its two weighted
terms, and both image gradients, for both precisions.  No reference text is written anywhere.
"""
import json
import math
import os
import sys
import textwrap
import types
from typing import Any

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import step_loss_lib as L  # noqa: E402


def reference_text(ref):
    src = open(os.path.join(ref, "wildgaussians", "method.py")).read()

    def function(header):
        a = src.index(header)
        return src[a:src.index("\n\n\n", a)]

    a = src.index("        # Apply mask\n")
    b = src.index("            # Densification\n", a)
    return function("def scale_grads(values, scale):"), function("def ssim(img1, img2, window_size=11, size_average=True):"), \
        textwrap.dedent(src[a:b])


def run_reference(text, case, inputs, dtype):
    scale_grads_src, ssim_src, block = text
    ns = {"torch": torch, "F": F, "math": math, "Any": Any}
    exec(scale_grads_src, ns)
    exec(ssim_src, ns)
    toned, raw, gt, mask, mult = (None if t is None else t.to(dtype) for t in inputs)
    leaf_toned, leaf_raw = toned.clone().requires_grad_(True), raw.clone().requires_grad_(True)
    um = None
    if case["schedule"] is not None:
        um = types.SimpleNamespace(get_loss=lambda gt_image, prediction, _cache_entry=None: (0, {}, mult))
    it, start, iters = case["schedule"] or (5000, 0, 0)
    config = types.SimpleNamespace(uncertainty_warmup_start=start, uncertainty_warmup_iters=iters, uncertainty_center_mult=False,
                                   uncertainty_scale_grad=False, lambda_dssim=L.LAMBDA, densify_until_iter=15000, opacity_reset_interval=3000,
                                   uncertainty_protected_iters=500)
    ns.update(self=types.SimpleNamespace(model=types.SimpleNamespace(uncertainty_model=um, xyz=[0] * 7), config=config), iteration=it,
              camera_id=0, image=leaf_raw, image_toned=leaf_toned, gt_image=gt, mask=mask)
    exec(block, ns)
    metrics = dict(ns["metrics"])
    assert metrics.pop("num_gaussians") == 7
    assert set(metrics) == set(L.LOGGED) | (set(L.LOGGED_MASKED) if mask is not None else set()), sorted(metrics)
    with torch.no_grad():   # the loss's two weighted terms: tensors the statements formed on the way (method.py:1962-1963)
        metrics["l1_weighted"] = (ns["Ll1"] * ns["loss_mult"]).mean().item()
        metrics["dssim_weighted"] = ((1.0 - ns["ssim_value"]) * ns["loss_mult"]).mean().item()
    stats = np.array([metrics.get(k, float("nan")) for k in L.STATS], dtype=np.float64)
    return stats, leaf_toned.grad.numpy(), leaf_raw.grad.numpy()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    text = reference_text(ref)
    arrays = {}
    for i, case in enumerate(L.CASES):
        inputs = L.make_inputs(case["shape"], case["mask"], case["schedule"] is not None, case["seed"])
        for name, t in zip(("toned", "raw", "gt", "mask", "mult"), inputs):
            if t is not None:
                arrays[f"{i}_{name}"] = t.numpy()
        for p, dtype in (("32", torch.float32), ("64", torch.float64)):
            stats, g_toned, g_raw = run_reference(text, case, inputs, dtype)
            arrays[f"{i}_stats{p}"], arrays[f"{i}_grad_toned{p}"], arrays[f"{i}_grad_raw{p}"] = stats, g_toned, g_raw
        print(case["name"], " ".join(f"{k}={v:.6g}" for k, v in zip(L.STATS, arrays[f"{i}_stats64"])))
    arrays["cases"] = np.array(json.dumps(L.CASES))
    np.savez(L.GOLDEN, **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
