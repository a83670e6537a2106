#!/usr/bin/env python3
"""What the train step's image loss and its logged metrics cost between the render and the Python floats, three ways, on the same GPU in the same run.

    python scripts/bench_step_loss.py [--calls 30] [--warmup 5] [--out-dir profiles/step_loss]

Writes <out-dir>/bench.json.  Per size (1600x1200, 1920x1080) and scenario (no mask; mask; mask and a thresholded multiplier after the warm-up)
three legs alternate call by call in one process.  Each starts from the two float32 [3, H, W] renders (requiring gradients), the ground
truth, the mask and the raw multiplier on the device, and ends with both image gradients on the device and every logged metric as a Python
float on the host (wildgaussians/method.py:1920-1992):

    reference    the reference's statements in PyTorch with wg_fused_ssim.ssim swapped in (what apply_optins gives today), the metrics read
                 with one .cpu().item() each as the reference reads them
    l1_ssim      wg_fused_ssim.l1_ssim_loss plus the PyTorch statements still needed around it: scale_grads, the multiplier's threshold,
                 the mse map and the reductions; the unweighted l1 / ssim and the masked ssim come from PyTorch and one more fused SSIM map
                 under no_grad when a multiplier or a mask is present (return_parts gives only the weighted means).  Runs on the parent
                 commit unchanged: the yardstick
    step_loss    wg_fused_ssim.step_loss plus step_metrics

Host wall time per call, ended by the metrics read (device events would hide the synchronisations that are the point).  Medians of --calls
with p10 / p90.  Kernel launches, copies and host synchronisations per call are counted with torch.profiler over one call of each leg.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wild-gaussians_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
LAMBDA = 0.2


def scale_grads(values, scale):   # method.py:120-123
    grad_values = values * scale
    rest_values = values.detach() * (1 - scale)
    return grad_values + rest_values


def _logged(Ll1, ssim_value, image_toned, gt, loss, mask):
    """method.py:1968-1992 as it stands: one host read per metric."""
    metrics = {}
    with torch.no_grad():
        mse = (image_toned - gt).pow_(2)
        psnr_value = 20 * math.log10(1.) - 10 * torch.log10(mse.mean())
        metrics.update({"l1_loss": Ll1.detach().mean().cpu().item(), "ssim": ssim_value.detach().mean().cpu().item(),
                        "mse": mse.detach().mean().cpu().item(), "loss": loss.detach().cpu().item(), "psnr": psnr_value.detach().cpu().item()})

        def _reduce_masked(tensor, mask):
            return ((tensor * mask).sum() / mask.sum()).detach().cpu().item()

        if mask is not None:
            metrics["mask_percentage"] = mask.detach().mean().cpu().item()
            metrics["ssim_masked"] = _reduce_masked(ssim_value, mask)
            metrics["mse_masked"] = masked_mse = _reduce_masked(mse, mask)
            metrics["psnr_masked"] = 20 * math.log10(1.) - 10 * math.log10(masked_mse)
            metrics["l1_loss_masked"] = _reduce_masked(Ll1, mask)
    return metrics


def leg_reference(toned, raw, gt, mask, mult):
    from wg_fused_ssim import ssim
    image, image_toned = raw, toned
    if mask is not None:
        image = scale_grads(image, mask)
        image_toned = scale_grads(image_toned, mask)
    loss_mult = 1.
    if mult is not None:
        loss_mult = (mult > 1).to(dtype=mult.dtype)
    Ll1 = F.l1_loss(image_toned, gt, reduction="none")
    ssim_value = ssim(image, gt, size_average=False)
    loss = (1.0 - LAMBDA) * (Ll1 * loss_mult).mean() + LAMBDA * ((1.0 - ssim_value) * loss_mult).mean()
    loss.backward()
    return _logged(Ll1, ssim_value, image_toned, gt, loss, mask)


def leg_l1_ssim(toned, raw, gt, mask, mult):
    from wg_fused_ssim import l1_ssim_loss, ssim
    image, image_toned = raw, toned
    if mask is not None:
        image = scale_grads(image, mask)
        image_toned = scale_grads(image_toned, mask)
    loss_mult = None
    if mult is not None:
        loss_mult = (mult > 1).to(dtype=mult.dtype)
    loss, l1_mean, ssim_mean = l1_ssim_loss(image_toned, image, gt, LAMBDA, loss_mult=loss_mult, return_parts=True)
    loss.backward()
    if mask is None and mult is None:   # the parts are the logged values: only the mse is left
        with torch.no_grad():
            mse = (image_toned - gt).pow_(2).mean()
            psnr_value = 20 * math.log10(1.) - 10 * torch.log10(mse)
            return {"l1_loss": l1_mean.cpu().item(), "ssim": ssim_mean.cpu().item(), "mse": mse.cpu().item(), "loss": loss.detach().cpu().item(),
                    "psnr": psnr_value.cpu().item()}
    with torch.no_grad():               # the parts are weighted and there is no map: the reference's statements for the rest
        Ll1 = (image_toned - gt).abs()
        ssim_value = ssim(image.detach(), gt, size_average=False)
    return _logged(Ll1, ssim_value, image_toned, gt, loss, mask)


def leg_step_loss(toned, raw, gt, mask, mult):
    from wg_fused_ssim import step_loss, step_metrics
    loss, stats = step_loss(toned, raw, gt, LAMBDA, mask=mask, loss_mult=mult, mult_threshold=None if mult is None else 1.0, mult_blend=1.0)
    loss.backward()
    return step_metrics(stats)


LEGS = {"reference": leg_reference, "l1_ssim": leg_l1_ssim, "step_loss": leg_step_loss}


def stats(ms):
    v = np.sort(np.array(ms))
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "calls": len(ms)}


def count_launches(fn):
    """{"kernel_launches", "memcpy", "host_syncs"} of one call, from torch.profiler's device and runtime events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = memcpy = syncs = 0
        for e in prof.events():
            name = e.name
            if str(e.device_type).endswith("CUDA"):
                if "memcpy" in name.lower() or "copy" in name.lower() and "kernel" not in name.lower():
                    memcpy += 1
                else:
                    kernels += 1
            elif name in ("hipStreamSynchronize", "hipEventSynchronize", "hipMemcpyWithStream", "hipMemcpy"):
                syncs += 1
        return {"kernel_launches": kernels, "memcpy": memcpy, "host_syncs": syncs}
    except Exception as e:   # the profiler is an extra: the timings do not depend on it
        return {"not counted": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "step_loss"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_step_loss.py needs a GPU: there is no CPU path")
    os.makedirs(args.out_dir, exist_ok=True)
    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "lambda_dssim": LAMBDA,
              "timing": "host wall time per call: forward, backward and the metrics read to Python floats; the legs alternate call by call",
              "yardstick": "l1_ssim (code of the parent commit)", "sizes": {}}
    for (W, H) in ((1600, 1200), (1920, 1080)):
        g = torch.Generator().manual_seed(W)
        gt = torch.rand(3, H, W, generator=g)
        toned = (gt * 0.6 + 0.4 * torch.rand(3, H, W, generator=g)).to(DEV).requires_grad_(True)
        raw = (gt * 0.5 + 0.5 * torch.rand(3, H, W, generator=g)).to(DEV).requires_grad_(True)
        gt = gt.to(DEV)
        mask_t = (torch.rand(1, H, W, generator=g) < 0.7).float().to(DEV)
        mult_t = (torch.rand(1, H, W, generator=g) * 2.0).to(DEV)
        for label, mask, mult in (("no_mask", None, None), ("mask", mask_t, None), ("mask_and_multiplier", mask_t, mult_t)):
            def call(fn):
                toned.grad = raw.grad = None
                return fn(toned, raw, gt, mask, mult)

            for _ in range(args.warmup):
                for fn in LEGS.values():
                    call(fn)
            times, values = {k: [] for k in LEGS}, {}
            for _ in range(args.calls):
                for k, fn in LEGS.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    values[k] = call(fn)
                    times[k].append((time.perf_counter() - t) * 1e3)
            row = {k: stats(v) for k, v in times.items()}
            row["values"] = values
            row["step_loss_minus_reference"] = {k: values["step_loss"][k] - values["reference"][k] for k in values["reference"]}
            row["per_call"] = {k: count_launches(lambda fn=fn: call(fn)) for k, fn in LEGS.items()}
            row["step_loss_over_l1_ssim"] = row["step_loss"]["median_ms"] / row["l1_ssim"]["median_ms"]
            row["step_loss_over_reference"] = row["step_loss"]["median_ms"] / row["reference"]["median_ms"]
            result["sizes"][f"{W}x{H}_{label}"] = row
            print(f"{W}x{H} {label}: " + "  ".join(f"{k} {row[k]['median_ms']:.3f} ms" for k in LEGS), flush=True)
    with open(os.path.join(args.out_dir, "bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("bench.json written")


if __name__ == "__main__":
    main()
